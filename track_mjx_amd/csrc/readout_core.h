// csrc/readout_core.h — the bodies of the linear-readout kernels (DESIGN.md "Readout"; include/tmjx.h: tmjx_readout_*): ridge regression from
// recorded activations x [n][d] to targets y [n][m] in the eigenbasis the wide PCA leaves on the device.  Written with the PCA_WG / PCA_PAR /
// PCA_SYNC / PCA_PRIVATE discipline of csrc/wg_core.h, so that they also compile on the host (tests/hostemu/readout_emu.cpp); the moments are
// csrc/moments_core.h, the eigenbasis and the transform's stage sizes csrc/pca_wide_core.h.  Every product is a chain of float32 FMAs in a fixed
// order; every sum across workgroups is float64 in a fixed order: no atomics, the same bits on every run.
#pragma once
#include "pca_wide_core.h"

#define READOUT_MAX_M 512
#define READOUT_MAX_L 16
#define READOUT_TILE_M 64        // targets of a cross-moment tile (its features: PCA_WIDE_TILE)
#define READOUT_TILE 64          // side of an output tile of the two small GEMMs, and the columns of a tile of the score / predict product
#define READOUT_LD 65            // row stride of their stages
#define READOUT_ROWS 64          // rows of x per pass of the score / predict product
#define READOUT_SCORE_SUB 4      // passes of a score workgroup: its row block is PCA_ROWS_PER_WG = 256 rows, one float64 partial per block and column

struct ReadoutLambdas { float v[READOUT_MAX_L]; };

PCA_HD int readout_tiles(int v, int tile) { return (v + tile - 1) / tile; }

// ----------------------------------------------------------------------------------------------- cross moment
// Output tile (ti, tj) of (x - mean_x)^T (y - mean_y) over super-chunk s of pca_wide_split(n): the features [128 ti, 128 ti + 128) against the
// targets [64 tj, 64 tj + 64), moments_tile_wg<8, 4>.  partial: [S][d][m] float64.  s_x: [PCA_KB][PCA_WIDE_TILE], s_y: [PCA_KB][READOUT_TILE_M] floats
// of LDS.
PCA_WG void readout_cross_wg(const float *x, int64_t ldx, const float *y, int64_t ldy, int n, int d, int m, const float *mean_x, const float *mean_y, int ti,
                             int tj, int s, double *partial, float *s_x, float *s_y) {
  const PcaWideSplit sp = pca_wide_split(n);
  const int chunk0 = s * sp.per, chunk1 = chunk0 + sp.per < sp.nchunks ? chunk0 + sp.per : sp.nchunks;
  moments_tile_wg<8, 4>(x, ldx, mean_x, d, ti * PCA_WIDE_TILE, y, ldy, mean_y, m, tj * READOUT_TILE_M, n, chunk0, chunk1, partial + (int64_t)s * d * m, m, s_x, s_y);
}

// element e of C [d][m]: the super-chunks' partials added in order, in float64, over n - 1
TM_DEV float readout_cross_reduce(const double *partial, int S, int d, int m, int n, int e) {
  return (float)(wg_sum(partial + e, S, (int64_t)d * m) / (double)(n - 1));
}

// ----------------------------------------------------------------------------------------------- Z and the weights
// out[r][c] = sum_k A(r, k) scale(k) b[k][c] for the rows [r0, r0 + 64) and the columns [c0, c0 + 64), r and k below d, c below m; one fmaf chain per
// output in ascending k.  TA = false: A(r, k) = a[r][k] (Z = components . C);  TA = true: A(r, k) = a[k][r] (W = components^T . diag . Z).
// variance = NULL: scale = 1; else scale(k) = 1 / (variance[k] + lambda), applied to the row of b as it is staged.  Thread (ty, tx) owns the rows
// ty + 16 u and the columns tx + 16 v.  s_a, s_b: [PCA_KB][READOUT_LD] floats of LDS.
template <bool TA>
PCA_WG void readout_gemm_wg(const float *a, const float *b, const float *variance, float lambda, int d, int m, float *out, int r0, int c0, float *s_a,
                            float *s_b) {
  PCA_PRIVATE(float, acc, 16);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < 16; e++) PCA_MINE(acc, tid)[e] = 0.f;
  }
  for (int k0 = 0; k0 < d; k0 += PCA_KB) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < PCA_KB * READOUT_TILE; e += PCA_THREADS) {
        const int kk = TA ? e / READOUT_TILE : e % PCA_KB, r = TA ? e % READOUT_TILE : e / PCA_KB;
        const bool in = k0 + kk < d && r0 + r < d;
        s_a[kk * READOUT_LD + r] = in ? (TA ? a[(int64_t)(k0 + kk) * d + r0 + r] : a[(int64_t)(r0 + r) * d + k0 + kk]) : 0.f;
      }
      for (int e = tid; e < PCA_KB * READOUT_TILE; e += PCA_THREADS) {
        const int kk = e / READOUT_TILE, c = e % READOUT_TILE;
        float v = 0.f;
        if (k0 + kk < d && c0 + c < m) {
          v = b[(int64_t)(k0 + kk) * m + c0 + c];
          if (variance) v *= 1.f / (variance[k0 + kk] + lambda);
        }
        s_b[kk * READOUT_LD + c] = v;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
      float *mine = PCA_MINE(acc, tid);
#pragma unroll 4
      for (int kk = 0; kk < PCA_KB; kk++) {
        float fa[4], fb[4];
#pragma unroll
        for (int u = 0; u < 4; u++) fa[u] = s_a[kk * READOUT_LD + ty + 16 * u];
#pragma unroll
        for (int v = 0; v < 4; v++) fb[v] = s_b[kk * READOUT_LD + tx + 16 * v];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
          for (int v = 0; v < 4; v++) mine[u * 4 + v] = fmaf(fa[u], fb[v], mine[u * 4 + v]);
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int r = r0 + ty + 16 * u, c = c0 + tx + 16 * v;
        if (r < d && c < m) out[(int64_t)r * m + c] = PCA_MINE(acc, tid)[u * 4 + v];
      }
  }
}

// ----------------------------------------------------------------------------------------------- score and predict
// The product (x - mean_x) . W for `nsub` passes of 64 rows from row r0 and the 64 columns from q0 of the Q = L m output columns: column q is
// target q % m under penalty q / m, its weights w[q / m][k][q % m] (w: [L][d][m]).  One fmaf chain per output in ascending k; PCA_WIDE_TK features
// at a time are staged as s_x[k][row] and s_w[k][column].  Thread (ty, tx) owns the rows ty + 16 u and the columns tx + 16 v.  The prediction is
// yhat = product + mean_y[q % m], rounded to float32.
//   SCORE = false: out[row][q] = yhat (L = 1: Q = m); nsub = 1.
//   SCORE = true:  nothing is stored; the thread adds (y[row][q % m] - yhat)^2 of its rows, in row order, into one float64 sum per column; the 16
//                  ty of a column are then added in order: partial[block][q], block = r0 / (64 nsub).  s_red: [16][READOUT_TILE] doubles of LDS.
template <bool SCORE>
PCA_WG void readout_apply_wg(const float *x, int n, int d, int64_t ldx, const float *mean_x, const float *w, int m, int Q, const float *mean_y, const float *y,
                             int64_t ldy, float *out, int64_t ldo, double *partial, int64_t r0, int nsub, int q0, float *s_x, float *s_w, double *s_red) {
  PCA_PRIVATE(float, acc, 16);
  PCA_PRIVATE(double, sum, 4);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int v = 0; v < 4; v++) PCA_MINE(sum, tid)[v] = 0.0;
  }
  for (int sub = 0; sub < nsub; sub++) {
    const int64_t rs = r0 + (int64_t)sub * READOUT_ROWS;
    if (rs >= n) break;                                        // (uniform over the workgroup)
    PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
      for (int e = 0; e < 16; e++) PCA_MINE(acc, tid)[e] = 0.f;
    }
    for (int k0 = 0; k0 < d; k0 += PCA_WIDE_TK) {
      PCA_PAR(tid, PCA_THREADS) {
        for (int e = tid; e < READOUT_ROWS * PCA_WIDE_TK; e += PCA_THREADS) {
          const int row = e / PCA_WIDE_TK, k = e % PCA_WIDE_TK;
          s_x[k * READOUT_LD + row] = (rs + row < n && k0 + k < d) ? x[(rs + row) * ldx + k0 + k] - mean_x[k0 + k] : 0.f;
        }
        for (int e = tid; e < PCA_WIDE_TK * READOUT_TILE; e += PCA_THREADS) {
          const int k = e / READOUT_TILE, c = e % READOUT_TILE, q = q0 + c;
          s_w[k * READOUT_LD + c] = (q < Q && k0 + k < d) ? w[((int64_t)(q / m) * d + k0 + k) * m + q % m] : 0.f;
        }
      }
      PCA_SYNC();
      PCA_PAR(tid, PCA_THREADS) {
        const int ty = tid >> 4, tx = tid & 15, kn = d - k0 < PCA_WIDE_TK ? d - k0 : PCA_WIDE_TK;
        float *mine = PCA_MINE(acc, tid);
        for (int k = 0; k < kn; k++) {
          float a[4], b[4];
#pragma unroll
          for (int u = 0; u < 4; u++) a[u] = s_x[k * READOUT_LD + ty + 16 * u];
#pragma unroll
          for (int v = 0; v < 4; v++) b[v] = s_w[k * READOUT_LD + tx + 16 * v];
#pragma unroll
          for (int u = 0; u < 4; u++)
#pragma unroll
            for (int v = 0; v < 4; v++) mine[u * 4 + v] = fmaf(a[u], b[v], mine[u * 4 + v]);
        }
      }
      PCA_SYNC();
    }
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int q = q0 + tx + 16 * v;
        if (q < Q) {
          const int c = q % m;
          const float my = mean_y[c];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int64_t row = rs + ty + 16 * u;
            if (row < n) {
              const float yhat = PCA_MINE(acc, tid)[u * 4 + v] + my;
              if (SCORE) {
                const double e = (double)y[row * ldy + c] - (double)yhat;
                PCA_MINE(sum, tid)[v] += e * e;
              } else {
                out[row * ldo + q] = yhat;
              }
            }
          }
        }
      }
    }
  }
  if (SCORE) {
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
      for (int v = 0; v < 4; v++) s_red[ty * READOUT_TILE + tx + 16 * v] = PCA_MINE(sum, tid)[v];
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      if (tid < READOUT_TILE && q0 + tid < Q) {
        double s = 0.0;
        for (int ty = 0; ty < 16; ty++) s += s_red[ty * READOUT_TILE + tid];
        partial[(r0 / (READOUT_ROWS * (int64_t)nsub)) * Q + q0 + tid] = s;
      }
    }
  }
}

// sse of output column q: the row blocks' partials added in block order
TM_DEV double readout_sse_col(const double *partial, int nblocks, int Q, int q) { return wg_sum(partial + q, nblocks, Q); }

// The centred sum of squares of y over super-chunk s and the columns [128 cb, 128 cb + 128): the column-sum body with the term (y - mean)^2, the
// column mean in float64 from colsum's partials [S][m].  partial: [S][m].  s_sum: [2][128] doubles of LDS.
PCA_WG void readout_sst_wg(const float *y, int64_t ldy, int n, int m, int s, int cb, const double *colsum, double *partial, double *s_sum) {
  pca_wide_colsum_wg<true>(y, ldy, n, m, s, cb, partial, s_sum, colsum);
}

// sst of column c: the super-chunks' partials added in order
TM_DEV double readout_sst_col(const double *partial, int S, int m, int c) { return wg_sum(partial + c, S, m); }
