// csrc/compare_core.h — the bodies of the representation-comparison kernels (DESIGN.md "Representation comparison"; include/tmjx.h: tmjx_cka_linear,
// tmjx_rdm_corr, tmjx_cca, tmjx_compare_svd): the Frobenius norms of the centred covariances, the all-pairs pass over two feature sets at once
// that never writes either distance matrix, the small float64 products of the whitened cross matrix, and a one-sided Jacobi singular value
// decomposition in one workgroup.  Written with the PCA_WG / PCA_PAR / PCA_SYNC / PCA_PRIVATE discipline of csrc/wg_core.h, so that they also
// compile on the host (tests/hostemu/compare_emu.cpp).  The moments are csrc/moments_core.h in the readout's tiling (readout_cross_wg: float32
// FMAs inside a chunk of 256 rows, float64 across chunks and super-chunks); the tournament of the decomposition is pca_pair; every pair of rows is one chain of float32 operations in ascending feature order; every sum across
// pairs, tiles, rows of a matrix or workgroups is float64 in a fixed order: no atomics of any kind, the same bits on every run.
#pragma once
#include "pca_core.h"

#define COMPARE_MAX_D 1024
#define COMPARE_MAX_N 32768       // rows of the all-pairs entry: 5.4e8 pairs
#define COMPARE_MAX_RANK 128      // components kept on a side of the CCA: a [128][129] float64 image is 129 KB of the CU's 160 KB of LDS
#define COMPARE_ROWS 128          // rows i of a pair tile (the kNN kernel's queries)
#define COMPARE_TILE 64           // rows j of a pair tile (its references)
#define COMPARE_TK 32             // features staged per barrier pair
#define COMPARE_LDI 132           // row stride of the staged i rows  s_i[feature][row]: a thread reads its 8 rows as two 16-byte words
#define COMPARE_LDJ 68            // row stride of the staged j rows  s_j[feature][row]: its 4 rows as one
#define COMPARE_STAGE (COMPARE_TK * (COMPARE_LDI + COMPARE_LDJ))      // floats of the stage (25.6 KB: six workgroups a CU)
#define COMPARE_SVD_SWEEPS 60
#define COMPARE_SVD_QUAD 4        // threads that share a column pair of the decomposition
#define COMPARE_SVD_PAIRS (PCA_THREADS / COMPARE_SVD_QUAD)
#define COMPARE_SVD_TOL 9.094947017729282e-13      // 2^-40: a column pair is rotated while |g_p . g_q| > 2^-40 ||g_p|| ||g_q||
#define COMPARE_EIG_FLOOR 9.5367431640625e-07      // 2^-20: a component is never kept at or below this share of the largest eigenvalue

#define COMPARE_SQEUCLIDEAN 0
#define COMPARE_EUCLIDEAN 1
#define COMPARE_CORRELATION 2
#define COMPARE_LABEL 3

static_assert(5 * PCA_THREADS * sizeof(double) <= COMPARE_STAGE * sizeof(float), "a tile's five sums are reduced in the room of the stage");
static_assert(2 * COMPARE_SVD_PAIRS >= COMPARE_MAX_RANK, "one pass of the workgroup covers every pair of a round");

typedef float cmp_f4 __attribute__((vector_size(16)));

// ----------------------------------------------------------------------------------------------- the Frobenius norm of a moment
// Row `row` of C [d][m] = (the super-chunks' float64 partials added in order) / (n - 1): thread t squares the columns t, t + 256, ... in order and
// the 256 sums meet in a fixed tree.  rowsum[row] = sum_j C_ij^2.  s_red: [PCA_THREADS] doubles of LDS.
PCA_WG void compare_frob_row_wg(const double *partial, int S, int d, int m, int n, int row, double *rowsum, double *s_red) {
  PCA_PAR(tid, PCA_THREADS) {
    double s = 0.0;
    for (int j = tid; j < m; j += PCA_THREADS) {
      const double c = wg_sum(partial + (int64_t)row * m + j, S, (int64_t)d * m) / (double)(n - 1);
      s = fma(c, c, s);
    }
    s_red[tid] = s;
  }
  PCA_SYNC();
  wg_tree<1>(s_red);
  PCA_PAR(tid, PCA_THREADS) {
    if (tid == 0) rowsum[row] = s_red[0];
  }
}

// `count` values in index order
TM_DEV double compare_total(const double *v, int count) { return wg_sum(v, count, 1); }

// element e of C [d][m] in float64: the super-chunks' partials added in order, over n - 1
TM_DEV double compare_cross_reduce(const double *partial, int S, int d, int m, int n, int64_t e) { return wg_sum(partial + e, S, (int64_t)d * m) / (double)(n - 1); }

// ----------------------------------------------------------------------------------------------- the rows of a dissimilarity
// One feature set of the all-pairs pass.  A value is staged as ((x - mean) - shift) scale, three single float32 operations.  Metrics 0 and 1:
// shift 0, scale 1.  Metric 2: shift = the mean of the row's column-centred values across the features, scale = 1 / their centred norm (float64
// sums in feature order, rounded once): the correlation distance of two rows is then half the squared distance of their staged forms; a row
// whose centred norm is 0 has scale 0 and ok 0.  Metric 3 (labels) stages the column as it is: mean is not read.
struct CompareSide {
  const float *x;
  int64_t ld;
  int d, metric;
  const float *mean, *shift, *scale;
  const int32_t *ok;
};

TM_DEV void compare_rowstat(const float *x, int64_t ldx, const float *mean, int d, int metric, int64_t row, float *shift, float *scale, int32_t *ok) {
  float sh = 0.f, sc = 1.f;
  int good = 1;
  if (metric == COMPARE_CORRELATION) {
    double s = 0.0;
    for (int c = 0; c < d; c++) s += (double)(x[row * ldx + c] - mean[c]);
    sh = (float)(s / (double)d);
    double q = 0.0;
    for (int c = 0; c < d; c++) {
      const double v = (double)((x[row * ldx + c] - mean[c]) - sh);
      q = fma(v, v, q);
    }
    good = q > 0.0 ? 1 : 0;
    sc = good ? (float)(1.0 / sqrt(q)) : 0.f;
  }
  shift[row] = sh;
  scale[row] = sc;
  ok[row] = good;
}

TM_DEV float compare_staged(const CompareSide &sd, int64_t row, int c) {
  const float v = sd.x[row * sd.ld + c];
  if (sd.metric == COMPARE_LABEL) return v;
  return ((v - sd.mean[c]) - sd.shift[row]) * sd.scale[row];
}

// One side of the pair tile (i0, j0): acc[u * 4 + v] = the sum over the features, in ascending order, of (a_f - b_f)^2 for the staged rows
// i = i0 + 8 ty + u and j = j0 + 4 tx + v of thread (ty, tx): one subtraction and one fmaf a term.  Rows at or behind n are staged as zeros.
// acc: a PCA_PRIVATE array of 32 floats a thread.  s_i: [COMPARE_TK][COMPARE_LDI], s_j: [COMPARE_TK][COMPARE_LDJ] floats of LDS.
PCA_WG void compare_side_wg(const CompareSide &sd, int n, int i0, int j0, float *s_i, float *s_j, float *acc) {
  PCA_PAR(tid, PCA_THREADS) {
    float *mine = acc + COMPARE_SLOT(tid) * 32;
#pragma unroll
    for (int e = 0; e < 32; e++) mine[e] = 0.f;
  }
  for (int k0 = 0; k0 < sd.d; k0 += COMPARE_TK) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < COMPARE_ROWS * COMPARE_TK; e += PCA_THREADS) {
        const int row = e / COMPARE_TK, f = e % COMPARE_TK;
        s_i[f * COMPARE_LDI + row] = (i0 + row < n && k0 + f < sd.d) ? compare_staged(sd, i0 + row, k0 + f) : 0.f;
      }
      for (int e = tid; e < COMPARE_TILE * COMPARE_TK; e += PCA_THREADS) {
        const int row = e / COMPARE_TK, f = e % COMPARE_TK;
        s_j[f * COMPARE_LDJ + row] = (j0 + row < n && k0 + f < sd.d) ? compare_staged(sd, j0 + row, k0 + f) : 0.f;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
      float *mine = acc + COMPARE_SLOT(tid) * 32;
#pragma unroll 4
      for (int f = 0; f < COMPARE_TK; f++) {
        const cmp_f4 a0 = *(const cmp_f4 *)(s_i + f * COMPARE_LDI + 8 * ty), a1 = *(const cmp_f4 *)(s_i + f * COMPARE_LDI + 8 * ty + 4);
        const cmp_f4 b = *(const cmp_f4 *)(s_j + f * COMPARE_LDJ + 4 * tx);
#pragma unroll
        for (int u = 0; u < 8; u++)
#pragma unroll
          for (int v = 0; v < 4; v++) {
            const float df = (u < 4 ? a0[u] : a1[u - 4]) - b[v];
            mine[u * 4 + v] = fmaf(df, df, mine[u * 4 + v]);
          }
      }
    }
    PCA_SYNC();
  }
}

// the dissimilarity of a pair from its float32 chain s, in float64
TM_DEV double compare_dissimilarity(int metric, float s, int ok_i, int ok_j) {
  const double v = (double)s;
  if (metric == COMPARE_SQEUCLIDEAN) return v;
  if (metric == COMPARE_EUCLIDEAN) return sqrt(v);
  if (metric == COMPARE_CORRELATION) return ok_i && ok_j ? 0.5 * v : 1.0;
  return s != 0.f ? 1.0 : 0.0;
}

// Pair tile (ib, jt): the rows i of [128 ib, 128 ib + 128) against the rows j of [64 jt, 64 jt + 64), the pairs i < j < n only; a tile without
// one writes zeros.  First the x side, then the y side through the same stage; thread (ty, tx) then adds its 32 pairs in (u, v) order into five
// float64 sums  Dx, Dy, Dx^2, Dy^2, Dx Dy  (each product one fma), and the 256 threads' sums meet in a fixed tree in the room of the stage.
// parts: [tiles of i][tiles of j][5] float64.  s_stage: [COMPARE_STAGE] floats of LDS, 16-byte aligned.
PCA_WG void compare_pairs_wg(const CompareSide &sx, const CompareSide &sy, int n, int ib, int jt, int ntj, double *parts, float *s_stage) {
  double *out = parts + ((int64_t)ib * ntj + jt) * 5;
  const int i0 = ib * COMPARE_ROWS, j0 = jt * COMPARE_TILE;
  if (j0 + COMPARE_TILE - 1 <= i0) {      // (uniform over the workgroup, in front of every barrier)
    PCA_PAR(tid, PCA_THREADS) {
      if (tid < 5) out[tid] = 0.0;
    }
    return;
  }
  float *s_i = s_stage, *s_j = s_stage + COMPARE_TK * COMPARE_LDI;
  double *s_red = (double *)s_stage;
  PCA_PRIVATE(float, ax, 32);
  PCA_PRIVATE(float, ay, 32);
  compare_side_wg(sx, n, i0, j0, s_i, s_j, PCA_MINE(ax, 0));
  compare_side_wg(sy, n, i0, j0, s_i, s_j, PCA_MINE(ay, 0));
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int i = i0 + 8 * ty + u, j = j0 + 4 * tx + v;
        if (i < j && j < n) {
          const double dx = compare_dissimilarity(sx.metric, PCA_MINE(ax, tid)[u * 4 + v], sx.ok[i], sx.ok[j]);
          const double dy = compare_dissimilarity(sy.metric, PCA_MINE(ay, tid)[u * 4 + v], sy.ok[i], sy.ok[j]);
          s0 += dx;
          s1 += dy;
          s2 = fma(dx, dx, s2);
          s3 = fma(dy, dy, s3);
          s4 = fma(dx, dy, s4);
        }
      }
    s_red[0 * PCA_THREADS + tid] = s0;
    s_red[1 * PCA_THREADS + tid] = s1;
    s_red[2 * PCA_THREADS + tid] = s2;
    s_red[3 * PCA_THREADS + tid] = s3;
    s_red[4 * PCA_THREADS + tid] = s4;
  }
  PCA_SYNC();
  wg_tree<5>(s_red);
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < 5) out[tid] = s_red[tid * PCA_THREADS];
  }
}

// the five sums of every tile: thread t adds the tiles t, t + 256, ... in order, the 256 sums meet in a fixed tree.  s_red: [5][256] doubles of LDS.
PCA_WG void compare_pairs_total_wg(const double *parts, int64_t tiles, double *sums, double *s_red) {
  PCA_PAR(tid, PCA_THREADS) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t t = tid; t < tiles; t += PCA_THREADS)
#pragma unroll
      for (int k = 0; k < 5; k++) s[k] += parts[t * 5 + k];
#pragma unroll
    for (int k = 0; k < 5; k++) s_red[k * PCA_THREADS + tid] = s[k];
  }
  PCA_SYNC();
  wg_tree<5>(s_red);
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < 5) sums[tid] = s_red[tid * PCA_THREADS];
  }
}

// ----------------------------------------------------------------------------------------------- the small float64 products of the CCA
// element e of the rows of q [k][k] scaled for the whitening: q[i][:] / sqrt(sigma[i]); a sigma that is not positive gives zeros
TM_DEV double compare_inv_sqrt_row(const double *q, const double *sigma, int k, int e) {
  const double s = sigma[e / k];
  return s > 0.0 ? q[e] / sqrt(s) : 0.0;
}

// sum_k a[i][k] B(k, j) in ascending k, one fma a term: B(k, j) = b[k][j], or b[j][k] with TB
template <bool TB>
TM_DEV double compare_dot(const double *a, int64_t lda, const double *b, int64_t ldb, int K, int i, int j) {
  double s = 0.0;
  for (int k = 0; k < K; k++) s = fma(a[(int64_t)i * lda + k], TB ? b[(int64_t)j * ldb + k] : b[(int64_t)k * ldb + j], s);
  return s;
}

// ----------------------------------------------------------------------------------------------- the singular value decomposition
// doubles of LDS of compare_svd_wg for a [ra][ca] matrix: the image G [nn][mm + 1], the quads' partial sums, the norms, the order, the flag
PCA_HD int compare_svd_lds_doubles(int ra, int ca) {
  const int mm = ra > ca ? ra : ca, nn = ra > ca ? ca : ra;
  return nn * (mm + 1) + 3 * PCA_THREADS + 2 * nn + 2;
}

// One workgroup of 256 threads: a [ra][ca] (row stride lda) = U diag(sigma) V^T by one-sided (Hestenes) Jacobi.  G = a, or a^T when ra < ca, so
// that G is [mm][nn] with mm >= nn; it lives in LDS column by column in float64, W = I [nn][nn] beside it in `work` (global, this workgroup's
// alone).  A sweep is the nn - 1 rounds of the round-robin tournament (pca_pair); the pairs of a round are disjoint and rotate side by side, four
// threads a pair: each adds alpha = g_p . g_p, beta = g_q . g_q, gamma = g_p . g_q over its rows t, t + 4, ..., the four parts are added in order,
// and where |gamma| > 2^-40 sqrt(alpha beta) the columns p, q of G and of W are turned by the angle that makes them orthogonal.  A sweep that
// turns nothing ends the iteration; COMPARE_SVD_SWEEPS sweeps without one leave info[1] = 0.  Then sigma_j = ||g_j||, sorted descending (ties
// in column order); the normalised columns of G (zeros where sigma_j = 0) are the singular vectors of the longer side, the columns of W those of
// the shorter.  sigma [nn], u [nn][ra], v [nn][ca] (rows: the vectors), info = {sweeps, converged}.
PCA_WG void compare_svd_wg(const double *a, int ra, int ca, int64_t lda, double *sigma, double *u, double *v, int32_t *info, double *work, double *lds) {
  const bool tr = ra < ca;
  const int mm = tr ? ca : ra, nn = tr ? ra : ca, ldg = mm + 1;
  const int players = (nn + 1) & ~1, rounds = players - 1, pairs = players / 2;
  double *g = lds, *s_part = g + nn * ldg, *s_sig = s_part + 3 * PCA_THREADS;
  int32_t *s_order = (int32_t *)(s_sig + nn), *s_flag = (int32_t *)(s_sig + 2 * nn);
  PCA_PAR(tid, PCA_THREADS) {
    for (int e = tid; e < mm * nn; e += PCA_THREADS) {
      const int row = e / nn, col = e % nn;
      g[col * ldg + row] = tr ? a[(int64_t)col * lda + row] : a[(int64_t)row * lda + col];
    }
    for (int e = tid; e < nn * nn; e += PCA_THREADS) work[e] = e / nn == e % nn ? 1.0 : 0.0;
  }
  PCA_SYNC();
  int sweeps = 0, converged = 0;
  while (sweeps < COMPARE_SVD_SWEEPS) {
    PCA_PAR(tid, PCA_THREADS) {
      if (tid == 0) s_flag[0] = 0;
    }
    PCA_SYNC();
    for (int r = 0; r < rounds; r++) {
      PCA_PAR(tid, PCA_THREADS) {
        const int k = tid / COMPARE_SVD_QUAD, t = tid % COMPARE_SVD_QUAD;
        double al = 0.0, be = 0.0, ga = 0.0;
        if (k < pairs) {
          int p, q;
          pca_pair(players, r, k, p, q);
          if (q < nn) {
            const double *gp = g + p * ldg, *gq = g + q * ldg;
            for (int row = t; row < mm; row += COMPARE_SVD_QUAD) {
              al = fma(gp[row], gp[row], al);
              be = fma(gq[row], gq[row], be);
              ga = fma(gp[row], gq[row], ga);
            }
          }
        }
        s_part[3 * tid] = al; s_part[3 * tid + 1] = be; s_part[3 * tid + 2] = ga;
      }
      PCA_SYNC();
      PCA_PAR(tid, PCA_THREADS) {
        const int k = tid / COMPARE_SVD_QUAD, t = tid % COMPARE_SVD_QUAD;
        int p = 0, q = nn;
        if (k < pairs) pca_pair(players, r, k, p, q);
        if (q < nn) {
          double al = 0.0, be = 0.0, ga = 0.0;
          for (int z = 0; z < COMPARE_SVD_QUAD; z++) {
            const double *part = s_part + 3 * (k * COMPARE_SVD_QUAD + z);
            al += part[0]; be += part[1]; ga += part[2];
          }
          if (fabs(ga) > COMPARE_SVD_TOL * sqrt(al * be)) {
            s_flag[0] = 1;      // (every writer stores the same value)
            const double zeta = (be - al) / (2.0 * ga);
            const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
            double *gp = g + p * ldg, *gq = g + q * ldg, *wp = work + (int64_t)p * nn, *wq = work + (int64_t)q * nn;
            for (int row = t; row < mm; row += COMPARE_SVD_QUAD) {
              const double x0 = gp[row], x1 = gq[row];
              gp[row] = cs * x0 - sn * x1;
              gq[row] = sn * x0 + cs * x1;
            }
            for (int row = t; row < nn; row += COMPARE_SVD_QUAD) {
              const double x0 = wp[row], x1 = wq[row];
              wp[row] = cs * x0 - sn * x1;
              wq[row] = sn * x0 + cs * x1;
            }
          }
        }
      }
      PCA_SYNC();
    }
    sweeps++;
    const int rotated = s_flag[0];
    PCA_SYNC();
    if (!rotated) { converged = 1; break; }
  }
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < nn) {
      double s = 0.0;
      for (int row = 0; row < mm; row++) s = fma(g[tid * ldg + row], g[tid * ldg + row], s);
      s_sig[tid] = sqrt(s);
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < nn) {      // the position of column tid: the columns before it by (sigma descending, index ascending)
      int rank = 0;
      for (int j = 0; j < nn; j++) rank += (s_sig[j] > s_sig[tid] || (s_sig[j] == s_sig[tid] && j < tid)) ? 1 : 0;
      s_order[rank] = tid;
    }
  }
  PCA_SYNC();
  double *longer = tr ? v : u, *shorter = tr ? u : v;      // [nn][mm] and [nn][nn]
  PCA_PAR(tid, PCA_THREADS) {
    for (int e = tid; e < nn * mm; e += PCA_THREADS) {
      const int rk = e / mm, row = e % mm, col = s_order[rk];
      longer[e] = s_sig[col] > 0.0 ? g[col * ldg + row] / s_sig[col] : 0.0;
    }
    for (int e = tid; e < nn * nn; e += PCA_THREADS) shorter[e] = work[(int64_t)s_order[e / nn] * nn + e % nn];
    if (tid < nn) sigma[tid] = s_sig[s_order[tid]];
    if (tid == 0) { info[0] = sweeps; info[1] = converged; }
  }
}
