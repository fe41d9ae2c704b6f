// csrc/pca_wide_core.h — the bodies of the wide PCA kernels, 129 <= d <= 1024 (DESIGN.md "PCA", wide fit; include/tmjx.h: tmjx_pca_*_wide).
// Written with the PCA_WG / PCA_PAR / PCA_SYNC / PCA_PRIVATE discipline of csrc/wg_core.h, so that they also compile on the host
// (tests/hostemu/pca_wide_emu.cpp); the moments are csrc/moments_core.h, the inner solver csrc/pca_core.h.  The covariance and V^T live in
// global memory; the eigen-decomposition is block Jacobi: the columns are cut into blocks of PCA_WIDE_BLOCK, the blocks are paired by the
// round-robin tournament of pca_pair, and the (at most 128 x 128) sub-matrix of a pair is diagonalised by pca_jacobi_wg, whose sorted unit eigenvector rows J rotate the pair's rows (J A, J V^T) and then its columns (A J^T).
#pragma once
#include "pca_core.h"

#define PCA_WIDE_MAX_D 1024
#define PCA_WIDE_BLOCK 64        // columns of a Jacobi block: a pair is PCA_MAX_D = 128 wide, the inner solver's limit
#define PCA_WIDE_PASS 64         // columns (row pass) or rows (column pass) of one workgroup of a rotation pass
#define PCA_WIDE_LDA 129         // row stride of the staged slice of J: 16 consecutive k of one row go to 16 different banks
#define PCA_WIDE_LDB 65          // row stride of the staged slice of A
#define PCA_WIDE_TK 64           // features staged per barrier pair of the transform kernel
#define PCA_WIDE_TLD 65          // row stride of that stage

PCA_HD int pca_wide_blocks(int d) { return (d + PCA_WIDE_BLOCK - 1) / PCA_WIDE_BLOCK; }
PCA_HD int pca_wide_players(int d) { return (pca_wide_blocks(d) + 1) & ~1; }      // with the empty "bye" block of an odd count

// ----------------------------------------------------------------------------------------------- moments
// Pass 1: the float64 column sums of every super-chunk of pca_wide_split(n) and the mean from them (moments_colsum_wg, moments_mean_col).
// Pass 2: output tile (ti, tj), tj >= ti, of (x - mean)^T (x - mean) over super-chunk s: moments_tile_wg<8, 8> with both sides taken from x.
// partial: [S][d][d] float64, of which only the tiles with tj >= ti are written.  s_tile: [2][PCA_KB][PCA_WIDE_TILE] floats of LDS.  In a diagonal
// tile (i, j) and (j, i) see the same products in the same order.
PCA_WG void pca_wide_gram_wg(const float *x, int64_t ldx, int n, int d, const float *mean, int ti, int tj, int s, double *partial, float *s_tile) {
  const PcaWideSplit sp = pca_wide_split(n);
  const int chunk0 = s * sp.per, chunk1 = chunk0 + sp.per < sp.nchunks ? chunk0 + sp.per : sp.nchunks;
  moments_tile_wg<8, 8>(x, ldx, mean, d, ti * PCA_WIDE_TILE, x, ldx, mean, d, tj * PCA_WIDE_TILE, n, chunk0, chunk1, partial + (int64_t)s * d * d, d, s_tile,
                        s_tile + PCA_KB * PCA_WIDE_TILE);
}

// element (i, j) of the covariance: the super-chunks' partials added in order, in float64, over n - 1; below the diagonal tiles the mirror image
TM_DEV float pca_wide_gram_reduce(const double *partial, int S, int d, int n, int i, int j) {
  const bool up = i / PCA_WIDE_TILE <= j / PCA_WIDE_TILE;
  return (float)(wg_sum(partial + (up ? (int64_t)i * d + j : (int64_t)j * d + i), S, (int64_t)d * d) / (double)(n - 1));
}

// ----------------------------------------------------------------------------------------------- norms
// ||row||^2 and its off-diagonal part in float64: every thread sums the elements 256 apart, the threads are added as a binary tree.
// rowsum: [2][d].  s_red: [2][PCA_THREADS] doubles of LDS.
PCA_WG void pca_wide_rownorm_wg(const float *A, int d, int row, double *rowsum, double *s_red) {
  PCA_PAR(tid, PCA_THREADS) {
    double s = 0.0, o = 0.0;
    for (int j = tid; j < d; j += PCA_THREADS) {
      const double v = (double)A[(int64_t)row * d + j];
      s += v * v;
      if (j != row) o += v * v;
    }
    s_red[tid] = s; s_red[PCA_THREADS + tid] = o;
  }
  PCA_SYNC();
  wg_tree<2>(s_red);
  PCA_PAR(tid, PCA_THREADS) {
    if (tid == 0) { rowsum[row] = s_red[0]; rowsum[d + row] = s_red[PCA_THREADS]; }
  }
}

// which = 0: ||A||_F^2, which = 1: off(A)^2 — the rows' sums added in row order
TM_DEV double pca_wide_norm_total(const double *rowsum, int d, int which) { return wg_sum(rowsum + which * d, d, 1); }

// ----------------------------------------------------------------------------------------------- block Jacobi
// pair k of round r: the blocks p < q as column ranges [p0, p0 + sp) and [q0, q0 + sq); m = sp + sq <= 128 is the sub-matrix's size, 0 when q is
// the bye (the pair rests).  Local index i of the sub-matrix is column p0 + i for i < sp, else q0 + i - sp.
struct PcaWidePair { int p0, sp, q0, sq, m; };
TM_DEV PcaWidePair pca_wide_pair(int d, int r, int k) {
  const int nb = pca_wide_blocks(d);
  int p, q;
  pca_pair(pca_wide_players(d), r, k, p, q);
  PcaWidePair pr = {0, 0, 0, 0, 0};
  if (q >= nb) return pr;
  pr.p0 = p * PCA_WIDE_BLOCK; pr.q0 = q * PCA_WIDE_BLOCK;
  pr.sp = d - pr.p0 < PCA_WIDE_BLOCK ? d - pr.p0 : PCA_WIDE_BLOCK;
  pr.sq = d - pr.q0 < PCA_WIDE_BLOCK ? d - pr.q0 : PCA_WIDE_BLOCK;
  pr.m = pr.sp + pr.sq;
  return pr;
}
TM_DEV int pca_wide_global(const PcaWidePair &pr, int i) { return i < pr.sp ? pr.p0 + i : pr.q0 + i - pr.sp; }
TM_DEV int pca_wide_local(const PcaWidePair &pr, int g) {      // -1: column g is not of this pair
  if (g >= pr.p0 && g < pr.p0 + pr.sp) return g - pr.p0;
  if (g >= pr.q0 && g < pr.q0 + pr.sq) return pr.sp + g - pr.q0;
  return -1;
}

// One workgroup of nt threads: gathers the sub-matrix of pair k (its upper triangle mirrored, so that the inner solver sees an exactly symmetric
// matrix) and solves it with pca_jacobi_wg.  sub, J: [pairs][128][128] (row stride m), lam: [pairs][128], info: [pairs].  J's rows are the unit
// eigenvectors by descending eigenvalue: block p takes the larger ones.
PCA_WG void pca_wide_solve_wg(const float *A, int d, int r, int k, float *sub, float *J, float *lam, PcaInfo *info, float *lds, int nt) {
  const PcaWidePair pr = pca_wide_pair(d, r, k);
  if (pr.m == 0) return;
  float *mine = sub + (int64_t)k * PCA_MAX_D * PCA_MAX_D;
  PCA_PAR(tid, nt) {
    for (int e = tid; e < pr.m * pr.m; e += nt) {
      const int i = e / pr.m, j = e % pr.m, gi = pca_wide_global(pr, i), gj = pca_wide_global(pr, j);
      mine[e] = i <= j ? A[(int64_t)gi * d + gj] : A[(int64_t)gj * d + gi];
    }
  }
  PCA_SYNC();      // (the workgroup reads back what it wrote itself)
  pca_jacobi_wg(mine, pr.m, J + (int64_t)k * PCA_MAX_D * PCA_MAX_D, lam + k * PCA_MAX_D, info + k, lds, nt);
}

// the PCA_KB columns [k0, k0 + 16) of J staged as s_a[kk][e] = J[e][k0 + kk] (0 beyond m)
PCA_WG void pca_wide_stage_rot(const float *J, int m, int k0, float *s_a) {
  PCA_PAR(tid, PCA_THREADS) {
    for (int e = tid; e < PCA_KB * PCA_MAX_D; e += PCA_THREADS) {
      const int kk = e % PCA_KB, row = e / PCA_KB;
      s_a[kk * PCA_WIDE_LDA + row] = (row < m && k0 + kk < m) ? J[row * m + k0 + kk] : 0.f;
    }
  }
}

// Row pass: X[g(e)][c] <- sum_i J[e][i] X[g(i)][c] for the pair's rows and the columns [c0, c0 + 64) — X is A, or V^T.  256 threads as 16 x 16:
// thread (ty, tx) owns the rows ty + 16 u and the columns tx + 16 v.  The workgroup reads its m x 64 slice completely before it writes it, and no
// other workgroup of the launch touches it.  s_a: [PCA_KB][PCA_WIDE_LDA], s_b: [PCA_KB][PCA_WIDE_LDB] floats of LDS.
PCA_WG void pca_wide_rows_wg(float *X, int d, int r, int k, const float *J, int c0, float *s_a, float *s_b) {
  const PcaWidePair pr = pca_wide_pair(d, r, k);
  if (pr.m == 0) return;
  const float *Jk = J + (int64_t)k * PCA_MAX_D * PCA_MAX_D;
  PCA_PRIVATE(float, acc, 32);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < 32; e++) PCA_MINE(acc, tid)[e] = 0.f;
  }
  for (int k0 = 0; k0 < pr.m; k0 += PCA_KB) {
    pca_wide_stage_rot(Jk, pr.m, k0, s_a);
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < PCA_KB * PCA_WIDE_PASS; e += PCA_THREADS) {
        const int kk = e / PCA_WIDE_PASS, c = e % PCA_WIDE_PASS;
        s_b[kk * PCA_WIDE_LDB + c] = (k0 + kk < pr.m && c0 + c < d) ? X[(int64_t)pca_wide_global(pr, k0 + kk) * d + c0 + c] : 0.f;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
      float *mine = PCA_MINE(acc, tid);
#pragma unroll 4
      for (int kk = 0; kk < PCA_KB; kk++) {
        float a[8], b[4];
#pragma unroll
        for (int u = 0; u < 8; u++) a[u] = s_a[kk * PCA_WIDE_LDA + ty + 16 * u];
#pragma unroll
        for (int v = 0; v < 4; v++) b[v] = s_b[kk * PCA_WIDE_LDB + tx + 16 * v];
#pragma unroll
        for (int u = 0; u < 8; u++)
#pragma unroll
          for (int v = 0; v < 4; v++) mine[u * 4 + v] = fmaf(a[u], b[v], mine[u * 4 + v]);
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int e = ty + 16 * u, c = c0 + tx + 16 * v;
        if (e < pr.m && c < d) X[(int64_t)pca_wide_global(pr, e) * d + c] = PCA_MINE(acc, tid)[u * 4 + v];
      }
  }
}

// Column pass: A[row][g(e)] <- sum_i A[row][g(i)] J[e][i] for the rows [r0, r0 + 64) and the pair's columns; thread (ty, tx) owns the columns
// tx + 16 u and the rows ty + 16 v.  Where the row is one of the pair's own, the element is the sub-matrix's: it is written as diag(lam), the
// annihilated block exactly 0.  lam: the inner solver's eigenvalues (clamped at 0, like the variances they become).
PCA_WG void pca_wide_cols_wg(float *A, int d, int r, int k, const float *J, const float *lam, int r0, float *s_a, float *s_b) {
  const PcaWidePair pr = pca_wide_pair(d, r, k);
  if (pr.m == 0) return;
  const float *Jk = J + (int64_t)k * PCA_MAX_D * PCA_MAX_D, *lk = lam + k * PCA_MAX_D;
  PCA_PRIVATE(float, acc, 32);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < 32; e++) PCA_MINE(acc, tid)[e] = 0.f;
  }
  for (int k0 = 0; k0 < pr.m; k0 += PCA_KB) {
    pca_wide_stage_rot(Jk, pr.m, k0, s_a);
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < PCA_KB * PCA_WIDE_PASS; e += PCA_THREADS) {
        const int kk = e % PCA_KB, row = e / PCA_KB;
        s_b[kk * PCA_WIDE_LDB + row] = (k0 + kk < pr.m && r0 + row < d) ? A[(int64_t)(r0 + row) * d + pca_wide_global(pr, k0 + kk)] : 0.f;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
      float *mine = PCA_MINE(acc, tid);
#pragma unroll 4
      for (int kk = 0; kk < PCA_KB; kk++) {
        float a[8], b[4];
#pragma unroll
        for (int u = 0; u < 8; u++) a[u] = s_a[kk * PCA_WIDE_LDA + tx + 16 * u];
#pragma unroll
        for (int v = 0; v < 4; v++) b[v] = s_b[kk * PCA_WIDE_LDB + ty + 16 * v];
#pragma unroll
        for (int u = 0; u < 8; u++)
#pragma unroll
          for (int v = 0; v < 4; v++) mine[u * 4 + v] = fmaf(b[v], a[u], mine[u * 4 + v]);
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int e = tx + 16 * u, row = r0 + ty + 16 * v;
        if (e < pr.m && row < d) {
          const int li = pca_wide_local(pr, row);
          A[(int64_t)row * d + pca_wide_global(pr, e)] = li < 0 ? PCA_MINE(acc, tid)[u * 4 + v] : (li == e ? lk[e] : 0.f);
        }
      }
  }
}

// Row i of the result, by the rule of pca_jacobi_wg: the eigenvalue clamped at 0 and ranked by descending value (the lower index first among
// equals), the row of V^T at unit norm with its largest-magnitude coefficient positive (the lowest index among equals).
TM_DEV void pca_wide_finish_row(const float *A, const float *Vt, int d, int i, float *components, float *variance) {
  const float di = A[(int64_t)i * d + i], li = di > 0.f ? di : 0.f;
  int rk = 0;
  for (int j = 0; j < d; j++) {
    const float dj = A[(int64_t)j * d + j], lj = dj > 0.f ? dj : 0.f;
    rk += (lj > li) || (lj == li && j < i);
  }
  double n2 = 0.0;
  float big = 0.f, sgn = 1.f;
  for (int j = 0; j < d; j++) {
    const float v = Vt[(int64_t)i * d + j];
    n2 += (double)v * (double)v;
    if (fabsf(v) > big) { big = fabsf(v); sgn = v < 0.f ? -1.f : 1.f; }
  }
  const float scale = n2 > 0.0 ? sgn / (float)sqrt(n2) : sgn;
  for (int j = 0; j < d; j++) components[(int64_t)rk * d + j] = Vt[(int64_t)i * d + j] * scale;
  variance[rk] = li;
}

// ----------------------------------------------------------------------------------------------- transform
// out[row][c] = (x[row] - mean) . components[c] for the rows [r0, r0 + 64) and the components [c0, c0 + 16 NC): one fmaf chain per output in
// ascending j, as pca_project does.  PCA_WIDE_TK features at a time are staged as s_x[j][row] and s_c[j][c] (row stride PCA_WIDE_TLD: the 64
// consecutive j a wave writes go to different banks); thread (ty, tx) owns the rows ty + 16 u and the components tx + 16 v.
template <int NC>
PCA_WG void pca_wide_transform_wg(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, float *out, int64_t ldo,
                                  int r0, int c0, float *s_x, float *s_c) {
  PCA_PRIVATE(float, acc, 4 * NC);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < 4 * NC; e++) PCA_MINE(acc, tid)[e] = 0.f;
  }
  for (int j0 = 0; j0 < d; j0 += PCA_WIDE_TK) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < PCA_TROWS * PCA_WIDE_TK; e += PCA_THREADS) {
        const int row = e / PCA_WIDE_TK, j = e % PCA_WIDE_TK;
        s_x[j * PCA_WIDE_TLD + row] = (r0 + row < n && j0 + j < d) ? x[(int64_t)(r0 + row) * ldx + j0 + j] - mean[j0 + j] : 0.f;
      }
      for (int e = tid; e < 16 * NC * PCA_WIDE_TK; e += PCA_THREADS) {
        const int c = e / PCA_WIDE_TK, j = e % PCA_WIDE_TK;
        s_c[j * PCA_WIDE_TLD + c] = (c0 + c < k && j0 + j < d) ? components[(int64_t)(c0 + c) * d + j0 + j] : 0.f;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15, jn = d - j0 < PCA_WIDE_TK ? d - j0 : PCA_WIDE_TK;
      float *mine = PCA_MINE(acc, tid);
      for (int j = 0; j < jn; j++) {
        float a[4], b[NC];
#pragma unroll
        for (int u = 0; u < 4; u++) a[u] = s_x[j * PCA_WIDE_TLD + ty + 16 * u];
#pragma unroll
        for (int v = 0; v < NC; v++) b[v] = s_c[j * PCA_WIDE_TLD + tx + 16 * v];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
          for (int v = 0; v < NC; v++) mine[u * NC + v] = fmaf(a[u], b[v], mine[u * NC + v]);
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int v = 0; v < NC; v++) {
        const int row = r0 + ty + 16 * u, c = c0 + tx + 16 * v;
        if (row < n && c < k) out[(int64_t)row * ldo + c] = PCA_MINE(acc, tid)[u * NC + v];
      }
  }
}
