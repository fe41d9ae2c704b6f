// csrc/moments_core.h — what the analyses share about column moments (DESIGN.md "PCA", moments): the fixed row splits, the float64 column sums and
// the means they give, the chunked product behind every covariance and cross moment, and the one pair of kernels that forms a column mean.
// Written with the discipline of csrc/wg_core.h, so that the bodies also compile on the host.  Every product is a chain of float32 FMAs in a
// fixed order; every sum across rows, chunks or workgroups is float64 in a fixed order: no atomics, the same bits on every run and on every grid.
#pragma once
#include "wg_core.h"

#define PCA_KB 16                // rows of x staged in LDS per barrier pair of a moment tile
#define PCA_WIDE_TILE 128        // columns of a column-sum workgroup, and the side of a Gram output tile
#define PCA_WIDE_MAX_SUPER 16    // row super-chunks of the moment passes: the partials are [S][d][d] float64, whatever n is
#define KMEANS_MIN_PART 32       // row parts of the k-means update: the partial sums [P][k][d] float64 take at most 64 MB (2^23 doubles) or, where k d is
#define KMEANS_PART_DOUBLES (1 << 23)      // large, 32 parts, whatever n is

// the fixed row split of the moment passes: chunks of PCA_ROWS_PER_WG rows, `per` consecutive chunks to a super-chunk, S <= 16 super-chunks.
// It depends on n only.
struct PcaWideSplit { int nchunks, per, S; };
PCA_HD PcaWideSplit pca_wide_split(int n) {
  PcaWideSplit s;
  s.nchunks = pca_nwg(n);
  s.per = (s.nchunks + PCA_WIDE_MAX_SUPER - 1) / PCA_WIDE_MAX_SUPER;
  s.S = (s.nchunks + s.per - 1) / s.per;
  return s;
}
PCA_HD int pca_wide_tiles(int d) { return (d + PCA_WIDE_TILE - 1) / PCA_WIDE_TILE; }

// the fixed row split of the k-means update: chunks of 256 rows, `per` consecutive chunks to a part, at most max(32, 2^23 / (k d)) parts.  It
// depends on n, k and d only.
struct KmeansSplit { int nchunks, per, P; };
PCA_HD KmeansSplit kmeans_split(int n, int k, int d) {
  KmeansSplit s;
  int cap = KMEANS_PART_DOUBLES / (k * d);
  if (cap < KMEANS_MIN_PART) cap = KMEANS_MIN_PART;
  s.nchunks = pca_nwg(n);
  s.per = (s.nchunks + cap - 1) / cap;
  s.P = (s.nchunks + s.per - 1) / s.per;
  return s;
}

// the rows of a group that starts at row0 and spans `span` rows of the n
PCA_HD int moments_rows(int n, int64_t row0, int64_t span) { return (int)(n - row0 < span ? n - row0 : span); }

// ----------------------------------------------------------------------------------------------- column sums
// The float64 column sums of the rows [row0, row0 + rows) over the columns [128 cb, 128 cb + 128).  Thread (h, c) = (tid / 128, tid % 128) adds the
// rows of parity h (counted from row0) of its column in row order; the two halves are added in a fixed order.  The caller chooses the rows: one
// chunk, one super-chunk, or one workgroup's.  out_row: [d], this group's row of the partials.  s_sum: [2][128] doubles of LDS.
// SQUARES: the term of a value is (x - mean)^2, the centred sum of squares, with the column mean in float64: colsum's partials [S][d] added in
// order, over n.
template <bool SQUARES = false>
PCA_WG void moments_colsum_wg(const float *x, int64_t ldx, int64_t row0, int rows, int d, int cb, double *out_row, double *s_sum, const double *colsum = nullptr,
                              int S = 0, int n = 0) {
  PCA_PAR(tid, PCA_THREADS) {
    const int c = cb * PCA_WIDE_TILE + (tid & (PCA_WIDE_TILE - 1)), h = tid / PCA_WIDE_TILE;
    if (c < d) {
      const double mean = SQUARES ? wg_sum(colsum + c, S, d) / (double)n : 0.0;
      double sum = 0.0;
#pragma unroll 8
      for (int r = h; r < rows; r += 2) {
        const double v = (double)x[(row0 + r) * ldx + c];
        if (SQUARES) {
          const double e = v - mean;
          sum += e * e;
        } else {
          sum += v;
        }
      }
      s_sum[h * PCA_WIDE_TILE + (tid & (PCA_WIDE_TILE - 1))] = sum;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    const int c = cb * PCA_WIDE_TILE + tid;
    if (tid < PCA_WIDE_TILE && c < d) out_row[c] = s_sum[tid] + s_sum[PCA_WIDE_TILE + tid];
  }
}

// the two groupings of the rows: chunk `chunk` of 256 rows (partial: [chunks][d]), and super-chunk s of pca_wide_split(n) (partial: [S][d])
PCA_WG void kmeans_colsum_wg(const float *x, int64_t ldx, int n, int d, int chunk, int cb, double *partial, double *s_sum) {
  const int64_t row0 = (int64_t)chunk * PCA_ROWS_PER_WG;
  moments_colsum_wg(x, ldx, row0, moments_rows(n, row0, PCA_ROWS_PER_WG), d, cb, partial + (int64_t)chunk * d, s_sum);
}
template <bool SQUARES = false>
PCA_WG void pca_wide_colsum_wg(const float *x, int64_t ldx, int n, int d, int s, int cb, double *partial, double *s_sum, const double *colsum = nullptr) {
  const PcaWideSplit sp = pca_wide_split(n);
  const int64_t span = (int64_t)sp.per * PCA_ROWS_PER_WG, row0 = s * span;
  moments_colsum_wg<SQUARES>(x, ldx, row0, moments_rows(n, row0, span), d, cb, partial + (int64_t)s * d, s_sum, colsum, sp.S, n);
}

// the mean of column c: the groups' sums (chunks, super-chunks or workgroups) added in group order, in float64
TM_DEV float moments_mean_col(const double *partial, int groups, int d, int n, int c) { return (float)(wg_sum(partial + c, groups, d) / (double)n); }
TM_DEV float pca_wide_mean_col(const double *partial, int S, int d, int n, int c) { return moments_mean_col(partial, S, d, n, c); }
TM_DEV float kmeans_mean_col(const double *partial, int nchunks, int d, int n, int c) { return moments_mean_col(partial, nchunks, d, n, c); }

// ----------------------------------------------------------------------------------------------- the moment tile
// PCA_KB staged rows of a tile: thread (ty, tx) of the 16 x 16 grid reads its NU values ty + 16 u of every row of s_a and its NV values tx + 16 v
// of s_b (the 16 lanes of a row read 16 consecutive floats, the four ty of a wave broadcast) and adds the NU x NV products, one fmaf each, in
// ascending row order.
template <int NU, int NV>
TM_DEV void moments_fma_rows(const float *s_a, int lda, const float *s_b, int ldb, int ty, int tx, float *mine) {
#pragma unroll 4
  for (int k = 0; k < PCA_KB; k++) {
    float a[NU], b[NV];
#pragma unroll
    for (int u = 0; u < NU; u++) a[u] = s_a[k * lda + ty + 16 * u];
#pragma unroll
    for (int v = 0; v < NV; v++) b[v] = s_b[k * ldb + tx + 16 * v];
#pragma unroll
    for (int u = 0; u < NU; u++)
#pragma unroll
      for (int v = 0; v < NV; v++) mine[u * NV + v] = fmaf(a[u], b[v], mine[u * NV + v]);
  }
}

// The tile of (a - mean_a)^T (b - mean_b) over the chunks [chunk0, chunk1) of 256 rows: the columns [ci0, ci0 + 16 NU) of a [n][da] against the
// columns [cj0, cj0 + 16 NV) of b [n][db], both centred as they are staged, edge tiles masked.  Within a chunk the products are float32 FMAs in
// ascending row order; after each chunk the thread adds its NU x NV float32 sums into float64 accumulators, in chunk order.  Thread (ty, tx)
// owns the elements (ci0 + ty + 16 u, cj0 + tx + 16 v): with b == a and cj0 == ci0, (i, j) and (j, i) see the same products in the same order
// and the tile is symmetric to the bit.  out: [da][ld_out] float64 of this group of chunks.  s_a: [PCA_KB][16 NU], s_b: [PCA_KB][16 NV] floats of
// LDS.
template <int NU, int NV>
PCA_WG void moments_tile_wg(const float *a, int64_t lda, const float *mean_a, int da, int ci0, const float *b, int64_t ldb, const float *mean_b, int db, int cj0,
                            int n, int chunk0, int chunk1, double *out, int64_t ld_out, float *s_a, float *s_b) {
  constexpr int WA = 16 * NU, WB = 16 * NV;
  PCA_PRIVATE(float, acc, NU * NV);
  PCA_PRIVATE(double, sum, NU * NV);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < NU * NV; e++) PCA_MINE(sum, tid)[e] = 0.0;
  }
  for (int chunk = chunk0; chunk < chunk1; chunk++) {
    const int64_t row0 = (int64_t)chunk * PCA_ROWS_PER_WG;
    const int rows = moments_rows(n, row0, PCA_ROWS_PER_WG);
    PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
      for (int e = 0; e < NU * NV; e++) PCA_MINE(acc, tid)[e] = 0.f;
    }
    for (int kb = 0; kb < rows; kb += PCA_KB) {
      PCA_PAR(tid, PCA_THREADS) {
        for (int e = tid; e < PCA_KB * WA; e += PCA_THREADS) {
          const int r = e / WA, c = e % WA;
          s_a[r * WA + c] = (kb + r < rows && ci0 + c < da) ? a[(row0 + kb + r) * lda + ci0 + c] - mean_a[ci0 + c] : 0.f;
        }
        for (int e = tid; e < PCA_KB * WB; e += PCA_THREADS) {
          const int r = e / WB, c = e % WB;
          s_b[r * WB + c] = (kb + r < rows && cj0 + c < db) ? b[(row0 + kb + r) * ldb + cj0 + c] - mean_b[cj0 + c] : 0.f;
        }
      }
      PCA_SYNC();
      PCA_PAR(tid, PCA_THREADS) { moments_fma_rows<NU, NV>(s_a, WA, s_b, WB, tid >> 4, tid & 15, PCA_MINE(acc, tid)); }
      PCA_SYNC();
    }
    PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
      for (int e = 0; e < NU * NV; e++) PCA_MINE(sum, tid)[e] += (double)PCA_MINE(acc, tid)[e];
    }
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int u = 0; u < NU; u++)
#pragma unroll
      for (int v = 0; v < NV; v++) {
        const int i = ci0 + ty + 16 * u, j = cj0 + tx + 16 * v;
        if (i < da && j < db) out[(int64_t)i * ld_out + j] = PCA_MINE(sum, tid)[u * NV + v];
      }
  }
}

// ----------------------------------------------------------------------------------------------- the column mean of a call
#if defined(__HIPCC__) && !defined(TM_HOST_EMU)
// One workgroup per (group of rows, 128 columns); partial: [groups][d].  CHUNKS: a group is one chunk of 256 rows and blockIdx.x, the columns
// blockIdx.y (k-means, HMM, t-SNE and the narrow PCA); else a group is a super-chunk of pca_wide_split(n) and blockIdx.y, the columns blockIdx.x.
template <bool CHUNKS>
static __global__ __launch_bounds__(PCA_THREADS) void k_moments_colsum(const float *__restrict__ x, int64_t ldx, int n, int d, double *__restrict__ partial) {
  __shared__ double s_sum[2 * PCA_WIDE_TILE];
  if (CHUNKS) kmeans_colsum_wg(x, ldx, n, d, blockIdx.x, blockIdx.y, partial, s_sum);
  else pca_wide_colsum_wg(x, ldx, n, d, blockIdx.y, blockIdx.x, partial, s_sum);
}

static __global__ __launch_bounds__(PCA_THREADS) void k_moments_mean(const double *__restrict__ partial, int groups, int d, int n, float *__restrict__ mean) {
  const int c = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (c < d) mean[c] = moments_mean_col(partial, groups, d, n, c);
}

// the column sums of x [n][d] into colsum [groups][d] and, where `mean` is given, the column mean from them
template <bool CHUNKS>
static inline void moments_launch_mean(const float *x, int64_t ldx, int n, int d, double *colsum, float *mean, hipStream_t s) {
  const int tiles = pca_wide_tiles(d), groups = CHUNKS ? pca_nwg(n) : pca_wide_split(n).S;
  hipLaunchKernelGGL(k_moments_colsum<CHUNKS>, CHUNKS ? dim3(groups, tiles) : dim3(tiles, groups), dim3(PCA_THREADS), 0, s, x, ldx, n, d, colsum);
  if (mean) hipLaunchKernelGGL(k_moments_mean, dim3((d + PCA_THREADS - 1) / PCA_THREADS), dim3(PCA_THREADS), 0, s, colsum, groups, d, n, mean);
}
#endif
