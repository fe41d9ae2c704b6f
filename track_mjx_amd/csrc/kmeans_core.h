// csrc/kmeans_core.h — the bodies of the k-means kernels (DESIGN.md "Clustering"; include/tmjx.h: tmjx_kmeans_*): Lloyd's iteration with k-means++
// seeding on recorded activations x [n][d] against k centroids.  Written with the PCA_WG / PCA_PAR / PCA_SYNC / PCA_PRIVATE discipline of
// csrc/wg_core.h, so that they also compile on the host (tests/hostemu/kmeans_emu.cpp); the column mean and the row split are csrc/moments_core.h.  Every product is a chain of float32 FMAs in a fixed
// order; every sum across rows or workgroups is float64 in a fixed order: no floating-point atomics, the same bits on every run.
#pragma once
#include "moments_core.h"

#define KMEANS_MAX_D 1024
#define KMEANS_MAX_K 256
#define KMEANS_ROWS 128          // rows of x an assign workgroup owns
#define KMEANS_TILE 64           // centroids of one tile of its walk
#define KMEANS_TK 32             // features staged per barrier pair
#define KMEANS_LDX 132           // row stride of the staged rows  s_x[feature][row]: a multiple of 4, a thread reads its 8 rows as two 16-byte words
#define KMEANS_LDC 68            // row stride of the staged centroids  s_c[feature][centroid]: likewise its 4 centroids as one
#define KMEANS_UTILE 64          // columns of an update workgroup: its LDS image is [k][64] float64, 128 KB at k = 256
#define KMEANS_UTHREADS 256      // its threads: four waves, wave w owns the clusters j = w (mod 4)
#define KMEANS_SEED_ROWS 256     // rows of one workgroup of the seeding distance pass, and of one block of its prefix sum

PCA_HD int kmeans_tiles(int v, int tile) { return (v + tile - 1) / tile; }
PCA_HD float kmeans_inf() { return __builtin_inff(); }

typedef float km_f4 __attribute__((vector_size(16)));

// ----------------------------------------------------------------------------------------------- assign
// ||c_j - mean||^2 of centroid j: one fmaf chain over the features in ascending order, the centroid centred as the rows are
TM_DEV float kmeans_cnorm(const float *centroids, const float *mean, int d, int j) {
  float s = 0.f;
  for (int c = 0; c < d; c++) {
    const float v = centroids[(int64_t)j * d + c] - mean[c];
    s = fmaf(v, v, s);
  }
  return s;
}

// The fused pass for the rows [r0, r0 + 128): with xc = x - mean and cc_j = c_j - mean (float32), score_j = cnorm_j - 2 xc . cc_j, the dot product
// one fmaf chain per (row, centroid) in ascending feature order.  The workgroup walks the centroid tiles in order; thread (ty, tx) owns the rows
// 8 ty + u and, in a tile, the centroids 4 tx + v (16-byte reads of the stage), and keeps a running minimum per row (strictly smaller wins: ascending j, so the lowest index
// keeps a tie).  The 16 tx of a row are then compared in order (smaller score, then lower index).  dist2 = max(0, ||xc||^2 + score), ||xc||^2
// one fmaf chain per row gathered from the stage during the first tile.  The workgroup's float64 sum of its dist2 in row order goes to
// part_inertia[wg], its count of rows with labels_prev != label to part_changed[wg] (all its rows when labels_prev is NULL): no atomics at all.
// s_x: [KMEANS_TK][KMEANS_LDX], s_c: [KMEANS_TK][KMEANS_LDC], s_val: [128][16] floats; s_idx: [128][16] ints of LDS; s_val may be s_x and s_idx s_c
// (the epilogue starts behind the last barrier of the walk).
PCA_WG void kmeans_assign_wg(const float *x, int n, int d, int64_t ldx, const float *centroids, int k, const float *mean, const float *cnorm,
                             const int32_t *labels_prev, int32_t *labels, float *dist2, double *part_inertia, int32_t *part_changed, int wg, float *s_x,
                             float *s_c, float *s_val, int32_t *s_idx) {
  const int64_t r0 = (int64_t)wg * KMEANS_ROWS;
  PCA_PRIVATE(float, acc, 32);
  PCA_PRIVATE(float, best, 8);
  PCA_PRIVATE(int, arg, 8);
  PCA_PRIVATE(float, xn, 1);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int u = 0; u < 8; u++) { PCA_MINE(best, tid)[u] = kmeans_inf(); PCA_MINE(arg, tid)[u] = 0x7fffffff; }
    PCA_MINE(xn, tid)[0] = 0.f;
  }
  for (int c0 = 0; c0 < k; c0 += KMEANS_TILE) {
    PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
      for (int e = 0; e < 32; e++) PCA_MINE(acc, tid)[e] = 0.f;
    }
    for (int k0 = 0; k0 < d; k0 += KMEANS_TK) {
      PCA_PAR(tid, PCA_THREADS) {
        for (int e = tid; e < KMEANS_ROWS * KMEANS_TK; e += PCA_THREADS) {
          const int row = e / KMEANS_TK, f = e % KMEANS_TK;
          s_x[f * KMEANS_LDX + row] = (r0 + row < n && k0 + f < d) ? x[(r0 + row) * ldx + k0 + f] - mean[k0 + f] : 0.f;
        }
        for (int e = tid; e < KMEANS_TILE * KMEANS_TK; e += PCA_THREADS) {
          const int j = e / KMEANS_TK, f = e % KMEANS_TK;
          s_c[f * KMEANS_LDC + j] = (c0 + j < k && k0 + f < d) ? centroids[(int64_t)(c0 + j) * d + k0 + f] - mean[k0 + f] : 0.f;
        }
      }
      PCA_SYNC();
      PCA_PAR(tid, PCA_THREADS) {
        const int ty = tid >> 4, tx = tid & 15;
        float *mine = PCA_MINE(acc, tid);
#pragma unroll 4
        for (int f = 0; f < KMEANS_TK; f++) {
          const km_f4 a0 = *(const km_f4 *)(s_x + f * KMEANS_LDX + 8 * ty), a1 = *(const km_f4 *)(s_x + f * KMEANS_LDX + 8 * ty + 4);
          const km_f4 b = *(const km_f4 *)(s_c + f * KMEANS_LDC + 4 * tx);
#pragma unroll
          for (int u = 0; u < 8; u++)
#pragma unroll
            for (int v = 0; v < 4; v++) mine[u * 4 + v] = fmaf(u < 4 ? a0[u] : a1[u - 4], b[v], mine[u * 4 + v]);
        }
        if (c0 == 0 && tid < KMEANS_ROWS) {      // (uniform over a wave: the first two waves)
          float s = PCA_MINE(xn, tid)[0];
          for (int f = 0; f < KMEANS_TK; f++) {
            const float v = s_x[f * KMEANS_LDX + tid];
            s = fmaf(v, v, s);
          }
          PCA_MINE(xn, tid)[0] = s;
        }
      }
      PCA_SYNC();
    }
    PCA_PAR(tid, PCA_THREADS) {
      const int tx = tid & 15;
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int j = c0 + 4 * tx + v;
        if (j < k) {
          const float cn = cnorm[j];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const float score = fmaf(-2.f, PCA_MINE(acc, tid)[u * 4 + v], cn);
            if (score < PCA_MINE(best, tid)[u]) { PCA_MINE(best, tid)[u] = score; PCA_MINE(arg, tid)[u] = j; }
          }
        }
      }
    }
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int u = 0; u < 8; u++) {
      s_val[(8 * ty + u) * 16 + tx] = PCA_MINE(best, tid)[u];
      s_idx[(8 * ty + u) * 16 + tx] = PCA_MINE(arg, tid)[u];
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < KMEANS_ROWS && r0 + tid < n) {
      float bv = s_val[tid * 16];
      int bi = s_idx[tid * 16];
      for (int t = 1; t < 16; t++) {
        const float v = s_val[tid * 16 + t];
        const int i = s_idx[tid * 16 + t];
        if (v < bv || (v == bv && i < bi)) { bv = v; bi = i; }
      }
      if (bi >= k) bi = 0;                         // (every score a NaN: the first centroid)
      const float dd = fmaxf(PCA_MINE(xn, tid)[0] + bv, 0.f);
      labels[r0 + tid] = bi;
      if (dist2) dist2[r0 + tid] = dd;
      s_val[tid * 16] = dd;
      s_idx[tid * 16] = labels_prev ? (labels_prev[r0 + tid] != bi) : 1;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    if (tid == 0) {
      double s = 0.0;
      int ch = 0;
      for (int r = 0; r < KMEANS_ROWS && r0 + r < n; r++) { s += (double)s_val[r * 16]; ch += s_idx[r * 16]; }
      part_inertia[wg] = s;
      part_changed[wg] = ch;
    }
  }
}

// The totals of an assign, one workgroup: thread t adds the partials of the workgroups [t per, t per + per) in order, thread 0 then the 256
// sums in order.  s_sum: [256] doubles, s_cnt: [256] ints of LDS.
PCA_WG void kmeans_totals_wg(const double *part_inertia, const int32_t *part_changed, int nwg, double *inertia, int32_t *changed, double *s_sum,
                             int32_t *s_cnt) {
  const int per = (nwg + PCA_THREADS - 1) / PCA_THREADS;
  PCA_PAR(tid, PCA_THREADS) {
    double s = 0.0;
    int ch = 0;
    for (int w = tid * per; w < (tid + 1) * per && w < nwg; w++) { s += part_inertia[w]; ch += part_changed[w]; }
    s_sum[tid] = s;
    s_cnt[tid] = ch;
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    if (tid == 0) {
      double s = 0.0;
      int ch = 0;
      for (int t = 0; t < PCA_THREADS; t++) { s += s_sum[t]; ch += s_cnt[t]; }
      *inertia = s;
      if (changed) *changed = ch;
    }
  }
}

// ----------------------------------------------------------------------------------------------- update
// Part p of kmeans_split(n, k, d), the columns [64 cb, 64 cb + 64): thread (w, c) = (tid / 64, tid % 64) walks the part's rows in order and adds
// x[r][column c] into row labels[r] of the float64 image s_img [k][64] of LDS where labels[r] % 4 == w: wave w owns the clusters j = w (mod 4), so
// no two threads share a cell, every cell is summed in row order, float64 from the first add, and four waves have loads in flight.  The image
// then goes to part_sum[p][k][d].  The workgroups of cb = 0 also count the rows of each cluster: part_cnt[p][k].  A label outside [0, k) is
// skipped.  KMEANS_UTHREADS threads.  s_cnt: [k] ints of LDS.
PCA_WG void kmeans_update_wg(const float *x, int n, int d, int64_t ldx, const int32_t *labels, int k, int p, int cb, double *part_sum, int32_t *part_cnt,
                             double *s_img, int32_t *s_cnt) {
  const KmeansSplit sp = kmeans_split(n, k, d);
  const int64_t row0 = (int64_t)p * sp.per * PCA_ROWS_PER_WG;
  const int64_t left = (int64_t)n - row0, span = (int64_t)sp.per * PCA_ROWS_PER_WG;
  const int rows = (int)(left < span ? left : span);
  PCA_PAR(tid, KMEANS_UTHREADS) {
    for (int e = tid; e < k * KMEANS_UTILE; e += KMEANS_UTHREADS) s_img[e] = 0.0;
    for (int j = tid; j < k; j += KMEANS_UTHREADS) s_cnt[j] = 0;
  }
  PCA_SYNC();
  PCA_PAR(tid, KMEANS_UTHREADS) {
    const int lane = tid & (KMEANS_UTILE - 1), w = tid / KMEANS_UTILE, c = cb * KMEANS_UTILE + lane;
    const bool in = c < d;
    for (int r = 0; r < rows; r += 16) {      // 16 rows in flight; the adds below stay in row order
      float v[16];
      int l[16];
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const bool ok = r + q < rows;
        l[q] = ok ? labels[row0 + r + q] : -1;
        if (l[q] < 0 || l[q] >= k || (l[q] & 3) != w) l[q] = -1;      // (uniform over the wave)
        v[q] = l[q] >= 0 && in ? x[(row0 + r + q) * ldx + c] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 16; q++)
        if (l[q] >= 0) {
          s_img[l[q] * KMEANS_UTILE + lane] += (double)v[q];
          if (cb == 0 && lane == 0) s_cnt[l[q]] += 1;
        }
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, KMEANS_UTHREADS) {
    const int lane = tid & (KMEANS_UTILE - 1), c = cb * KMEANS_UTILE + lane;
    if (c < d)
      for (int j = tid / KMEANS_UTILE; j < k; j += KMEANS_UTHREADS / KMEANS_UTILE) part_sum[((int64_t)p * k + j) * d + c] = s_img[j * KMEANS_UTILE + lane];
    if (cb == 0)
      for (int j = tid; j < k; j += KMEANS_UTHREADS) part_cnt[(int64_t)p * k + j] = s_cnt[j];
  }
}

// element e = j d + c of the centroids: the parts' sums added in part order over the parts' counts, rounded once; an empty cluster is not stored to
TM_DEV void kmeans_update_reduce(const double *part_sum, const int32_t *part_cnt, int P, int k, int d, float *centroids, int32_t *counts, int e) {
  const int j = e / d, c = e % d;
  double s = 0.0;
  int cnt = 0;
  for (int p = 0; p < P; p++) { s += part_sum[((int64_t)p * k + j) * d + c]; cnt += part_cnt[(int64_t)p * k + j]; }
  if (cnt > 0) centroids[e] = (float)(s / (double)cnt);
  if (c == 0) counts[j] = cnt;
}

// ----------------------------------------------------------------------------------------------- seed
// The distance pass of one k-means++ step for the rows [256 wg, 256 wg + 256): dist = sum_c (x[r][c] - centre[c])^2, the 16 lanes q of a row each
// one fmaf chain over the columns q, q + 16, ..., the 16 partials of a row then added in lane order, float32; d2[r] = first ? dist :
// min(d2[r], dist).  The workgroup's float64 sum of its d2 in row order goes to blocksum[wg].  s_p: [256][17] floats of LDS.
PCA_WG void kmeans_seed_dist_wg(const float *x, int n, int d, int64_t ldx, const float *centre, int first, float *d2, double *blocksum, int wg, float *s_p) {
  const int64_t r0 = (int64_t)wg * KMEANS_SEED_ROWS;
  PCA_PAR(tid, PCA_THREADS) {
    const int q = tid & 15, g = tid >> 4;
    for (int pass = 0; pass < 16; pass++) {
      const int row = pass * 16 + g;
      float s = 0.f;
      if (r0 + row < n)
        for (int c = q; c < d; c += 16) {
          const float v = x[(r0 + row) * ldx + c] - centre[c];
          s = fmaf(v, v, s);
        }
      s_p[row * 17 + q] = s;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    float s = 0.f;
    if (r0 + tid < n) {
      for (int q = 0; q < 16; q++) s += s_p[tid * 17 + q];
      if (!first) s = fminf(d2[r0 + tid], s);
      d2[r0 + tid] = s;
    }
    s_p[tid * 17 + 16] = s;
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    if (tid == 0) {
      double s = 0.0;
      for (int r = 0; r < KMEANS_SEED_ROWS && r0 + r < n; r++) s += (double)s_p[r * 17 + 16];
      blocksum[wg] = s;
    }
  }
}

// The pick of centre j, one workgroup.  nb = 0 (the first centre) or a total of 0 (fewer distinct rows than centres): row min(floor(u n), n - 1).
// Else the smallest row i with cum[i] > u total, cum the float64 prefix sum of d2 in row order, formed as: thread t adds the block sums of the
// blocks [t per, t per + per) in order; thread 0 adds those 256 sums in order to the total, finds the first segment, then the first block of it,
// then the first row of that block whose running sum exceeds u total.  Should rounding leave no such row, the last row of non-zero weight is
// taken: a row of zero weight is never picked.  The row is copied to centroids[j] and its index to picks[j].
// s_seg: [256] doubles, s_pick: [1] int of LDS.
PCA_WG void kmeans_seed_pick_wg(const float *x, int n, int d, int64_t ldx, const float *d2, const double *blocksum, int nb, double u, int j, float *centroids,
                                int32_t *picks, double *s_seg, int32_t *s_pick) {
  const int per = (nb + PCA_THREADS - 1) / PCA_THREADS;
  PCA_PAR(tid, PCA_THREADS) {
    double s = 0.0;
    for (int b = tid * per; b < (tid + 1) * per && b < nb; b++) s += blocksum[b];
    s_seg[tid] = s;
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    if (tid == 0) {
      double total = 0.0;
      for (int t = 0; t < PCA_THREADS; t++) total += s_seg[t];
      int64_t pick = (int64_t)((double)n * u);
      if (pick > n - 1) pick = n - 1;
      if (pick < 0) pick = 0;
      if (total > 0.0) {
        const double target = u * total;
        double cum = 0.0;
        int t = 0;
        while (t < PCA_THREADS && !(cum + s_seg[t] > target)) { cum += s_seg[t]; t++; }
        int b = t * per;
        if (t < PCA_THREADS)
          while (b < nb && !(cum + blocksum[b] > target)) { cum += blocksum[b]; b++; }
        if (t == PCA_THREADS || b >= nb) {                            // rounding: nothing exceeds the target; the last block of non-zero weight
          b = nb - 1;
          while (b > 0 && !(blocksum[b] > 0.0)) b--;
          cum = -1.0;                                                  // (no row of it passes the test below: its last weighted row is taken)
        }
        const int64_t r0 = (int64_t)b * KMEANS_SEED_ROWS;
        int64_t last = r0;
        pick = -1;
        for (int r = 0; r < KMEANS_SEED_ROWS && r0 + r < n; r++) {
          const float w = d2[r0 + r];
          if (w > 0.f) last = r0 + r;
          if (cum >= 0.0) {
            cum += (double)w;
            if (cum > target) { pick = r0 + r; break; }
          }
        }
        if (pick < 0) pick = last;
      }
      s_pick[0] = (int32_t)pick;
      picks[j] = (int32_t)pick;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    const int64_t pick = s_pick[0];
    for (int c = tid; c < d; c += PCA_THREADS) centroids[(int64_t)j * d + c] = x[pick * ldx + c];
  }
}
