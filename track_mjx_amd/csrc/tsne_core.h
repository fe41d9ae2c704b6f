// csrc/tsne_core.h — the bodies of the behaviour-map kernels (DESIGN.md "Behaviour map"; include/tmjx.h: tmjx_knn, tmjx_tsne_*): a brute-force
// k-nearest-neighbour search with a fused top-k, the perplexity search, the exact t-SNE gradient (all-pairs repulsion, CSR attraction), the
// delta-bar-delta step and the out-of-sample placement.  Written with the PCA_WG / PCA_PAR / PCA_SYNC / PCA_PRIVATE discipline of csrc/wg_core.h,
// so that they also compile on the host (tests/hostemu/tsne_emu.cpp); the column mean is csrc/moments_core.h, km_f4 and kmeans_inf the k-means'.  Every pair is a chain of float32 operations in a fixed order, every
// division is a correctly rounded one, every sum across points, tiles or workgroups is float64 in a fixed order: no atomics of any kind, the same
// bits on every run.
#pragma once
#include <string.h>

#include "kmeans_core.h"
#include "moments_core.h"

#define TSNE_MAX_D 1024
#define TSNE_MAX_N 65536         // reference / training rows: a neighbour's index fits 16 bits of LDS
#define TSNE_MAX_K 128
#define TSNE_ROWS 128            // query rows a search workgroup owns
#define TSNE_TILE 64             // reference rows of one tile of its walk
#define TSNE_TK 32               // features staged per barrier pair
#define TSNE_LDQ 132             // row stride of the staged queries  s_q[feature][query]: a thread reads its 8 queries as two 16-byte words
#define TSNE_LDR 68              // row stride of the staged references  s_r[feature][reference]: its 4 references as one
#define TSNE_LDC 65              // row stride of a tile's scores  s_cand[query][reference]: thread r scans row r, 65 keeps the 32 lanes of a group on 32 banks
#define TSNE_STAGE (TSNE_ROWS * TSNE_LDC)      // floats of the stage: the scores of a tile reuse the room of s_q and s_r
#define TSNE_BLOCK 256           // points of a workgroup of the gradient, update and placement kernels, and of a tile of the repulsion walk
#define TSNE_TARGET_WGS 1024     // the repulsion grid: the walk of a block of points is cut into parts until about this many workgroups exist
#define TSNE_BISECT 100          // iterations of the perplexity search: a bracket from 2^-100 to 2^100, then down to one float32 step

static_assert(TSNE_TK * (TSNE_LDQ + TSNE_LDR) <= TSNE_STAGE, "the scores of a tile reuse the stages");

// single float32 operations that no compiler may contract into an FMA: what numpy restates exactly
#ifdef TM_HOST_EMU
static inline float tsne_mul(float a, float b) { volatile float r = a * b; return r; }
static inline float tsne_add(float a, float b) { volatile float r = a + b; return r; }
static inline float tsne_sub(float a, float b) { volatile float r = a - b; return r; }
#else
// (HIP's __fmul_rn is a plain product that the compiler does fuse; the pragma takes the permission to contract off these operations, and hipcc's
// default contraction mode honours it after inlining)
TM_DEV float tsne_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
TM_DEV float tsne_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
TM_DEV float tsne_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
#endif

// the bits of a float32
#ifdef TM_HOST_EMU
static inline uint32_t tsne_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
#else
TM_DEV uint32_t tsne_bits(float v) { return __float_as_uint(v); }
#endif

// the fixed split of the repulsion walk: `tiles` tiles of 256 points, `per` consecutive tiles to a part.  It depends on n only.
struct TsneSplit { int tiles, per, P; };
PCA_HD TsneSplit tsne_split(int n) {
  TsneSplit s;
  s.tiles = (n + TSNE_BLOCK - 1) / TSNE_BLOCK;
  int want = TSNE_TARGET_WGS / s.tiles;
  if (want < 1) want = 1;
  if (want > s.tiles) want = s.tiles;
  s.per = (s.tiles + want - 1) / want;
  s.P = (s.tiles + s.per - 1) / s.per;
  return s;
}

// ----------------------------------------------------------------------------------------------- nearest neighbours
// ||row - mean||^2: one fmaf chain over the features in ascending order
TM_DEV float tsne_rownorm(const float *x, int64_t ldx, const float *mean, int d, int64_t row) {
  float s = 0.f;
  for (int c = 0; c < d; c++) {
    const float v = x[row * ldx + c] - mean[c];
    s = fmaf(v, v, s);
  }
  return s;
}

// The fused search for the queries [128 wg, 128 wg + 128): with qc = q - mean and xc_j = x_j - mean (float32, the column mean of x),
// score_j = xnorm_j - 2 qc . xc_j, the dot product one fmaf chain per pair in ascending feature order, dist2 = max(0, qnorm + score_j).  The
// workgroup walks the reference tiles in order; thread (ty, tx) owns the queries 8 ty + u and, in a tile, the references 4 tx + v, and leaves the
// tile's scores in LDS.  Thread r < 128 then scans row r of them in index order against the running k best of query r: the lists live in LDS,
// position-major (s_ld[p][r] float32 distances, s_li[p][r] 16-bit indices: 6 k bytes a query, 96 KB at k = 128 beside the 33 KB stage), unordered,
// with the farthest entry known: a candidate strictly nearer than it takes its place (an equal one came later: the lower index stays), and the
// farthest, the greatest (distance, index), is found again by one pass over the k.  No entry ever moves, so the lanes of a wave that do not
// insert wait for one pass, not for a shifted list.  At the end every entry goes to the position that counts the entries before it by
// (distance, index): sorted ascending, ties in index order.  With `self` the reference j = the query's own row is skipped.  idx [m][k],
// dist2 [m][k]; a list that never filled (fewer than k references left) ends in idx -1, dist2 inf.
// s_stage: [TSNE_STAGE] floats; s_ld: [k][128] floats; s_li: [k][128] uint16 of LDS.
PCA_WG void tsne_knn_wg(const float *x, int n, int d, int64_t ldx, const float *q, int64_t m, int64_t ldq, int self, int k, const float *mean,
                        const float *xnorm, const float *qnorm, int32_t *idx, float *dist2, int64_t wg, float *s_stage, float *s_ld, uint16_t *s_li) {
  const int64_t r0 = wg * TSNE_ROWS;
  float *s_q = s_stage, *s_r = s_stage + TSNE_TK * TSNE_LDQ, *s_cand = s_stage;
  PCA_PRIVATE(float, acc, 32);
  PCA_PRIVATE(float, worst, 1);
  PCA_PRIVATE(float, qn, 1);
  PCA_PRIVATE(int, cnt, 1);
  PCA_PRIVATE(int, wpos, 1);
  PCA_PAR(tid, PCA_THREADS) {
    PCA_MINE(worst, tid)[0] = kmeans_inf();
    PCA_MINE(cnt, tid)[0] = 0;
    PCA_MINE(wpos, tid)[0] = 0;
    PCA_MINE(qn, tid)[0] = (tid < TSNE_ROWS && r0 + tid < m) ? qnorm[r0 + tid] : 0.f;
  }
  for (int c0 = 0; c0 < n; c0 += TSNE_TILE) {
    PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
      for (int e = 0; e < 32; e++) PCA_MINE(acc, tid)[e] = 0.f;
    }
    for (int k0 = 0; k0 < d; k0 += TSNE_TK) {
      PCA_PAR(tid, PCA_THREADS) {
        for (int e = tid; e < TSNE_ROWS * TSNE_TK; e += PCA_THREADS) {
          const int row = e / TSNE_TK, f = e % TSNE_TK;
          s_q[f * TSNE_LDQ + row] = (r0 + row < m && k0 + f < d) ? q[(r0 + row) * ldq + k0 + f] - mean[k0 + f] : 0.f;
        }
        for (int e = tid; e < TSNE_TILE * TSNE_TK; e += PCA_THREADS) {
          const int j = e / TSNE_TK, f = e % TSNE_TK;
          s_r[f * TSNE_LDR + j] = (c0 + j < n && k0 + f < d) ? x[(int64_t)(c0 + j) * ldx + k0 + f] - mean[k0 + f] : 0.f;
        }
      }
      PCA_SYNC();
      PCA_PAR(tid, PCA_THREADS) {
        const int ty = tid >> 4, tx = tid & 15;
        float *mine = PCA_MINE(acc, tid);
#pragma unroll 4
        for (int f = 0; f < TSNE_TK; f++) {
          const km_f4 a0 = *(const km_f4 *)(s_q + f * TSNE_LDQ + 8 * ty), a1 = *(const km_f4 *)(s_q + f * TSNE_LDQ + 8 * ty + 4);
          const km_f4 b = *(const km_f4 *)(s_r + f * TSNE_LDR + 4 * tx);
#pragma unroll
          for (int u = 0; u < 8; u++)
#pragma unroll
            for (int v = 0; v < 4; v++) mine[u * 4 + v] = fmaf(u < 4 ? a0[u] : a1[u - 4], b[v], mine[u * 4 + v]);
        }
      }
      PCA_SYNC();
    }
    // the tile's scores (the stages are dead behind the barrier above)
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int j = c0 + 4 * tx + v;
        const float xn = j < n ? xnorm[j] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; u++) s_cand[(8 * ty + u) * TSNE_LDC + 4 * tx + v] = fmaf(-2.f, PCA_MINE(acc, tid)[u * 4 + v], xn);
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      if (tid < TSNE_ROWS && r0 + tid < m) {      // (uniform over a wave but for the last block of queries)
        float w = PCA_MINE(worst, tid)[0];
        int c = PCA_MINE(cnt, tid)[0], wp = PCA_MINE(wpos, tid)[0];
        const float mine = PCA_MINE(qn, tid)[0];
        const int left = n - c0 < TSNE_TILE ? n - c0 : TSNE_TILE;
        for (int jj = 0; jj < left; jj++) {
          const float dd = fmaxf(mine + s_cand[tid * TSNE_LDC + jj], 0.f);
          if ((c < k || dd < w) && !(self && c0 + jj == r0 + tid)) {
            const int p = c < k ? c : wp;
            s_ld[p * TSNE_ROWS + tid] = dd;
            s_li[p * TSNE_ROWS + tid] = (uint16_t)(c0 + jj);
            if (c < k) c++;
            if (c == k) {      // the farthest of the k: the greatest (distance, index), as one 48-bit key (a distance >= +0 orders as its bits)
              uint64_t far = 0;
              wp = 0;
#pragma unroll 8
              for (int t = 0; t < k; t++) {      // (no branch, no dependent address: the reads of eight entries are in flight together)
                const uint64_t key = ((uint64_t)tsne_bits(s_ld[t * TSNE_ROWS + tid]) << 16) | s_li[t * TSNE_ROWS + tid];
                const bool more = key > far;
                far = more ? key : far;
                wp = more ? t : wp;
              }
              w = s_ld[wp * TSNE_ROWS + tid];
            }
          }
        }
        PCA_MINE(worst, tid)[0] = w;
        PCA_MINE(cnt, tid)[0] = c;
        PCA_MINE(wpos, tid)[0] = wp;
      }
    }
    PCA_SYNC();
  }
  int32_t *s_cnt = (int32_t *)s_stage;
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < TSNE_ROWS) s_cnt[tid] = PCA_MINE(cnt, tid)[0];
  }
  PCA_SYNC();
  // the lists in order: entry p of a row goes to the position that counts the entries before it by (distance, index); two threads a row
  PCA_PAR(tid, PCA_THREADS) {
    const int row = tid & (TSNE_ROWS - 1);
    if (r0 + row < m) {
      const int c = s_cnt[row];
      const int64_t base = (r0 + row) * k;
      for (int p = tid / TSNE_ROWS; p < k; p += PCA_THREADS / TSNE_ROWS) {
        if (p < c) {
          const float dp = s_ld[p * TSNE_ROWS + row];
          const int ip = s_li[p * TSNE_ROWS + row];
          int rank = 0;
#pragma unroll 8
          for (int t = 0; t < c; t++) {
            const float dt = s_ld[t * TSNE_ROWS + row];
            const int it = s_li[t * TSNE_ROWS + row];
            rank += (dt < dp) | ((dt == dp) & (it < ip));
          }
          idx[base + rank] = ip;
          dist2[base + rank] = dp;
        } else {
          idx[base + p] = -1;
          dist2[base + p] = kmeans_inf();
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- affinities
// The entropy of p_j ~ exp(-b (d_j - dmin)) over one row: float32 exponentials, float64 sums in list order.  *S = the sum of the weights.
TM_DEV double tsne_entropy(const float *d, int k, float dmin, float b, double *S) {
  double s = 0.0, se = 0.0;
  for (int j = 0; j < k; j++) {
    const float e = d[j] - dmin, w = expf(-b * e);
    s += (double)w;
    if (w > 0.f) se += (double)w * (double)e;
  }
  *S = s;
  return log(s) + (double)b * se / s;
}

// Row i: a bisection on beta, TSNE_BISECT iterations from beta = 1 (doubling while no upper end is known), so that the entropy equals logu =
// log(perplexity); then p_j = exp(-beta (d_j - dmin)) / S, rounded once.  A row whose distances are all equal is the uniform row with beta = 1.
TM_DEV void tsne_affinity_row(const float *dist2, int k, double logu, float *p, float *beta, int64_t i) {
  const float *d = dist2 + i * k;
  float dmin = d[0], dmax = d[0];
  for (int j = 1; j < k; j++) { dmin = fminf(dmin, d[j]); dmax = fmaxf(dmax, d[j]); }
  if (!(dmax > dmin)) {
    for (int j = 0; j < k; j++) p[i * k + j] = 1.f / (float)k;
    beta[i] = 1.f;
    return;
  }
  float b = 1.f, lo = 0.f, hi = kmeans_inf();
  double S;
  for (int it = 0; it < TSNE_BISECT; it++) {
    if (tsne_entropy(d, k, dmin, b, &S) > logu) { lo = b; b = hi == kmeans_inf() ? b * 2.f : 0.5f * (lo + hi); }
    else { hi = b; b = 0.5f * (lo + hi); }
  }
  (void)tsne_entropy(d, k, dmin, b, &S);
  for (int j = 0; j < k; j++) p[i * k + j] = (float)((double)expf(-b * (d[j] - dmin)) / S);
  beta[i] = b;
}

// ----------------------------------------------------------------------------------------------- gradient
// Part `part` of the repulsion of the points [256 ib, 256 ib + 256): thread t owns point i = 256 ib + t and walks the part's tiles of 256 points,
// staged in LDS, in index order.  Per pair: dx, dy = y_i - y_j, q = fma(dy, dy, fma(dx, dx, 1)), w = 1 / q (correctly rounded), w2 = w w, and
// float64 sums of w, w2 dx, w2 dy; the pair j = i adds zeros.  parts [P][n][3] doubles.  s_y: [256][2] floats of LDS.
PCA_WG void tsne_rep_wg(const float *y, int n, TsneSplit sp, int ib, int part, double *parts, float *s_y) {
  PCA_PRIVATE(double, sum, 3);
  PCA_PRIVATE(float, yi, 2);
  PCA_PAR(tid, TSNE_BLOCK) {
    const int i = ib * TSNE_BLOCK + tid;
    PCA_MINE(yi, tid)[0] = i < n ? y[2 * (int64_t)i] : 0.f;
    PCA_MINE(yi, tid)[1] = i < n ? y[2 * (int64_t)i + 1] : 0.f;
    PCA_MINE(sum, tid)[0] = PCA_MINE(sum, tid)[1] = PCA_MINE(sum, tid)[2] = 0.0;
  }
  const int t1 = (part + 1) * sp.per < sp.tiles ? (part + 1) * sp.per : sp.tiles;
  for (int t = part * sp.per; t < t1; t++) {
    PCA_PAR(tid, TSNE_BLOCK) {
      const int j = t * TSNE_BLOCK + tid;
      s_y[2 * tid] = j < n ? y[2 * (int64_t)j] : 0.f;
      s_y[2 * tid + 1] = j < n ? y[2 * (int64_t)j + 1] : 0.f;
    }
    PCA_SYNC();
    PCA_PAR(tid, TSNE_BLOCK) {
      const int i = ib * TSNE_BLOCK + tid, j0 = t * TSNE_BLOCK;
      if (i < n) {
        const int left = n - j0 < TSNE_BLOCK ? n - j0 : TSNE_BLOCK;
        const float y0 = PCA_MINE(yi, tid)[0], y1 = PCA_MINE(yi, tid)[1];
        double sz = PCA_MINE(sum, tid)[0], sx = PCA_MINE(sum, tid)[1], sy = PCA_MINE(sum, tid)[2];
#pragma unroll 4
        for (int jj = 0; jj < left; jj++) {
          const float dx = y0 - s_y[2 * jj], dy = y1 - s_y[2 * jj + 1];
          const float q = fmaf(dy, dy, fmaf(dx, dx, 1.f));
          const float w = j0 + jj == i ? 0.f : 1.f / q;
          const float w2 = w * w;
          sz += (double)w;
          sx += (double)(w2 * dx);
          sy += (double)(w2 * dy);
        }
        PCA_MINE(sum, tid)[0] = sz; PCA_MINE(sum, tid)[1] = sx; PCA_MINE(sum, tid)[2] = sy;
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, TSNE_BLOCK) {
    const int i = ib * TSNE_BLOCK + tid;
    if (i < n)
      for (int c = 0; c < 3; c++) parts[((int64_t)part * n + i) * 3 + c] = PCA_MINE(sum, tid)[c];
  }
}

// Block b: the parts of every point added in part order (rep [n][2] doubles), and the block's sum of the points' Z in point order (zblock [b]).
// s_z: [256] doubles of LDS.
PCA_WG void tsne_rowsum_wg(const double *parts, int n, int P, int b, double *rep, double *zblock, double *s_z) {
  PCA_PAR(tid, TSNE_BLOCK) {
    const int i = b * TSNE_BLOCK + tid;
    double z = 0.0, rx = 0.0, ry = 0.0;
    if (i < n) {
      for (int p = 0; p < P; p++) {
        const double *e = parts + ((int64_t)p * n + i) * 3;
        z += e[0]; rx += e[1]; ry += e[2];
      }
      rep[2 * (int64_t)i] = rx;
      rep[2 * (int64_t)i + 1] = ry;
    }
    s_z[tid] = z;
  }
  PCA_SYNC();
  PCA_PAR(tid, TSNE_BLOCK) {
    if (tid == 0) {
      double s = 0.0;
      for (int t = 0; t < TSNE_BLOCK && b * TSNE_BLOCK + t < n; t++) s += s_z[t];
      zblock[b] = s;
    }
  }
}

// Block b: Z = the blocks' sums in block order; then thread t walks the CSR row of point i in order.  Per entry: dx, dy, q and w as above,
// attr += (P w) dx in float64 (the products float32), kl += P log(P Z / w) in float64 (an entry with P <= 0 adds nothing; a column outside
// [0, n) is skipped).  grad_i = 4 (exaggeration attr_i - rep_i / Z) in float64, rounded once; klblock [b] = the block's kl in point order; block 0
// stores Z.  s_kl: [256] doubles, s_tot: [1] double of LDS.
PCA_WG void tsne_attr_wg(const float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, double exaggeration, const double *rep,
                         const double *zblock, int nb, float *grad, double *z, double *klblock, int b, double *s_kl, double *s_tot) {
  PCA_PAR(tid, TSNE_BLOCK) {
    if (tid == 0) {
      double s = 0.0;
      for (int t = 0; t < nb; t++) s += zblock[t];
      s_tot[0] = s;
      if (b == 0) *z = s;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, TSNE_BLOCK) {
    const int i = b * TSNE_BLOCK + tid;
    double kl = 0.0;
    if (i < n) {
      const double Z = s_tot[0];
      const float y0 = y[2 * (int64_t)i], y1 = y[2 * (int64_t)i + 1];
      double ax = 0.0, ay = 0.0;
      for (int e = row_ptr[i]; e < row_ptr[i + 1]; e++) {
        const int j = col[e];
        if ((unsigned)j >= (unsigned)n) continue;
        const float pv = val[e];
        const float dx = y0 - y[2 * (int64_t)j], dy = y1 - y[2 * (int64_t)j + 1];
        const float q = fmaf(dy, dy, fmaf(dx, dx, 1.f));
        const float w = 1.f / q, pw = pv * w;
        ax += (double)(pw * dx);
        ay += (double)(pw * dy);
        if (pv > 0.f) kl += (double)pv * log((double)pv * Z / (double)w);
      }
      grad[2 * (int64_t)i] = (float)(4.0 * (exaggeration * ax - rep[2 * (int64_t)i] / Z));
      grad[2 * (int64_t)i + 1] = (float)(4.0 * (exaggeration * ay - rep[2 * (int64_t)i + 1] / Z));
    }
    s_kl[tid] = kl;
  }
  PCA_SYNC();
  PCA_PAR(tid, TSNE_BLOCK) {
    if (tid == 0) {
      double s = 0.0;
      for (int t = 0; t < TSNE_BLOCK && b * TSNE_BLOCK + t < n; t++) s += s_kl[t];
      klblock[b] = s;
    }
  }
}

// the blocks' sums in block order
TM_DEV double tsne_total(const double *block, int nb) { return wg_sum(block, nb, 1); }

// ----------------------------------------------------------------------------------------------- update
TM_DEV int tsne_sign(float v) { return (v > 0.f) - (v < 0.f); }

// Block b, delta-bar-delta: per component, gain += 0.2 where the signs of grad and velocity differ, gain *= 0.8 where they agree, floored at
// min_gain; velocity = momentum velocity - (eta gain) grad; y += velocity: single float32 operations, none fused.  ysum [b][2] = the block's
// float64 column sums of the new y in point order.  s_s: [256][2] doubles of LDS.
PCA_WG void tsne_update_wg(float *y, const float *grad, float *velocity, float *gains, int n, float momentum, float eta, float min_gain, int b, double *ysum,
                           double *s_s) {
  PCA_PAR(tid, TSNE_BLOCK) {
    const int i = b * TSNE_BLOCK + tid;
    for (int c = 0; c < 2; c++) {
      double out = 0.0;
      if (i < n) {
        const int64_t e = 2 * (int64_t)i + c;
        const float g = grad[e];
        float v = velocity[e], ga = gains[e];
        ga = tsne_sign(g) != tsne_sign(v) ? tsne_add(ga, 0.2f) : tsne_mul(ga, 0.8f);
        if (ga < min_gain) ga = min_gain;
        v = tsne_sub(tsne_mul(momentum, v), tsne_mul(tsne_mul(eta, ga), g));
        const float yy = tsne_add(y[e], v);
        gains[e] = ga; velocity[e] = v; y[e] = yy;
        out = (double)yy;
      }
      s_s[2 * tid + c] = out;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, TSNE_BLOCK) {
    if (tid < 2) {
      double s = 0.0;
      for (int t = 0; t < TSNE_BLOCK && b * TSNE_BLOCK + t < n; t++) s += s_s[2 * t + tid];
      ysum[2 * b + tid] = s;
    }
  }
}

// Block b: the column means of y (the blocks' sums in block order, over n) subtracted in float64, rounded once.  s_m: [2] doubles of LDS.
PCA_WG void tsne_center_wg(float *y, int n, const double *ysum, int nb, int b, double *s_m) {
  PCA_PAR(tid, TSNE_BLOCK) {
    if (tid < 2) {
      double s = 0.0;
      for (int t = 0; t < nb; t++) s += ysum[2 * t + tid];
      s_m[tid] = s / (double)n;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, TSNE_BLOCK) {
    const int i = b * TSNE_BLOCK + tid;
    if (i < n)
      for (int c = 0; c < 2; c++) y[2 * (int64_t)i + c] = (float)((double)y[2 * (int64_t)i + c] - s_m[c]);
  }
}

// ----------------------------------------------------------------------------------------------- placement
// Query i: y_out = sum_j p_ij y_train[idx_ij] in list order, a float32 product and a float32 add per term, none fused; an index outside [0, n) is skipped.
TM_DEV void tsne_place_row(const int32_t *idx, const float *p, int k, const float *y_train, int n, float *y_out, int64_t i) {
  float ox = 0.f, oy = 0.f;
  for (int j = 0; j < k; j++) {
    const int id = idx[i * k + j];
    if ((unsigned)id >= (unsigned)n) continue;
    const float w = p[i * k + j];
    ox = tsne_add(ox, tsne_mul(w, y_train[2 * (int64_t)id]));
    oy = tsne_add(oy, tsne_mul(w, y_train[2 * (int64_t)id + 1]));
  }
  y_out[2 * i] = ox;
  y_out[2 * i + 1] = oy;
}
