// csrc/spectrogram_core.h — the bodies of the wavelet-spectrogram kernels (DESIGN.md "Spectrogram"; include/tmjx.h: tmjx_spectrogram): a bank of
// complex Morlet FIR filters over every channel of a recorded signal x [n][C], the rows split into S sequences; no tap crosses a sequence
// boundary.  Written with the PCA_WG / PCA_PAR / PCA_SYNC discipline of csrc/wg_core.h, so that they also compile on the host
// (tests/hostemu/spectrogram_emu.cpp): whatever a thread carries from one PCA_PAR region to the next is PCA_PRIVATE or lives in LDS.
//   re, im   one float32 FMA chain per output in ascending tap order.  Rows outside the sequence are zeros in the LDS image: a zero product leaves
//            the chain's bits as they are, so the bits of an output depend on its sequence alone, not on the tiling or on what else is in the call.
//   G        the in-range sum of the envelope: a difference of two entries of its float64 prefix sums, rounded once
//   mean     float64 sums of four interleaved row classes in row order, the classes added in order, rounded once
// No atomics: the same bits on every run.
#pragma once
#include "wg_core.h"

#define SPEC_MAX_C 1024
#define SPEC_MAX_F 64
#define SPEC_MAX_R 4096
#define SPEC_U 8                   // consecutive rows of one channel a thread holds in registers: one LDS read per tap serves 8 outputs
#define SPEC_THREADS 256           // at most; a narrow signal takes fewer (SpecGeom.threads)
#define SPEC_CW 64                 // at most this many channels to a channel block
#define SPEC_MAX_TT (SPEC_U * 64)  // rows of the largest tile
#define SPEC_LDS_FLOATS 10240      // the signal image of a workgroup: at most 40 KB, with s_G three workgroups to a CU
#define SPEC_MEAN_CLASSES 4        // interleaved row classes of the sequence mean
#define SPEC_BATCH 4               // global loads a thread has in flight while it fills the image

#ifdef TM_HOST_EMU
struct sp_f2 { float x, y; };
#else
typedef float sp_f2 __attribute__((ext_vector_type(2)));
#endif

// what the compiler must not carry across the frequency loop: hoisted there, the eight row masks of the epilogue cost more scalar registers than there are
#ifdef TM_HOST_EMU
#define SPEC_OPAQUE(v) ((void)0)
#else
#define SPEC_OPAQUE(v) asm volatile("" : "+v"(v))
#endif

// (re, im) += (wr, wi) x: one v_pk_fma_f32 on the GPU, two fmaf on the host, the same bits
TM_DEV sp_f2 spec_fma2(sp_f2 w, float x, sp_f2 acc) {
#ifdef TM_HOST_EMU
  sp_f2 r = {fmaf(w.x, x, acc.x), fmaf(w.y, x, acc.y)};
  return r;
#else
  sp_f2 xx = {x, x};
  return __builtin_elementwise_fma(w, xx, acc);
#endif
}

// How a call is cut into workgroups.  It depends on C and the largest radius only: the channels go into `cblocks` blocks of `cw` (<= 64), a
// workgroup owns `tt` = 8 tg rows of one sequence (tiles are counted from the sequence's first row) and one channel block, thread (g, c) =
// (tid / cw, tid % cw) the rows 8 g .. 8 g + 7 of channel c: a wave stores runs of cw consecutive floats, and a narrow signal packs many row
// groups into a wave.  The image holds `sr` rows at the odd stride `ldc`; a frequency whose window is wider walks it in stages of `ts` taps.
struct SpecGeom { int cblocks, cw, tg, tt, threads, ldc, sr, ts, lds_floats; };
PCA_HD SpecGeom spec_geom(int C, int rmax) {
  SpecGeom g;
  g.cblocks = (C + SPEC_CW - 1) / SPEC_CW;
  g.cw = (C + g.cblocks - 1) / g.cblocks;
  const int cap = 64 / g.cw > 16 ? 64 / g.cw : 16;
  g.tg = SPEC_THREADS / g.cw < cap ? SPEC_THREADS / g.cw : cap;
  g.tt = SPEC_U * g.tg;
  g.threads = (g.tg * g.cw + 63) / 64 * 64;
  g.ldc = g.cw | 1;
  const int want = g.tt + (2 * rmax + 1 + SPEC_U - 1) / SPEC_U * SPEC_U, fit = SPEC_LDS_FLOATS / g.ldc;
  g.sr = want < fit ? want : fit;
  g.ts = (g.sr - g.tt) / SPEC_U * SPEC_U;      // >= 56: at ldc = 65 the budget holds 157 rows, the tile there 32
  g.lds_floats = g.sr * g.ldc;
  return g;
}
PCA_HD int spec_tiles_of(int T, int tt) { return (T + tt - 1) / tt; }
// where the float64 prefix sums of frequency j's envelope start: offset[j] / 3 envelope entries precede it, and j sums of one more entry each
PCA_HD int64_t spec_prefix_at(const int32_t *offset, int j) { return (int64_t)offset[j] / 3 + j; }

// ----------------------------------------------------------------------------------------------- preparation
// tile_start [S + 1]: the first tile of every sequence; prefix [sum_j (2 R_j + 2)] float64: P_j[k] = g_j[-R_j] + .. + g_j[-R_j + k - 1] in
// ascending order.  One workgroup: thread i counts the tiles of its run of sequences, thread 0 adds the 256 counts in order, thread i numbers
// its run; thread j < F sums the envelope of frequency j.  s_cnt: [SPEC_THREADS + 1] ints of LDS.
PCA_WG void spec_prepare_wg(const int32_t *seq_start, int S, int tt, const float *bank, const int32_t *offset, const int32_t *radius, int F, int32_t *tile_start,
                            double *prefix, int32_t *s_cnt) {
  const int per = (S + SPEC_THREADS - 1) / SPEC_THREADS;
  PCA_PAR(tid, SPEC_THREADS) {
    int cnt = 0;
    for (int s = tid * per; s < (tid + 1) * per && s < S; s++) cnt += spec_tiles_of(seq_start[s + 1] - seq_start[s], tt);
    s_cnt[tid + 1] = cnt;
    if (tid < F) {
      const int R = radius[tid];
      const float *gt = bank + offset[tid];
      double *P = prefix + spec_prefix_at(offset, tid);
      double sum = 0.0;
      P[0] = 0.0;
      for (int k = 0; k <= 2 * R; k++) { sum += (double)gt[k]; P[k + 1] = sum; }
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, SPEC_THREADS) {
    if (tid == 0) {
      s_cnt[0] = 0;
      for (int i = 0; i < SPEC_THREADS; i++) s_cnt[i + 1] += s_cnt[i];
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, SPEC_THREADS) {
    int at = s_cnt[tid];
    for (int s = tid * per; s < (tid + 1) * per && s < S; s++) {
      tile_start[s] = at;
      at += spec_tiles_of(seq_start[s + 1] - seq_start[s], tt);
    }
    if (tid == SPEC_THREADS - 1) tile_start[S] = s_cnt[SPEC_THREADS];
  }
}

// mean [S][C] of sequence s, the channels 64 cb .. 64 cb + 63: thread (h, c) = (tid / 64, tid % 64) adds the rows h, h + 4, .. of channel c in
// float64, the four classes are added in order, the quotient is rounded once.  s_sum: [256] doubles of LDS.
PCA_WG void spec_mean_wg(const float *x, int C, int64_t ldx, const int32_t *seq_start, int s, int cb, float *mean, double *s_sum) {
  const int r0 = seq_start[s], T = seq_start[s + 1] - r0;
  PCA_PAR(tid, SPEC_THREADS) {
    const int h = tid >> 6, c = cb * 64 + (tid & 63);
    double sum = 0.0;
    if (c < C)
      for (int t = h; t < T; t += SPEC_MEAN_CLASSES) sum += (double)x[(int64_t)(r0 + t) * ldx + c];
    s_sum[tid] = sum;
  }
  PCA_SYNC();
  PCA_PAR(tid, SPEC_THREADS) {
    const int c = cb * 64 + tid;
    if (tid < 64 && c < C) mean[(int64_t)s * C + c] = (float)((((s_sum[tid] + s_sum[64 + tid]) + s_sum[128 + tid]) + s_sum[192 + tid]) / (double)T);
  }
}

// ----------------------------------------------------------------------------------------------- the transform
// the sequence of a tile: the last s with tile_start[s] <= tile
TM_DEV int spec_seq_of(const int32_t *tile_start, int S, int tile) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Tile `tile` of the call, channel block cb, every frequency in turn.  For frequency j with radius R and the tile's rows [t0, t0 + tt) of a
// sequence of T rows, the taps that reach any row of the sequence are [max(-R, -(t0 + tv - 1)), min(R, T - 1 - t0)], tv the rows the tile holds;
// they are walked in ascending order in stages of g.ts: a stage [a, b) needs the rows t0 + a .. t0 + tt + (b - a) - 1 of x - mean in LDS
// (zeros outside the sequence and beyond C) and loads them unless the image at hand already holds them, then every thread slides its window of 8 values along them: one LDS read and 8 packed FMAs per
// tap, the tap weights the same in every lane.  A = 2 sqrt(re^2 + im^2) / G goes out in runs along c.
// s_img: g.lds_floats floats of LDS; s_G: [2][SPEC_MAX_TT] floats.
PCA_WG void spec_tile_wg(const float *x, int C, int64_t ldx, const int32_t *seq_start, const int32_t *tile_start, int S, const float *mean, const float *bank,
                         const int32_t *offset, const int32_t *radius, const double *prefix, int F, int log_output, float log_floor, float *out, int64_t ldo,
                         float *coverage, SpecGeom g, int tile, int cb, float *s_img, float *s_G) {
  const int s = spec_seq_of(tile_start, S, tile);
  const int r0 = seq_start[s], T = seq_start[s + 1] - r0, t0 = (tile - tile_start[s]) * g.tt, tv = T - t0 < g.tt ? T - t0 : g.tt;
  const int c0 = cb * g.cw, rows_per_pass = g.threads / g.cw;
  PCA_PRIVATE(sp_f2, acc, SPEC_U);
  int have_lo = 0, have_n = 0;      // the rows of the sequence that the image holds: [have_lo, have_lo + have_n)
  for (int j = 0; j < F; j++) {
    const int R = radius[j];
    const float *gt = bank + offset[j] + R, *wr = gt + (2 * R + 1), *wi = wr + (2 * R + 1);      // centred: the entry of tap tau is [tau]
    const double *P = prefix + spec_prefix_at(offset, j);
    const int tlo = -R > -(t0 + tv - 1) ? -R : -(t0 + tv - 1), thi = R < T - 1 - t0 ? R : T - 1 - t0;
    float *sG = s_G + (j & 1) * SPEC_MAX_TT;      // two buffers: the next frequency's G is written while a slower wave still reads this one's
    PCA_PAR(tid, g.threads) {
      for (int r = tid; r < tv; r += g.threads) {
        const int t = t0 + r, lo = -R > -t ? -R : -t, hi = R < T - 1 - t ? R : T - 1 - t;
        const float G = (float)(P[hi + R + 1] - P[lo + R]);
        sG[r] = G;
        if (cb == 0) coverage[(int64_t)(r0 + t) * F + j] = G / (float)P[2 * R + 1];
      }
#pragma unroll
      for (int u = 0; u < SPEC_U; u++) { sp_f2 z = {0.f, 0.f}; PCA_MINE(acc, tid)[u] = z; }
    }
    for (int a = tlo; a <= thi; a += g.ts) {
      const int b = a + g.ts < thi + 1 ? a + g.ts : thi + 1, nr = g.tt + (b - a), need_lo = t0 + a;
      int shift = need_lo - have_lo;
      if (shift < 0 || shift + nr > have_n) {      // (a bank in ascending frequency: the image of a wider window serves the narrower ones after it)
        PCA_SYNC();                                // every thread is done with the old image
        PCA_PAR(tid, g.threads) {
          const int lr = tid / g.cw, lc = tid - lr * g.cw, c = c0 + lc;
          if (lr < rows_per_pass) {
            const bool col = c < C;
            const float m = col && mean ? mean[(int64_t)s * C + c] : 0.f;
            for (int q0 = lr; q0 < nr; q0 += SPEC_BATCH * rows_per_pass) {      // four loads in flight
              float v[SPEC_BATCH];
#pragma unroll
              for (int i = 0; i < SPEC_BATCH; i++) {      // (outside the sequence m itself: m - m is the zero of the image, and a NaN mean has made NaNs of the whole sequence)
                const int q = q0 + i * rows_per_pass, t = need_lo + q;
                v[i] = q < nr && col && t >= 0 && t < T ? x[(int64_t)(r0 + t) * ldx + c] : m;
              }
#pragma unroll
              for (int i = 0; i < SPEC_BATCH; i++)
                if (q0 + i * rows_per_pass < nr) s_img[(q0 + i * rows_per_pass) * g.ldc + lc] = v[i] - m;
            }
          }
        }
        PCA_SYNC();
        have_lo = need_lo;
        have_n = nr;
        shift = 0;
      }
      PCA_PAR(tid, g.threads) {
        const int tgi = tid / g.cw, lc = tid - tgi * g.cw;
        if (tgi < g.tg) {
          const float *base = s_img + (shift + tgi * SPEC_U) * g.ldc + lc;
          sp_f2 *mine = PCA_MINE(acc, tid);
          float win[SPEC_U];
#pragma unroll
          for (int u = 0; u < SPEC_U; u++) win[u] = base[u * g.ldc];
          const int taps = b - a, full = taps / SPEC_U * SPEC_U;
          for (int k0 = 0; k0 < full; k0 += SPEC_U) {
#pragma unroll
            for (int k = 0; k < SPEC_U; k++) {      // tap a + k0 + k: win[(k + u) % 8] holds the row shift + 8 tgi + k0 + k + u of the image
              const sp_f2 w = {wr[a + k0 + k], wi[a + k0 + k]};
#pragma unroll
              for (int u = 0; u < SPEC_U; u++) mine[u] = spec_fma2(w, win[(k + u) % SPEC_U], mine[u]);
              win[k] = base[(k0 + k + SPEC_U) * g.ldc];
            }
          }
          for (int k = full; k < taps; k++) {
            const sp_f2 w = {wr[a + k], wi[a + k]};
#pragma unroll
            for (int u = 0; u < SPEC_U; u++) mine[u] = spec_fma2(w, base[(k + u) * g.ldc], mine[u]);
          }
        }
      }
    }
    PCA_SYNC();      // G is written
    PCA_PAR(tid, g.threads) {
      const int tgi = tid / g.cw, lc = tid - tgi * g.cw, c = c0 + lc;
      if (tgi < g.tg && c < C) {
        int mine_rows = tv - tgi * SPEC_U;      // the rows of this thread that the tile holds
        SPEC_OPAQUE(mine_rows);
#pragma unroll
        for (int u = 0; u < SPEC_U; u++) {
          const int r = tgi * SPEC_U + u;
          if (u < mine_rows) {
            const sp_f2 v = PCA_MINE(acc, tid)[u];
            const float A = 2.f * sqrtf(fmaf(v.x, v.x, v.y * v.y)) / sG[r];
            out[(int64_t)(r0 + t0 + r) * ldo + (int64_t)j * C + c] = log_output ? logf(A < log_floor ? log_floor : A) : A;      // (a NaN stays one)
          }
        }
      }
    }
  }
}
