// csrc/spectrogram_host.h — the host side the spectrogram entry points share with the host emulation (tests/hostemu/spectrogram_emu.cpp): the
// wavelet bank builder (float64 on the host, rounded once), the argument checks (an empty string: accepted) and the workspace layout.
#pragma once
#include <math.h>

#include "hmm_host.h"
#include "spectrogram_core.h"

namespace tmjx_host {

// sigma_j = omega0 rate / (2 pi f_j) samples, R_j = ceil(support sigma_j): written once, so that every caller rounds alike
static inline double spec_sigma(double rate, double f, double omega0) { return omega0 * rate / (2.0 * M_PI * f); }
static inline double spec_radius(double rate, double f, double omega0, double support) { return ceil(support * spec_sigma(rate, f, omega0)); }

static inline std::string spec_check_bank(double rate, const double *freqs, int F, double omega0, double support) {
  if (F < 1) return "F must be >= 1 (got " + std::to_string(F) + ")";
  if (F > SPEC_MAX_F) return "F = " + std::to_string(F) + " exceeds the spectrogram limit of " + std::to_string(SPEC_MAX_F) + " frequencies";
  if (!freqs) return "null argument";
  if (!(rate > 0.0) || !(rate < INFINITY)) return "rate must be positive and finite (got " + std::to_string(rate) + ")";
  if (!(omega0 > 0.0) || !(omega0 < INFINITY)) return "omega0 must be positive and finite (got " + std::to_string(omega0) + ")";
  if (!(support > 0.0) || !(support < INFINITY)) return "support must be positive and finite (got " + std::to_string(support) + ")";
  for (int j = 0; j < F; j++) {
    if (!(freqs[j] > 0.0) || !(freqs[j] <= 0.5 * rate))
      return "frequency " + std::to_string(j) + " = " + std::to_string(freqs[j]) + " Hz is outside (0, rate / 2 = " + std::to_string(0.5 * rate) + "]";
    const double R = spec_radius(rate, freqs[j], omega0, support);
    if (!(R <= (double)SPEC_MAX_R))
      return "frequency " + std::to_string(j) + " = " + std::to_string(freqs[j]) + " Hz needs a radius of " + std::to_string(R) +
             " samples: it exceeds the spectrogram limit of " + std::to_string(SPEC_MAX_R);
  }
  return "";
}

static inline int64_t spec_bank_floats(double rate, const double *freqs, int F, double omega0, double support) {
  int64_t floats = 0;
  for (int j = 0; j < F; j++) floats += 3 * (2 * (int64_t)spec_radius(rate, freqs[j], omega0, support) + 1);
  return floats;
}

// bank: for every frequency g [2 R + 1], wr [2 R + 1], wi [2 R + 1]; offset [F + 1]: where each starts; radius [F]
static inline void spec_build_bank(double rate, const double *freqs, int F, double omega0, double support, float *bank, int32_t *offset, int32_t *radius) {
  int32_t at = 0;
  for (int j = 0; j < F; j++) {
    const double sigma = spec_sigma(rate, freqs[j], omega0);
    const int R = (int)spec_radius(rate, freqs[j], omega0, support), L = 2 * R + 1;
    offset[j] = at;
    radius[j] = R;
    for (int tau = -R; tau <= R; tau++) {
      const double g = exp(-(double)tau * tau / (2.0 * sigma * sigma)), ph = 2.0 * M_PI * freqs[j] * tau / rate;
      bank[at + tau + R] = (float)g;
      bank[at + L + tau + R] = (float)(g * cos(ph));
      bank[at + 2 * L + tau + R] = (float)(-g * sin(ph));
    }
    at += 3 * L;
  }
  offset[F] = at;
}

static inline std::string spec_check_shape(int n, int C, int F, int S) {
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (C < 1) return "C must be >= 1 (got " + std::to_string(C) + ")";
  if (C > SPEC_MAX_C) return "C = " + std::to_string(C) + " exceeds the spectrogram limit of " + std::to_string(SPEC_MAX_C) + " channels";
  if (F < 1) return "F must be >= 1 (got " + std::to_string(F) + ")";
  if (F > SPEC_MAX_F) return "F = " + std::to_string(F) + " exceeds the spectrogram limit of " + std::to_string(SPEC_MAX_F) + " frequencies";
  if (S < 1) return "S must be >= 1 (got " + std::to_string(S) + ")";
  if (S > n) return "S = " + std::to_string(S) + " sequences asked of n = " + std::to_string(n) + " rows (every sequence has a row)";
  return "";
}

// one workspace for the call, in floats (every part starts at a multiple of 4 floats):
//   seq_start [S + 1] int | tile_start [S + 1] int | offset [F + 1] int | radius [F] int | mean [S][C] | float64 prefix sums of the envelopes, sized
//   for F frequencies of the largest radius
struct SpecWorkspace { int64_t seq, tile, offset, radius, mean, prefix, floats; };
static inline SpecWorkspace spec_workspace(int C, int F, int S) {
  SpecWorkspace w;
  w.seq = 0;
  w.tile = w.seq + kmeans_up4((int64_t)S + 1);
  w.offset = w.tile + kmeans_up4((int64_t)S + 1);
  w.radius = w.offset + kmeans_up4(F + 1);
  w.mean = w.radius + kmeans_up4(F);
  w.prefix = w.mean + kmeans_up4((int64_t)S * C);
  w.floats = w.prefix + kmeans_up4(2 * (int64_t)F * (2 * SPEC_MAX_R + 2));
  return w;
}

static inline std::string spec_check_workspace(int n, int C, int F, int S, const int64_t *floats) {
  std::string e = spec_check_shape(n, C, F, S);
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string spec_check(const float *x, int n, int C, int64_t ldx, const int32_t *seq_start, int S, const float *bank, const int32_t *offset,
                                     const int32_t *radius, int F, int output_kind, float log_floor, const float *out, int64_t ldo, const float *coverage,
                                     const float *workspace) {
  std::string e = spec_check_shape(n, C, F, S);
  if (!e.empty()) return e;
  if (ldx < C) return "ldx = " + std::to_string((long long)ldx) + " is smaller than C = " + std::to_string(C);
  if (ldo < (int64_t)F * C) return "ldo = " + std::to_string((long long)ldo) + " is smaller than F C = " + std::to_string(F * C);
  if (!x || !bank || !offset || !radius || !out || !coverage) return "null argument";
  if (!(e = hmm_check_seq(seq_start, n, S)).empty()) return e;
  if (offset[0] != 0) return "offset[0] = " + std::to_string(offset[0]) + " must be 0";
  for (int j = 0; j < F; j++) {
    if (radius[j] < 0 || radius[j] > SPEC_MAX_R)
      return "radius[" + std::to_string(j) + "] = " + std::to_string(radius[j]) + " is outside 0 .. " + std::to_string(SPEC_MAX_R) + " (the spectrogram limit)";
    if (offset[j + 1] - offset[j] != 3 * (2 * radius[j] + 1))
      return "offset[" + std::to_string(j + 1) + "] = " + std::to_string(offset[j + 1]) + " does not follow offset[" + std::to_string(j) + "] by 3 (2 radius + 1) floats";
  }
  if (output_kind != TMJX_SPECTROGRAM_AMPLITUDE && output_kind != TMJX_SPECTROGRAM_LOG)
    return "output_kind = " + std::to_string(output_kind) + " is neither TMJX_SPECTROGRAM_AMPLITUDE nor TMJX_SPECTROGRAM_LOG";
  if (output_kind == TMJX_SPECTROGRAM_LOG && !(log_floor > 0.f)) return "log_floor must be > 0 (got " + std::to_string(log_floor) + ")";
  if (!workspace) return "null argument";
  if (!pca_al16(workspace)) return "the workspace must be a 16-byte aligned device buffer of tmjx_spectrogram_workspace's size";
  return "";
}

static inline int spec_max_radius(const int32_t *radius, int F) {
  int r = 0;
  for (int j = 0; j < F; j++) r = radius[j] > r ? radius[j] : r;
  return r;
}
static inline int64_t spec_count_tiles(const int32_t *seq_start, int S, int tt) {
  int64_t tiles = 0;
  for (int s = 0; s < S; s++) tiles += spec_tiles_of(seq_start[s + 1] - seq_start[s], tt);
  return tiles;
}

}  // namespace tmjx_host
