// csrc/readout_host.h — the host side the readout entry points share with the host emulation (tests/hostemu/readout_emu.cpp): the argument checks
// (an empty string: accepted) and the workspace layouts.
#pragma once
#include <math.h>
#include <stdio.h>

#include "pca_wide_host.h"
#include "readout_core.h"

namespace tmjx_host {

static inline std::string readout_check_dm(int d, int m) {
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > PCA_WIDE_MAX_D) return "d = " + std::to_string(d) + " exceeds the readout limit of " + std::to_string(PCA_WIDE_MAX_D) + " features";
  if (m < 1) return "m must be >= 1 (got " + std::to_string(m) + ")";
  if (m > READOUT_MAX_M) return "m = " + std::to_string(m) + " exceeds the readout limit of " + std::to_string(READOUT_MAX_M) + " targets";
  return "";
}
static inline std::string readout_check_l(int n_lambda) {
  if (n_lambda < 1 || n_lambda > READOUT_MAX_L)
    return "n_lambda = " + std::to_string(n_lambda) + " penalties: a call takes 1 .. " + std::to_string(READOUT_MAX_L);
  return "";
}
static inline std::string readout_check_rows(int n, int least, const char *what) {
  if (n < least) return std::string(what) + " needs n >= " + std::to_string(least) + " rows (got " + std::to_string(n) + ")";
  return "";
}
static inline std::string readout_check_ld(const char *name, int64_t ld, const char *of, int width) {
  if (ld < width) return std::string(name) + " = " + std::to_string((long long)ld) + " is smaller than " + of + " = " + std::to_string(width);
  return "";
}
static inline std::string readout_misaligned() { return "the workspace must be a 16-byte aligned device buffer of tmjx_readout_workspace's size"; }

// workspace of a fit, in floats (every part starts at a multiple of 4 floats):
//   the PCA's workspace (tmjx_pca_wide_workspace: `pca_floats`) | [S][m] float64 column sums of y | [S][d][m] float64 partial cross moments | C [d][m]
// and of a score of n rows, from the start of the same buffer (a score needs nothing a fit left there):
//   [16][m] float64 column sums of y' | [16][m] float64 partial sst | [row blocks of 256][L m] float64 partial sse
// (the first two have PCA_WIDE_MAX_SUPER slots of which S are used, so the offsets do not depend on n and the size only grows with it).
// The weights and predict need none.  S is NOT monotone in n (16 chunks are 16 super-chunks, 17 chunks are 9 of two), so a buffer for "up to n
// rows" is sized at the rows n' <= n with the most super-chunks: readout_workspace_floats.
struct ReadoutFitWorkspace { PcaWideSplit split; int64_t ysum, cross, c, floats; };
struct ReadoutScoreWorkspace { PcaWideSplit split; int64_t ysum, sst, sse, floats; };
static inline int64_t readout_up4(int64_t v) { return (v + 3) & ~(int64_t)3; }
static inline ReadoutFitWorkspace readout_fit_workspace(int n, int d, int m, int64_t pca_floats) {
  ReadoutFitWorkspace w;
  w.split = pca_wide_split(n);
  w.ysum = readout_up4(pca_floats);
  w.cross = w.ysum + readout_up4(2 * (int64_t)w.split.S * m);
  w.c = w.cross + readout_up4(2 * (int64_t)w.split.S * d * m);
  w.floats = w.c + readout_up4((int64_t)d * m);
  return w;
}
static inline ReadoutScoreWorkspace readout_score_workspace(int n, int m, int n_lambda) {
  ReadoutScoreWorkspace w;
  w.split = pca_wide_split(n);
  w.ysum = 0;
  w.sst = readout_up4(2 * (int64_t)PCA_WIDE_MAX_SUPER * m);
  w.sse = w.sst + readout_up4(2 * (int64_t)PCA_WIDE_MAX_SUPER * m);
  w.floats = w.sse + readout_up4(2 * (int64_t)w.split.nchunks * n_lambda * m);
  return w;
}

// The rows n' <= n whose split has the most super-chunks, min(chunks of n, 16): every n' <= n has at most that many.
static inline int readout_widest_rows(int n) {
  const int full = PCA_WIDE_MAX_SUPER * PCA_ROWS_PER_WG;
  return n < full ? n : full;
}
// tmjx_readout_workspace's answer: what covers a fit and a score of every n' <= n rows (2 <= n').  pca_n and pca_widest: tmjx_pca_wide_workspace
// of n and of readout_widest_rows(n) rows; the narrow PCA's grows with n, the wide one's with S, so the larger of the two covers every n'.  A fit
// of n' rows ends at up4(pca of n') + a part that grows with S(n') only, and a score's size grows with n'.
static inline int64_t readout_workspace_floats(int n, int d, int m, int n_lambda, int64_t pca_n, int64_t pca_widest) {
  const int64_t fit = readout_fit_workspace(readout_widest_rows(n), d, m, pca_n > pca_widest ? pca_n : pca_widest).floats;
  const int64_t score = readout_score_workspace(n, m, n_lambda).floats;
  return fit > score ? fit : score;
}

static inline std::string readout_check_workspace(int n, int d, int m, int n_lambda, const int64_t *floats) {
  std::string e = readout_check_dm(d, m);
  if (e.empty()) e = readout_check_l(n_lambda);
  if (e.empty()) e = readout_check_rows(n, 2, "a readout");
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string readout_check_fit(const float *x, int n, int d, int64_t ldx, const float *y, int m, int64_t ldy, const float *mean_x,
                                            const float *components, const float *variance, const float *mean_y, const float *z, const float *workspace,
                                            const tmjx_pca_info_t *info) {
  std::string e = readout_check_dm(d, m);
  if (e.empty()) e = readout_check_rows(n, 2, "a readout fit");
  if (e.empty()) e = readout_check_ld("ldx", ldx, "d", d);
  if (e.empty()) e = readout_check_ld("ldy", ldy, "m", m);
  if (!e.empty()) return e;
  if (!x || !y || !mean_x || !components || !variance || !mean_y || !z || !workspace || !info) return "null argument";
  if (!pca_al16(workspace)) return readout_misaligned();
  return "";
}

static inline std::string readout_check_weights(const float *components, const float *variance, const float *z, int d, int m, const double *lambdas,
                                                int n_lambda, const float *w) {
  std::string e = readout_check_dm(d, m);
  if (e.empty()) e = readout_check_l(n_lambda);
  if (!e.empty()) return e;
  if (!components || !variance || !z || !lambdas || !w) return "null argument";
  for (int i = 0; i < n_lambda; i++)
    if (!(lambdas[i] <= 3.4028234e38) || !((float)lambdas[i] > 0.f)) {      // (NaN fails both; the kernels take it as float32)
      char v[32];
      snprintf(v, sizeof v, "%g", lambdas[i]);
      return "lambda[" + std::to_string(i) + "] = " + v + " must be finite and > 0 as a float32 (the kernels round it to one)";
    }
  return "";
}

static inline std::string readout_check_predict(const float *x, int n, int d, int64_t ldx, const float *mean_x, const float *w, const float *mean_y, int m,
                                                const float *out, int64_t ldo) {
  std::string e = readout_check_dm(d, m);
  if (e.empty()) e = readout_check_rows(n, 1, "a prediction");
  if (e.empty()) e = readout_check_ld("ldx", ldx, "d", d);
  if (e.empty()) e = readout_check_ld("ldo", ldo, "m", m);
  if (!e.empty()) return e;
  if (!x || !mean_x || !w || !mean_y || !out) return "null argument";
  return "";
}

static inline std::string readout_check_score(const float *x, int n, int d, int64_t ldx, const float *y, int m, int64_t ldy, const float *mean_x,
                                              const float *w, const float *mean_y, int n_lambda, const double *sse, const double *sst,
                                              const float *workspace) {
  std::string e = readout_check_dm(d, m);
  if (e.empty()) e = readout_check_l(n_lambda);
  if (e.empty()) e = readout_check_rows(n, 2, "a readout score");
  if (e.empty()) e = readout_check_ld("ldx", ldx, "d", d);
  if (e.empty()) e = readout_check_ld("ldy", ldy, "m", m);
  if (!e.empty()) return e;
  if (!x || !y || !mean_x || !w || !mean_y || !sse || !sst || !workspace) return "null argument";
  if (!pca_al16(workspace)) return readout_misaligned();
  return "";
}

}  // namespace tmjx_host
