// csrc/arhmm_host.h — the host side the autoregressive-HMM entry points share with the host emulation (tests/hostemu/arhmm_emu.cpp): the argument
// checks (an empty string: accepted) and the workspace layout.  The stopping rule of the fit is hmm_converged (csrc/hmm_host.h).
#pragma once
#include <math.h>

#include "arhmm_core.h"
#include "hmm_host.h"

namespace tmjx_host {

static inline std::string arhmm_check_shape(int n, int d, int lags, int k, int S) {
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > ARHMM_MAX_D)
    return "d = " + std::to_string(d) + " exceeds the autoregressive HMM's limit of " + std::to_string(ARHMM_MAX_D) + " features (project wider layers with the PCA first)";
  if (lags < 0 || lags > ARHMM_MAX_LAGS) return "lags = " + std::to_string(lags) + " is outside 0 .. " + std::to_string(ARHMM_MAX_LAGS);
  if (lags * d > ARHMM_MAX_LD)
    return "lags x d = " + std::to_string(lags * d) + " exceeds the limit of " + std::to_string(ARHMM_MAX_LD) + " lagged regressor columns";
  if (k < 1) return "k must be >= 1 (got " + std::to_string(k) + ")";
  if (k > HMM_MAX_K) return "k = " + std::to_string(k) + " exceeds the HMM limit of " + std::to_string(HMM_MAX_K) + " states";
  if (S < 1) return "S must be >= 1 (got " + std::to_string(S) + ")";
  if (S > n) return "S = " + std::to_string(S) + " sequences asked of n = " + std::to_string(n) + " rows (every sequence has a row)";
  return "";
}
static inline std::string arhmm_check_warmup(int lags, int warmup) {
  if (warmup < lags) return "warmup = " + std::to_string(warmup) + " is smaller than lags = " + std::to_string(lags) + " (a scored row has all of its lags)";
  return "";
}
static inline std::string arhmm_check_ws(const float *workspace) {
  if (!workspace) return "null argument";
  if (!pca_al16(workspace)) return "the workspace must be a 16-byte aligned device buffer of tmjx_arhmm_workspace's size";
  return "";
}

// one workspace for every call, in floats (every part starts at a multiple of 4 floats).  What depends on d, lags and k only comes first, so that
// the solve, which has no n, finds its parts; then the workspace of the reused HMM steps (hmm_workspace(n, 1, k): the forward-backward's and the
// Viterbi's scratch, and logb, gamma, xi, start, loglik, path and total of a fit); then what scales with the rows:
//   status [k] int | cj [k] | weight [k] float64 | dg [k][p] float64 | rhs [k][d][p] float64 | fac [k][p][p] float64 | moments [k][q][q] float64 |
//   the HMM workspace | seq_start [S + 1] int | pos [n] int | [P][k][q][q] float64 parts of the moments
struct ArhmmWorkspace {
  KmeansSplit split;
  int p, q;
  int64_t status, cj, weight, dg, rhs, fac, moments, hmm, seq, pos, parts, floats;
};
static inline ArhmmWorkspace arhmm_workspace(int n, int d, int lags, int k, int S) {
  ArhmmWorkspace w;
  w.p = arhmm_p(d, lags);
  w.q = w.p + d;
  w.split = arhmm_split(n, k, w.q);
  w.status = 0;
  w.cj = w.status + kmeans_up4(k);
  w.weight = w.cj + kmeans_up4(k);
  w.dg = w.weight + kmeans_up4(2 * k);
  w.rhs = w.dg + kmeans_up4(2 * (int64_t)k * w.p);
  w.fac = w.rhs + kmeans_up4(2 * (int64_t)k * d * w.p);
  w.moments = w.fac + kmeans_up4(2 * (int64_t)k * w.p * w.p);
  w.hmm = w.moments + kmeans_up4(2 * (int64_t)k * w.q * w.q);
  w.seq = w.hmm + kmeans_up4(hmm_workspace(n, 1, k).floats);
  w.pos = w.seq + kmeans_up4((int64_t)S + 1);
  w.parts = w.pos + kmeans_up4(n);
  w.floats = w.parts + kmeans_up4(2 * (int64_t)w.split.P * k * w.q * w.q);
  return w;
}

static inline std::string arhmm_check_workspace(int n, int d, int lags, int k, int S, const int64_t *floats) {
  std::string e = arhmm_check_shape(n, d, lags, k, S);
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string arhmm_check_rows(int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, int k) {
  std::string e = arhmm_check_shape(n, d, lags, k, S);
  if (!e.empty()) return e;
  if (!(e = arhmm_check_warmup(lags, warmup)).empty()) return e;
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  return hmm_check_seq(seq_start, n, S);
}

static inline std::string arhmm_check_emission(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup,
                                               const float *weights, const float *vars, int k, const float *logb, const float *workspace) {
  std::string e = arhmm_check_rows(n, d, ldx, seq_start, S, lags, warmup, k);
  if (!e.empty()) return e;
  if (!x || !weights || !vars || !logb) return "null argument";
  return arhmm_check_ws(workspace);
}

static inline std::string arhmm_check_moments(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *gamma,
                                              int k, const double *moments, const double *weight, const float *workspace) {
  std::string e = arhmm_check_rows(n, d, ldx, seq_start, S, lags, warmup, k);
  if (!e.empty()) return e;
  if (!x || !gamma || !moments || !weight) return "null argument";
  return arhmm_check_ws(workspace);
}

static inline std::string arhmm_check_solve(const double *moments, const double *weight, int k, int d, int lags, double ridge, double min_var, double min_weight,
                                            const float *weights, const float *vars, const int32_t *status, const float *workspace) {
  std::string e = arhmm_check_shape(1, d, lags, k, 1);
  if (!e.empty()) return e;
  if (!moments || !weight || !weights || !vars || !status) return "null argument";
  if (!(e = hmm_check_nonneg("ridge", ridge)).empty()) return e;
  if (!(e = hmm_check_nonneg("min_var", min_var)).empty()) return e;
  if (!(e = hmm_check_nonneg("min_weight", min_weight)).empty()) return e;
  return arhmm_check_ws(workspace);
}

static inline std::string arhmm_check_fit(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, int k,
                                          const float *weights, const float *vars, const float *transmat, const float *startprob, const int32_t *labels,
                                          int max_iter, double tol, double prior, double kappa, double ridge, double min_var, double min_weight,
                                          const tmjx_arhmm_info_t *info, const float *workspace) {
  std::string e = arhmm_check_rows(n, d, ldx, seq_start, S, lags, warmup, k);
  if (!e.empty()) return e;
  if (!x || !weights || !vars || !transmat || !startprob || !labels || !info) return "null argument";
  if (!(e = arhmm_check_ws(workspace)).empty()) return e;
  if (max_iter < 1) return "max_iter must be >= 1 (got " + std::to_string(max_iter) + ")";
  if (!(e = hmm_check_nonneg("tol", tol)).empty()) return e;
  if (!(e = hmm_check_nonneg("prior", prior)).empty()) return e;
  if (!(e = hmm_check_nonneg("kappa", kappa)).empty()) return e;
  if (!(e = hmm_check_nonneg("ridge", ridge)).empty()) return e;
  if (!(e = hmm_check_nonneg("min_var", min_var)).empty()) return e;
  return hmm_check_nonneg("min_weight", min_weight);
}

}  // namespace tmjx_host
