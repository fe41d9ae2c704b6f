// csrc/hmm_host.h — the host side the hidden-Markov-model entry points share with the host emulation (tests/hostemu/hmm_emu.cpp): the argument
// checks (an empty string: accepted), the workspace layout and the stopping rule of the fit.
#pragma once
#include <math.h>

#include "hmm_core.h"
#include "kmeans_host.h"

namespace tmjx_host {

static inline std::string hmm_check_shape(int n, int d, int k, int S) {
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > HMM_MAX_D) return "d = " + std::to_string(d) + " exceeds the HMM limit of " + std::to_string(HMM_MAX_D) + " features";
  if (k < 1) return "k must be >= 1 (got " + std::to_string(k) + ")";
  if (k > HMM_MAX_K) return "k = " + std::to_string(k) + " exceeds the HMM limit of " + std::to_string(HMM_MAX_K) + " states";
  if (S < 1) return "S must be >= 1 (got " + std::to_string(S) + ")";
  if (S > n) return "S = " + std::to_string(S) + " sequences asked of n = " + std::to_string(n) + " rows (every sequence has a row)";
  return "";
}
static inline std::string hmm_check_seq(const int32_t *seq_start, int n, int S) {
  if (!seq_start) return "null argument";
  if (seq_start[0] != 0) return "seq_start[0] = " + std::to_string(seq_start[0]) + " must be 0";
  for (int s = 0; s < S; s++)
    if (seq_start[s + 1] <= seq_start[s])
      return "seq_start[" + std::to_string(s + 1) + "] = " + std::to_string(seq_start[s + 1]) + " does not exceed seq_start[" + std::to_string(s) +
             "] = " + std::to_string(seq_start[s]) + " (strictly increasing offsets)";
  if (seq_start[S] != n) return "seq_start[S] = " + std::to_string(seq_start[S]) + " must be n = " + std::to_string(n);
  return "";
}
static inline std::string hmm_misaligned() { return "the workspace must be a 16-byte aligned device buffer of tmjx_hmm_workspace's size"; }
static inline std::string hmm_check_nonneg(const char *name, double v) {
  if (!(v >= 0.0)) return std::string(name) + " must be >= 0 (got " + std::to_string(v) + ")";
  return "";
}

// one workspace for every call, in floats (every part starts at a multiple of 4 floats).  Unlike the k-means', it scales with n k.  What does not
// depend on d comes first, and the parts per sequence are sized for n sequences, so every entry finds its parts from the arguments it has:
//   mrow [n] | cs [n] | cj [k] | logb [n][k] | alphahat [n][k] | vnext [n][k] | gamma [n][k] | back-pointers [n][k] uint8 |
//   [Px][k][k] float64 parts of the expected transitions | xi [k][k] float64 | start [k] float64 | weight [k] float64 | the fit's float64 total |
//   seq_start [n + 1] int | loglik [n] float64 | path_logprob [n] float64 |
//   [chunks of 256 rows][d] float64 column sums | mean [d] | [P][k][d] float64 S1 parts | the same of S2 | [P][k] float64 weight parts
// The parts are capped (hmm_split), so nothing scales with n k d.
struct HmmWorkspace {
  KmeansSplit msplit, xsplit;
  int nchunks;
  int64_t mrow, cs, cj, logb, alphahat, vnext, gamma, bp, xipart, xi, start, weight, total, seq, loglik, path, colsum, mean, part1, part2, partw, floats;
};
static inline HmmWorkspace hmm_workspace(int n, int d, int k) {
  HmmWorkspace w;
  const int64_t nk = (int64_t)n * k;
  w.msplit = hmm_split(n, k, d);
  w.xsplit = hmm_split(n, k, k);
  w.nchunks = pca_nwg(n);
  w.mrow = 0;
  w.cs = w.mrow + kmeans_up4(n);
  w.cj = w.cs + kmeans_up4(n);
  w.logb = w.cj + kmeans_up4(k);
  w.alphahat = w.logb + kmeans_up4(nk);
  w.vnext = w.alphahat + kmeans_up4(nk);
  w.gamma = w.vnext + kmeans_up4(nk);
  w.bp = w.gamma + kmeans_up4(nk);
  w.xipart = w.bp + kmeans_up4((nk + 3) / 4);
  w.xi = w.xipart + kmeans_up4(2 * (int64_t)w.xsplit.P * k * k);
  w.start = w.xi + kmeans_up4(2 * (int64_t)k * k);
  w.weight = w.start + kmeans_up4(2 * k);
  w.total = w.weight + kmeans_up4(2 * k);
  w.seq = w.total + 4;
  w.loglik = w.seq + kmeans_up4((int64_t)n + 1);
  w.path = w.loglik + kmeans_up4(2 * (int64_t)n);
  w.colsum = w.path + kmeans_up4(2 * (int64_t)n);
  w.mean = w.colsum + kmeans_up4(2 * (int64_t)w.nchunks * d);
  w.part1 = w.mean + kmeans_up4(d);
  w.part2 = w.part1 + kmeans_up4(2 * (int64_t)w.msplit.P * k * d);
  w.partw = w.part2 + kmeans_up4(2 * (int64_t)w.msplit.P * k * d);
  w.floats = w.partw + kmeans_up4(2 * (int64_t)w.msplit.P * k);
  return w;
}

static inline std::string hmm_check_workspace(int n, int d, int k, int S, const int64_t *floats) {
  std::string e = hmm_check_shape(n, d, k, S);
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string hmm_check_ws(const float *workspace) {
  if (!workspace) return "null argument";
  if (!pca_al16(workspace)) return hmm_misaligned();
  return "";
}

static inline std::string hmm_check_emission(const float *x, int n, int d, int64_t ldx, const float *means, const float *vars, int k, const float *logb,
                                             const float *workspace) {
  std::string e = hmm_check_shape(n, d, k, 1);
  if (!e.empty()) return e;
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  if (!x || !means || !vars || !logb) return "null argument";
  return hmm_check_ws(workspace);
}

static inline std::string hmm_check_fb(const float *logb, int n, int k, const int32_t *seq_start, int S, const float *transmat, const float *startprob,
                                       const float *gamma, const double *xi, const double *start, const double *loglik, const double *total,
                                       const float *workspace) {
  std::string e = hmm_check_shape(n, 1, k, S);
  if (!e.empty()) return e;
  if (!logb || !transmat || !startprob || !gamma || !xi || !start || !loglik || !total) return "null argument";
  if (!(e = hmm_check_seq(seq_start, n, S)).empty()) return e;
  return hmm_check_ws(workspace);
}

static inline std::string hmm_check_mstep(const float *x, int n, int d, int64_t ldx, const float *gamma, int k, double min_var, double min_weight,
                                          const float *means, const float *vars, const double *weight, const float *workspace) {
  std::string e = hmm_check_shape(n, d, k, 1);
  if (!e.empty()) return e;
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  if (!x || !gamma || !means || !vars || !weight) return "null argument";
  if (!(e = hmm_check_nonneg("min_var", min_var)).empty()) return e;
  if (!(e = hmm_check_nonneg("min_weight", min_weight)).empty()) return e;
  return hmm_check_ws(workspace);
}

static inline std::string hmm_check_transitions(const double *xi, const double *start, int k, double prior, double kappa, const float *transmat,
                                                const float *startprob) {
  std::string e = hmm_check_shape(1, 1, k, 1);
  if (!e.empty()) return e;
  if (!xi || !start || !transmat || !startprob) return "null argument";
  if (!(e = hmm_check_nonneg("prior", prior)).empty()) return e;
  return hmm_check_nonneg("kappa", kappa);
}

static inline std::string hmm_check_viterbi(const float *logb, int n, int k, const int32_t *seq_start, int S, const float *transmat, const float *startprob,
                                            const int32_t *labels, const double *path_logprob, const float *workspace) {
  std::string e = hmm_check_shape(n, 1, k, S);
  if (!e.empty()) return e;
  if (!logb || !transmat || !startprob || !labels || !path_logprob) return "null argument";
  if (!(e = hmm_check_seq(seq_start, n, S)).empty()) return e;
  return hmm_check_ws(workspace);
}

static inline std::string hmm_check_fit(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int k, const float *means,
                                        const float *vars, const float *transmat, const float *startprob, const int32_t *labels, int max_iter, double tol,
                                        double prior, double kappa, double min_var, double min_weight, const tmjx_hmm_info_t *info,
                                        const float *workspace) {
  std::string e = hmm_check_shape(n, d, k, S);
  if (!e.empty()) return e;
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  if (!x || !means || !vars || !transmat || !startprob || !labels || !info) return "null argument";
  if (!(e = hmm_check_seq(seq_start, n, S)).empty()) return e;
  if (!(e = hmm_check_ws(workspace)).empty()) return e;
  if (max_iter < 1) return "max_iter must be >= 1 (got " + std::to_string(max_iter) + ")";
  if (!(e = hmm_check_nonneg("tol", tol)).empty()) return e;
  if (!(e = hmm_check_nonneg("prior", prior)).empty()) return e;
  if (!(e = hmm_check_nonneg("kappa", kappa)).empty()) return e;
  if (!(e = hmm_check_nonneg("min_var", min_var)).empty()) return e;
  return hmm_check_nonneg("min_weight", min_weight);
}

// the stopping rule of EM after the forward-backward of iteration `it` (0-based): the loglik rose by no more than tol x |the previous one|
static inline bool hmm_converged(int it, double loglik, double previous, double tol) { return it > 0 && loglik - previous <= tol * fabs(previous); }

}  // namespace tmjx_host
