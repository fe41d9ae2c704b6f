// csrc/pca_wide_host.h — the host side the wide PCA entry points share with the host emulation (tests/hostemu/pca_wide_emu.cpp): the argument
// checks (an empty string: accepted), the workspace layout and the stopping rule of the block iteration.
#pragma once
#include "pca_host.h"
#include "pca_wide_core.h"

namespace tmjx_host {

static inline std::string pca_wide_check_shape(int n, int d, int64_t ldx) {
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > PCA_WIDE_MAX_D) return "d = " + std::to_string(d) + " exceeds the wide PCA limit of " + std::to_string(PCA_WIDE_MAX_D) + " features";
  if (n < 2) return "PCA needs n >= 2 rows (got " + std::to_string(n) + ")";
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  return "";
}

// workspace of a fit with d > 128, in floats (every part starts at a multiple of 4 floats):
//   [S][d] float64 column sums | [S][d][d] float64 partial Gram matrices | A [d][d] | V^T [d][d] | per pair: the gathered sub-matrix [128][128],
//   its eigenvector rows [128][128], its eigenvalues [128], the inner solver's report | [2][d] float64 row norms | ||A||_F^2 and off(A)^2, float64
// S <= 16 whatever n is: the size grows with d^2 only.
struct PcaWideWorkspace { PcaWideSplit split; int pairs; int64_t colsum, gram, cov, vt, sub, rot, lam, info, rowsum, norms, floats; };
static inline PcaWideWorkspace pca_wide_workspace(int n, int d) {
  PcaWideWorkspace w;
  auto up4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  w.split = pca_wide_split(n);
  w.pairs = pca_wide_players(d) / 2;
  w.colsum = 0;
  w.gram = up4(2 * (int64_t)w.split.S * d);
  w.cov = w.gram + up4(2 * (int64_t)w.split.S * d * d);
  w.vt = w.cov + up4((int64_t)d * d);
  w.sub = w.vt + up4((int64_t)d * d);
  w.rot = w.sub + (int64_t)w.pairs * PCA_MAX_D * PCA_MAX_D;
  w.lam = w.rot + (int64_t)w.pairs * PCA_MAX_D * PCA_MAX_D;
  w.info = w.lam + (int64_t)w.pairs * PCA_MAX_D;
  w.rowsum = w.info + 4 * (int64_t)w.pairs;
  w.norms = w.rowsum + up4(4 * (int64_t)d);
  w.floats = w.norms + 4;
  return w;
}

static inline std::string pca_wide_check_fit(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, const float *variance,
                                             const float *workspace, const tmjx_pca_info_t *info) {
  const std::string e = pca_wide_check_shape(n, d, ldx);
  if (!e.empty()) return e;
  if (!x || !mean || !components || !variance || !workspace || !info) return "null argument";
  if (!pca_al16(workspace)) return "the workspace must be a 16-byte aligned device buffer of tmjx_pca_wide_workspace's size";
  return "";
}

static inline std::string pca_wide_check_transform(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k,
                                                   const float *out, int64_t ldo) {
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > PCA_WIDE_MAX_D) return "d = " + std::to_string(d) + " exceeds the wide PCA limit of " + std::to_string(PCA_WIDE_MAX_D) + " features";
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  if (k < 1 || k > d) return "k = " + std::to_string(k) + " components asked of d = " + std::to_string(d) + " (1 <= k <= d)";
  if (ldo < k) return "ldo = " + std::to_string((long long)ldo) + " is smaller than k = " + std::to_string(k);
  if (!x || !mean || !components || !out) return "null argument";
  return "";
}

// norms[0] = ||A||_F^2, norms[1] = off(A)^2
static inline bool pca_wide_finite(const double *norms) { return norms[0] <= 1.7976931348623157e308 && norms[1] <= 1.7976931348623157e308; }      // false for NaN and inf
static inline bool pca_wide_converged(const double *norms) { return norms[1] <= (double)PCA_TOL * (double)PCA_TOL * norms[0]; }
static inline float pca_wide_off_rel(const double *norms) { return norms[0] > 0.0 ? (float)sqrt(norms[1] / norms[0]) : 0.f; }
static inline std::string pca_wide_nonfinite_message() {
  return "tmjx_pca_fit_wide: the covariance is non-finite (is every value of x finite?); nothing was rotated";
}
static inline std::string pca_wide_noconv_message(int sweeps, float off_rel) {
  return "tmjx_pca_fit_wide: the block Jacobi iteration did not converge in " + std::to_string(sweeps) + " block sweeps (off / norm = " +
         std::to_string(off_rel) + ")";
}

}  // namespace tmjx_host
