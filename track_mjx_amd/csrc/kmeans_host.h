// csrc/kmeans_host.h — the host side the k-means entry points share with the host emulation (tests/hostemu/kmeans_emu.cpp): the argument checks
// (an empty string: accepted) and the workspace layout.
#pragma once
#include "kmeans_core.h"
#include "pca_wide_host.h"

namespace tmjx_host {

static inline std::string kmeans_check_shape(int n, int d, int k) {
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > KMEANS_MAX_D) return "d = " + std::to_string(d) + " exceeds the k-means limit of " + std::to_string(KMEANS_MAX_D) + " features";
  if (k < 1) return "k must be >= 1 (got " + std::to_string(k) + ")";
  if (k > KMEANS_MAX_K) return "k = " + std::to_string(k) + " exceeds the k-means limit of " + std::to_string(KMEANS_MAX_K) + " centroids";
  if (k > n) return "k = " + std::to_string(k) + " centroids asked of n = " + std::to_string(n) + " rows (k <= n)";
  return "";
}
static inline std::string kmeans_check_x(int n, int d, int k, int64_t ldx) {
  std::string e = kmeans_check_shape(n, d, k);
  if (e.empty() && ldx < d) e = "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  return e;
}
static inline std::string kmeans_misaligned() { return "the workspace must be a 16-byte aligned device buffer of tmjx_kmeans_workspace's size"; }

// one workspace for every call, in floats (every part starts at a multiple of 4 floats):
//   [chunks of 256 rows][d] float64 column sums | mean [d] | cnorm [k] | [assign workgroups] float64 inertia partials | [assign workgroups] int changed partials |
//   [P][k][d] float64 partial sums of the update | [P][k] int partial counts | d2 [n] of the seeding | [blocks of 256 rows] float64 block sums |
//   picks [k] int | the fit's second label buffer [n] int | the fit's {float64 inertia, int changed} read-back
// The update's partials are capped (kmeans_split), so no part scales with n k d.
struct KmeansWorkspace {
  int nwg_assign, nb_seed;
  KmeansSplit split;
  int64_t colsum, mean, cnorm, part_inertia, part_changed, part_sum, part_cnt, d2, blocksum, picks, labels2, result, floats;
};
static inline int64_t kmeans_up4(int64_t v) { return (v + 3) & ~(int64_t)3; }
static inline KmeansWorkspace kmeans_workspace(int n, int d, int k) {
  KmeansWorkspace w;
  w.nwg_assign = kmeans_tiles(n, KMEANS_ROWS);
  w.nb_seed = kmeans_tiles(n, KMEANS_SEED_ROWS);
  w.split = kmeans_split(n, k, d);
  w.colsum = 0;
  w.mean = w.colsum + kmeans_up4(2 * (int64_t)w.split.nchunks * d);
  w.cnorm = w.mean + kmeans_up4(d);
  w.part_inertia = w.cnorm + kmeans_up4(k);
  w.part_changed = w.part_inertia + kmeans_up4(2 * (int64_t)w.nwg_assign);
  w.part_sum = w.part_changed + kmeans_up4(w.nwg_assign);
  w.part_cnt = w.part_sum + kmeans_up4(2 * (int64_t)w.split.P * k * d);
  w.d2 = w.part_cnt + kmeans_up4((int64_t)w.split.P * k);
  w.blocksum = w.d2 + kmeans_up4(n);
  w.picks = w.blocksum + kmeans_up4(2 * (int64_t)w.nb_seed);
  w.labels2 = w.picks + kmeans_up4(k);
  w.result = w.labels2 + kmeans_up4(n);
  w.floats = w.result + 4;
  return w;
}

static inline std::string kmeans_check_workspace(int n, int d, int k, const int64_t *floats) {
  std::string e = kmeans_check_shape(n, d, k);
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string kmeans_check_assign(const float *x, int n, int d, int64_t ldx, const float *centroids, int k, const int32_t *labels,
                                              const double *inertia, const float *workspace) {
  const std::string e = kmeans_check_x(n, d, k, ldx);
  if (!e.empty()) return e;
  if (!x || !centroids || !labels || !inertia || !workspace) return "null argument";
  if (!pca_al16(workspace)) return kmeans_misaligned();
  return "";
}

static inline std::string kmeans_check_update(const float *x, int n, int d, int64_t ldx, const int32_t *labels, int k, const float *centroids,
                                              const int32_t *counts, const float *workspace) {
  const std::string e = kmeans_check_x(n, d, k, ldx);
  if (!e.empty()) return e;
  if (!x || !labels || !centroids || !counts || !workspace) return "null argument";
  if (!pca_al16(workspace)) return kmeans_misaligned();
  return "";
}

static inline std::string kmeans_check_seed(const float *x, int n, int d, int64_t ldx, int k, const double *u, const float *centroids, const int32_t *index,
                                            const float *workspace) {
  const std::string e = kmeans_check_x(n, d, k, ldx);
  if (!e.empty()) return e;
  if (!x || !u || !centroids || !index || !workspace) return "null argument";
  if (!pca_al16(workspace)) return kmeans_misaligned();
  for (int j = 0; j < k; j++)
    if (!(u[j] >= 0.0) || !(u[j] < 1.0)) return "u[" + std::to_string(j) + "] = " + std::to_string(u[j]) + " is not a uniform in [0, 1)";
  return "";
}

static inline std::string kmeans_check_fit(const float *x, int n, int d, int64_t ldx, int k, const float *centroids, const int32_t *labels, int max_iter,
                                           double tol, const tmjx_kmeans_info_t *info, const float *workspace) {
  const std::string e = kmeans_check_x(n, d, k, ldx);
  if (!e.empty()) return e;
  if (!x || !centroids || !labels || !info || !workspace) return "null argument";
  if (!pca_al16(workspace)) return kmeans_misaligned();
  if (max_iter < 1) return "max_iter must be >= 1 (got " + std::to_string(max_iter) + ")";
  if (!(tol >= 0.0)) return "tol must be >= 0 (got " + std::to_string(tol) + ")";
  return "";
}

// the stopping rule of the Lloyd loop after the assign of iteration `it` (0-based): no label changed, or the inertia fell by no more than
// tol x the previous one
static inline bool kmeans_converged(int it, int changed, double inertia, double previous, double tol) {
  if (changed == 0) return true;
  return it > 0 && previous - inertia <= tol * previous;
}

}  // namespace tmjx_host
