// csrc/tsne_host.h — the host side the behaviour-map entry points share with the host emulation (tests/hostemu/tsne_emu.cpp): the argument checks
// (an empty string: accepted) and the workspace layout.
#pragma once
#include "tsne_core.h"
#include "kmeans_host.h"

namespace tmjx_host {

static inline std::string tsne_misaligned() { return "the workspace must be a 16-byte aligned device buffer of tmjx_tsne_workspace's size"; }
static inline std::string tsne_check_n(int n) {
  if (n < 2) return "n must be >= 2 (got " + std::to_string(n) + ")";
  if (n > TSNE_MAX_N) return "n = " + std::to_string(n) + " exceeds the behaviour map's limit of " + std::to_string(TSNE_MAX_N) + " reference rows";
  return "";
}
static inline std::string tsne_check_k(int k) {
  if (k < 1) return "k must be >= 1 (got " + std::to_string(k) + ")";
  if (k > TSNE_MAX_K) return "k = " + std::to_string(k) + " exceeds the behaviour map's limit of " + std::to_string(TSNE_MAX_K) + " neighbours";
  return "";
}
static inline std::string tsne_check_shape(int n, int64_t m, int d, int k) {
  std::string e = tsne_check_n(n);
  if (!e.empty()) return e;
  if (m < 1) return "m must be >= 1 (got " + std::to_string((long long)m) + ")";
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > TSNE_MAX_D) return "d = " + std::to_string(d) + " exceeds the behaviour map's limit of " + std::to_string(TSNE_MAX_D) + " features";
  return tsne_check_k(k);
}

// one workspace for every call, in floats (every part starts at a multiple of 4 floats).  What the gradient, the update and the fit take depends
// on n only and comes first, so that a workspace sized for (n, m, d, k) serves them too:
//   row_ptr [n + 1] int | [P][n][3] float64 parts of the repulsion | rep [n][2] float64 | [blocks] float64 Z | [blocks] float64 kl |
//   [blocks][2] float64 column sums of y | the fit's grad [n][2] | the fit's {Z, kl} read-back |
//   [chunks of 256 rows][d] float64 column sums of x | mean [d] | xnorm [n] | qnorm [m]
// P blocks <= 1024 + blocks: nothing scales with n n or m n.
struct TsneWorkspace {
  TsneSplit split;
  int nb, nchunks;
  int64_t row_ptr, parts, rep, zblock, klblock, ysum, grad, result, colsum, mean, xnorm, qnorm, floats;
};
static inline TsneWorkspace tsne_workspace(int n, int64_t m, int d, int k) {
  (void)k;
  TsneWorkspace w;
  w.split = tsne_split(n);
  w.nb = w.split.tiles;
  w.nchunks = pca_nwg(n);
  w.row_ptr = 0;
  w.parts = w.row_ptr + kmeans_up4((int64_t)n + 1);
  w.rep = w.parts + kmeans_up4(2 * 3 * (int64_t)w.split.P * n);
  w.zblock = w.rep + kmeans_up4(2 * 2 * (int64_t)n);
  w.klblock = w.zblock + kmeans_up4(2 * (int64_t)w.nb);
  w.ysum = w.klblock + kmeans_up4(2 * (int64_t)w.nb);
  w.grad = w.ysum + kmeans_up4(4 * (int64_t)w.nb);
  w.result = w.grad + kmeans_up4(2 * (int64_t)n);
  w.colsum = w.result + 4;
  w.mean = w.colsum + kmeans_up4(2 * (int64_t)w.nchunks * d);
  w.xnorm = w.mean + kmeans_up4(d);
  w.qnorm = w.xnorm + kmeans_up4(n);
  w.floats = w.qnorm + kmeans_up4(m);
  return w;
}
// the bytes of LDS a search workgroup takes: the stage, then the k best of its 128 queries (float32 distances, 16-bit indices)
static inline size_t tsne_knn_lds(int k) { return sizeof(float) * TSNE_STAGE + (size_t)k * TSNE_ROWS * (sizeof(float) + sizeof(uint16_t)); }

static inline std::string tsne_check_workspace(int n, int64_t m, int d, int k, const int64_t *floats) {
  std::string e = tsne_check_shape(n, m, d, k);
  if (e.empty() && !floats) e = "null argument";
  return e;
}

// whether row i is left out of query i's list: only a search of x against itself
static inline bool tsne_knn_self(const float *x, int n, int64_t ldx, const float *q, int64_t m, int64_t ldq, int exclude_self) {
  return exclude_self && q == x && m == n && ldq == ldx;
}

static inline std::string tsne_check_knn(const float *x, int n, int d, int64_t ldx, const float *q, int64_t m, int64_t ldq, int exclude_self, int k,
                                         const int32_t *idx, const float *dist2, const float *workspace) {
  std::string e = tsne_check_shape(n, m, d, k);
  if (!e.empty()) return e;
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  if (ldq < d) return "ldq = " + std::to_string((long long)ldq) + " is smaller than d = " + std::to_string(d);
  if (!x || !q || !idx || !dist2 || !workspace) return "null argument";
  const int have = n - (tsne_knn_self(x, n, ldx, q, m, ldq, exclude_self) ? 1 : 0);
  if (k > have) return "k = " + std::to_string(k) + " neighbours asked of " + std::to_string(have) + " candidate rows (k <= n, and k <= n - 1 without self)";
  if (!pca_al16(workspace)) return tsne_misaligned();
  if (((uintptr_t)x | (uintptr_t)q | (uintptr_t)idx | (uintptr_t)dist2) & 3) return "x, q, idx and dist2 must be 4-byte aligned";
  return "";
}

static inline std::string tsne_check_affinities(const float *dist2, int64_t m, int k, double perplexity, const float *p, const float *beta) {
  if (m < 1) return "m must be >= 1 (got " + std::to_string((long long)m) + ")";
  std::string e = tsne_check_k(k);
  if (!e.empty()) return e;
  if (!(perplexity >= 1.0)) return "perplexity must be >= 1 (got " + std::to_string(perplexity) + ")";
  if (!(perplexity < (double)k)) return "perplexity = " + std::to_string(perplexity) + " must be below k = " + std::to_string(k) + " neighbours";
  if (!dist2 || !p || !beta) return "null argument";
  if (((uintptr_t)dist2 | (uintptr_t)p | (uintptr_t)beta) & 3) return "dist2, p and beta must be 4-byte aligned";
  return "";
}

// row_ptr is a HOST array: row_ptr[0] = 0, non-decreasing, row_ptr[n] = nnz
static inline std::string tsne_check_csr(int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz) {
  if (!row_ptr) return "null argument";
  if (nnz < 0 || nnz > 2 * (int64_t)TSNE_MAX_N * TSNE_MAX_K) return "nnz = " + std::to_string((long long)nnz) + " is outside 0 .. 2 n k at the limits";
  if (row_ptr[0] != 0) return "row_ptr[0] must be 0 (got " + std::to_string(row_ptr[0]) + ")";
  for (int i = 0; i < n; i++)
    if (row_ptr[i + 1] < row_ptr[i]) return "row_ptr decreases at row " + std::to_string(i);
  if (row_ptr[n] != nnz) return "row_ptr[n] = " + std::to_string(row_ptr[n]) + " disagrees with nnz = " + std::to_string((long long)nnz);
  if (nnz > 0 && (!col || !val)) return "null argument";
  if (((uintptr_t)col | (uintptr_t)val) & 3) return "col and val must be 4-byte aligned";
  return "";
}

static inline std::string tsne_check_gradient(const float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz,
                                              double exaggeration, const float *grad, const double *z, const double *kl, const float *workspace) {
  std::string e = tsne_check_n(n);
  if (!e.empty()) return e;
  if (!y || !grad || !z || !kl || !workspace) return "null argument";
  if (!(e = tsne_check_csr(n, row_ptr, col, val, nnz)).empty()) return e;
  if (!(exaggeration > 0.0) || !(exaggeration < 1e30)) return "exaggeration must be positive and finite (got " + std::to_string(exaggeration) + ")";
  if (!pca_al16(workspace)) return tsne_misaligned();
  if (((uintptr_t)y | (uintptr_t)grad) & 7 || ((uintptr_t)z | (uintptr_t)kl) & 7) return "y, grad, z and kl must be 8-byte aligned";
  return "";
}

static inline std::string tsne_check_step(float momentum, float eta, float min_gain) {
  if (!(momentum >= 0.f) || !(momentum < 1.f)) return "momentum must be in [0, 1) (got " + std::to_string(momentum) + ")";
  if (!(eta > 0.f) || !(eta < 1e30f)) return "eta must be positive and finite (got " + std::to_string(eta) + ")";
  if (!(min_gain >= 0.f) || !(min_gain < 1e30f)) return "min_gain must be >= 0 and finite (got " + std::to_string(min_gain) + ")";
  return "";
}

static inline std::string tsne_check_update(const float *y, const float *grad, const float *velocity, const float *gains, int n, float momentum, float eta,
                                            float min_gain, const float *workspace) {
  std::string e = tsne_check_n(n);
  if (!e.empty()) return e;
  if (!y || !grad || !velocity || !gains || !workspace) return "null argument";
  if (!(e = tsne_check_step(momentum, eta, min_gain)).empty()) return e;
  if (!pca_al16(workspace)) return tsne_misaligned();
  if (((uintptr_t)y | (uintptr_t)grad | (uintptr_t)velocity | (uintptr_t)gains) & 7) return "y, grad, velocity and gains must be 8-byte aligned";
  return "";
}

static inline std::string tsne_check_fit(const float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz, int n_iter,
                                         double exaggeration, int exaggeration_iters, float momentum_early, float momentum_late, float eta, float min_gain,
                                         const float *velocity, const float *gains, const tmjx_tsne_info_t *info, const float *workspace) {
  std::string e = tsne_check_n(n);
  if (!e.empty()) return e;
  if (!y || !velocity || !gains || !info || !workspace) return "null argument";
  if (!(e = tsne_check_csr(n, row_ptr, col, val, nnz)).empty()) return e;
  if (n_iter < 0 || n_iter > 100000) return "n_iter must be in 0 .. 100000 (got " + std::to_string(n_iter) + ")";
  if (exaggeration_iters < 0) return "exaggeration_iters must be >= 0 (got " + std::to_string(exaggeration_iters) + ")";
  if (!(exaggeration > 0.0) || !(exaggeration < 1e30)) return "exaggeration must be positive and finite (got " + std::to_string(exaggeration) + ")";
  if (!(e = tsne_check_step(momentum_early, eta, min_gain)).empty()) return e;
  if (!(e = tsne_check_step(momentum_late, eta, min_gain)).empty()) return e;
  if (!pca_al16(workspace)) return tsne_misaligned();
  if (((uintptr_t)y | (uintptr_t)velocity | (uintptr_t)gains) & 7) return "y, velocity and gains must be 8-byte aligned";
  return "";
}

static inline std::string tsne_check_place(const int32_t *idx, const float *p, int64_t m, int k, const float *y_train, int n, const float *y_out) {
  if (m < 1) return "m must be >= 1 (got " + std::to_string((long long)m) + ")";
  std::string e = tsne_check_k(k);
  if (e.empty()) e = tsne_check_n(n);
  if (!e.empty()) return e;
  if (!idx || !p || !y_train || !y_out) return "null argument";
  if (((uintptr_t)idx | (uintptr_t)p | (uintptr_t)y_train | (uintptr_t)y_out) & 3) return "idx, p, y_train and y_out must be 4-byte aligned";
  return "";
}

// the exaggeration and the momentum of iteration `it` (0-based) of a fit
static inline double tsne_exaggeration_at(int it, double exaggeration, int exaggeration_iters) { return it < exaggeration_iters ? exaggeration : 1.0; }
static inline float tsne_momentum_at(int it, int exaggeration_iters, float early, float late) { return it < exaggeration_iters ? early : late; }

}  // namespace tmjx_host
