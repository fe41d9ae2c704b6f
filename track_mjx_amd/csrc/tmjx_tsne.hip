// csrc/tmjx_tsne.hip — the behaviour map of recorded features: exact k nearest neighbours, perplexity-calibrated affinities, the exact t-SNE
// gradient and step, and out-of-sample placement (include/tmjx.h: tmjx_tsne_workspace, tmjx_knn, tmjx_tsne_affinities, tmjx_tsne_gradient,
// tmjx_tsne_update, tmjx_tsne_fit, tmjx_tsne_place; DESIGN.md "Behaviour map").  The bodies are csrc/tsne_core.h (they also compile on the host);
// the argument checks and the workspace layout csrc/tsne_host.h.
//   k_moments_colsum / _mean the column mean of x, as the k-means forms it        k_ts_norms    ||row - mean||^2, one thread per row
//   k_ts_knn      the fused search: 128 queries per workgroup, the k best in LDS    k_ts_affinity the perplexity search, one thread per row
//   k_ts_rep      all-pairs repulsion: (256 points, part of the walk) per workgroup k_ts_rowsum   the parts in part order, Z per block
//   k_ts_attr     the CSR attraction, the gradient and kl per block                 k_ts_kl       kl: the blocks in block order
//   k_ts_update   delta-bar-delta and the blocks' column sums                       k_ts_center   the float64 column mean subtracted
//   k_ts_place    the weighted mean of the neighbours' positions, one thread per query
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "tsne_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(PCA_THREADS) void k_ts_norms(const float *__restrict__ x, int64_t rows, int d, int64_t ldx, const float *__restrict__ mean,
                                                          float *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (r < rows) out[r] = tsne_rownorm(x, ldx, mean, d, r);
}

// Dynamic LDS (tsne_knn_lds(k) bytes): the stage, [k][128] float distances, [k][128] 16-bit indices.  x and q may be the same buffer: no restrict.
__global__ __launch_bounds__(PCA_THREADS) void k_ts_knn(const float *x, int n, int d, int64_t ldx, const float *q, int64_t m, int64_t ldq, int self, int k,
                                                        const float *__restrict__ mean, const float *__restrict__ xnorm, const float *__restrict__ qnorm,
                                                        int32_t *__restrict__ idx, float *__restrict__ dist2) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  float *s_ld = s_dyn + TSNE_STAGE;
  tsne_knn_wg(x, n, d, ldx, q, m, ldq, self, k, mean, xnorm, qnorm, idx, dist2, blockIdx.x, s_dyn, s_ld, (uint16_t *)(s_ld + (size_t)k * TSNE_ROWS));
}

__global__ __launch_bounds__(PCA_THREADS) void k_ts_affinity(const float *__restrict__ dist2, int64_t m, int k, double logu, float *__restrict__ p,
                                                             float *__restrict__ beta) {
  const int64_t i = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (i < m) tsne_affinity_row(dist2, k, logu, p, beta, i);
}

__global__ __launch_bounds__(TSNE_BLOCK) void k_ts_rep(const float *__restrict__ y, int n, TsneSplit sp, double *__restrict__ parts) {
  __shared__ __attribute__((aligned(16))) float s_y[2 * TSNE_BLOCK];
  tsne_rep_wg(y, n, sp, blockIdx.x, blockIdx.y, parts, s_y);
}

__global__ __launch_bounds__(TSNE_BLOCK) void k_ts_rowsum(const double *__restrict__ parts, int n, int P, double *__restrict__ rep, double *__restrict__ zblock) {
  __shared__ double s_z[TSNE_BLOCK];
  tsne_rowsum_wg(parts, n, P, blockIdx.x, rep, zblock, s_z);
}

__global__ __launch_bounds__(TSNE_BLOCK) void k_ts_attr(const float *__restrict__ y, int n, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                        const float *__restrict__ val, double exaggeration, const double *__restrict__ rep,
                                                        const double *__restrict__ zblock, int nb, float *__restrict__ grad, double *__restrict__ z,
                                                        double *__restrict__ klblock) {
  __shared__ double s_kl[TSNE_BLOCK + 1];
  tsne_attr_wg(y, n, row_ptr, col, val, exaggeration, rep, zblock, nb, grad, z, klblock, blockIdx.x, s_kl, s_kl + TSNE_BLOCK);
}

__global__ void k_ts_kl(const double *__restrict__ klblock, int nb, double *__restrict__ kl) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *kl = tsne_total(klblock, nb);
}

__global__ __launch_bounds__(TSNE_BLOCK) void k_ts_update(float *__restrict__ y, const float *__restrict__ grad, float *__restrict__ velocity,
                                                          float *__restrict__ gains, int n, float momentum, float eta, float min_gain,
                                                          double *__restrict__ ysum) {
  __shared__ double s_s[2 * TSNE_BLOCK];
  tsne_update_wg(y, grad, velocity, gains, n, momentum, eta, min_gain, blockIdx.x, ysum, s_s);
}

__global__ __launch_bounds__(TSNE_BLOCK) void k_ts_center(float *__restrict__ y, int n, const double *__restrict__ ysum, int nb) {
  __shared__ double s_m[2];
  tsne_center_wg(y, n, ysum, nb, blockIdx.x, s_m);
}

__global__ __launch_bounds__(PCA_THREADS) void k_ts_place(const int32_t *__restrict__ idx, const float *__restrict__ p, int64_t m, int k,
                                                          const float *__restrict__ y_train, int n, float *__restrict__ y_out) {
  const int64_t i = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (i < m) tsne_place_row(idx, p, k, y_train, n, y_out, i);
}

// ----------------------------------------------------------------------------------------------- launches
static inline unsigned blocks_of(int64_t rows, int per) { return (unsigned)((rows + per - 1) / per); }

// row_ptr must already be in the workspace
static int launch_gradient(const float *y, int n, const int32_t *col, const float *val, double exaggeration, float *grad, double *z, double *kl,
                           float *workspace, const TsneWorkspace &w, hipStream_t s) {
  double *parts = (double *)(workspace + w.parts), *rep = (double *)(workspace + w.rep), *zblock = (double *)(workspace + w.zblock),
         *klblock = (double *)(workspace + w.klblock);
  const int32_t *row_ptr = (const int32_t *)(workspace + w.row_ptr);
  hipLaunchKernelGGL(k_ts_rep, dim3(w.nb, w.split.P), dim3(TSNE_BLOCK), 0, s, y, n, w.split, parts);
  hipLaunchKernelGGL(k_ts_rowsum, dim3(w.nb), dim3(TSNE_BLOCK), 0, s, parts, n, w.split.P, rep, zblock);
  hipLaunchKernelGGL(k_ts_attr, dim3(w.nb), dim3(TSNE_BLOCK), 0, s, y, n, row_ptr, col, val, exaggeration, rep, zblock, w.nb, grad, z, klblock);
  hipLaunchKernelGGL(k_ts_kl, dim3(1), dim3(64), 0, s, klblock, w.nb, kl);
  return check_launch("tmjx_tsne_gradient");
}

static int launch_update(float *y, const float *grad, float *velocity, float *gains, int n, float momentum, float eta, float min_gain, float *workspace,
                         const TsneWorkspace &w, hipStream_t s) {
  double *ysum = (double *)(workspace + w.ysum);
  hipLaunchKernelGGL(k_ts_update, dim3(w.nb), dim3(TSNE_BLOCK), 0, s, y, grad, velocity, gains, n, momentum, eta, min_gain, ysum);
  hipLaunchKernelGGL(k_ts_center, dim3(w.nb), dim3(TSNE_BLOCK), 0, s, y, n, ysum, w.nb);
  return check_launch("tmjx_tsne_update");
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_tsne_workspace(int n, int64_t m, int d, int k, int64_t *floats) {
  TM_TRY(tsne_check_workspace(n, m, d, k, floats));
  *floats = tsne_workspace(n, m, d, k).floats;
  return TMJX_OK;
}

int tmjx_knn(const float *x, int n, int d, int64_t ldx, const float *q, int64_t m, int64_t ldq, int exclude_self, int k, int32_t *idx, float *dist2,
             float *workspace, void *stream) {
  TM_TRY(tsne_check_knn(x, n, d, ldx, q, m, ldq, exclude_self, k, idx, dist2, workspace));
  const TsneWorkspace w = tsne_workspace(n, m, d, k);
  hipStream_t s = (hipStream_t)stream;
  double *colsum = (double *)(workspace + w.colsum);
  float *mean = workspace + w.mean, *xnorm = workspace + w.xnorm, *qnorm = workspace + w.qnorm;
  const int self = tsne_knn_self(x, n, ldx, q, m, ldq, exclude_self) ? 1 : 0;
  moments_launch_mean<true>(x, ldx, n, d, colsum, mean, s);
  hipLaunchKernelGGL(k_ts_norms, dim3(blocks_of(n, PCA_THREADS)), dim3(PCA_THREADS), 0, s, x, (int64_t)n, d, ldx, mean, xnorm);
  hipLaunchKernelGGL(k_ts_norms, dim3(blocks_of(m, PCA_THREADS)), dim3(PCA_THREADS), 0, s, q, m, d, ldq, mean, qnorm);
  int rc = check_launch("tmjx_knn");
  if (rc) return rc;
  return launch_lds<k_ts_knn>("tmjx_knn", dim3(blocks_of(m, TSNE_ROWS)), dim3(PCA_THREADS), tsne_knn_lds(TSNE_MAX_K), tsne_knn_lds(k), s, x, n, d, ldx, q, m, ldq, self, k,
                              mean, xnorm, qnorm, idx, dist2);
}

int tmjx_tsne_affinities(const float *dist2, int64_t m, int k, double perplexity, float *p, float *beta, void *stream) {
  TM_TRY(tsne_check_affinities(dist2, m, k, perplexity, p, beta));
  hipLaunchKernelGGL(k_ts_affinity, dim3(blocks_of(m, PCA_THREADS)), dim3(PCA_THREADS), 0, (hipStream_t)stream, dist2, m, k, log(perplexity), p, beta);
  return check_launch("tmjx_tsne_affinities");
}

int tmjx_tsne_gradient(const float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz, double exaggeration, float *grad,
                       double *z, double *kl, float *workspace, void *stream) {
  TM_TRY(tsne_check_gradient(y, n, row_ptr, col, val, nnz, exaggeration, grad, z, kl, workspace));
  const TsneWorkspace w = tsne_workspace(n, 1, 1, 1);
  hipStream_t s = (hipStream_t)stream;
  TM_HIP("tmjx_tsne_gradient", hipMemcpyAsync(workspace + w.row_ptr, row_ptr, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, s));
  return launch_gradient(y, n, col, val, exaggeration, grad, z, kl, workspace, w, s);
}

int tmjx_tsne_update(float *y, const float *grad, float *velocity, float *gains, int n, float momentum, float eta, float min_gain, float *workspace,
                     void *stream) {
  TM_TRY(tsne_check_update(y, grad, velocity, gains, n, momentum, eta, min_gain, workspace));
  return launch_update(y, grad, velocity, gains, n, momentum, eta, min_gain, workspace, tsne_workspace(n, 1, 1, 1), (hipStream_t)stream);
}

int tmjx_tsne_fit(float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz, int n_iter, double exaggeration,
                  int exaggeration_iters, float momentum_early, float momentum_late, float eta, float min_gain, float *velocity, float *gains,
                  tmjx_tsne_info_t *info, float *workspace, void *stream) {
  TM_TRY(tsne_check_fit(y, n, row_ptr, col, val, nnz, n_iter, exaggeration, exaggeration_iters, momentum_early, momentum_late, eta, min_gain, velocity, gains,
                        info, workspace));
  const TsneWorkspace w = tsne_workspace(n, 1, 1, 1);
  hipStream_t s = (hipStream_t)stream;
  float *grad = workspace + w.grad;
  double *dev = (double *)(workspace + w.result), host[2] = {0.0, 0.0};      // {Z, kl}
  info->n_iter = 0; info->pad_ = 0; info->kl = 0.0; info->z = 0.0; info->gradient_ms = 0.f; info->update_ms = 0.f;
  // one event in front of every gradient and every update, read after the single wait at the end
  std::vector<hipEvent_t> ev;
  auto finish = [&](int code) { for (hipEvent_t e : ev) (void)hipEventDestroy(e); return code; };
  auto mark = [&]() -> int {
    hipEvent_t e;
    TM_HIP("hipEventCreate", hipEventCreate(&e));
    ev.push_back(e);
    TM_HIP("hipEventRecord", hipEventRecord(e, s));
    return TMJX_OK;
  };
  int rc = TMJX_OK;
  hipError_t e = hipMemcpyAsync(workspace + w.row_ptr, row_ptr, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return fail(TMJX_EHIP, std::string("tmjx_tsne_fit: ") + hipGetErrorString(e));
  for (int it = 0; it < n_iter; it++) {
    if ((rc = mark())) return finish(rc);
    if ((rc = launch_gradient(y, n, col, val, tsne_exaggeration_at(it, exaggeration, exaggeration_iters), grad, dev, dev + 1, workspace, w, s))) return finish(rc);
    if ((rc = mark())) return finish(rc);
    if ((rc = launch_update(y, grad, velocity, gains, n, tsne_momentum_at(it, exaggeration_iters, momentum_early, momentum_late), eta, min_gain, workspace, w, s)))
      return finish(rc);
  }
  if ((rc = mark())) return finish(rc);
  if ((rc = launch_gradient(y, n, col, val, 1.0, grad, dev, dev + 1, workspace, w, s))) return finish(rc);
  if ((rc = mark())) return finish(rc);
  e = hipMemcpyAsync(host, dev, sizeof(host), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return finish(fail(TMJX_EHIP, std::string("tmjx_tsne_fit: ") + hipGetErrorString(e)));
  float ms = 0.f;
  for (size_t i = 0; i + 1 < ev.size(); i++)
    if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) (i % 2 == 0 ? info->gradient_ms : info->update_ms) += ms;
  info->n_iter = n_iter;
  info->z = host[0];
  info->kl = host[1];
  return finish(TMJX_OK);
}

int tmjx_tsne_place(const int32_t *idx, const float *p, int64_t m, int k, const float *y_train, int n, float *y_out, void *stream) {
  TM_TRY(tsne_check_place(idx, p, m, k, y_train, n, y_out));
  hipLaunchKernelGGL(k_ts_place, dim3(blocks_of(m, PCA_THREADS)), dim3(PCA_THREADS), 0, (hipStream_t)stream, idx, p, m, k, y_train, n, y_out);
  return check_launch("tmjx_tsne_place");
}

}  // extern "C"
