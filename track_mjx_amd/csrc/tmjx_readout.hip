// csrc/tmjx_readout.hip — the linear readout: ridge regression from recorded activations (include/tmjx.h: tmjx_readout_workspace, tmjx_readout_fit,
// tmjx_readout_weights, tmjx_readout_predict, tmjx_readout_score; DESIGN.md "Readout").  The bodies are csrc/readout_core.h (they also compile on the
// host); the argument checks and workspace layouts csrc/readout_host.h.  The eigen-decomposition is tmjx_pca_fit_wide's, called as it is.
//   k_moments_colsum, k_moments_mean   the column mean of y by super-chunk (csrc/moments_core.h)
//   k_ro_cross    one workgroup per (128 features x 64 targets, super-chunk)                  k_ro_c        the partials added in order, over n - 1
//   k_ro_gemm<0>  Z = components . C                                                           k_ro_gemm<1>  W_l = components^T diag(1 / (s + lambda_l)) Z, every l
//   k_ro_apply<0> predictions, 64 rows x 64 targets per workgroup                              k_ro_apply<1> the fused score: 256 rows x 64 of the L m columns
//   k_ro_sst      centred sums of squares of y' by the column-sum split                        k_ro_totals   sse and sst: the partials added in order
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "readout_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
// blockIdx.x: the feature tile; blockIdx.y: the target tile; blockIdx.z: the super-chunk
__global__ __launch_bounds__(PCA_THREADS) void k_ro_cross(const float *__restrict__ x, int64_t ldx, const float *__restrict__ y, int64_t ldy, int n, int d, int m,
                                                          const float *__restrict__ mean_x, const float *__restrict__ mean_y, double *__restrict__ partial) {
  __shared__ float s_x[PCA_KB * PCA_WIDE_TILE], s_y[PCA_KB * READOUT_TILE_M];
  readout_cross_wg(x, ldx, y, ldy, n, d, m, mean_x, mean_y, blockIdx.x, blockIdx.y, blockIdx.z, partial, s_x, s_y);
}

__global__ __launch_bounds__(PCA_THREADS) void k_ro_c(const double *__restrict__ partial, int S, int d, int m, int n, float *__restrict__ c) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < d * m) c[e] = readout_cross_reduce(partial, S, d, m, n, e);
}

// blockIdx.x: 64 rows of the output; blockIdx.y: 64 columns; blockIdx.z: the penalty (TA only)
template <bool TA>
__global__ __launch_bounds__(PCA_THREADS) void k_ro_gemm(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ variance,
                                                         ReadoutLambdas lam, int d, int m, float *__restrict__ out) {
  __shared__ float s_a[PCA_KB * READOUT_LD], s_b[PCA_KB * READOUT_LD];
  readout_gemm_wg<TA>(a, b, TA ? variance : nullptr, lam.v[blockIdx.z], d, m, out + (int64_t)blockIdx.z * d * m, blockIdx.x * READOUT_TILE,
                      blockIdx.y * READOUT_TILE, s_a, s_b);
}

// blockIdx.x: the row block (64 rows, or 256 for the score); blockIdx.y: 64 of the output columns
template <bool SCORE>
__global__ __launch_bounds__(PCA_THREADS) void k_ro_apply(const float *__restrict__ x, int n, int d, int64_t ldx, const float *__restrict__ mean_x,
                                                          const float *__restrict__ w, int m, int Q, const float *__restrict__ mean_y,
                                                          const float *__restrict__ y, int64_t ldy, float *__restrict__ out, int64_t ldo,
                                                          double *__restrict__ partial) {
  __shared__ float s_x[PCA_WIDE_TK * READOUT_LD], s_w[PCA_WIDE_TK * READOUT_LD];
  __shared__ double s_red[SCORE ? 16 * READOUT_TILE : 1];
  const int nsub = SCORE ? READOUT_SCORE_SUB : 1;
  readout_apply_wg<SCORE>(x, n, d, ldx, mean_x, w, m, Q, mean_y, y, ldy, out, ldo, partial, (int64_t)blockIdx.x * READOUT_ROWS * nsub, nsub,
                          blockIdx.y * READOUT_TILE, s_x, s_w, s_red);
}

__global__ __launch_bounds__(PCA_THREADS) void k_ro_sst(const float *__restrict__ y, int64_t ldy, int n, int m, const double *__restrict__ colsum,
                                                        double *__restrict__ partial) {
  __shared__ double s_sum[2 * PCA_WIDE_TILE];
  readout_sst_wg(y, ldy, n, m, blockIdx.y, blockIdx.x, colsum, partial, s_sum);
}

// threads [0, Q): sse; threads [Q, Q + m): sst
__global__ __launch_bounds__(PCA_THREADS) void k_ro_totals(const double *__restrict__ sse_partial, int nblocks, int Q, const double *__restrict__ sst_partial,
                                                           int S, int m, double *__restrict__ sse, double *__restrict__ sst) {
  const int t = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (t < Q) sse[t] = readout_sse_col(sse_partial, nblocks, Q, t);
  else if (t < Q + m) sst[t - Q] = readout_sst_col(sst_partial, S, m, t - Q);
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_readout_workspace(int n, int d, int m, int n_lambda, int64_t *floats) {
  TM_TRY(readout_check_workspace(n, d, m, n_lambda, floats));
  int64_t pca = 0, pca_widest = 0;
  int rc = tmjx_pca_wide_workspace(n, d, &pca);
  if (!rc) rc = tmjx_pca_wide_workspace(readout_widest_rows(n), d, &pca_widest);
  if (rc) return rc;
  *floats = readout_workspace_floats(n, d, m, n_lambda, pca, pca_widest);
  return TMJX_OK;
}

int tmjx_readout_fit(const float *x, int n, int d, int64_t ldx, const float *y, int m, int64_t ldy, float *mean_x, float *components, float *variance,
                     float *mean_y, float *z, float *workspace, tmjx_pca_info_t *info, void *stream) {
  TM_TRY(readout_check_fit(x, n, d, ldx, y, m, ldy, mean_x, components, variance, mean_y, z, workspace, info));
  int64_t pca = 0;
  int rc = tmjx_pca_wide_workspace(n, d, &pca);
  if (rc) return rc;
  if ((rc = tmjx_pca_fit_wide(x, n, d, ldx, mean_x, components, variance, workspace, info, stream))) return rc;      // (it has waited for the stream)
  const ReadoutFitWorkspace w = readout_fit_workspace(n, d, m, pca);
  hipStream_t s = (hipStream_t)stream;
  double *ysum = (double *)(workspace + w.ysum), *cross = (double *)(workspace + w.cross);
  float *c = workspace + w.c;
  const int S = w.split.S;
  moments_launch_mean<false>(y, ldy, n, m, ysum, mean_y, s);
  hipLaunchKernelGGL(k_ro_cross, dim3(pca_wide_tiles(d), readout_tiles(m, READOUT_TILE_M), S), dim3(PCA_THREADS), 0, s, x, ldx, y, ldy, n, d, m, mean_x, mean_y,
                     cross);
  hipLaunchKernelGGL(k_ro_c, dim3(readout_tiles(d * m, PCA_THREADS)), dim3(PCA_THREADS), 0, s, cross, S, d, m, n, c);
  hipLaunchKernelGGL(k_ro_gemm<false>, dim3(readout_tiles(d, READOUT_TILE), readout_tiles(m, READOUT_TILE), 1), dim3(PCA_THREADS), 0, s, components, c,
                     (const float *)nullptr, ReadoutLambdas{}, d, m, z);
  if ((rc = check_launch("tmjx_readout_fit"))) return rc;
  hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(TMJX_EHIP, std::string("tmjx_readout_fit: ") + hipGetErrorString(e));
  return TMJX_OK;
}

int tmjx_readout_weights(const float *components, const float *variance, const float *z, int d, int m, const double *lambdas, int n_lambda, float *w,
                         void *stream) {
  TM_TRY(readout_check_weights(components, variance, z, d, m, lambdas, n_lambda, w));
  ReadoutLambdas lam{};
  for (int i = 0; i < n_lambda; i++) lam.v[i] = (float)lambdas[i];
  hipLaunchKernelGGL(k_ro_gemm<true>, dim3(readout_tiles(d, READOUT_TILE), readout_tiles(m, READOUT_TILE), n_lambda), dim3(PCA_THREADS), 0, (hipStream_t)stream,
                     components, z, variance, lam, d, m, w);
  return check_launch("tmjx_readout_weights");
}

int tmjx_readout_predict(const float *x, int n, int d, int64_t ldx, const float *mean_x, const float *w, const float *mean_y, int m, float *out, int64_t ldo,
                         void *stream) {
  TM_TRY(readout_check_predict(x, n, d, ldx, mean_x, w, mean_y, m, out, ldo));
  hipLaunchKernelGGL(k_ro_apply<false>, dim3(readout_tiles(n, READOUT_ROWS), readout_tiles(m, READOUT_TILE)), dim3(PCA_THREADS), 0, (hipStream_t)stream, x, n, d,
                     ldx, mean_x, w, m, m, mean_y, (const float *)nullptr, (int64_t)0, out, ldo, (double *)nullptr);
  return check_launch("tmjx_readout_predict");
}

int tmjx_readout_score(const float *x, int n, int d, int64_t ldx, const float *y, int m, int64_t ldy, const float *mean_x, const float *w, const float *mean_y,
                       int n_lambda, double *sse, double *sst, float *workspace, void *stream) {
  TM_TRY(readout_check_score(x, n, d, ldx, y, m, ldy, mean_x, w, mean_y, n_lambda, sse, sst, workspace));
  const ReadoutScoreWorkspace ws = readout_score_workspace(n, m, n_lambda);
  hipStream_t s = (hipStream_t)stream;
  double *ysum = (double *)(workspace + ws.ysum), *sstp = (double *)(workspace + ws.sst), *ssep = (double *)(workspace + ws.sse);
  const int S = ws.split.S, Q = n_lambda * m, nblocks = ws.split.nchunks;
  moments_launch_mean<false>(y, ldy, n, m, ysum, nullptr, s);
  hipLaunchKernelGGL(k_ro_sst, dim3(pca_wide_tiles(m), S), dim3(PCA_THREADS), 0, s, y, ldy, n, m, ysum, sstp);
  hipLaunchKernelGGL(k_ro_apply<true>, dim3(nblocks, readout_tiles(Q, READOUT_TILE)), dim3(PCA_THREADS), 0, s, x, n, d, ldx, mean_x, w, m, Q, mean_y, y, ldy,
                     (float *)nullptr, (int64_t)0, ssep);
  hipLaunchKernelGGL(k_ro_totals, dim3(readout_tiles(Q + m, PCA_THREADS)), dim3(PCA_THREADS), 0, s, ssep, nblocks, Q, sstp, S, m, sse, sst);
  return check_launch("tmjx_readout_score");
}

}  // extern "C"
