// csrc/tmjx_pca_wide.hip — PCA of features 129 .. 1024 wide (include/tmjx.h: tmjx_pca_wide_workspace, tmjx_pca_fit_wide, tmjx_pca_transform_wide;
// DESIGN.md "PCA", wide fit).  The bodies are csrc/pca_wide_core.h (they also compile on the host); the argument checks csrc/pca_wide_host.h.
//   k_moments_colsum, k_moments_mean   the column mean by super-chunk (csrc/moments_core.h)
//   k_pcaw_gram    one workgroup per (128 x 128 tile with j >= i, super-chunk)           k_pcaw_cov    the partials added in order, mirrored; V^T = I
//   k_pcaw_rownorm, k_pcaw_norms   ||A||_F^2 and off(A)^2 in float64, fixed order
//   k_pcaw_solve   one workgroup per pair of blocks: gathers the sub-matrix, pca_jacobi_wg in LDS
//   k_pcaw_rows    J A and J V^T, the pair's rows over 64 columns per workgroup           k_pcaw_cols   A J^T, the pair's columns over 64 rows
//   k_pcaw_finish  ranking, normalisation and sign of every row                           k_pcaw_transform
// A round of the block iteration is solve -> rows -> cols in stream order: a pass reads nothing another workgroup of the same launch writes.
// The GEMMs are plain float32 FMAs: the inner solves take most of the fit (profiles/pca_wide_bench.txt).  d <= 128 forwards to csrc/tmjx_pca.hip.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "pca_wide_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
// blockIdx.x: the upper-triangle tile, row by row; blockIdx.y: the super-chunk
__global__ __launch_bounds__(PCA_THREADS) void k_pcaw_gram(const float *__restrict__ x, int64_t ldx, int n, int d, const float *__restrict__ mean,
                                                           double *__restrict__ partial) {
  __shared__ float s_tile[2 * PCA_KB * PCA_WIDE_TILE];
  const int nt = pca_wide_tiles(d);
  int ti = 0, t = blockIdx.x;
  while (t >= nt - ti) { t -= nt - ti; ti++; }
  pca_wide_gram_wg(x, ldx, n, d, mean, ti, ti + t, blockIdx.y, partial, s_tile);
}

__global__ __launch_bounds__(PCA_THREADS) void k_pcaw_cov(const double *__restrict__ partial, int S, int d, int n, float *__restrict__ cov,
                                                          float *__restrict__ vt) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e >= d * d) return;
  const int i = e / d, j = e % d;
  cov[e] = pca_wide_gram_reduce(partial, S, d, n, i, j);
  vt[e] = i == j ? 1.f : 0.f;
}

__global__ __launch_bounds__(PCA_THREADS) void k_pcaw_rownorm(const float *__restrict__ A, int d, double *__restrict__ rowsum) {
  __shared__ double s_red[2 * PCA_THREADS];
  pca_wide_rownorm_wg(A, d, blockIdx.x, rowsum, s_red);
}

__global__ __launch_bounds__(64) void k_pcaw_norms(const double *__restrict__ rowsum, int d, double *__restrict__ norms) {
  if (threadIdx.x < 2) norms[threadIdx.x] = pca_wide_norm_total(rowsum, d, threadIdx.x);
}

__global__ __launch_bounds__(1024) void k_pcaw_solve(const float *A, int d, int r, float *sub, float *J, float *lam, PcaInfo *info) {
  extern __shared__ __align__(16) float s_solve[];
  pca_wide_solve_wg(A, d, r, blockIdx.x, sub, J, lam, info, s_solve, blockDim.x);
}

// blockIdx.x: the 64-column slice; blockIdx.y: the pair; blockIdx.z: 0 = A, 1 = V^T
__global__ __launch_bounds__(PCA_THREADS) void k_pcaw_rows(float *A, float *Vt, int d, int r, const float *__restrict__ J) {
  __shared__ float s_a[PCA_KB * PCA_WIDE_LDA], s_b[PCA_KB * PCA_WIDE_LDB];
  pca_wide_rows_wg(blockIdx.z ? Vt : A, d, r, blockIdx.y, J, blockIdx.x * PCA_WIDE_PASS, s_a, s_b);
}

// blockIdx.x: the 64-row slice; blockIdx.y: the pair
__global__ __launch_bounds__(PCA_THREADS) void k_pcaw_cols(float *A, int d, int r, const float *__restrict__ J, const float *__restrict__ lam) {
  __shared__ float s_a[PCA_KB * PCA_WIDE_LDA], s_b[PCA_KB * PCA_WIDE_LDB];
  pca_wide_cols_wg(A, d, r, blockIdx.y, J, lam, blockIdx.x * PCA_WIDE_PASS, s_a, s_b);
}

__global__ __launch_bounds__(64) void k_pcaw_finish(const float *__restrict__ A, const float *__restrict__ Vt, int d, float *__restrict__ components,
                                                    float *__restrict__ variance) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < d) pca_wide_finish_row(A, Vt, d, i, components, variance);
}

// blockIdx.x: 64 rows; blockIdx.y: 16 NC components
template <int NC>
__global__ __launch_bounds__(PCA_THREADS) void k_pcaw_transform(const float *__restrict__ x, int n, int d, int64_t ldx, const float *__restrict__ mean,
                                                                const float *__restrict__ components, int k, float *__restrict__ out, int64_t ldo) {
  __shared__ float s_x[PCA_WIDE_TK * PCA_WIDE_TLD], s_c[PCA_WIDE_TK * PCA_WIDE_TLD];
  pca_wide_transform_wg<NC>(x, n, d, ldx, mean, components, k, out, ldo, blockIdx.x * PCA_TROWS, blockIdx.y * 16 * NC, s_x, s_c);
}

// ----------------------------------------------------------------------------------------------- launches
struct WideFit {
  const float *x; int n, d; int64_t ldx; float *mean, *components, *variance, *workspace; tmjx_pca_info_t *info; hipStream_t s;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

// ||A||_F^2 and off(A)^2 into norms[2]; the call waits for the stream
static int wide_norms(const WideFit &f, const PcaWideWorkspace &w, double *norms) {
  float *ws = f.workspace;
  hipLaunchKernelGGL(k_pcaw_rownorm, dim3(f.d), dim3(PCA_THREADS), 0, f.s, ws + w.cov, f.d, (double *)(ws + w.rowsum));
  hipLaunchKernelGGL(k_pcaw_norms, dim3(1), dim3(64), 0, f.s, (const double *)(ws + w.rowsum), f.d, (double *)(ws + w.norms));
  int rc = check_launch("tmjx_pca_fit_wide (norms)");
  if (rc) return rc;
  TM_HIP("hipMemcpyAsync(norms, ws + w.norms, 2 * sizeof(double), hipMemcpyDeviceToHost, f.s)", hipMemcpyAsync(norms, ws + w.norms, 2 * sizeof(double), hipMemcpyDeviceToHost, f.s));
  TM_HIP("hipStreamSynchronize(f.s)", hipStreamSynchronize(f.s));
  return TMJX_OK;
}

static int wide_fit(WideFit &f) {
  const int n = f.n, d = f.d;
  const PcaWideWorkspace w = pca_wide_workspace(n, d);
  float *ws = f.workspace;
  double *colsum = (double *)(ws + w.colsum), *gram = (double *)(ws + w.gram);
  float *A = ws + w.cov, *Vt = ws + w.vt, *sub = ws + w.sub, *J = ws + w.rot, *lam = ws + w.lam;
  PcaInfo *pinfo = (PcaInfo *)(ws + w.info);
  const int tiles = pca_wide_tiles(d), S = w.split.S;
  TM_HIP("hipEventRecord(f.ev[0], f.s)", hipEventRecord(f.ev[0], f.s));
  moments_launch_mean<false>(f.x, f.ldx, n, d, colsum, f.mean, f.s);
  hipLaunchKernelGGL(k_pcaw_gram, dim3(tiles * (tiles + 1) / 2, S), dim3(PCA_THREADS), 0, f.s, f.x, f.ldx, n, d, f.mean, gram);
  hipLaunchKernelGGL(k_pcaw_cov, dim3((d * d + PCA_THREADS - 1) / PCA_THREADS), dim3(PCA_THREADS), 0, f.s, gram, S, d, n, A, Vt);
  int rc = check_launch("tmjx_pca_fit_wide (moments)");
  if (rc) return rc;
  double norms[2] = {0.0, 0.0};
  if ((rc = wide_norms(f, w, norms))) return rc;
  TM_HIP("hipEventRecord(f.ev[1], f.s)", hipEventRecord(f.ev[1], f.s));
  if (!pca_wide_finite(norms)) return fail(TMJX_EINVAL, pca_wide_nonfinite_message());      // before any rotation launch
  const int players = pca_wide_players(d), slices = (d + PCA_WIDE_PASS - 1) / PCA_WIDE_PASS;
  const size_t lds = sizeof(float) * pca_jacobi_lds_floats(PCA_MAX_D);      // (beyond 64 KiB)
  int sweeps = 0;
  bool converged = pca_wide_converged(norms);
  while (!converged && sweeps < PCA_SWEEP_LIMIT) {
    for (int r = 0; r < players - 1; r++) {
      if ((rc = launch_lds<k_pcaw_solve>("k_pcaw_solve", dim3(w.pairs), dim3(1024), lds, lds, f.s, A, d, r, sub, J, lam, pinfo))) return rc;
      hipLaunchKernelGGL(k_pcaw_rows, dim3(slices, w.pairs, 2), dim3(PCA_THREADS), 0, f.s, A, Vt, d, r, J);
      hipLaunchKernelGGL(k_pcaw_cols, dim3(slices, w.pairs), dim3(PCA_THREADS), 0, f.s, A, d, r, J, lam);
    }
    if ((rc = check_launch("tmjx_pca_fit_wide (block sweep)"))) return rc;
    sweeps++;
    if ((rc = wide_norms(f, w, norms))) return rc;
    if (!pca_wide_finite(norms)) break;
    converged = pca_wide_converged(norms);
  }
  hipLaunchKernelGGL(k_pcaw_finish, dim3((d + 63) / 64), dim3(64), 0, f.s, A, Vt, d, f.components, f.variance);
  TM_HIP("hipEventRecord(f.ev[2], f.s)", hipEventRecord(f.ev[2], f.s));
  if ((rc = check_launch("tmjx_pca_fit_wide (finish)"))) return rc;
  TM_HIP("hipStreamSynchronize(f.s)", hipStreamSynchronize(f.s));
  f.info->sweeps = sweeps; f.info->converged = converged ? 1 : 0; f.info->off_rel = pca_wide_off_rel(norms);
  hipEventElapsedTime(&f.info->moments_ms, f.ev[0], f.ev[1]);
  hipEventElapsedTime(&f.info->jacobi_ms, f.ev[1], f.ev[2]);
  if (!converged) return fail(TMJX_ENOCONV, pca_wide_noconv_message(sweeps, f.info->off_rel));
  return TMJX_OK;
}

extern "C" {

int tmjx_pca_wide_workspace(int n, int d, int64_t *floats) {
  if (d >= 1 && d <= PCA_MAX_D) return tmjx_pca_workspace(n, d, floats);
  if (!floats) return fail(TMJX_EINVAL, "null argument");
  TM_TRY(pca_wide_check_shape(n, d, d));
  *floats = pca_wide_workspace(n, d).floats;
  return TMJX_OK;
}

int tmjx_pca_fit_wide(const float *x, int n, int d, int64_t ldx, float *mean, float *components, float *variance, float *workspace, tmjx_pca_info_t *info,
                      void *stream) {
  if (d >= 1 && d <= PCA_MAX_D) return tmjx_pca_fit(x, n, d, ldx, mean, components, variance, workspace, info, stream);
  TM_TRY(pca_wide_check_fit(x, n, d, ldx, mean, components, variance, workspace, info));
  WideFit f{x, n, d, ldx, mean, components, variance, workspace, info, (hipStream_t)stream};
  for (int i = 0; i < 3; i++) {
    hipError_t e = hipEventCreate(&f.ev[i]);
    if (e != hipSuccess) {
      for (int j = 0; j < i; j++) hipEventDestroy(f.ev[j]);
      return fail(TMJX_EHIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
    }
  }
  info->sweeps = info->converged = 0;
  info->off_rel = info->moments_ms = info->jacobi_ms = 0.f;
  const int rc = wide_fit(f);
  for (int i = 0; i < 3; i++) hipEventDestroy(f.ev[i]);
  return rc;
}

int tmjx_pca_transform_wide(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, float *out, int64_t ldo,
                            void *stream) {
  if (d >= 1 && d <= PCA_MAX_D) return tmjx_pca_transform(x, n, d, ldx, mean, components, k, out, ldo, stream);
  TM_TRY(pca_wide_check_transform(x, n, d, ldx, mean, components, k, out, ldo));
  const unsigned row_groups = (unsigned)((n + PCA_TROWS - 1) / PCA_TROWS);
  if (k <= 16)
    hipLaunchKernelGGL(k_pcaw_transform<1>, dim3(row_groups, 1), dim3(PCA_THREADS), 0, (hipStream_t)stream, x, n, d, ldx, mean, components, k, out, ldo);
  else
    hipLaunchKernelGGL(k_pcaw_transform<4>, dim3(row_groups, (k + 63) / 64), dim3(PCA_THREADS), 0, (hipStream_t)stream, x, n, d, ldx, mean, components, k, out, ldo);
  return check_launch("k_pcaw_transform");
}

}  // extern "C"
