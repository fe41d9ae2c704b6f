// csrc/tmjx_pca.hip — PCA of recorded activations and the progression panel (include/tmjx.h: tmjx_pca_*, tmjx_plot_strips; DESIGN.md "PCA").
// The bodies are csrc/pca_core.h (they also compile on the host); the argument checks csrc/pca_host.h.  Kernels:
//   k_moments_colsum  (csrc/moments_core.h) one workgroup per PCA_ROWS_PER_WG rows    k_pca_mean    the sums added in workgroup order
//   k_pca_gram    one workgroup per PCA_ROWS_PER_WG rows: the centred partial Gram   k_pca_cov     the partials added in workgroup order, float64
//   k_pca_jacobi  one workgroup: parallel-ordered cyclic Jacobi, A and V in LDS      k_pca_transform, k_plot_strips
// The partial Gram tiles are plain float32 FMAs, not the fp32 MFMA: both run at the same 64 FLOP/clk/SIMD on gfx950, the fit of 210 000 x 128 is
// bounded by the single-workgroup eigen-solver (profiles/pca_bench.txt), and the FMA form is the one the host emulation runs unchanged.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "pca_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(PCA_MAX_D) void k_pca_mean(const double *__restrict__ partial, int nwg, int d, int n, float *__restrict__ mean) {
  if ((int)threadIdx.x < d) mean[threadIdx.x] = pca_mean_col(partial, nwg, d, n, threadIdx.x);
}

template <int NT>
__global__ __launch_bounds__(PCA_THREADS) void k_pca_gram(const float *__restrict__ x, int64_t ldx, int n, int d, const float *__restrict__ mean,
                                                          float *__restrict__ partial) {
  __shared__ float s_tile[PCA_KB * PCA_TILE_LD];
  pca_gram_wg<NT>(x, ldx, n, d, mean, blockIdx.x, partial, s_tile);
}

__global__ __launch_bounds__(PCA_THREADS) void k_pca_cov(const float *__restrict__ partial, int nwg, int d, int n, float *__restrict__ cov) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < d * d) cov[e] = pca_gram_reduce(partial, nwg, d, n, e);
}

__global__ __launch_bounds__(1024) void k_pca_jacobi(const float *__restrict__ cov, int d, float *__restrict__ components, float *__restrict__ variance,
                                                     PcaInfo *info) {
  extern __shared__ __align__(16) float s_jacobi[];
  pca_jacobi_wg(cov, d, components, variance, info, s_jacobi, blockDim.x);
}

// One workgroup per PCA_TROWS rows: the k components, the mean and the centred rows in LDS (row stride d | 1: odd, so that lanes walking different
// rows at the same column touch different banks), then one thread per output.
__global__ __launch_bounds__(PCA_THREADS) void k_pca_transform(const float *__restrict__ x, int n, int d, int64_t ldx, const float *__restrict__ mean,
                                                               const float *__restrict__ components, int k, float *__restrict__ out, int64_t ldo) {
  extern __shared__ __align__(16) float s_tr[];
  const int ld = d | 1, tid = threadIdx.x, row0 = blockIdx.x * PCA_TROWS, rows = n - row0 < PCA_TROWS ? n - row0 : PCA_TROWS;
  float *s_comp = s_tr, *s_x = s_comp + k * ld;
  for (int e = tid; e < k * d; e += PCA_THREADS) s_comp[(e / d) * ld + e % d] = components[e];
  for (int e = tid; e < rows * d; e += PCA_THREADS) {
    const int r = e / d, j = e % d;
    s_x[r * ld + j] = x[(int64_t)(row0 + r) * ldx + j] - mean[j];
  }
  __syncthreads();
  for (int e = tid; e < rows * k; e += PCA_THREADS) {
    const int r = e / k, c = e % k;
    out[(int64_t)(row0 + r) * ldo + c] = pca_project(s_x + r * ld, s_comp + c * ld, d);
  }
}

__global__ __launch_bounds__(PCA_THREADS) void k_plot_strips(PcaStrip s, const float *__restrict__ proj, const int32_t *__restrict__ frame_idx,
                                                             const uint8_t *__restrict__ flags, uint32_t *__restrict__ rgba) {
  const int pix = blockIdx.x * PCA_THREADS + threadIdx.x, f = blockIdx.y;
  if (pix >= s.W * s.H) return;
  rgba[(size_t)f * s.W * s.H + pix] = pca_strip_pixel(s, proj, frame_idx[f], flags ? flags[f] : 0, pix % s.W, pix / s.W);
}

// ----------------------------------------------------------------------------------------------- launches
template <int NT>
static void launch_gram(const float *x, int64_t ldx, int n, int d, const float *mean, float *partial, int nwg, hipStream_t s) {
  hipLaunchKernelGGL(k_pca_gram<NT>, dim3(nwg), dim3(PCA_THREADS), 0, s, x, ldx, n, d, mean, partial);
}

extern "C" {

int tmjx_pca_workspace(int n, int d, int64_t *floats) {
  if (!floats) return fail(TMJX_EINVAL, "null argument");
  TM_TRY(pca_check_shape(n, d, d));
  *floats = pca_workspace(n, d).floats;
  return TMJX_OK;
}

int tmjx_pca_fit(const float *x, int n, int d, int64_t ldx, float *mean, float *components, float *variance, float *workspace, tmjx_pca_info_t *info,
                 void *stream) {
  TM_TRY(pca_check_fit(x, n, d, ldx, mean, components, variance, workspace, info));
  hipStream_t s = (hipStream_t)stream;
  const PcaWorkspace w = pca_workspace(n, d);
  double *colsum = (double *)(workspace + w.colsum);
  float *gram = workspace + w.gram, *cov = workspace + w.cov;
  PcaInfo *dinfo = (PcaInfo *)(workspace + w.info);
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; i++) TM_HIP("hipEventCreate(&ev[i])", hipEventCreate(&ev[i]));
  hipEventRecord(ev[0], s);
  moments_launch_mean<true>(x, ldx, n, d, colsum, nullptr, s);
  hipLaunchKernelGGL(k_pca_mean, dim3(1), dim3(PCA_MAX_D), 0, s, colsum, w.nwg, d, n, mean);
  if (d <= 32) launch_gram<2>(x, ldx, n, d, mean, gram, w.nwg, s);
  else if (d <= 64) launch_gram<4>(x, ldx, n, d, mean, gram, w.nwg, s);
  else launch_gram<8>(x, ldx, n, d, mean, gram, w.nwg, s);
  hipLaunchKernelGGL(k_pca_cov, dim3((d * d + PCA_THREADS - 1) / PCA_THREADS), dim3(PCA_THREADS), 0, s, gram, w.nwg, d, n, cov);
  hipEventRecord(ev[1], s);
  const int m = (d + 1) & ~1;
  int nt = ((m / 2) * m / 4 + 63) / 64 * 64;      // four (pair, element) items per thread and step, within [64, 1024] threads
  nt = nt < 64 ? 64 : (nt > 1024 ? 1024 : nt);
  const int rc = launch_lds<k_pca_jacobi>("k_pca_jacobi", dim3(1), dim3(nt), sizeof(float) * pca_jacobi_lds_floats(PCA_MAX_D), sizeof(float) * pca_jacobi_lds_floats(d), s,
                                    cov, d, components, variance, dinfo);      // (its check covers every launch of the fit)
  hipEventRecord(ev[2], s);
  PcaInfo hinfo = {0, 0, 0.f, 0};
  hipError_t e = rc ? hipSuccess : hipMemcpyAsync(&hinfo, dinfo, sizeof hinfo, hipMemcpyDeviceToHost, s);
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
  info->moments_ms = info->jacobi_ms = 0.f;
  if (!rc && e == hipSuccess) { hipEventElapsedTime(&info->moments_ms, ev[0], ev[1]); hipEventElapsedTime(&info->jacobi_ms, ev[1], ev[2]); }
  for (int i = 0; i < 3; i++) hipEventDestroy(ev[i]);
  if (rc) return rc;
  if (e != hipSuccess) return fail(TMJX_EHIP, std::string("tmjx_pca_fit: ") + hipGetErrorString(e));
  info->sweeps = hinfo.sweeps; info->converged = hinfo.converged; info->off_rel = hinfo.off_rel;
  if (!hinfo.converged)
    return fail(TMJX_ENOCONV, "tmjx_pca_fit: the Jacobi solver did not converge in " + std::to_string(hinfo.sweeps) + " sweeps (off / norm = " +
                                  std::to_string(hinfo.off_rel) + "; is every value of x finite?)");
  return TMJX_OK;
}

int tmjx_pca_transform(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, float *out, int64_t ldo, void *stream) {
  TM_TRY(pca_check_transform(x, n, d, ldx, mean, components, k, out, ldo));
  return launch_lds<k_pca_transform>("k_pca_transform", dim3((n + PCA_TROWS - 1) / PCA_TROWS), dim3(PCA_THREADS), sizeof(float) * (PCA_MAX_D + PCA_TROWS) * (PCA_MAX_D | 1),
                                     sizeof(float) * (k + PCA_TROWS) * (d | 1), (hipStream_t)stream, x, n, d, ldx, mean, components, k, out, ldo);
}

int tmjx_plot_strips(const float *proj, int T, int k, int64_t ldp, const int32_t *frame_idx, const uint8_t *flags, int F, float ymin, float ymax, int window,
                     const tmjx_strip_style_t *style, int W, int H, uint8_t *rgba, void *stream) {
  PcaStrip s;
  TM_TRY(pca_check_strips(proj, T, k, ldp, frame_idx, F, ymin, ymax, window, style, W, H, rgba, s));
  if (F > 65535) return fail(TMJX_EINVAL, "F exceeds the 65535 frames of one launch: draw fewer frames per call");
  if ((long long)W * H > 0x7fffffffLL) return fail(TMJX_EINVAL, "W * H exceeds the pixels of one launch");
  hipLaunchKernelGGL(k_plot_strips, dim3((unsigned)(((long long)W * H + PCA_THREADS - 1) / PCA_THREADS), (unsigned)F), dim3(PCA_THREADS), 0, (hipStream_t)stream, s,
                     proj, frame_idx, flags, (uint32_t *)rgba);
  return check_launch("k_plot_strips");
}

}  // extern "C"
