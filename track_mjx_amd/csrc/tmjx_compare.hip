// csrc/tmjx_compare.hip — how two representations of the same time steps relate: linear CKA, the correlation of two dissimilarity matrices and
// canonical correlations (include/tmjx.h: tmjx_compare_workspace, tmjx_cka_linear, tmjx_rdm_corr, tmjx_cca, tmjx_compare_svd; DESIGN.md
// "Representation comparison").  The bodies are csrc/compare_core.h (they also compile on the host); the argument checks and the workspace layout
// csrc/compare_host.h.  The moments are csrc/moments_core.h in the readout's tiling, the eigen-decompositions tmjx_pca_fit_wide's, called as it is.
//   k_moments_colsum / k_moments_mean  the column means by super-chunk               k_cmp_cross   one workgroup per (128 x 64 of the moment, super-chunk)
//   k_cmp_frob    one workgroup per row of a moment: sum_j C_ij^2                     k_cmp_total   the rows in row order
//   k_cmp_rowstat shift, scale and ok of every row of a side                          k_cmp_pairs   the all-pairs pass: a (128 x 64) pair tile per workgroup
//   k_cmp_sums    the tiles' five sums in a fixed order                               k_cmp_c       C in float64
//   k_cmp_widen   the kept components in float64                                      k_cmp_gemm    the small float64 products, one thread per output
//   k_cmp_scale   the rows of Q over sqrt(sigma)                                      k_cmp_svd     one-sided Jacobi in one workgroup, the matrix in LDS
//   k_cmp_round   rho, a and b rounded to float32
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "compare_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
// blockIdx.x: the tile of 128 columns of x; blockIdx.y: the tile of 64 columns of y; blockIdx.z: the super-chunk.  x and y may be the same buffer.
__global__ __launch_bounds__(PCA_THREADS) void k_cmp_cross(const float *x, int64_t ldx, const float *y, int64_t ldy, int n, int d, int m, const float *mean_x,
                                                           const float *mean_y, double *__restrict__ partial) {
  __shared__ float s_x[PCA_KB * PCA_WIDE_TILE], s_y[PCA_KB * READOUT_TILE_M];
  readout_cross_wg(x, ldx, y, ldy, n, d, m, mean_x, mean_y, blockIdx.x, blockIdx.y, blockIdx.z, partial, s_x, s_y);
}

__global__ __launch_bounds__(PCA_THREADS) void k_cmp_frob(const double *__restrict__ partial, int S, int d, int m, int n, double *__restrict__ rowsum) {
  __shared__ double s_red[PCA_THREADS];
  compare_frob_row_wg(partial, S, d, m, n, blockIdx.x, rowsum, s_red);
}

__global__ void k_cmp_total(const double *__restrict__ rowsum, int d, double *__restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out = compare_total(rowsum, d);
}

__global__ __launch_bounds__(PCA_THREADS) void k_cmp_rowstat(const float *__restrict__ x, int64_t ldx, const float *__restrict__ mean, int n, int d, int metric,
                                                             float *__restrict__ shift, float *__restrict__ scale, int32_t *__restrict__ ok) {
  const int64_t r = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (r < n) compare_rowstat(x, ldx, mean, d, metric, r, shift, scale, ok);
}

// blockIdx.x: the tile of 64 rows j; blockIdx.y: the tile of 128 rows i
__global__ __launch_bounds__(PCA_THREADS) void k_cmp_pairs(CompareSide sx, CompareSide sy, int n, int ntj, double *__restrict__ parts) {
  __shared__ __attribute__((aligned(16))) float s_stage[COMPARE_STAGE];
  compare_pairs_wg(sx, sy, n, blockIdx.y, blockIdx.x, ntj, parts, s_stage);
}

__global__ __launch_bounds__(PCA_THREADS) void k_cmp_sums(const double *__restrict__ parts, int64_t tiles, double *__restrict__ sums) {
  __shared__ double s_red[5 * PCA_THREADS];
  compare_pairs_total_wg(parts, tiles, sums, s_red);
}

__global__ __launch_bounds__(PCA_THREADS) void k_cmp_c(const double *__restrict__ partial, int S, int d, int m, int n, double *__restrict__ c) {
  const int64_t e = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < (int64_t)d * m) c[e] = compare_cross_reduce(partial, S, d, m, n, e);
}

__global__ __launch_bounds__(PCA_THREADS) void k_cmp_widen(const float *__restrict__ in, int count, double *__restrict__ out) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < count) out[e] = (double)in[e];
}

__global__ __launch_bounds__(PCA_THREADS) void k_cmp_scale(double *__restrict__ q, const double *__restrict__ sigma, int k) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < k * k) q[e] = compare_inv_sqrt_row(q, sigma, k, e);
}

// out [rows][cols] = a [rows][K] . B; B = b [K][cols], or b [cols][K] with TB
template <bool TB>
__global__ __launch_bounds__(PCA_THREADS) void k_cmp_gemm(const double *__restrict__ a, int64_t lda, const double *__restrict__ b, int64_t ldb, int K, int rows,
                                                          int cols, double *__restrict__ out) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < rows * cols) out[e] = compare_dot<TB>(a, lda, b, ldb, K, e / cols, e % cols);
}

__global__ __launch_bounds__(PCA_THREADS) void k_cmp_svd(const double *__restrict__ a, int ra, int ca, int64_t lda, double *__restrict__ sigma,
                                                         double *__restrict__ u, double *__restrict__ v, int32_t *__restrict__ info, double *work) {
  extern __shared__ __attribute__((aligned(16))) double s_svd[];
  compare_svd_wg(a, ra, ca, lda, sigma, u, v, info, work, s_svd);
}

__global__ __launch_bounds__(PCA_THREADS) void k_cmp_round(const double *__restrict__ in, int count, float *__restrict__ out) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < count) out[e] = (float)in[e];
}

// ----------------------------------------------------------------------------------------------- launches
static inline unsigned blocks_of(int64_t count, int per) { return (unsigned)((count + per - 1) / per); }

static void launch_means(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, float *workspace, const CompareWorkspace &w,
                         hipStream_t s) {
  moments_launch_mean<false>(x, ldx, n, d1, (double *)(workspace + w.xsum), workspace + w.mean_x, s);
  moments_launch_mean<false>(y, ldy, n, d2, (double *)(workspace + w.ysum), workspace + w.mean_y, s);
}

static void launch_cross(const float *x, int64_t ldx, int d, const float *mean_x, const float *y, int64_t ldy, int m, const float *mean_y, int n, float *workspace,
                         const CompareWorkspace &w, hipStream_t s) {
  hipLaunchKernelGGL(k_cmp_cross, dim3(pca_wide_tiles(d), readout_tiles(m, READOUT_TILE_M), w.split.S), dim3(PCA_THREADS), 0, s, x, ldx, y, ldy, n, d, m, mean_x,
                     mean_y, (double *)(workspace + w.cross));
}

static int launch_svd(const double *a, int ra, int ca, int64_t lda, double *sigma, double *u, double *v, int32_t *info, double *work, hipStream_t s) {
  return launch_lds<k_cmp_svd>("k_cmp_svd", dim3(1), dim3(PCA_THREADS), sizeof(double) * compare_svd_lds_doubles(COMPARE_MAX_RANK, COMPARE_MAX_RANK),
                               sizeof(double) * (size_t)compare_svd_lds_doubles(ra, ca), s, a, ra, ca, lda, sigma, u, v, info, work);
}

// The whitening matrix of one side, W [k][d] float64 with W Cxx W^T = I on the span of its k leading components: E = components[:k] in float64,
// S = E Cxx E^T [k][k] from the float64 moment, S = Q diag(sigma) Q^T by the decomposition, W = diag(sigma)^-1/2 Q^T E.  The PCA's float32
// eigenvalues pick the components; they do not scale them.  dinfo: {sweeps, converged} of this decomposition, then of the window's.
static int launch_whitener(const float *x, int64_t ldx, int d, const float *mean, const float *comp, int k, int n, float *workspace, const CompareWorkspace &w,
                           double *W, int32_t *dinfo, hipStream_t s) {
  double *cross = (double *)(workspace + w.cross), *c = (double *)(workspace + w.c), *e = (double *)(workspace + w.e), *t = (double *)(workspace + w.t),
         *m = (double *)(workspace + w.m), *sigma = (double *)(workspace + w.sigma), *u = (double *)(workspace + w.u), *v = (double *)(workspace + w.v),
         *work = (double *)(workspace + w.w);
  const CompareWindow win = compare_window(d, k);
  const int top = win.hi > k ? win.hi : k, nw = win.hi - win.lo;
  int rc;
  launch_cross(x, ldx, d, mean, x, ldx, d, mean, n, workspace, w, s);
  hipLaunchKernelGGL(k_cmp_c, dim3(blocks_of((int64_t)d * d, PCA_THREADS)), dim3(PCA_THREADS), 0, s, cross, w.split.S, d, d, n, c);
  hipLaunchKernelGGL(k_cmp_widen, dim3(blocks_of((int64_t)top * d, PCA_THREADS)), dim3(PCA_THREADS), 0, s, comp, top * d, e);
  if (nw > 0) {
    // the cut sharpened (a Ritz step in float64): the float32 PCA mixes components whose eigenvalues are close, and the cut falls between two
    // of them.  Within the window around it, S = Ew Cxx Ew^T = Q diag(s) Q^T, and the leading rows of Q^T Ew replace the kept rows of the window
    double *ew = e + (int64_t)win.lo * d, *ritz = e + 2 * (int64_t)COMPARE_MAX_RANK * d;
    hipLaunchKernelGGL(k_cmp_gemm<false>, dim3(blocks_of((int64_t)nw * d, PCA_THREADS)), dim3(PCA_THREADS), 0, s, ew, (int64_t)d, c, (int64_t)d, d, nw, d, t);
    hipLaunchKernelGGL(k_cmp_gemm<true>, dim3(blocks_of((int64_t)nw * nw, PCA_THREADS)), dim3(PCA_THREADS), 0, s, t, (int64_t)d, ew, (int64_t)d, d, nw, nw, m);
    if ((rc = check_launch("tmjx_cca (window)"))) return rc;
    if ((rc = launch_svd(m, nw, nw, nw, sigma, u, v, dinfo + 2, work, s))) return rc;
    hipLaunchKernelGGL(k_cmp_gemm<false>, dim3(blocks_of((int64_t)(k - win.lo) * d, PCA_THREADS)), dim3(PCA_THREADS), 0, s, v, (int64_t)nw, ew, (int64_t)d, nw,
                       k - win.lo, d, ritz);
    if ((rc = check_launch("tmjx_cca (window)"))) return rc;
    TM_HIP("tmjx_cca (window)", hipMemcpyAsync(ew, ritz, sizeof(double) * (size_t)(k - win.lo) * d, hipMemcpyDeviceToDevice, s));
  }
  hipLaunchKernelGGL(k_cmp_gemm<false>, dim3(blocks_of((int64_t)k * d, PCA_THREADS)), dim3(PCA_THREADS), 0, s, e, (int64_t)d, c, (int64_t)d, d, k, d, t);
  hipLaunchKernelGGL(k_cmp_gemm<true>, dim3(blocks_of((int64_t)k * k, PCA_THREADS)), dim3(PCA_THREADS), 0, s, t, (int64_t)d, e, (int64_t)d, d, k, k, m);
  if ((rc = check_launch("tmjx_cca (whitening)"))) return rc;
  if ((rc = launch_svd(m, k, k, k, sigma, u, v, dinfo, work, s))) return rc;
  hipLaunchKernelGGL(k_cmp_scale, dim3(blocks_of((int64_t)k * k, PCA_THREADS)), dim3(PCA_THREADS), 0, s, v, sigma, k);
  hipLaunchKernelGGL(k_cmp_gemm<false>, dim3(blocks_of((int64_t)k * d, PCA_THREADS)), dim3(PCA_THREADS), 0, s, v, (int64_t)k, e, (int64_t)d, k, k, d, W);
  return check_launch("tmjx_cca (whitening)");
}

static int pca_floats_of(int n, int d1, int d2, int64_t *floats) {
  int64_t p1 = 0, p2 = 0;
  int rc = tmjx_pca_wide_workspace(n, d1, &p1);
  if (!rc) rc = tmjx_pca_wide_workspace(n, d2, &p2);
  *floats = p1 > p2 ? p1 : p2;
  return rc;
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_compare_workspace(int n, int d1, int d2, int64_t *floats) {
  TM_TRY(compare_check_workspace(n, d1, d2, floats));
  int64_t pca = 0;
  const int rc = pca_floats_of(n, d1, d2, &pca);
  if (rc) return rc;
  *floats = compare_workspace(n, d1, d2, pca).floats;
  return TMJX_OK;
}

int tmjx_cka_linear(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, double *out, float *workspace, void *stream) {
  TM_TRY(compare_check_cka(x, n, d1, ldx, y, d2, ldy, out, workspace));
  const CompareWorkspace w = compare_workspace(n, d1, d2, 0);
  hipStream_t s = (hipStream_t)stream;
  const float *mean_x = workspace + w.mean_x, *mean_y = workspace + w.mean_y;
  double *cross = (double *)(workspace + w.cross), *rowsum = (double *)(workspace + w.rowsum);
  launch_means(x, n, d1, ldx, y, d2, ldy, workspace, w, s);
  const struct { const float *a; int64_t lda; int da; const float *ma; const float *b; int64_t ldb; int db; const float *mb; } pass[3] = {
      {x, ldx, d1, mean_x, y, ldy, d2, mean_y}, {x, ldx, d1, mean_x, x, ldx, d1, mean_x}, {y, ldy, d2, mean_y, y, ldy, d2, mean_y}};
  for (int k = 0; k < 3; k++) {      // (the three moments one after the other through the same partials: the stream orders them)
    launch_cross(pass[k].a, pass[k].lda, pass[k].da, pass[k].ma, pass[k].b, pass[k].ldb, pass[k].db, pass[k].mb, n, workspace, w, s);
    hipLaunchKernelGGL(k_cmp_frob, dim3(pass[k].da), dim3(PCA_THREADS), 0, s, cross, w.split.S, pass[k].da, pass[k].db, n, rowsum);
    hipLaunchKernelGGL(k_cmp_total, dim3(1), dim3(64), 0, s, rowsum, pass[k].da, out + k);
  }
  return check_launch("tmjx_cka_linear");
}

int tmjx_rdm_corr(const float *x, int n, int d1, int64_t ldx, int metric_x, const float *y, int d2, int64_t ldy, int metric_y, double *sums, float *workspace,
                  void *stream) {
  TM_TRY(compare_check_rdm(x, n, d1, ldx, metric_x, y, d2, ldy, metric_y, sums, workspace));
  const CompareWorkspace w = compare_workspace(n, d1, d2, 0);
  hipStream_t s = (hipStream_t)stream;
  const int64_t up = (n + 3) & ~3;
  float *stat_x = workspace + w.stat_x, *stat_y = workspace + w.stat_y;
  const CompareSide sx = {x, ldx, d1, metric_x, workspace + w.mean_x, stat_x, stat_x + up, (const int32_t *)(stat_x + 2 * up)};
  const CompareSide sy = {y, ldy, d2, metric_y, workspace + w.mean_y, stat_y, stat_y + up, (const int32_t *)(stat_y + 2 * up)};
  double *parts = (double *)(workspace + w.parts);
  launch_means(x, n, d1, ldx, y, d2, ldy, workspace, w, s);
  hipLaunchKernelGGL(k_cmp_rowstat, dim3(blocks_of(n, PCA_THREADS)), dim3(PCA_THREADS), 0, s, x, ldx, sx.mean, n, d1, metric_x, stat_x, stat_x + up,
                     (int32_t *)(stat_x + 2 * up));
  hipLaunchKernelGGL(k_cmp_rowstat, dim3(blocks_of(n, PCA_THREADS)), dim3(PCA_THREADS), 0, s, y, ldy, sy.mean, n, d2, metric_y, stat_y, stat_y + up,
                     (int32_t *)(stat_y + 2 * up));
  hipLaunchKernelGGL(k_cmp_pairs, dim3(w.ntj, w.nib), dim3(PCA_THREADS), 0, s, sx, sy, n, w.ntj, parts);
  hipLaunchKernelGGL(k_cmp_sums, dim3(1), dim3(PCA_THREADS), 0, s, parts, (int64_t)w.nib * w.ntj, sums);
  return check_launch("tmjx_rdm_corr");
}

int tmjx_compare_svd(const double *a, int rows, int cols, int64_t lda, double *sigma, double *u, double *v, int32_t *sweeps, float *workspace, void *stream) {
  TM_TRY(compare_check_svd(a, rows, cols, lda, sigma, u, v, sweeps, workspace));
  hipStream_t s = (hipStream_t)stream;
  const int nn = rows < cols ? rows : cols;
  int32_t *dinfo = (int32_t *)(workspace + 2 * (int64_t)nn * nn), host[2] = {0, 0};
  int rc = launch_svd(a, rows, cols, lda, sigma, u, v, dinfo, (double *)workspace, s);
  if (rc) return rc;
  TM_HIP("tmjx_compare_svd", hipMemcpyAsync(host, dinfo, sizeof(host), hipMemcpyDeviceToHost, s));
  TM_HIP("tmjx_compare_svd", hipStreamSynchronize(s));
  *sweeps = host[0];
  if (!host[1]) return fail(TMJX_ENOCONV, "tmjx_compare_svd: " + compare_svd_noconv_message(host[0]));
  return TMJX_OK;
}

int tmjx_cca(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, double var_keep, int max_rank, float *rho, float *a, float *b,
             tmjx_cca_info_t *info, float *workspace, void *stream) {
  TM_TRY(compare_check_cca(x, n, d1, ldx, y, d2, ldy, var_keep, max_rank, rho, a, b, info, workspace));
  int64_t pca = 0;
  int rc = pca_floats_of(n, d1, d2, &pca);
  if (rc) return rc;
  const CompareWorkspace w = compare_workspace(n, d1, d2, pca);
  hipStream_t s = (hipStream_t)stream;
  float *mean_x = workspace + w.mean_x, *mean_y = workspace + w.mean_y, *comp_x = workspace + w.comp_x, *var_x = workspace + w.var_x,
        *comp_y = workspace + w.comp_y, *var_y = workspace + w.var_y;
  double *cross = (double *)(workspace + w.cross), *c = (double *)(workspace + w.c), *wx = (double *)(workspace + w.wx), *wy = (double *)(workspace + w.wy),
         *t = (double *)(workspace + w.t), *m = (double *)(workspace + w.m), *sigma = (double *)(workspace + w.sigma), *u = (double *)(workspace + w.u),
         *v = (double *)(workspace + w.v), *work = (double *)(workspace + w.w);
  int32_t *dinfo = (int32_t *)(workspace + w.info);
  *info = tmjx_cca_info_t{};
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  auto finish = [&](int code) { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); return code; };
  for (int i = 0; i < 3; i++)
    if (hipEventCreate(&ev[i]) != hipSuccess) return finish(fail(TMJX_EHIP, "tmjx_cca: hipEventCreate failed"));
  // both eigen-decompositions, as they are (each waits for the stream); their times are the PCA's own
  tmjx_pca_info_t px, py;
  if ((rc = tmjx_pca_fit_wide(x, n, d1, ldx, mean_x, comp_x, var_x, workspace + w.pca, &px, stream))) return finish(rc);
  if ((rc = tmjx_pca_fit_wide(y, n, d2, ldy, mean_y, comp_y, var_y, workspace + w.pca, &py, stream))) return finish(rc);
  info->pca_ms = px.moments_ms + px.jacobi_ms + py.moments_ms + py.jacobi_ms;
  std::vector<float> hx(d1), hy(d2);
  hipError_t e = hipMemcpyAsync(hx.data(), var_x, sizeof(float) * d1, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(hy.data(), var_y, sizeof(float) * d2, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return finish(fail(TMJX_EHIP, std::string("tmjx_cca: ") + hipGetErrorString(e)));
  const int kx = compare_keep(hx.data(), d1, var_keep, max_rank), ky = compare_keep(hy.data(), d2, var_keep, max_rank);
  if (kx == 0) return finish(fail(TMJX_EINVAL, compare_flat_message("x")));
  if (ky == 0) return finish(fail(TMJX_EINVAL, compare_flat_message("y")));
  const int r = kx < ky ? kx : ky;
  info->kx = kx; info->ky = ky;
  // the whitened cross matrix M = Wx C Wy^T [kx][ky], all of it float64
  (void)hipEventRecord(ev[0], s);
  if ((rc = launch_whitener(x, ldx, d1, mean_x, comp_x, kx, n, workspace, w, wx, dinfo + 2, s))) return finish(rc);
  if ((rc = launch_whitener(y, ldy, d2, mean_y, comp_y, ky, n, workspace, w, wy, dinfo + 6, s))) return finish(rc);
  launch_cross(x, ldx, d1, mean_x, y, ldy, d2, mean_y, n, workspace, w, s);
  hipLaunchKernelGGL(k_cmp_c, dim3(blocks_of((int64_t)d1 * d2, PCA_THREADS)), dim3(PCA_THREADS), 0, s, cross, w.split.S, d1, d2, n, c);
  hipLaunchKernelGGL(k_cmp_gemm<false>, dim3(blocks_of((int64_t)kx * d2, PCA_THREADS)), dim3(PCA_THREADS), 0, s, wx, (int64_t)d1, c, (int64_t)d2, d1, kx, d2, t);
  hipLaunchKernelGGL(k_cmp_gemm<true>, dim3(blocks_of((int64_t)kx * ky, PCA_THREADS)), dim3(PCA_THREADS), 0, s, t, (int64_t)d2, wy, (int64_t)d2, d2, kx, ky, m);
  (void)hipEventRecord(ev[1], s);
  if ((rc = check_launch("tmjx_cca (cross)"))) return finish(rc);
  if ((rc = launch_svd(m, kx, ky, ky, sigma, u, v, dinfo, work, s))) return finish(rc);
  (void)hipEventRecord(ev[2], s);
  // the directions in feature space: b = V Wy, then a = U Wx, in float64 in the room of the moment partials (dead now, and larger than any
  // [128][d]), each rounded once
  double *dir = cross;
  hipLaunchKernelGGL(k_cmp_gemm<false>, dim3(blocks_of((int64_t)r * d2, PCA_THREADS)), dim3(PCA_THREADS), 0, s, v, (int64_t)ky, wy, (int64_t)d2, ky, r, d2, dir);
  hipLaunchKernelGGL(k_cmp_round, dim3(blocks_of((int64_t)r * d2, PCA_THREADS)), dim3(PCA_THREADS), 0, s, dir, r * d2, b);
  hipLaunchKernelGGL(k_cmp_gemm<false>, dim3(blocks_of((int64_t)r * d1, PCA_THREADS)), dim3(PCA_THREADS), 0, s, u, (int64_t)kx, wx, (int64_t)d1, kx, r, d1, dir);
  hipLaunchKernelGGL(k_cmp_round, dim3(blocks_of((int64_t)r * d1, PCA_THREADS)), dim3(PCA_THREADS), 0, s, dir, r * d1, a);
  hipLaunchKernelGGL(k_cmp_round, dim3(1), dim3(PCA_THREADS), 0, s, sigma, r, rho);
  if ((rc = check_launch("tmjx_cca (directions)"))) return finish(rc);
  int32_t host[10] = {0};      // {sweeps, converged} of M's decomposition, then of x's whitening and window, then of y's
  e = hipMemcpyAsync(host, dinfo, sizeof(host), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return finish(fail(TMJX_EHIP, std::string("tmjx_cca: ") + hipGetErrorString(e)));
  (void)hipEventElapsedTime(&info->cross_ms, ev[0], ev[1]);
  (void)hipEventElapsedTime(&info->svd_ms, ev[1], ev[2]);
  if (compare_window(d1, kx).hi == 0) host[5] = 1;      // (no window: nothing was decomposed there)
  if (compare_window(d2, ky).hi == 0) host[9] = 1;
  info->sweeps = host[0];
  info->converged = 1;
  for (int i = 0; i < 5; i++)
    if (!host[2 * i + 1]) {
      info->converged = 0;
      return finish(fail(TMJX_ENOCONV, "tmjx_cca: " + compare_svd_noconv_message(host[2 * i])));
    }
  return finish(TMJX_OK);
}

}  // extern "C"
