// csrc/tmjx_kmeans.hip — k-means of recorded activations: Lloyd's iteration with k-means++ seeding (include/tmjx.h: tmjx_kmeans_workspace,
// tmjx_kmeans_assign, tmjx_kmeans_update, tmjx_kmeans_seed, tmjx_kmeans_fit; DESIGN.md "Clustering").  The bodies are csrc/kmeans_core.h (they also
// compile on the host); the argument checks and the workspace layout csrc/kmeans_host.h.
//   k_moments_colsum, k_moments_mean   the column mean of x by chunk of 256 rows (csrc/moments_core.h)
//   k_km_cnorm    ||c_j - mean||^2, one thread per centroid                                    k_km_assign   the fused pass: 128 rows per workgroup
//   k_km_totals   inertia and changed: the workgroups' partials added in order                 k_km_update   four waves per (row part, 64 columns)
//   k_km_reduce   the parts' sums over the parts' counts                                       k_km_dist / k_km_pick   one k-means++ step
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "kmeans_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(PCA_THREADS) void k_km_cnorm(const float *__restrict__ centroids, const float *__restrict__ mean, int d, int k,
                                                          float *__restrict__ cnorm) {
  const int j = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (j < k) cnorm[j] = kmeans_cnorm(centroids, mean, d, j);
}

__global__ __launch_bounds__(PCA_THREADS, 4) void k_km_assign(const float *__restrict__ x, int n, int d, int64_t ldx, const float *__restrict__ centroids, int k,
                                                           const float *__restrict__ mean, const float *__restrict__ cnorm,
                                                           const int32_t *__restrict__ labels_prev, int32_t *__restrict__ labels, float *__restrict__ dist2,
                                                           double *__restrict__ part_inertia, int32_t *__restrict__ part_changed) {
  __shared__ __attribute__((aligned(16))) float s_x[KMEANS_TK * KMEANS_LDX], s_c[KMEANS_TK * KMEANS_LDC];
  static_assert(KMEANS_ROWS * 16 <= KMEANS_TK * KMEANS_LDX && KMEANS_ROWS * 16 <= KMEANS_TK * KMEANS_LDC, "the epilogue's arrays reuse the stages");
  kmeans_assign_wg(x, n, d, ldx, centroids, k, mean, cnorm, labels_prev, labels, dist2, part_inertia, part_changed, blockIdx.x, s_x, s_c, s_x, (int32_t *)s_c);
}

__global__ __launch_bounds__(PCA_THREADS) void k_km_totals(const double *__restrict__ part_inertia, const int32_t *__restrict__ part_changed, int nwg,
                                                           double *__restrict__ inertia, int32_t *__restrict__ changed) {
  __shared__ double s_sum[PCA_THREADS];
  __shared__ int32_t s_cnt[PCA_THREADS];
  kmeans_totals_wg(part_inertia, part_changed, nwg, inertia, changed, s_sum, s_cnt);
}

// blockIdx.x: 64 columns; blockIdx.y: the row part.  Dynamic LDS: [k][64] doubles, then [k] ints.
__global__ __launch_bounds__(KMEANS_UTHREADS) void k_km_update(const float *__restrict__ x, int n, int d, int64_t ldx, const int32_t *__restrict__ labels, int k,
                                                            double *__restrict__ part_sum, int32_t *__restrict__ part_cnt) {
  extern __shared__ double s_dyn[];
  kmeans_update_wg(x, n, d, ldx, labels, k, blockIdx.y, blockIdx.x, part_sum, part_cnt, s_dyn, (int32_t *)(s_dyn + (size_t)k * KMEANS_UTILE));
}

__global__ __launch_bounds__(PCA_THREADS) void k_km_reduce(const double *__restrict__ part_sum, const int32_t *__restrict__ part_cnt, int P, int k, int d,
                                                           float *__restrict__ centroids, int32_t *__restrict__ counts) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < k * d) kmeans_update_reduce(part_sum, part_cnt, P, k, d, centroids, counts, e);
}

__global__ __launch_bounds__(PCA_THREADS) void k_km_dist(const float *__restrict__ x, int n, int d, int64_t ldx, const float *__restrict__ centre, int first,
                                                         float *__restrict__ d2, double *__restrict__ blocksum) {
  __shared__ float s_p[KMEANS_SEED_ROWS * 17];
  kmeans_seed_dist_wg(x, n, d, ldx, centre, first, d2, blocksum, blockIdx.x, s_p);
}

__global__ __launch_bounds__(PCA_THREADS) void k_km_pick(const float *__restrict__ x, int n, int d, int64_t ldx, const float *__restrict__ d2,
                                                         const double *__restrict__ blocksum, int nb, double u, int j, float *__restrict__ centroids,
                                                         int32_t *__restrict__ picks) {
  __shared__ double s_seg[PCA_THREADS];
  __shared__ int32_t s_pick[1];
  kmeans_seed_pick_wg(x, n, d, ldx, d2, blocksum, nb, u, j, centroids, picks, s_seg, s_pick);
}

// ----------------------------------------------------------------------------------------------- launches
static int launch_assign(const float *x, int n, int d, int64_t ldx, const float *centroids, int k, const int32_t *labels_prev, int32_t *labels, float *dist2,
                         double *inertia, int32_t *changed, float *workspace, hipStream_t s, bool have_mean = false) {
  const KmeansWorkspace w = kmeans_workspace(n, d, k);
  double *colsum = (double *)(workspace + w.colsum), *pin = (double *)(workspace + w.part_inertia);
  float *mean = workspace + w.mean, *cnorm = workspace + w.cnorm;
  int32_t *pch = (int32_t *)(workspace + w.part_changed);
  if (!have_mean) moments_launch_mean<true>(x, ldx, n, d, colsum, mean, s);      // (a fit forms the column mean of x once: the rows do not change between its assigns)
  hipLaunchKernelGGL(k_km_cnorm, dim3(kmeans_tiles(k, PCA_THREADS)), dim3(PCA_THREADS), 0, s, centroids, mean, d, k, cnorm);
  hipLaunchKernelGGL(k_km_assign, dim3(w.nwg_assign), dim3(PCA_THREADS), 0, s, x, n, d, ldx, centroids, k, mean, cnorm, labels_prev, labels, dist2, pin, pch);
  hipLaunchKernelGGL(k_km_totals, dim3(1), dim3(PCA_THREADS), 0, s, pin, pch, w.nwg_assign, inertia, changed);
  return check_launch("tmjx_kmeans_assign");
}

static int launch_update(const float *x, int n, int d, int64_t ldx, const int32_t *labels, int k, float *centroids, int32_t *counts, float *workspace,
                         hipStream_t s) {
  const KmeansWorkspace w = kmeans_workspace(n, d, k);
  double *psum = (double *)(workspace + w.part_sum);
  int32_t *pcnt = (int32_t *)(workspace + w.part_cnt);
  const int rc = launch_lds<k_km_update>("k_km_update", dim3(kmeans_tiles(d, KMEANS_UTILE), w.split.P), dim3(KMEANS_UTHREADS), KMEANS_MAX_K * (KMEANS_UTILE * 8 + 4),
                                         (size_t)k * (KMEANS_UTILE * 8 + 4), s, x, n, d, ldx, labels, k, psum, pcnt);
  if (rc) return rc;
  hipLaunchKernelGGL(k_km_reduce, dim3(kmeans_tiles(k * d, PCA_THREADS)), dim3(PCA_THREADS), 0, s, psum, pcnt, w.split.P, k, d, centroids, counts);
  return check_launch("tmjx_kmeans_update");
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_kmeans_workspace(int n, int d, int k, int64_t *floats) {
  TM_TRY(kmeans_check_workspace(n, d, k, floats));
  *floats = kmeans_workspace(n, d, k).floats;
  return TMJX_OK;
}

int tmjx_kmeans_assign(const float *x, int n, int d, int64_t ldx, const float *centroids, int k, const int32_t *labels_prev, int32_t *labels, float *dist2,
                       double *inertia, int32_t *changed, float *workspace, void *stream) {
  TM_TRY(kmeans_check_assign(x, n, d, ldx, centroids, k, labels, inertia, workspace));
  return launch_assign(x, n, d, ldx, centroids, k, labels_prev, labels, dist2, inertia, changed, workspace, (hipStream_t)stream);
}

int tmjx_kmeans_update(const float *x, int n, int d, int64_t ldx, const int32_t *labels, int k, float *centroids, int32_t *counts, float *workspace,
                       void *stream) {
  TM_TRY(kmeans_check_update(x, n, d, ldx, labels, k, centroids, counts, workspace));
  return launch_update(x, n, d, ldx, labels, k, centroids, counts, workspace, (hipStream_t)stream);
}

int tmjx_kmeans_seed(const float *x, int n, int d, int64_t ldx, int k, const double *u, float *centroids, int32_t *index, float *workspace, void *stream) {
  TM_TRY(kmeans_check_seed(x, n, d, ldx, k, u, centroids, index, workspace));
  const KmeansWorkspace w = kmeans_workspace(n, d, k);
  hipStream_t s = (hipStream_t)stream;
  float *d2 = workspace + w.d2;
  double *blocksum = (double *)(workspace + w.blocksum);
  int32_t *picks = (int32_t *)(workspace + w.picks);
  for (int j = 0; j < k; j++) {
    if (j > 0)
      hipLaunchKernelGGL(k_km_dist, dim3(w.nb_seed), dim3(PCA_THREADS), 0, s, x, n, d, ldx, centroids + (int64_t)(j - 1) * d, j == 1 ? 1 : 0, d2, blocksum);
    hipLaunchKernelGGL(k_km_pick, dim3(1), dim3(PCA_THREADS), 0, s, x, n, d, ldx, d2, blocksum, j > 0 ? w.nb_seed : 0, u[j], j, centroids, picks);
  }
  int rc = check_launch("tmjx_kmeans_seed");
  if (rc) return rc;
  TM_HIP("tmjx_kmeans_seed", hipMemcpyAsync(index, picks, sizeof(int32_t) * k, hipMemcpyDeviceToHost, s));
  TM_HIP("tmjx_kmeans_seed", hipStreamSynchronize(s));
  return TMJX_OK;
}

int tmjx_kmeans_fit(const float *x, int n, int d, int64_t ldx, int k, float *centroids, int32_t *labels, float *dist2, int max_iter, double tol,
                    tmjx_kmeans_info_t *info, float *workspace, void *stream) {
  TM_TRY(kmeans_check_fit(x, n, d, ldx, k, centroids, labels, max_iter, tol, info, workspace));
  const KmeansWorkspace w = kmeans_workspace(n, d, k);
  hipStream_t s = (hipStream_t)stream;
  struct Result { double inertia; int32_t changed, pad_; } host = {0.0, 0, 0};
  Result *dev = (Result *)(workspace + w.result);
  int32_t *buf[2] = {labels, (int32_t *)(workspace + w.labels2)}, *counts = (int32_t *)(workspace + w.picks);      // (the seeding's picks are dead by now)
  hipEvent_t ev[4];
  for (int i = 0; i < 4; i++) TM_HIP("hipEventCreate", hipEventCreate(&ev[i]));
  int rc = TMJX_OK, it = 0, cur = 0;
  bool update_pending = false;
  double previous = 0.0;
  float ms = 0.f;
  info->n_iter = 0; info->assign_ms = 0.f; info->update_ms = 0.f;
  auto finish = [&](int code) { for (int i = 0; i < 4; i++) (void)hipEventDestroy(ev[i]); return code; };
  // one assign and the read-back of its {inertia, changed}: the only synchronisation of an iteration
  bool have_mean = false;
  auto assign = [&](const int32_t *prev, int32_t *out) -> int {
    (void)hipEventRecord(ev[0], s);
    int r = launch_assign(x, n, d, ldx, centroids, k, prev, out, dist2, &dev->inertia, &dev->changed, workspace, s, have_mean);
    have_mean = true;
    if (r) return r;
    (void)hipEventRecord(ev[1], s);
    hipError_t e = hipMemcpyAsync(&host, dev, sizeof(Result), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(TMJX_EHIP, std::string("tmjx_kmeans_fit: ") + hipGetErrorString(e));
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) info->assign_ms += ms;
    if (update_pending && hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) info->update_ms += ms;
    update_pending = false;
    return TMJX_OK;
  };
  for (; it < max_iter; it++) {
    if ((rc = assign(it > 0 ? buf[cur ^ 1] : nullptr, buf[cur]))) return finish(rc);
    info->n_iter = it + 1;
    if (kmeans_converged(it, host.changed, host.inertia, previous, tol)) break;
    previous = host.inertia;
    (void)hipEventRecord(ev[2], s);
    if ((rc = launch_update(x, n, d, ldx, buf[cur], k, centroids, counts, workspace, s))) return finish(rc);
    (void)hipEventRecord(ev[3], s);
    update_pending = true;
    cur ^= 1;
  }
  // the labels of the last assign of the loop are in buf[cur] after a break, in buf[cur ^ 1] after max_iter updates; the final assign writes `labels`
  const int32_t *last = it < max_iter ? buf[cur] : buf[cur ^ 1];
  if (last == labels) {      // the final assign may not read what it writes: move the last labels aside
    hipError_t e = hipMemcpyAsync(buf[1], labels, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return finish(fail(TMJX_EHIP, std::string("tmjx_kmeans_fit: ") + hipGetErrorString(e)));
    last = buf[1];
  }
  if ((rc = assign(last, labels))) return finish(rc);
  info->inertia = host.inertia;
  info->changed = host.changed;
  return finish(TMJX_OK);
}

}  // extern "C"
