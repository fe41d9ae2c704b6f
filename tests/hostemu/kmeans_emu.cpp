// tests/hostemu/kmeans_emu.cpp — TEST-ONLY host emulation of the k-means C-ABI (include/tmjx.h: tmjx_kmeans_workspace, tmjx_kmeans_assign,
// tmjx_kmeans_update, tmjx_kmeans_seed, tmjx_kmeans_fit): the bodies of csrc/kmeans_core.h and the checks of csrc/kmeans_host.h compiled with g++,
// one loop iteration where the GPU has one workgroup, in the order of the launches of csrc/tmjx_kmeans.hip.  It includes pca_wide_emu.cpp for the
// column sums it shares with the wide PCA.  With -DKMEANS_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   kmeans_emu [n d k] — seeds, fits and re-assigns one blob problem (257 x 3 into 2 by default, strided) and prints a checksum.
#pragma once
#ifdef KMEANS_EMU_MAIN
#undef PCA_WIDE_EMU_MAIN
#undef PCA_EMU_MAIN
#endif
#include "pca_wide_emu.cpp"

#include "../../track_mjx_amd/csrc/kmeans_host.h"

static void kemu_assign_run(const float *x, int n, int d, int64_t ldx, const float *centroids, int k, const int32_t *labels_prev, int32_t *labels, float *dist2,
                            double *inertia, int32_t *changed, float *workspace) {
  const KmeansWorkspace w = kmeans_workspace(n, d, k);
  double *colsum = (double *)(workspace + w.colsum), *pin = (double *)(workspace + w.part_inertia);
  float *mean = workspace + w.mean, *cnorm = workspace + w.cnorm;
  int32_t *pch = (int32_t *)(workspace + w.part_changed);
  std::vector<double> s_sum(2 * PCA_WIDE_TILE > PCA_THREADS ? 2 * PCA_WIDE_TILE : PCA_THREADS);
  std::vector<float> s_x(KMEANS_TK * KMEANS_LDX), s_c(KMEANS_TK * KMEANS_LDC);      // (the epilogue's arrays reuse the stages, as in the kernel)
  std::vector<int32_t> s_cnt(PCA_THREADS);
  for (int ch = 0; ch < w.split.nchunks; ch++)
    for (int cb = 0; cb < pca_wide_tiles(d); cb++) kmeans_colsum_wg(x, ldx, n, d, ch, cb, colsum, s_sum.data());
  for (int c = 0; c < d; c++) mean[c] = kmeans_mean_col(colsum, w.split.nchunks, d, n, c);
  for (int j = 0; j < k; j++) cnorm[j] = kmeans_cnorm(centroids, mean, d, j);
  for (int wg = 0; wg < w.nwg_assign; wg++)
    kmeans_assign_wg(x, n, d, ldx, centroids, k, mean, cnorm, labels_prev, labels, dist2, pin, pch, wg, s_x.data(), s_c.data(), s_x.data(), (int32_t *)s_c.data());
  kmeans_totals_wg(pin, pch, w.nwg_assign, inertia, changed, s_sum.data(), s_cnt.data());
}

static void kemu_update_run(const float *x, int n, int d, int64_t ldx, const int32_t *labels, int k, float *centroids, int32_t *counts, float *workspace) {
  const KmeansWorkspace w = kmeans_workspace(n, d, k);
  double *psum = (double *)(workspace + w.part_sum);
  int32_t *pcnt = (int32_t *)(workspace + w.part_cnt);
  std::vector<double> s_img((size_t)k * KMEANS_UTILE);
  std::vector<int32_t> s_cnt(k);
  for (int p = 0; p < w.split.P; p++)
    for (int cb = 0; cb < kmeans_tiles(d, KMEANS_UTILE); cb++) kmeans_update_wg(x, n, d, ldx, labels, k, p, cb, psum, pcnt, s_img.data(), s_cnt.data());
  for (int e = 0; e < k * d; e++) kmeans_update_reduce(psum, pcnt, w.split.P, k, d, centroids, counts, e);
}

extern "C" {
int tmjx_kmeans_workspace(int n, int d, int k, int64_t *floats) {
  EMU_TRY(kmeans_check_workspace(n, d, k, floats));
  *floats = kmeans_workspace(n, d, k).floats;
  return 0;
}

int tmjx_kmeans_assign(const float *x, int n, int d, int64_t ldx, const float *centroids, int k, const int32_t *labels_prev, int32_t *labels, float *dist2,
                       double *inertia, int32_t *changed, float *workspace, void *) {
  EMU_TRY(kmeans_check_assign(x, n, d, ldx, centroids, k, labels, inertia, workspace));
  kemu_assign_run(x, n, d, ldx, centroids, k, labels_prev, labels, dist2, inertia, changed, workspace);
  return 0;
}

int tmjx_kmeans_update(const float *x, int n, int d, int64_t ldx, const int32_t *labels, int k, float *centroids, int32_t *counts, float *workspace, void *) {
  EMU_TRY(kmeans_check_update(x, n, d, ldx, labels, k, centroids, counts, workspace));
  kemu_update_run(x, n, d, ldx, labels, k, centroids, counts, workspace);
  return 0;
}

int tmjx_kmeans_seed(const float *x, int n, int d, int64_t ldx, int k, const double *u, float *centroids, int32_t *index, float *workspace, void *) {
  EMU_TRY(kmeans_check_seed(x, n, d, ldx, k, u, centroids, index, workspace));
  const KmeansWorkspace w = kmeans_workspace(n, d, k);
  float *d2 = workspace + w.d2;
  double *blocksum = (double *)(workspace + w.blocksum);
  int32_t *picks = (int32_t *)(workspace + w.picks);
  std::vector<float> s_p(KMEANS_SEED_ROWS * 17);
  std::vector<double> s_seg(PCA_THREADS);
  int32_t s_pick[1];
  for (int j = 0; j < k; j++) {
    if (j > 0)
      for (int wg = 0; wg < w.nb_seed; wg++) kmeans_seed_dist_wg(x, n, d, ldx, centroids + (int64_t)(j - 1) * d, j == 1 ? 1 : 0, d2, blocksum, wg, s_p.data());
    kmeans_seed_pick_wg(x, n, d, ldx, d2, blocksum, j > 0 ? w.nb_seed : 0, u[j], j, centroids, picks, s_seg.data(), s_pick);
  }
  for (int j = 0; j < k; j++) index[j] = picks[j];
  return 0;
}

int tmjx_kmeans_fit(const float *x, int n, int d, int64_t ldx, int k, float *centroids, int32_t *labels, float *dist2, int max_iter, double tol,
                    tmjx_kmeans_info_t *info, float *workspace, void *) {
  EMU_TRY(kmeans_check_fit(x, n, d, ldx, k, centroids, labels, max_iter, tol, info, workspace));
  const KmeansWorkspace w = kmeans_workspace(n, d, k);
  int32_t *buf[2] = {labels, (int32_t *)(workspace + w.labels2)}, *counts = (int32_t *)(workspace + w.picks);
  double inertia = 0.0, previous = 0.0;
  int32_t changed = 0;
  int it = 0, cur = 0;
  info->n_iter = 0; info->assign_ms = 0.f; info->update_ms = 0.f;
  for (; it < max_iter; it++) {
    kemu_assign_run(x, n, d, ldx, centroids, k, it > 0 ? buf[cur ^ 1] : nullptr, buf[cur], dist2, &inertia, &changed, workspace);
    info->n_iter = it + 1;
    if (kmeans_converged(it, changed, inertia, previous, tol)) break;
    previous = inertia;
    kemu_update_run(x, n, d, ldx, buf[cur], k, centroids, counts, workspace);
    cur ^= 1;
  }
  const int32_t *last = it < max_iter ? buf[cur] : buf[cur ^ 1];
  if (last == labels) {
    memcpy(buf[1], labels, sizeof(int32_t) * (size_t)n);
    last = buf[1];
  }
  kemu_assign_run(x, n, d, ldx, centroids, k, last, labels, dist2, &inertia, &changed, workspace);
  info->inertia = inertia;
  info->changed = changed;
  return 0;
}
}  // extern "C"

#ifdef KMEANS_EMU_MAIN
static float klcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }

int main(int argc, char **argv) {
  const int n = argc > 3 ? atoi(argv[1]) : 257, d = argc > 3 ? atoi(argv[2]) : 3, k = argc > 3 ? atoi(argv[3]) : 2;
  const int ldx = d + 5;
  uint32_t seed = 29;
  std::vector<float> centre((size_t)k * d), x((size_t)n * ldx, 1e6f), c((size_t)k * d), dist2(n);
  for (float &v : centre) v = 8.f * klcg(seed) + 3.f;
  for (int r = 0; r < n; r++)
    for (int col = 0; col < d; col++) x[(size_t)r * ldx + col] = centre[(size_t)(r % k) * d + col] + klcg(seed);
  std::vector<double> u(k);
  for (double &v : u) v = (double)klcg(seed) + 0.5;
  std::vector<int32_t> index(k), labels(n), again(n), counts(k);
  int64_t floats = 0;
  if (tmjx_kmeans_workspace(n, d, k, &floats)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<double> ws((size_t)floats / 2 + 2);      // exactly the size asked for (rounded up to a double), so a sanitizer sees any overrun
  float *wsa = (float *)ws.data();
  tmjx_kmeans_info_t info;
  if (tmjx_kmeans_seed(x.data(), n, d, ldx, k, u.data(), c.data(), index.data(), wsa, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  if (tmjx_kmeans_fit(x.data(), n, d, ldx, k, c.data(), labels.data(), dist2.data(), 50, 0.0, &info, wsa, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  double inertia = 0.0;
  int32_t changed = -1;
  if (tmjx_kmeans_assign(x.data(), n, d, ldx, c.data(), k, labels.data(), again.data(), nullptr, &inertia, &changed, wsa, nullptr)) {
    fprintf(stderr, "%s\n", g_err.c_str());
    return 1;
  }
  if (tmjx_kmeans_update(x.data(), n, d, ldx, again.data(), k, c.data(), counts.data(), wsa, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  double sum = inertia;
  for (float v : c) sum += fabs(v);
  for (int32_t v : counts) sum += v;
  printf("kmeans_emu: %d x %d into %d (ld %d): %d iterations, inertia %.6f, %d labels changed on a second assign\n", n, d, k, ldx, info.n_iter, info.inertia,
         changed);
  printf("kmeans_emu: checksum %.6f\n", sum);
  return changed == 0 && inertia == info.inertia ? 0 : 1;
}
#endif
