// tests/hostemu/tsne_emu.cpp — TEST-ONLY host emulation of the behaviour-map C-ABI (include/tmjx.h: tmjx_tsne_workspace, tmjx_knn,
// tmjx_tsne_affinities, tmjx_tsne_gradient, tmjx_tsne_update, tmjx_tsne_fit, tmjx_tsne_place): the bodies of csrc/tsne_core.h and the checks of
// csrc/tsne_host.h compiled with g++, one loop iteration where the GPU has one workgroup or thread, in the order of the launches of
// csrc/tmjx_tsne.hip.  A library of its own: it includes analysis_emu.cpp for the column sums it shares with the k-means and for the wide PCA an
// embedding starts from, and adds the tmjx_knn and tmjx_tsne_* names.  With -DTSNE_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   tsne_emu [n d k] — searches, calibrates, embeds and places one blob problem (300 x 5, 12 neighbours by default, strided) and prints a checksum.
#pragma once
#ifdef TSNE_EMU_MAIN
#undef HMM_EMU_MAIN
#undef KMEANS_EMU_MAIN
#undef PCA_WIDE_EMU_MAIN
#undef PCA_EMU_MAIN
#undef READOUT_EMU_MAIN
#undef SPECTROGRAM_EMU_MAIN
#endif
#include "analysis_emu.cpp"

#include <utility>

#include "../../track_mjx_amd/csrc/tsne_host.h"

static void temu_gradient_run(const float *y, int n, const int32_t *col, const float *val, double exaggeration, float *grad, double *z, double *kl,
                              float *workspace, const TsneWorkspace &w) {
  double *parts = (double *)(workspace + w.parts), *rep = (double *)(workspace + w.rep), *zblock = (double *)(workspace + w.zblock),
         *klblock = (double *)(workspace + w.klblock);
  const int32_t *row_ptr = (const int32_t *)(workspace + w.row_ptr);
  std::vector<float> s_y(2 * TSNE_BLOCK);
  std::vector<double> s_d(TSNE_BLOCK + 1);
  for (int part = 0; part < w.split.P; part++)
    for (int ib = 0; ib < w.nb; ib++) tsne_rep_wg(y, n, w.split, ib, part, parts, s_y.data());
  for (int b = 0; b < w.nb; b++) tsne_rowsum_wg(parts, n, w.split.P, b, rep, zblock, s_d.data());
  for (int b = 0; b < w.nb; b++)
    tsne_attr_wg(y, n, row_ptr, col, val, exaggeration, rep, zblock, w.nb, grad, z, klblock, b, s_d.data(), s_d.data() + TSNE_BLOCK);
  *kl = tsne_total(klblock, w.nb);
}

static void temu_update_run(float *y, const float *grad, float *velocity, float *gains, int n, float momentum, float eta, float min_gain, float *workspace,
                            const TsneWorkspace &w) {
  double *ysum = (double *)(workspace + w.ysum);
  std::vector<double> s_s(2 * TSNE_BLOCK);
  for (int b = 0; b < w.nb; b++) tsne_update_wg(y, grad, velocity, gains, n, momentum, eta, min_gain, b, ysum, s_s.data());
  for (int b = 0; b < w.nb; b++) tsne_center_wg(y, n, ysum, w.nb, b, s_s.data());
}

extern "C" {
int tmjx_tsne_workspace(int n, int64_t m, int d, int k, int64_t *floats) {
  EMU_TRY(tsne_check_workspace(n, m, d, k, floats));
  *floats = tsne_workspace(n, m, d, k).floats;
  return 0;
}

int tmjx_knn(const float *x, int n, int d, int64_t ldx, const float *q, int64_t m, int64_t ldq, int exclude_self, int k, int32_t *idx, float *dist2,
             float *workspace, void *) {
  EMU_TRY(tsne_check_knn(x, n, d, ldx, q, m, ldq, exclude_self, k, idx, dist2, workspace));
  const TsneWorkspace w = tsne_workspace(n, m, d, k);
  double *colsum = (double *)(workspace + w.colsum);
  float *mean = workspace + w.mean, *xnorm = workspace + w.xnorm, *qnorm = workspace + w.qnorm;
  const int self = tsne_knn_self(x, n, ldx, q, m, ldq, exclude_self) ? 1 : 0;
  std::vector<double> s_sum(2 * PCA_WIDE_TILE);
  for (int ch = 0; ch < w.nchunks; ch++)
    for (int cb = 0; cb < pca_wide_tiles(d); cb++) kmeans_colsum_wg(x, ldx, n, d, ch, cb, colsum, s_sum.data());
  for (int c = 0; c < d; c++) mean[c] = kmeans_mean_col(colsum, w.nchunks, d, n, c);
  for (int64_t r = 0; r < n; r++) xnorm[r] = tsne_rownorm(x, ldx, mean, d, r);
  for (int64_t r = 0; r < m; r++) qnorm[r] = tsne_rownorm(q, ldq, mean, d, r);
  // the LDS of a workgroup, of exactly the size the launch asks for
  std::vector<float> lds((tsne_knn_lds(k) + 3) / 4);
  float *s_ld = lds.data() + TSNE_STAGE;
  for (int64_t wg = 0; wg < (m + TSNE_ROWS - 1) / TSNE_ROWS; wg++)
    tsne_knn_wg(x, n, d, ldx, q, m, ldq, self, k, mean, xnorm, qnorm, idx, dist2, wg, lds.data(), s_ld, (uint16_t *)(s_ld + (size_t)k * TSNE_ROWS));
  return 0;
}

int tmjx_tsne_affinities(const float *dist2, int64_t m, int k, double perplexity, float *p, float *beta, void *) {
  EMU_TRY(tsne_check_affinities(dist2, m, k, perplexity, p, beta));
  const double logu = log(perplexity);
  for (int64_t i = 0; i < m; i++) tsne_affinity_row(dist2, k, logu, p, beta, i);
  return 0;
}

int tmjx_tsne_gradient(const float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz, double exaggeration, float *grad,
                       double *z, double *kl, float *workspace, void *) {
  EMU_TRY(tsne_check_gradient(y, n, row_ptr, col, val, nnz, exaggeration, grad, z, kl, workspace));
  const TsneWorkspace w = tsne_workspace(n, 1, 1, 1);
  memcpy(workspace + w.row_ptr, row_ptr, sizeof(int32_t) * ((size_t)n + 1));
  temu_gradient_run(y, n, col, val, exaggeration, grad, z, kl, workspace, w);
  return 0;
}

int tmjx_tsne_update(float *y, const float *grad, float *velocity, float *gains, int n, float momentum, float eta, float min_gain, float *workspace, void *) {
  EMU_TRY(tsne_check_update(y, grad, velocity, gains, n, momentum, eta, min_gain, workspace));
  temu_update_run(y, grad, velocity, gains, n, momentum, eta, min_gain, workspace, tsne_workspace(n, 1, 1, 1));
  return 0;
}

int tmjx_tsne_fit(float *y, int n, const int32_t *row_ptr, const int32_t *col, const float *val, int64_t nnz, int n_iter, double exaggeration,
                  int exaggeration_iters, float momentum_early, float momentum_late, float eta, float min_gain, float *velocity, float *gains,
                  tmjx_tsne_info_t *info, float *workspace, void *) {
  EMU_TRY(tsne_check_fit(y, n, row_ptr, col, val, nnz, n_iter, exaggeration, exaggeration_iters, momentum_early, momentum_late, eta, min_gain, velocity, gains,
                         info, workspace));
  const TsneWorkspace w = tsne_workspace(n, 1, 1, 1);
  float *grad = workspace + w.grad;
  double *res = (double *)(workspace + w.result);
  memcpy(workspace + w.row_ptr, row_ptr, sizeof(int32_t) * ((size_t)n + 1));
  for (int it = 0; it < n_iter; it++) {
    temu_gradient_run(y, n, col, val, tsne_exaggeration_at(it, exaggeration, exaggeration_iters), grad, res, res + 1, workspace, w);
    temu_update_run(y, grad, velocity, gains, n, tsne_momentum_at(it, exaggeration_iters, momentum_early, momentum_late), eta, min_gain, workspace, w);
  }
  temu_gradient_run(y, n, col, val, 1.0, grad, res, res + 1, workspace, w);
  info->n_iter = n_iter; info->pad_ = 0; info->z = res[0]; info->kl = res[1]; info->gradient_ms = info->update_ms = 0.f;
  return 0;
}

int tmjx_tsne_place(const int32_t *idx, const float *p, int64_t m, int k, const float *y_train, int n, float *y_out, void *) {
  EMU_TRY(tsne_check_place(idx, p, m, k, y_train, n, y_out));
  for (int64_t i = 0; i < m; i++) tsne_place_row(idx, p, k, y_train, n, y_out, i);
  return 0;
}
}  // extern "C"

#ifdef TSNE_EMU_MAIN
static float tlcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }
#define TSNE_MAIN_TRY(call) do { if (call) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; } } while (0)

int main(int argc, char **argv) {
  const int n = argc > 3 ? atoi(argv[1]) : 300, d = argc > 3 ? atoi(argv[2]) : 5, k = argc > 3 ? atoi(argv[3]) : 12;
  const int ldx = d + 3, mq = n / 3 + 1, blobs = 3;
  uint32_t seed = 37;
  // every buffer of exactly the size its contract names, so that a sanitizer sees any overrun
  std::vector<float> x((size_t)(n - 1) * ldx + d), q((size_t)(mq - 1) * ldx + d);
  for (int r = 0; r < n; r++)
    for (int c = 0; c < d; c++) x[(size_t)r * ldx + c] = (c == r % blobs ? 6.f : 0.f) + tlcg(seed);
  for (int r = 0; r < mq; r++)
    for (int c = 0; c < d; c++) q[(size_t)r * ldx + c] = (c == r % blobs ? 6.f : 0.f) + tlcg(seed);
  int64_t floats = 0;
  TSNE_MAIN_TRY(tmjx_tsne_workspace(n, n > mq ? n : mq, d, k, &floats));
  std::vector<double> ws((size_t)floats / 2 + (floats & 1));
  float *wsa = (float *)ws.data();
  std::vector<int32_t> idx((size_t)n * k), qidx((size_t)mq * k);
  std::vector<float> dist2((size_t)n * k), p((size_t)n * k), beta(n), qd((size_t)mq * k), qp((size_t)mq * k), qbeta(mq);
  TSNE_MAIN_TRY(tmjx_knn(x.data(), n, d, ldx, x.data(), n, ldx, 1, k, idx.data(), dist2.data(), wsa, nullptr));
  TSNE_MAIN_TRY(tmjx_tsne_affinities(dist2.data(), n, k, k / 3.0 > 1.0 ? k / 3.0 : 1.0, p.data(), beta.data(), nullptr));
  // P = (Pc + Pc^T) / 2n as a CSR with ascending columns
  std::vector<std::vector<std::pair<int, float>>> rows(n);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < k; j++) {
      const int c = idx[(size_t)i * k + j];
      const float v = p[(size_t)i * k + j] / (2.f * (float)n);
      for (int side = 0; side < 2; side++) {
        auto &row = rows[side ? c : i];
        const int key = side ? i : c;
        auto it = row.begin();
        while (it != row.end() && it->first < key) ++it;
        if (it != row.end() && it->first == key) it->second += v; else row.insert(it, {key, v});
      }
    }
  std::vector<int32_t> row_ptr(n + 1, 0), col;
  std::vector<float> val;
  for (int i = 0; i < n; i++) {
    for (auto &e : rows[i]) { col.push_back(e.first); val.push_back(e.second); }
    row_ptr[i + 1] = (int32_t)col.size();
  }
  std::vector<float> y(2 * (size_t)n), vel(2 * (size_t)n, 0.f), gains(2 * (size_t)n, 1.f), y2, vel2, gains2, grad(2 * (size_t)n);
  for (float &v : y) v = 1e-4f * tlcg(seed);
  y2 = y; vel2 = vel; gains2 = gains;
  const int iters = 40, early = 15;
  tmjx_tsne_info_t info;
  TSNE_MAIN_TRY(tmjx_tsne_fit(y.data(), n, row_ptr.data(), col.data(), val.data(), (int64_t)col.size(), iters, 12.0, early, 0.5f, 0.8f, 50.f, 0.01f, vel.data(),
                              gains.data(), &info, wsa, nullptr));
  double z = 0.0, kl = 0.0;
  for (int it = 0; it <= iters; it++) {
    TSNE_MAIN_TRY(tmjx_tsne_gradient(y2.data(), n, row_ptr.data(), col.data(), val.data(), (int64_t)col.size(), it < early && it < iters ? 12.0 : 1.0, grad.data(), &z,
                                     &kl, wsa, nullptr));
    if (it < iters) TSNE_MAIN_TRY(tmjx_tsne_update(y2.data(), grad.data(), vel2.data(), gains2.data(), n, it < early ? 0.5f : 0.8f, 50.f, 0.01f, wsa, nullptr));
  }
  const bool same = !memcmp(y.data(), y2.data(), sizeof(float) * y.size()) && kl == info.kl && z == info.z;
  std::vector<float> out(2 * (size_t)mq);
  TSNE_MAIN_TRY(tmjx_knn(x.data(), n, d, ldx, q.data(), mq, ldx, 0, k, qidx.data(), qd.data(), wsa, nullptr));
  TSNE_MAIN_TRY(tmjx_tsne_affinities(qd.data(), mq, k, k / 3.0 > 1.0 ? k / 3.0 : 1.0, qp.data(), qbeta.data(), nullptr));
  TSNE_MAIN_TRY(tmjx_tsne_place(qidx.data(), qp.data(), mq, k, y.data(), n, out.data(), nullptr));
  double sum = info.kl + info.z;
  for (float v : out) sum += fabs(v);
  for (float v : beta) sum += v;
  printf("tsne_emu: %d x %d (ld %d), %d neighbours, %zu entries of P: %d iterations, kl %.6f, Z %.6f, the fit equals its steps: %d\n", n, d, ldx, k, col.size(),
         info.n_iter, info.kl, info.z, (int)same);
  printf("tsne_emu: checksum %.6f\n", sum);
  return same ? 0 : 1;
}
#endif
