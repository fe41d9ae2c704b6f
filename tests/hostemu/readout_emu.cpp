// tests/hostemu/readout_emu.cpp — TEST-ONLY host emulation of the readout C-ABI (include/tmjx.h: tmjx_readout_workspace, tmjx_readout_fit,
// tmjx_readout_weights, tmjx_readout_predict, tmjx_readout_score): the bodies of csrc/readout_core.h and the checks of csrc/readout_host.h compiled
// with g++, one loop iteration where the GPU has one workgroup, in the order of the launches of csrc/tmjx_readout.hip.  It includes
// pca_wide_emu.cpp, so the library also has the PCA entry points, whose fit the readout calls.  With -DREADOUT_EMU_MAIN it is a stand-alone
// program (for sanitizer builds):
//   readout_emu [n d m] — fits, weighs, predicts and scores one problem (300 x 140 -> 70 by default, strided) and prints a checksum.
#pragma once
#ifdef READOUT_EMU_MAIN
#undef PCA_WIDE_EMU_MAIN
#undef PCA_EMU_MAIN
#endif
#include "pca_wide_emu.cpp"

#include "../../track_mjx_amd/csrc/readout_host.h"

extern "C" {
int tmjx_readout_workspace(int n, int d, int m, int n_lambda, int64_t *floats) {
  EMU_TRY(readout_check_workspace(n, d, m, n_lambda, floats));
  int64_t pca = 0, pca_widest = 0;
  int rc = pwemu_workspace(n, d, &pca);
  if (!rc) rc = pwemu_workspace(readout_widest_rows(n), d, &pca_widest);
  if (rc) return rc;
  *floats = readout_workspace_floats(n, d, m, n_lambda, pca, pca_widest);
  return 0;
}

// The floats a fit (*fit) and a score (*score) of exactly n rows touch from the start of the workspace: the ends of the layouts tmjx_readout_fit and
// tmjx_readout_score use (for the test that tmjx_readout_workspace of n rows covers every n' <= n).
int remu_extents(int n, int d, int m, int n_lambda, int64_t *fit, int64_t *score) {
  EMU_TRY(readout_check_workspace(n, d, m, n_lambda, fit));
  int64_t pca = 0;
  int rc = pwemu_workspace(n, d, &pca);
  if (rc) return rc;
  const int64_t below = readout_fit_workspace(n, d, m, pca).floats;
  *fit = below > pca ? below : pca;
  *score = readout_score_workspace(n, m, n_lambda).floats;
  return 0;
}

int tmjx_readout_fit(const float *x, int n, int d, int64_t ldx, const float *y, int m, int64_t ldy, float *mean_x, float *components, float *variance,
                     float *mean_y, float *z, float *workspace, tmjx_pca_info_t *info, void *) {
  EMU_TRY(readout_check_fit(x, n, d, ldx, y, m, ldy, mean_x, components, variance, mean_y, z, workspace, info));
  int64_t pca = 0;
  int rc = pwemu_workspace(n, d, &pca);
  if (rc) return rc;
  if ((rc = pwemu_fit(x, n, d, ldx, mean_x, components, variance, workspace, info))) return rc;
  const ReadoutFitWorkspace w = readout_fit_workspace(n, d, m, pca);
  double *ysum = (double *)(workspace + w.ysum), *cross = (double *)(workspace + w.cross);
  float *c = workspace + w.c;
  const int S = w.split.S;
  std::vector<double> s_sum(2 * PCA_WIDE_TILE);
  std::vector<float> s_x(PCA_KB * PCA_WIDE_TILE), s_y(PCA_KB * READOUT_TILE_M), s_a(PCA_KB * READOUT_LD), s_b(PCA_KB * READOUT_LD);
  for (int s = 0; s < S; s++)
    for (int cb = 0; cb < pca_wide_tiles(m); cb++) pca_wide_colsum_wg(y, ldy, n, m, s, cb, ysum, s_sum.data());
  for (int j = 0; j < m; j++) mean_y[j] = pca_wide_mean_col(ysum, S, m, n, j);
  for (int s = 0; s < S; s++)
    for (int tj = 0; tj < readout_tiles(m, READOUT_TILE_M); tj++)
      for (int ti = 0; ti < pca_wide_tiles(d); ti++) readout_cross_wg(x, ldx, y, ldy, n, d, m, mean_x, mean_y, ti, tj, s, cross, s_x.data(), s_y.data());
  for (int e = 0; e < d * m; e++) c[e] = readout_cross_reduce(cross, S, d, m, n, e);
  for (int r0 = 0; r0 < d; r0 += READOUT_TILE)
    for (int c0 = 0; c0 < m; c0 += READOUT_TILE) readout_gemm_wg<false>(components, c, nullptr, 0.f, d, m, z, r0, c0, s_a.data(), s_b.data());
  return 0;
}

int tmjx_readout_weights(const float *components, const float *variance, const float *z, int d, int m, const double *lambdas, int n_lambda, float *w, void *) {
  EMU_TRY(readout_check_weights(components, variance, z, d, m, lambdas, n_lambda, w));
  std::vector<float> s_a(PCA_KB * READOUT_LD), s_b(PCA_KB * READOUT_LD);
  for (int l = 0; l < n_lambda; l++)
    for (int r0 = 0; r0 < d; r0 += READOUT_TILE)
      for (int c0 = 0; c0 < m; c0 += READOUT_TILE)
        readout_gemm_wg<true>(components, z, variance, (float)lambdas[l], d, m, w + (size_t)l * d * m, r0, c0, s_a.data(), s_b.data());
  return 0;
}

int tmjx_readout_predict(const float *x, int n, int d, int64_t ldx, const float *mean_x, const float *w, const float *mean_y, int m, float *out, int64_t ldo,
                         void *) {
  EMU_TRY(readout_check_predict(x, n, d, ldx, mean_x, w, mean_y, m, out, ldo));
  std::vector<float> s_x(PCA_WIDE_TK * READOUT_LD), s_w(PCA_WIDE_TK * READOUT_LD);
  for (int64_t r0 = 0; r0 < n; r0 += READOUT_ROWS)
    for (int q0 = 0; q0 < m; q0 += READOUT_TILE)
      readout_apply_wg<false>(x, n, d, ldx, mean_x, w, m, m, mean_y, nullptr, 0, out, ldo, nullptr, r0, 1, q0, s_x.data(), s_w.data(), nullptr);
  return 0;
}

int tmjx_readout_score(const float *x, int n, int d, int64_t ldx, const float *y, int m, int64_t ldy, const float *mean_x, const float *w, const float *mean_y,
                       int n_lambda, double *sse, double *sst, float *workspace, void *) {
  EMU_TRY(readout_check_score(x, n, d, ldx, y, m, ldy, mean_x, w, mean_y, n_lambda, sse, sst, workspace));
  const ReadoutScoreWorkspace ws = readout_score_workspace(n, m, n_lambda);
  double *ysum = (double *)(workspace + ws.ysum), *sstp = (double *)(workspace + ws.sst), *ssep = (double *)(workspace + ws.sse);
  const int S = ws.split.S, Q = n_lambda * m, nblocks = ws.split.nchunks;
  std::vector<double> s_sum(2 * PCA_WIDE_TILE), s_red(16 * READOUT_TILE);
  std::vector<float> s_x(PCA_WIDE_TK * READOUT_LD), s_w(PCA_WIDE_TK * READOUT_LD);
  for (int s = 0; s < S; s++)
    for (int cb = 0; cb < pca_wide_tiles(m); cb++) pca_wide_colsum_wg(y, ldy, n, m, s, cb, ysum, s_sum.data());
  for (int s = 0; s < S; s++)
    for (int cb = 0; cb < pca_wide_tiles(m); cb++) readout_sst_wg(y, ldy, n, m, s, cb, ysum, sstp, s_sum.data());
  for (int b = 0; b < nblocks; b++)
    for (int q0 = 0; q0 < Q; q0 += READOUT_TILE)
      readout_apply_wg<true>(x, n, d, ldx, mean_x, w, m, Q, mean_y, y, ldy, nullptr, 0, ssep, (int64_t)b * READOUT_ROWS * READOUT_SCORE_SUB, READOUT_SCORE_SUB,
                             q0, s_x.data(), s_w.data(), s_red.data());
  for (int q = 0; q < Q; q++) sse[q] = readout_sse_col(ssep, nblocks, Q, q);
  for (int c = 0; c < m; c++) sst[c] = readout_sst_col(sstp, S, m, c);
  return 0;
}
}  // extern "C"

#ifdef READOUT_EMU_MAIN
static float rlcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }

int main(int argc, char **argv) {
  const int n = argc > 3 ? atoi(argv[1]) : 300, d = argc > 3 ? atoi(argv[2]) : 140, m = argc > 3 ? atoi(argv[3]) : 70;
  const int ldx = d + 5, ldy = m + 3, ldo = m + 1, L = 3, nt = n / 3 + 2;
  uint32_t seed = 13;
  std::vector<float> x((size_t)n * ldx), y((size_t)n * ldy), mean_x(d), comp((size_t)d * d), var(d), mean_y(m), z((size_t)d * m), w((size_t)L * d * m),
      out((size_t)nt * ldo);
  for (float &v : x) v = rlcg(seed) + 3.f;
  for (int r = 0; r < n; r++)
    for (int c = 0; c < m; c++) y[(size_t)r * ldy + c] = x[(size_t)r * ldx + c % d] - 0.5f * x[(size_t)r * ldx + (c + 1) % d] + 0.1f * rlcg(seed) + 7.f;
  int64_t floats = 0;
  if (tmjx_readout_workspace(n, d, m, L, &floats)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<double> ws((size_t)floats / 2 + 2);
  float *wsa = (float *)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15);
  tmjx_pca_info_t info;
  if (tmjx_readout_fit(x.data(), n, d, ldx, y.data(), m, ldy, mean_x.data(), comp.data(), var.data(), mean_y.data(), z.data(), wsa, &info, nullptr)) {
    fprintf(stderr, "%s\n", g_err.c_str());
    return 1;
  }
  double total = 0.0;
  for (float v : var) total += v;
  const double lambdas[L] = {1e-3 * total / d, 1e-1 * total / d, 10.0 * total / d};
  if (tmjx_readout_weights(comp.data(), var.data(), z.data(), d, m, lambdas, L, w.data(), nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<double> sse((size_t)L * m), sst(m);
  // the score and the predictions on the last nt rows (a ragged block)
  const float *xt = x.data() + (size_t)(n - nt) * ldx, *yt = y.data() + (size_t)(n - nt) * ldy;
  if (tmjx_readout_score(xt, nt, d, ldx, yt, m, ldy, mean_x.data(), w.data(), mean_y.data(), L, sse.data(), sst.data(), wsa, nullptr)) {
    fprintf(stderr, "%s\n", g_err.c_str());
    return 1;
  }
  if (tmjx_readout_predict(xt, nt, d, ldx, mean_x.data(), w.data(), mean_y.data(), m, out.data(), ldo, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  double sum = 0.0, r2 = 0.0;
  for (int c = 0; c < m; c++) r2 += 1.0 - sse[c] / sst[c];
  for (int r = 0; r < nt; r++)
    for (int c = 0; c < m; c++) sum += fabs(out[(size_t)r * ldo + c]);
  for (double v : sse) sum += v;
  printf("readout_emu: %d x %d -> %d (ld %d, %d): %d sweeps, mean R2 of the smallest penalty on %d rows %.6f\n", n, d, m, ldx, ldy, info.sweeps, nt, r2 / m);
  printf("readout_emu: checksum %.6f\n", sum);
  return sum > 0.0 ? 0 : 1;
}
#endif
