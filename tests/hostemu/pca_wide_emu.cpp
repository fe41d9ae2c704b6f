// tests/hostemu/pca_wide_emu.cpp — TEST-ONLY host emulation of the wide PCA C-ABI (include/tmjx.h: tmjx_pca_wide_workspace, tmjx_pca_fit_wide,
// tmjx_pca_transform_wide): the bodies of csrc/pca_wide_core.h and the checks of csrc/pca_wide_host.h compiled with g++, one loop iteration where
// the GPU has one workgroup, in the order of the launches of csrc/tmjx_pca_wide.hip.  It includes pca_emu.cpp, so the library also has the narrow
// entry points (d <= 128 forwards to them) and the panel.  With -DPCA_WIDE_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   pca_wide_emu [n d] — fits and transforms one problem (130 x 192 by default) and prints a checksum.
#pragma once
#ifdef PCA_WIDE_EMU_MAIN
#undef PCA_EMU_MAIN
#endif
#include "pca_emu.cpp"

#include <stdlib.h>

#include "../../track_mjx_amd/csrc/pca_wide_host.h"

extern "C" {
// (static: the readout's fit is this fit)
static int pwemu_workspace(int n, int d, int64_t *floats) {
  if (d >= 1 && d <= PCA_MAX_D) return pemu_workspace(n, d, floats);
  if (!floats) return fail(TMJX_EINVAL, "null argument");
  EMU_TRY(pca_wide_check_shape(n, d, d));
  *floats = pca_wide_workspace(n, d).floats;
  return 0;
}

static void pwemu_norms(float *ws, const PcaWideWorkspace &w, int d, double *norms) {
  std::vector<double> s_red(2 * PCA_THREADS);
  double *rowsum = (double *)(ws + w.rowsum), *out = (double *)(ws + w.norms);
  for (int row = 0; row < d; row++) pca_wide_rownorm_wg(ws + w.cov, d, row, rowsum, s_red.data());
  for (int which = 0; which < 2; which++) out[which] = pca_wide_norm_total(rowsum, d, which);
  norms[0] = out[0]; norms[1] = out[1];
}

static int pwemu_fit(const float *x, int n, int d, int64_t ldx, float *mean, float *components, float *variance, float *workspace, tmjx_pca_info_t *info) {
  if (d >= 1 && d <= PCA_MAX_D) return pemu_fit(x, n, d, ldx, mean, components, variance, workspace, info);
  EMU_TRY(pca_wide_check_fit(x, n, d, ldx, mean, components, variance, workspace, info));
  const PcaWideWorkspace w = pca_wide_workspace(n, d);
  float *ws = workspace;
  double *colsum = (double *)(ws + w.colsum), *gram = (double *)(ws + w.gram);
  float *A = ws + w.cov, *Vt = ws + w.vt, *sub = ws + w.sub, *J = ws + w.rot, *lam = ws + w.lam;
  PcaInfo *pinfo = (PcaInfo *)(ws + w.info);
  const int tiles = pca_wide_tiles(d), S = w.split.S;
  std::vector<double> s_sum(2 * PCA_WIDE_TILE);
  std::vector<float> s_tile(2 * PCA_KB * PCA_TILE_LD), s_a(PCA_KB * PCA_WIDE_LDA), s_b(PCA_KB * PCA_WIDE_LDB);
  for (int s = 0; s < S; s++)
    for (int cb = 0; cb < tiles; cb++) pca_wide_colsum_wg(x, ldx, n, d, s, cb, colsum, s_sum.data());
  for (int c = 0; c < d; c++) mean[c] = pca_wide_mean_col(colsum, S, d, n, c);
  for (int s = 0; s < S; s++)
    for (int ti = 0; ti < tiles; ti++)
      for (int tj = ti; tj < tiles; tj++) pca_wide_gram_wg(x, ldx, n, d, mean, ti, tj, s, gram, s_tile.data());
  for (int i = 0; i < d; i++)
    for (int j = 0; j < d; j++) { A[(size_t)i * d + j] = pca_wide_gram_reduce(gram, S, d, n, i, j); Vt[(size_t)i * d + j] = i == j ? 1.f : 0.f; }
  info->sweeps = info->converged = 0;
  info->off_rel = info->moments_ms = info->jacobi_ms = 0.f;
  double norms[2];
  pwemu_norms(ws, w, d, norms);
  if (!pca_wide_finite(norms)) return fail(TMJX_EINVAL, pca_wide_nonfinite_message());
  const int players = pca_wide_players(d), slices = (d + PCA_WIDE_PASS - 1) / PCA_WIDE_PASS;
  std::vector<double> lds((pca_jacobi_lds_floats(PCA_MAX_D) + 1) / 2);
  int sweeps = 0;
  bool converged = pca_wide_converged(norms);
  while (!converged && sweeps < PCA_SWEEP_LIMIT) {
    for (int r = 0; r < players - 1; r++) {
      for (int k = 0; k < w.pairs; k++) pca_wide_solve_wg(A, d, r, k, sub, J, lam, pinfo, (float *)lds.data(), 64);
      for (int z = 0; z < 2; z++)
        for (int k = 0; k < w.pairs; k++)
          for (int sl = 0; sl < slices; sl++) pca_wide_rows_wg(z ? Vt : A, d, r, k, J, sl * PCA_WIDE_PASS, s_a.data(), s_b.data());
      for (int k = 0; k < w.pairs; k++)
        for (int sl = 0; sl < slices; sl++) pca_wide_cols_wg(A, d, r, k, J, lam, sl * PCA_WIDE_PASS, s_a.data(), s_b.data());
    }
    sweeps++;
    pwemu_norms(ws, w, d, norms);
    if (!pca_wide_finite(norms)) break;
    converged = pca_wide_converged(norms);
  }
  for (int i = 0; i < d; i++) pca_wide_finish_row(A, Vt, d, i, components, variance);
  info->sweeps = sweeps; info->converged = converged ? 1 : 0; info->off_rel = pca_wide_off_rel(norms);
  if (!converged) return fail(TMJX_ENOCONV, pca_wide_noconv_message(sweeps, info->off_rel));
  return 0;
}

int tmjx_pca_wide_workspace(int n, int d, int64_t *floats) { return pwemu_workspace(n, d, floats); }

int tmjx_pca_fit_wide(const float *x, int n, int d, int64_t ldx, float *mean, float *components, float *variance, float *workspace, tmjx_pca_info_t *info,
                      void *) {
  return pwemu_fit(x, n, d, ldx, mean, components, variance, workspace, info);
}

int tmjx_pca_transform_wide(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, float *out, int64_t ldo, void *) {
  if (d >= 1 && d <= PCA_MAX_D) return pemu_transform(x, n, d, ldx, mean, components, k, out, ldo);
  EMU_TRY(pca_wide_check_transform(x, n, d, ldx, mean, components, k, out, ldo));
  std::vector<float> s_x(PCA_WIDE_TK * PCA_WIDE_TLD), s_c(PCA_WIDE_TK * PCA_WIDE_TLD);
  for (int r0 = 0; r0 < n; r0 += PCA_TROWS) {
    if (k <= 16) pca_wide_transform_wg<1>(x, n, d, ldx, mean, components, k, out, ldo, r0, 0, s_x.data(), s_c.data());
    else
      for (int c0 = 0; c0 < k; c0 += 64) pca_wide_transform_wg<4>(x, n, d, ldx, mean, components, k, out, ldo, r0, c0, s_x.data(), s_c.data());
  }
  return 0;
}
}  // extern "C"

#ifdef PCA_WIDE_EMU_MAIN
static float wlcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }

int main(int argc, char **argv) {
  const int n = argc > 2 ? atoi(argv[1]) : 130, d = argc > 2 ? atoi(argv[2]) : 192, ldx = d + 5, k = 20, ldo = k + 1;
  uint32_t seed = 11;
  std::vector<float> x((size_t)n * ldx), mean(d), comp((size_t)d * d), var(d), out((size_t)n * ldo);
  for (float &v : x) v = wlcg(seed) + 3.f;
  for (int r = 0; r < n; r++)
    for (int j = 0; j < 6 && j < d; j++) x[(size_t)r * ldx + j * 7 % d] += (float)(6 - j) * wlcg(seed);
  int64_t floats = 0;
  if (tmjx_pca_wide_workspace(n, d, &floats)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<double> ws((size_t)floats / 2 + 2);
  float *wsa = (float *)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15);
  tmjx_pca_info_t info;
  if (tmjx_pca_fit_wide(x.data(), n, d, ldx, mean.data(), comp.data(), var.data(), wsa, &info, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  double sum = 0.0;
  for (int kk : {4, k}) {
    if (tmjx_pca_transform_wide(x.data(), n, d, ldx, mean.data(), comp.data(), kk, out.data(), ldo, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    for (int r = 0; r < n; r++)
      for (int c = 0; c < kk; c++) sum += fabs(out[(size_t)r * ldo + c]);
  }
  for (float v : var) sum += v;
  printf("pca_wide_emu: %d x %d (ld %d): %d block sweeps, off / norm %.2e, largest variance %.6f\n", n, d, ldx, info.sweeps, info.off_rel, var[0]);
  printf("pca_wide_emu: checksum %.6f\n", sum);
  return sum > 0.0 ? 0 : 1;
}
#endif
