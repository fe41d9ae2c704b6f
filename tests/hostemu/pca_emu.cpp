// tests/hostemu/pca_emu.cpp — TEST-ONLY host emulation of the PCA and panel C-ABI (include/tmjx.h: tmjx_pca_*, tmjx_plot_strips): the bodies of
// csrc/pca_core.h and the argument checks of csrc/pca_host.h compiled with g++, one loop iteration where the GPU has one thread or workgroup.
// Built like the other emulations; nothing in track_mjx_amd/ loads it.  With -DPCA_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   pca_emu — fits, transforms and draws a few small problems (odd d, a row stride, a scrolling panel with a NaN) and prints a checksum.
#pragma once
#define TM_HOST_EMU 1
#define TM_DEV static inline
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../track_mjx_amd/csrc/pca_host.h"

using namespace tmjx_host;
static std::string g_err;
static int fail(int code, const std::string &e) { g_err = e; return code; }
#define EMU_TRY(expr) do { const std::string e_ = (expr); if (!e_.empty()) return fail(TMJX_EINVAL, e_); } while (0)

extern "C" {
const char *tmjx_last_error(void) { return g_err.c_str(); }

// (static: the wide PCA forwards d <= 128 here, and no call inside the library goes through an exported name)
static int pemu_workspace(int n, int d, int64_t *floats) {
  if (!floats) return fail(TMJX_EINVAL, "null argument");
  EMU_TRY(pca_check_shape(n, d, d));
  *floats = pca_workspace(n, d).floats;
  return 0;
}

static int pemu_fit(const float *x, int n, int d, int64_t ldx, float *mean, float *components, float *variance, float *workspace, tmjx_pca_info_t *info) {
  EMU_TRY(pca_check_fit(x, n, d, ldx, mean, components, variance, workspace, info));
  const PcaWorkspace w = pca_workspace(n, d);
  double *colsum = (double *)(workspace + w.colsum);
  float *gram = workspace + w.gram, *cov = workspace + w.cov;
  PcaInfo *dinfo = (PcaInfo *)(workspace + w.info);
  std::vector<double> s_sum(2 * PCA_MAX_D);
  std::vector<float> s_tile(PCA_KB * PCA_TILE_LD);
  for (int wg = 0; wg < w.nwg; wg++) pca_colsum_wg(x, ldx, n, d, wg, colsum, s_sum.data());
  for (int c = 0; c < d; c++) mean[c] = pca_mean_col(colsum, w.nwg, d, n, c);
  for (int wg = 0; wg < w.nwg; wg++) {
    if (d <= 32) pca_gram_wg<2>(x, ldx, n, d, mean, wg, gram, s_tile.data());
    else if (d <= 64) pca_gram_wg<4>(x, ldx, n, d, mean, wg, gram, s_tile.data());
    else pca_gram_wg<8>(x, ldx, n, d, mean, wg, gram, s_tile.data());
  }
  for (int e = 0; e < d * d; e++) cov[e] = pca_gram_reduce(gram, w.nwg, d, n, e);
  std::vector<double> lds((pca_jacobi_lds_floats(d) + 1) / 2);      // (doubles: the 8-byte alignment the kernel's LDS has)
  pca_jacobi_wg(cov, d, components, variance, dinfo, (float *)lds.data(), 64);
  info->sweeps = dinfo->sweeps; info->converged = dinfo->converged; info->off_rel = dinfo->off_rel;
  info->moments_ms = info->jacobi_ms = 0.f;
  if (!dinfo->converged)
    return fail(TMJX_ENOCONV, "tmjx_pca_fit: the Jacobi solver did not converge in " + std::to_string(dinfo->sweeps) + " sweeps (off / norm = " +
                                  std::to_string(dinfo->off_rel) + "; is every value of x finite?)");
  return 0;
}

static int pemu_transform(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, float *out, int64_t ldo) {
  EMU_TRY(pca_check_transform(x, n, d, ldx, mean, components, k, out, ldo));
  std::vector<float> xc(d);
  for (int r = 0; r < n; r++) {
    for (int j = 0; j < d; j++) xc[j] = x[(int64_t)r * ldx + j] - mean[j];
    for (int c = 0; c < k; c++) out[(int64_t)r * ldo + c] = pca_project(xc.data(), components + (size_t)c * d, d);
  }
  return 0;
}

int tmjx_pca_workspace(int n, int d, int64_t *floats) { return pemu_workspace(n, d, floats); }

int tmjx_pca_fit(const float *x, int n, int d, int64_t ldx, float *mean, float *components, float *variance, float *workspace, tmjx_pca_info_t *info, void *) {
  return pemu_fit(x, n, d, ldx, mean, components, variance, workspace, info);
}

int tmjx_pca_transform(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, float *out, int64_t ldo, void *) {
  return pemu_transform(x, n, d, ldx, mean, components, k, out, ldo);
}

int tmjx_plot_strips(const float *proj, int T, int k, int64_t ldp, const int32_t *frame_idx, const uint8_t *flags, int F, float ymin, float ymax, int window,
                     const tmjx_strip_style_t *style, int W, int H, uint8_t *rgba, void *) {
  PcaStrip s;
  EMU_TRY(pca_check_strips(proj, T, k, ldp, frame_idx, F, ymin, ymax, window, style, W, H, rgba, s));
  for (int f = 0; f < F; f++)
    for (int pix = 0; pix < W * H; pix++) {
      const uint32_t c = pca_strip_pixel(s, proj, frame_idx[f], flags ? flags[f] : 0, pix % W, pix / W);
      memcpy(rgba + 4 * ((size_t)f * W * H + pix), &c, 4);
    }
  return 0;
}
}  // extern "C"

#ifdef PCA_EMU_MAIN
static float lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }

int main() {
  uint32_t seed = 7;
  double sum = 0.0;
  const int shapes[][3] = {{2, 1, 1}, {3, 2, 2}, {65, 7, 12}, {PCA_ROWS_PER_WG + 3, 33, 33}, {40, 65, 70}, {2 * PCA_ROWS_PER_WG + 1, 128, 128}};
  for (const auto &sh : shapes) {
    const int n = sh[0], d = sh[1], ldx = sh[2], k = d < 4 ? d : 4;
    std::vector<float> x((size_t)n * ldx), mean(d), comp((size_t)d * d), var(d), out((size_t)n * k);
    for (float &v : x) v = lcg(seed) + 3.f;
    for (int r = 0; r < n; r++) x[(size_t)r * ldx] += 2.f * lcg(seed);
    int64_t floats = 0;
    if (tmjx_pca_workspace(n, d, &floats)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    std::vector<double> ws((size_t)floats / 2 + 2);
    float *wsa = (float *)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15);
    tmjx_pca_info_t info;
    if (tmjx_pca_fit(x.data(), n, d, ldx, mean.data(), comp.data(), var.data(), wsa, &info, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    if (tmjx_pca_transform(x.data(), n, d, ldx, mean.data(), comp.data(), k, out.data(), k, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    for (float v : var) sum += v;
    for (float v : out) sum += fabs(v);
    printf("pca_emu: %d x %d (ld %d): %d sweeps, off / norm %.2e, largest variance %.6f\n", n, d, ldx, info.sweeps, info.off_rel, var[0]);
  }
  const int T = 12, k = 3, W = 57, H = 41, F = 4;
  std::vector<float> proj((size_t)T * k);
  for (float &v : proj) v = 4.f * lcg(seed);
  proj[5 * k + 1] = NAN;
  const int32_t idx[F] = {0, 1, 7, 12};
  const uint8_t flags[F] = {0, 0, 0, 1};
  tmjx_strip_style_t st;
  memset(&st, 0, sizeof st);
  st.margin_left = 5; st.margin_right = 3; st.margin_top = 2; st.margin_bottom = 4; st.line_half_width = 0.8f; st.marker_radius = 2.5f;
  for (int c = 0; c < 8; c++) st.colour[c][0] = (uint8_t)(30 * c + 20);
  memset(st.background, 255, 4);
  st.terminated[0] = 255;
  std::vector<uint8_t> rgba((size_t)F * W * H * 4);
  for (int window : {5, 530}) {
    if (tmjx_plot_strips(proj.data(), T, k, k, idx, flags, F, -2.2f, 2.2f, window, &st, W, H, rgba.data(), nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    for (uint8_t v : rgba) sum += v;
  }
  printf("pca_emu: checksum %.6f\n", sum);
  return sum > 0.0 ? 0 : 1;
}
#endif
