// csrc/pca_host.h — the host side the PCA entry points share with the host emulation (tests/hostemu/pca_emu.cpp): the argument checks (an empty
// string: accepted), the workspace layout and the panel descriptor built from the caller's style.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "pca_core.h"

namespace tmjx_host {

static inline bool pca_al16(const void *p) { return !((uintptr_t)p & 15); }

static inline std::string pca_check_shape(int n, int d, int64_t ldx) {
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > PCA_MAX_D)
    return "d = " + std::to_string(d) + " exceeds the PCA limit of " + std::to_string(PCA_MAX_D) + " features (A and V are held in one CU's LDS)";
  if (n < 2) return "PCA needs n >= 2 rows (got " + std::to_string(n) + ")";
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  return "";
}

// workspace, in floats: [nwg][d] float64 column sums | [nwg][d][d] partial Gram matrices | [d][d] covariance | the kernel's info
struct PcaWorkspace { int nwg; int64_t colsum, gram, cov, info, floats; };
static inline PcaWorkspace pca_workspace(int n, int d) {
  PcaWorkspace w;
  w.nwg = pca_nwg(n);
  w.colsum = 0;
  w.gram = 2 * (int64_t)w.nwg * d;
  w.cov = w.gram + (int64_t)w.nwg * d * d;
  w.info = (w.cov + (int64_t)d * d + 3) & ~(int64_t)3;
  w.floats = w.info + 4;
  return w;
}

static inline std::string pca_check_fit(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, const float *variance,
                                        const float *workspace, const tmjx_pca_info_t *info) {
  const std::string e = pca_check_shape(n, d, ldx);
  if (!e.empty()) return e;
  if (!x || !mean || !components || !variance || !workspace || !info) return "null argument";
  if (!pca_al16(workspace)) return "the workspace must be a 16-byte aligned device buffer of tmjx_pca_workspace's size";
  return "";
}

static inline std::string pca_check_transform(const float *x, int n, int d, int64_t ldx, const float *mean, const float *components, int k, const float *out,
                                              int64_t ldo) {
  if (d < 1) return "d must be >= 1 (got " + std::to_string(d) + ")";
  if (d > PCA_MAX_D) return "d = " + std::to_string(d) + " exceeds the PCA limit of " + std::to_string(PCA_MAX_D) + " features";
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (ldx < d) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d = " + std::to_string(d);
  if (k < 1 || k > d) return "k = " + std::to_string(k) + " components asked of d = " + std::to_string(d) + " (1 <= k <= d)";
  if (ldo < k) return "ldo = " + std::to_string((long long)ldo) + " is smaller than k = " + std::to_string(k);
  if (!x || !mean || !components || !out) return "null argument";
  return "";
}

static inline uint32_t pca_rgba(const uint8_t *c) { return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | 0xff000000u; }

static inline std::string pca_check_strips(const float *proj, int T, int k, int64_t ldp, const int32_t *frame_idx, int F, float ymin, float ymax, int window,
                                           const tmjx_strip_style_t *st, int W, int H, const uint8_t *rgba, PcaStrip &s) {
  if (!proj || !frame_idx || !st || !rgba) return "null argument";
  if (T < 1) return "T must be >= 1 (got " + std::to_string(T) + ")";
  if (k < 1 || k > PCA_MAX_K) return "k = " + std::to_string(k) + " curves: a panel draws 1 .. " + std::to_string(PCA_MAX_K);
  if (ldp < k) return "ldp = " + std::to_string((long long)ldp) + " is smaller than k = " + std::to_string(k);
  if (F < 1) return "F must be >= 1 (got " + std::to_string(F) + ")";
  if (W < 1 || H < 1) return "W and H must be >= 1 (got " + std::to_string(W) + " x " + std::to_string(H) + ")";
  if (window < 1) return "window must be >= 1 (got " + std::to_string(window) + ")";
  if (!(ymax > ymin) || !(ymax - ymin <= 3.4028234e38f)) return "the y range must be finite with ymax > ymin";
  if (st->margin_left < 0 || st->margin_right < 0 || st->margin_top < 0 || st->margin_bottom < 0) return "margins must be >= 0";
  if (W - st->margin_left - st->margin_right < 3 || H - st->margin_top - st->margin_bottom < 3)
    return "the margins leave a plot rectangle smaller than 3 x 3 pixels in a " + std::to_string(W) + " x " + std::to_string(H) + " panel";
  if (!(st->line_half_width > 0.f) || !(st->marker_radius >= 0.f) || !(st->line_half_width <= 1e4f) || !(st->marker_radius <= 1e4f))
    return "line_half_width must be in (0, 1e4] and marker_radius in [0, 1e4] pixels";
  s.W = W; s.H = H; s.T = T; s.k = k; s.window = window; s.ldp = ldp; s.ymin = ymin; s.ymax = ymax;
  s.x0 = st->margin_left; s.x1 = W - st->margin_right; s.y0 = st->margin_top; s.y1 = H - st->margin_bottom;
  s.hw = st->line_half_width; s.radius = st->marker_radius;
  for (int c = 0; c < PCA_MAX_K; c++) s.colour[c] = pca_rgba(st->colour[c]);
  s.background = pca_rgba(st->background); s.axes = pca_rgba(st->axes); s.terminated = pca_rgba(st->terminated);
  return "";
}

}  // namespace tmjx_host
