// csrc/jacobian_host.h — the host side the decoder-Jacobian entry points share with the host emulation (tests/hostemu/jacobian_emu.cpp): the
// argument checks (an empty string: accepted), the workspace layout and the shapes of one pass of the launches.
#pragma once
#include "jacobian_core.h"
#include "pca_host.h"

namespace tmjx_host {

static_assert(TMJX_JACOBIAN_MAX_LAYERS == JAC_MAX_LAYERS, "include/tmjx.h and csrc/jacobian_core.h agree on the layer limit");

static inline std::string jac_range(const char *name, long long v, long long lo, long long hi) {
  if (v < lo || v > hi) return std::string(name) + " = " + std::to_string(v) + " is outside " + std::to_string(lo) + " .. " + std::to_string(hi);
  return "";
}

static inline std::string jac_check_desc(const tmjx_jacobian_desc_t *d) {
  if (!d) return "null descriptor";
  std::string e = jac_range("L", d->L, 1, JAC_MAX_LAYERS);
  if (e.empty()) e = jac_range("d_in", d->d_in, 1, INT32_MAX);
  if (e.empty()) e = jac_range("A", d->A, 1, JAC_MAX_A);
  if (e.empty()) e = jac_range("wrt_cols", d->wrt_cols, 1, JAC_MAX_WRT);
  if (e.empty()) e = jac_range("wrt_col0", d->wrt_col0, 0, INT32_MAX);
  if (!e.empty()) return e;
  if ((int64_t)d->wrt_col0 + d->wrt_cols > d->d_in)
    return "the differentiated columns " + std::to_string(d->wrt_col0) + " .. " + std::to_string((int64_t)d->wrt_col0 + d->wrt_cols) + " exceed d_in = " +
           std::to_string(d->d_in);
  if (!(d->eps >= 0.f)) return "eps must be >= 0";
  int K = d->d_in;
  for (int l = 0; l < d->L; l++) {
    const tmjx_jacobian_layer_t &y = d->layer[l];
    const std::string name = "layer " + std::to_string(l);
    e = jac_range((name + ": width").c_str(), y.width, 1, JAC_MAX_WIDTH);
    if (!e.empty()) return e;
    if (y.ldw < K) return name + ": ldw = " + std::to_string(y.ldw) + " is smaller than its input width " + std::to_string(K);
    if (!y.W || !y.b || !y.gamma || !y.beta) return name + ": null argument";
    if (((uintptr_t)y.W | (uintptr_t)y.b | (uintptr_t)y.gamma | (uintptr_t)y.beta) & 3) return name + ": W, b, gamma and beta must be 4-byte aligned";
    K = y.width;
  }
  if (d->ldwh < K) return "ldwh = " + std::to_string(d->ldwh) + " is smaller than the last width " + std::to_string(K);
  if (!d->Wh || !d->bh) return "null argument (the head)";
  if (((uintptr_t)d->Wh | (uintptr_t)d->bh) & 3) return "Wh and bh must be 4-byte aligned";
  return "";
}

// one workspace, in floats (every part starts at a multiple of 4 floats), for R = min(m, JAC_CHUNK) rows of a pass:
//   h0, h1 [R][max(width, A)]: a layer's product and output, alternating | per layer xhat [R][H_l], rs [R][H_l] |
//   g0, g1 [R A][max(width, wrt_cols)]: the gradient rows, alternating (the last one holds J [R][A][wrt_cols]) |
//   [JAC_CHUNK / JAC_SUM_ROWS][elements of sums] float64 partial sums
struct JacWorkspace {
  int R, hmax, gmax, E;
  int64_t h[2], xhat[JAC_MAX_LAYERS], rs[JAC_MAX_LAYERS], g[2], partial, floats;
};
static inline JacWorkspace jac_workspace(const tmjx_jacobian_desc_t *d, int m) {
  JacWorkspace w;
  auto up4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  w.R = m < JAC_CHUNK ? m : JAC_CHUNK;
  w.hmax = d->A;
  w.gmax = d->wrt_cols;
  for (int l = 0; l < d->L; l++) {
    if (d->layer[l].width > w.hmax) w.hmax = d->layer[l].width;
    if (d->layer[l].width > w.gmax) w.gmax = d->layer[l].width;
  }
  w.E = jac_sum_elements(d->A, d->wrt_cols);
  int64_t at = 0;
  for (int k = 0; k < 2; k++) { w.h[k] = at; at += up4((int64_t)w.R * w.hmax); }
  for (int l = 0; l < d->L; l++) {
    w.xhat[l] = at; at += up4((int64_t)w.R * d->layer[l].width);
    w.rs[l] = at; at += up4((int64_t)w.R * d->layer[l].width);
  }
  for (int k = 0; k < 2; k++) { w.g[k] = at; at += up4((int64_t)w.R * d->A * w.gmax); }
  w.partial = at; at += up4(2 * (int64_t)(JAC_CHUNK / JAC_SUM_ROWS) * w.E);
  w.floats = at;
  return w;
}

static inline std::string jac_check_workspace(const tmjx_jacobian_desc_t *d, int m, const int64_t *floats) {
  std::string e = jac_check_desc(d);
  if (e.empty() && m < 1) e = "m must be >= 1 (got " + std::to_string(m) + ")";
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string jac_check_call(const tmjx_jacobian_desc_t *d, const float *x, int n, int64_t ldx, const int32_t *row_index, int m, const float *scale,
                                         int64_t ld_scale, int mode, const float *ctrl_out, const float *jac, const float *gain, const float *col2,
                                         const float *row2, const float *action_var, const double *sums, const float *workspace) {
  std::string e = jac_check_desc(d);
  if (!e.empty()) return e;
  if (m < 1) return "m must be >= 1 (got " + std::to_string(m) + ")";
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (!row_index && m > n) return "without a row_index the rows are 0 .. m - 1: m = " + std::to_string(m) + " exceeds n = " + std::to_string(n);
  if (ldx < d->d_in) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d_in = " + std::to_string(d->d_in);
  if (mode < 0 || mode > 1) return "mode = " + std::to_string(mode) + " is neither 0 (d ctrl / d x) nor 1 (d loc / d x)";
  if (action_var && !scale) return "action_var needs scale";
  if (scale && ld_scale < d->wrt_cols) return "ld_scale = " + std::to_string((long long)ld_scale) + " is smaller than wrt_cols = " + std::to_string(d->wrt_cols);
  if (!x || !sums || !workspace) return "null argument";
  if (!pca_al16(workspace)) return "the workspace must be a 16-byte aligned device buffer of tmjx_jacobian_workspace's size";
  if ((uintptr_t)sums & 7) return "sums must be 8-byte aligned";
  if (((uintptr_t)x | (uintptr_t)row_index | (uintptr_t)scale | (uintptr_t)ctrl_out | (uintptr_t)jac | (uintptr_t)gain | (uintptr_t)col2 | (uintptr_t)row2 |
       (uintptr_t)action_var) & 3)
    return "x, row_index, scale and the outputs must be 4-byte aligned";
  return "";
}

static inline int jac_tiles(int64_t count, int per) { return (int)((count + per - 1) / per); }

}  // namespace tmjx_host
