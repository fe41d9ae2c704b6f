// csrc/lstm_jacobian_host.h — the host side the LSTM-decoder-Jacobian entry points share with the host emulation
// (tests/hostemu/lstm_jacobian_emu.cpp): the argument checks (an empty string: accepted), the workspace layout and the shapes of one pass.
#pragma once
#include "jacobian_host.h"
#include "lstm_jacobian_core.h"

namespace tmjx_host {

static_assert(TMJX_LSTM_JACOBIAN_MAX_LAYERS == LSJ_MAX_LAYERS, "include/tmjx.h and csrc/lstm_jacobian_core.h agree on the layer limit");

static inline std::string lsj_check_desc(const tmjx_lstm_jacobian_desc_t *d) {
  if (!d) return "null descriptor";
  if (d->H != 32 && d->H != 64 && d->H != 128 && d->H != 256) return "H = " + std::to_string(d->H) + " is none of 32, 64, 128, 256";
  std::string e = jac_range("L", d->L, 1, LSJ_MAX_LAYERS);
  if (e.empty()) e = jac_range("d_in", d->d_in, 1, LSJ_MAX_DIN);
  if (e.empty()) e = jac_range("A", d->A, 1, JAC_MAX_A);
  if (e.empty()) e = jac_range("wrt_cols", d->wrt_cols, 1, JAC_MAX_WRT);
  if (e.empty()) e = jac_range("wrt_col0", d->wrt_col0, 0, INT32_MAX);
  if (!e.empty()) return e;
  if ((int64_t)d->wrt_col0 + d->wrt_cols > d->d_in)
    return "the differentiated columns " + std::to_string(d->wrt_col0) + " .. " + std::to_string((int64_t)d->wrt_col0 + d->wrt_cols) + " exceed d_in = " +
           std::to_string(d->d_in);
  int K = d->d_in;
  for (int k = 0; k < d->L; k++) {
    const tmjx_lstm_jacobian_layer_t &y = d->layer[k];
    const std::string name = "layer " + std::to_string(k);
    if (y.ldwi < K) return name + ": ldwi = " + std::to_string(y.ldwi) + " is smaller than its input width " + std::to_string(K);
    if (y.ldwh < d->H) return name + ": ldwh = " + std::to_string(y.ldwh) + " is smaller than H = " + std::to_string(d->H);
    if (!y.W_ih || !y.W_hh || !y.b_hh) return name + ": null argument";
    if (((uintptr_t)y.W_ih | (uintptr_t)y.W_hh | (uintptr_t)y.b_hh) & 3) return name + ": W_ih, W_hh and b_hh must be 4-byte aligned";
    K = d->H;
  }
  if (d->ldwp < d->H) return "ldwp = " + std::to_string(d->ldwp) + " is smaller than H = " + std::to_string(d->H);
  if (!d->Wp || !d->bp) return "null argument (the projection)";
  if (((uintptr_t)d->Wp | (uintptr_t)d->bp) & 3) return "Wp and bp must be 4-byte aligned";
  return "";
}

// one workspace, in floats (every part starts at a multiple of 4 floats), for R = min(m, JAC_CHUNK) rows of a pass:
//   xg, hg [R][4H]: a layer's two products | h0, h1 [R][max(H, A)]: a layer's new h and the head's product, alternating | per layer keep [R][6][H] |
//   g0, g1 [R A][max(H, wrt_cols)]: the gradient rows, alternating (the last one holds J [R][A][wrt_cols]) | d [R A][4H]: d out / d pre of a layer |
//   cj [R A][2 L H]: the carry Jacobian | float64 partial sums [JAC_CHUNK / JAC_SUM_ROWS][elements of the input sums], then [..][A 2 L H]
struct LsjWorkspace {
  int R, hmax, gmax, E, W;
  int64_t EC, xg, hg, h[2], keep[LSJ_MAX_LAYERS], g[2], d, cj, partial, partial_carry, floats;
};
static inline LsjWorkspace lsj_workspace(const tmjx_lstm_jacobian_desc_t *d, int m) {
  LsjWorkspace w;
  auto up4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  const int H = d->H, A = d->A;
  w.R = m < JAC_CHUNK ? m : JAC_CHUNK;
  w.hmax = H > A ? H : A;
  w.gmax = H > d->wrt_cols ? H : d->wrt_cols;
  w.E = jac_sum_elements(A, d->wrt_cols);
  w.W = 2 * d->L * H;
  w.EC = (int64_t)A * w.W;
  int64_t at = 0;
  w.xg = at; at += up4((int64_t)w.R * 4 * H);
  w.hg = at; at += up4((int64_t)w.R * 4 * H);
  for (int k = 0; k < 2; k++) { w.h[k] = at; at += up4((int64_t)w.R * w.hmax); }
  for (int k = 0; k < d->L; k++) { w.keep[k] = at; at += up4((int64_t)w.R * LSJ_KEEP * H); }
  for (int k = 0; k < 2; k++) { w.g[k] = at; at += up4((int64_t)w.R * A * w.gmax); }
  w.d = at; at += up4((int64_t)w.R * A * 4 * H);
  w.cj = at; at += up4((int64_t)w.R * w.EC);
  w.partial = at; at += up4(2 * (int64_t)(JAC_CHUNK / JAC_SUM_ROWS) * w.E);
  w.partial_carry = at; at += up4(2 * (int64_t)(JAC_CHUNK / JAC_SUM_ROWS) * w.EC);
  w.floats = at;
  return w;
}

static inline std::string lsj_check_workspace(const tmjx_lstm_jacobian_desc_t *d, int m, const int64_t *floats) {
  std::string e = lsj_check_desc(d);
  if (e.empty() && m < 1) e = "m must be >= 1 (got " + std::to_string(m) + ")";
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string lsj_check_call(const tmjx_lstm_jacobian_desc_t *d, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                                         const int32_t *row_index, int m, const float *scale, int64_t ld_scale, const float *carry_scale, int mode,
                                         const float *ctrl_out, const float *jac, const float *gain, const float *col2, const float *row2, const float *action_var,
                                         const float *carry_jac, const float *carry_gain, const double *sums, const float *workspace) {
  std::string e = lsj_check_desc(d);
  if (!e.empty()) return e;
  if (m < 1) return "m must be >= 1 (got " + std::to_string(m) + ")";
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (!row_index && m > n) return "without a row_index the rows are 0 .. m - 1: m = " + std::to_string(m) + " exceeds n = " + std::to_string(n);
  if (ldx < d->d_in) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d_in = " + std::to_string(d->d_in);
  if (ld_carry < (int64_t)d->L * d->H) return "ld_carry = " + std::to_string((long long)ld_carry) + " is smaller than L H = " + std::to_string(d->L * d->H);
  if (mode < 0 || mode > 1) return "mode = " + std::to_string(mode) + " is neither 0 (d ctrl) nor 1 (d loc)";
  if (action_var && !scale) return "action_var needs scale";
  if (scale && ld_scale < d->wrt_cols) return "ld_scale = " + std::to_string((long long)ld_scale) + " is smaller than wrt_cols = " + std::to_string(d->wrt_cols);
  if (!x || !h_in || !c_in || !sums || !workspace) return "null argument";
  if (!pca_al16(workspace)) return "the workspace must be a 16-byte aligned device buffer of tmjx_lstm_jacobian_workspace's size";
  if ((uintptr_t)sums & 7) return "sums must be 8-byte aligned";
  if (((uintptr_t)x | (uintptr_t)h_in | (uintptr_t)c_in | (uintptr_t)row_index | (uintptr_t)scale | (uintptr_t)carry_scale | (uintptr_t)ctrl_out | (uintptr_t)jac |
       (uintptr_t)gain | (uintptr_t)col2 | (uintptr_t)row2 | (uintptr_t)action_var | (uintptr_t)carry_jac | (uintptr_t)carry_gain) & 3)
    return "x, h_in, c_in, row_index, the scales and the outputs must be 4-byte aligned";
  return "";
}

}  // namespace tmjx_host
