// csrc/lstm_tangent_host.h — the host side the LSTM-decoder-dynamics entry points share with the host emulation
// (tests/hostemu/lstm_dynamics_emu.cpp): the argument checks (an empty string: accepted), the workspace layout and the schedule of the steps.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>

#include "lstm_jacobian_host.h"
#include "lstm_tangent_core.h"

namespace tmjx_host {

static_assert(TMJX_LSTM_TANGENT_MAX_K == LST_MAX_K, "include/tmjx.h and csrc/lstm_tangent_core.h agree on the tangent limit");
#define LST_MAX_SEQ 65536      // sequences of a call (the order kernel compares every pair; S K <= 2^21 tangent rows a step: 16384 product tiles)

// the cells of the descriptor: Wp, bp, ldwp, A and the wrt columns are not read
static inline std::string lst_check_desc(const tmjx_lstm_jacobian_desc_t *d) {
  if (!d) return "null descriptor";
  if (d->H != 32 && d->H != 64 && d->H != 128 && d->H != 256) return "H = " + std::to_string(d->H) + " is none of 32, 64, 128, 256";
  std::string e = jac_range("L", d->L, 1, LSJ_MAX_LAYERS);
  if (e.empty()) e = jac_range("d_in", d->d_in, 1, LSJ_MAX_DIN);
  if (!e.empty()) return e;
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
  return "";
}

static inline std::string lst_check_rows(int S, int K) {
  std::string e = jac_range("K", K, 1, LST_MAX_K);
  if (!e.empty()) return e;
  if (S < 1) return "S must be >= 1 (got " + std::to_string(S) + ")";
  if (S > LST_MAX_SEQ) return "S = " + std::to_string(S) + " sequences exceed " + std::to_string(LST_MAX_SEQ);
  return "";
}

// one workspace, in floats (every part starts at a multiple of 4 floats), for R rows of a step (R = S: the sequences; tmjx_lstm_tangent_step: the
// rows of a pass) and their R K tangent rows; nothing grows with n:
//   xg, hg [R][4H]: a layer's two forward products | h0, h1 [R][H]: a layer's new h, alternating | per layer keep [R][6][H] |
//   dxp, dhp [R K][4H]: a layer's two tangent products | q [R K][2 L H]: the bases of the sequences by slot (tmjx_lstm_lyapunov) |
//   ord [3][R] int32: the first row, the sequence and the length of every slot | seq [R + 1] int32: seq_start on the device
struct LstWorkspace {
  int R, W;
  int64_t xg, hg, h[2], keep[LSJ_MAX_LAYERS], dxp, dhp, q, ord, seq, floats;
};
static inline LstWorkspace lst_workspace(const tmjx_lstm_jacobian_desc_t *d, int R, int K) {
  LstWorkspace w;
  auto up4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  const int H = d->H;
  w.R = R;
  w.W = 2 * d->L * H;
  int64_t at = 0;
  w.xg = at; at += up4((int64_t)R * 4 * H);
  w.hg = at; at += up4((int64_t)R * 4 * H);
  for (int k = 0; k < 2; k++) { w.h[k] = at; at += up4((int64_t)R * H); }
  for (int k = 0; k < d->L; k++) { w.keep[k] = at; at += up4((int64_t)R * LSJ_KEEP * H); }
  w.dxp = at; at += up4((int64_t)R * K * 4 * H);
  w.dhp = at; at += up4((int64_t)R * K * 4 * H);
  w.q = at; at += up4((int64_t)R * K * w.W);
  w.ord = at; at += up4(3 * (int64_t)R);
  w.seq = at; at += up4((int64_t)R + 1);
  w.floats = at;
  return w;
}

static inline std::string lst_check_workspace(const tmjx_lstm_jacobian_desc_t *d, int S, int K, const int64_t *floats) {
  std::string e = lst_check_desc(d);
  if (e.empty()) e = lst_check_rows(S, K);
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string lst_check_common(const tmjx_lstm_jacobian_desc_t *d, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                                           const float *workspace) {
  std::string e = lst_check_desc(d);
  if (!e.empty()) return e;
  if (n < 1) return "n must be >= 1 (got " + std::to_string(n) + ")";
  if (ldx < d->d_in) return "ldx = " + std::to_string((long long)ldx) + " is smaller than d_in = " + std::to_string(d->d_in);
  if (ld_carry < (int64_t)d->L * d->H) return "ld_carry = " + std::to_string((long long)ld_carry) + " is smaller than L H = " + std::to_string(d->L * d->H);
  if (!x || !h_in || !c_in || !workspace) return "null argument";
  if (!pca_al16(workspace)) return "the workspace must be a 16-byte aligned device buffer of tmjx_lstm_tangent_workspace's size";
  if (((uintptr_t)x | (uintptr_t)h_in | (uintptr_t)c_in) & 3) return "x, h_in and c_in must be 4-byte aligned";
  return "";
}

static inline std::string lst_check_step(const tmjx_lstm_jacobian_desc_t *d, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                                         const float *v, int K, const float *out, const float *workspace) {
  std::string e = lst_check_common(d, x, n, ldx, h_in, c_in, ld_carry, workspace);
  if (e.empty()) e = jac_range("K", K, 1, LST_MAX_K);
  if (!e.empty()) return e;
  if (!v || !out) return "null argument";
  if (!pca_al16(v) || !pca_al16(out)) return "the tangents v and out must be 16-byte aligned";
  return "";
}

static inline std::string lst_check_lyapunov(const tmjx_lstm_jacobian_desc_t *d, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in,
                                             int64_t ld_carry, const int32_t *seq_start, int S, const float *q0, int q0_per_seq, int K, int warmup, const float *local,
                                             const float *energy, const float *q_out, const int32_t *status, const double *sums, const float *workspace) {
  std::string e = lst_check_common(d, x, n, ldx, h_in, c_in, ld_carry, workspace);
  if (e.empty()) e = lst_check_rows(S, K);
  if (!e.empty()) return e;
  if (warmup < 0) return "warmup must be >= 0 (got " + std::to_string(warmup) + ")";
  if (q0_per_seq < 0 || q0_per_seq > 1) return "q0_per_seq = " + std::to_string(q0_per_seq) + " is neither 0 (one basis) nor 1 (one a sequence)";
  if (!seq_start || !q0 || !sums) return "null argument";
  if (S > n) return "S = " + std::to_string(S) + " sequences exceed n = " + std::to_string(n) + " rows";
  if (seq_start[0] != 0) return "seq_start[0] = " + std::to_string(seq_start[0]) + " must be 0";
  for (int s = 0; s < S; s++)
    if (seq_start[s + 1] <= seq_start[s])
      return "seq_start[" + std::to_string(s + 1) + "] = " + std::to_string(seq_start[s + 1]) + " does not exceed seq_start[" + std::to_string(s) +
             "] = " + std::to_string(seq_start[s]) + " (ascending offsets, no empty sequence)";
  if (seq_start[S] != n) return "seq_start[S] = " + std::to_string(seq_start[S]) + " must be n = " + std::to_string(n);
  if (!pca_al16(q0) || !pca_al16(q_out)) return "the bases q0 and q_out must be 16-byte aligned";
  if ((uintptr_t)sums & 7) return "sums must be 8-byte aligned";
  if (((uintptr_t)local | (uintptr_t)energy | (uintptr_t)status) & 3) return "local, energy and status must be 4-byte aligned";
  return "";
}

// the lengths of the sequences in descending order: step t has the sequences longer than t, which are the first `active` slots
static inline std::vector<int32_t> lst_lengths(const int32_t *seq_start, int S) {
  std::vector<int32_t> len(S);
  for (int s = 0; s < S; s++) len[s] = seq_start[s + 1] - seq_start[s];
  std::sort(len.begin(), len.end(), std::greater<int32_t>());
  return len;
}

}  // namespace tmjx_host
