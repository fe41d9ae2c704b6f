// csrc/lstm_jacobian_core.h — the bodies the LSTM decoder's Jacobian adds to those of csrc/jacobian_core.h (DESIGN.md "LSTM decoder Jacobian";
// include/tmjx.h: tmjx_lstm_decoder_jacobian): the LSTM cell forward that keeps what its backward needs, the cell backward that turns a gradient with
// respect to a layer's new h into the left operand of the two products with that layer's weights (and into the gradient of the carried c), the
// carry outputs of a row and their float64 sums over the rows.  The products (jac_gemm_wg), the head (jac_head_wg), the input-side outputs
// (jac_outputs_wg) and their sums (jac_sum_rows_wg, jac_sum_add) are those of the MLP decoder's Jacobian.  Written with the PCA_WG / PCA_PAR /
// PCA_SYNC / PCA_PRIVATE discipline, so that they also compile on the host (tests/hostemu/lstm_jacobian_emu.cpp).  Every number is one chain of
// float32 operations in a stated order; no atomics; the bits of a row depend neither on how many rows the call has nor on where the row stands.
//
// The order in which a gate's pre-activation is joined (that of csrc/lstm_kernels.h):  pre = (xg + b_hh) + hg  with xg = the chain
// fmaf(x_k, W_ih[.][k], .) from 0 in ascending k and hg = the chain fmaf(h_k, W_hh[.][k], .) likewise: the input product and the bias first, the
// recurrent product added to their sum.
#pragma once
#include "jacobian_core.h"

#define LSJ_MAX_LAYERS 4
#define LSJ_MAX_H 256
#define LSJ_MAX_DIN 1024
#define LSJ_KEEP 6              // coefficients of a unit the forward keeps for the backward

static_assert(LSJ_MAX_H <= JAC_MAX_WIDTH, "the head and the products are those of the MLP Jacobian");

// ----------------------------------------------------------------------------------------------- the cell forward
// Units 256 blk .. of the pass's [R][H] units of one layer (unit e: row e / H, hidden unit j = e % H).  xg, hg [R][4H]: the two products, gate
// rows i | f | g | o;  c_src: the carried c of this layer (c_in + k H; the rows through `gather` as the products read x: an index outside
// 0 .. n_src - 1 reads zero; without a list row r of the pass is row r of c_src).  With sig = jac_sigmoid (the expression of lstm_sigmoid):
//   pre_q = (xg_q + b_q) + hg_q;  gi = sig(pre_i), gf = sig(pre_f), gg = tanhf(pre_g), go = sig(pre_o);
//   cn = (gf c) + (gi gg): two rounded products and their sum (the unit is built without contraction, as the host is);  tc = tanhf(cn);
//   h_out = go tc.
// Kept, keep [R][LSJ_KEEP][H]:  ka = go fmaf(-tc, tc, 1)  (d h' / d c'),  ki = gg (gi (1 - gi)),  kf = c (gf (1 - gf)),  kg = gi fmaf(-gg, gg, 1),
//   ko = tc (go (1 - go)),  gf.
PCA_WG void lsj_cell_fwd_wg(const float *xg, const float *hg, const float *b, const float *c_src, int64_t ld_carry, const int32_t *gather, int n_src, int R, int H,
                            int blk, float *h_out, float *keep) {
  PCA_PAR(tid, PCA_THREADS) {
    const int64_t e = (int64_t)blk * PCA_THREADS + tid;
    if (e < (int64_t)R * H) {
      const int row = (int)(e / H), j = (int)(e % H);
      const int64_t src = gather ? (int64_t)gather[row] : (int64_t)row;
      const float c = !gather || (src >= 0 && src < n_src) ? c_src[src * ld_carry + j] : 0.f;
      const float *xr = xg + (int64_t)row * 4 * H + j, *hr = hg + (int64_t)row * 4 * H + j;
      const float gi = jac_sigmoid((xr[0] + b[j]) + hr[0]), gf = jac_sigmoid((xr[H] + b[H + j]) + hr[H]);
      const float gg = tanhf((xr[2 * H] + b[2 * H + j]) + hr[2 * H]), go = jac_sigmoid((xr[3 * H] + b[3 * H + j]) + hr[3 * H]);
      const float fc = gf * c, ig = gi * gg, cn = fc + ig, tc = tanhf(cn);
      h_out[e] = go * tc;
      float *kp = keep + (int64_t)row * LSJ_KEEP * H + j;
      kp[0] = go * fmaf(-tc, tc, 1.f);
      kp[H] = gg * (gi * (1.f - gi));
      kp[2 * H] = c * (gf * (1.f - gf));
      kp[3 * H] = gi * fmaf(-gg, gg, 1.f);
      kp[4 * H] = tc * (go * (1.f - go));
      kp[5 * H] = gf;
    }
  }
}

// ----------------------------------------------------------------------------------------------- the cell backward
// Units 256 blk .. of the gradient rows gh [M][H] (row m belongs to row m / A of the pass) = d out / d h' of one layer:
//   gc = gh ka  (d out / d c');  d [M][4H] = gc ki | gc kf | gc kg | gh ko  (d out / d pre: the left operand of the products with W_hh and W_ih);
//   dc [m][j] (row stride ld_dc) = gc gf  (d out / d the carried c).
PCA_WG void lsj_cell_bwd_wg(const float *gh, const float *keep, int M, int A, int H, int blk, float *d, float *dc, int64_t ld_dc) {
  PCA_PAR(tid, PCA_THREADS) {
    const int64_t e = (int64_t)blk * PCA_THREADS + tid;
    if (e < (int64_t)M * H) {
      const int64_t m = e / H;
      const int j = (int)(e % H);
      const float *kp = keep + (m / A) * LSJ_KEEP * H + j;
      const float g = gh[e], gc = g * kp[0];
      float *dr = d + m * 4 * H + j;
      dr[0] = gc * kp[H];
      dr[H] = gc * kp[2 * H];
      dr[2 * H] = gc * kp[3 * H];
      dr[3 * H] = g * kp[4 * H];
      dc[m * ld_dc + j] = gc * kp[5 * H];
    }
  }
}

// ----------------------------------------------------------------------------------------------- the carry outputs of a row
// Row `row` of the pass (position `pos` of the list): C = cj + row A W, [A][W] with W = 2 L H: the h blocks of every layer, then the c blocks.
// carry_jac gets C;  carry_gain [pos][b], b = 0 .. 2 L - 1: with t = C[a][b H + j] carry_scale[b H + j] (t = C[a][b H + j] without a scale), thread
// `tid` folds the elements e = tid, tid + 256, ... of the block's A H (a = e / H, j = e % H) into the chain fmaf(t, t, .) from 0, and the 256
// sums meet in wg_tree.  s_red: [PCA_THREADS] floats of LDS.
PCA_WG void lsj_carry_outputs_wg(const float *cj, int A, int L, int H, int row, int64_t pos, const float *carry_scale, float *carry_jac, float *carry_gain,
                                 float *s_red) {
  const int W = 2 * L * H;
  const float *Cm = cj + (int64_t)row * A * W;
  if (carry_jac) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < A * W; e += PCA_THREADS) carry_jac[pos * A * W + e] = Cm[e];
    }
  }
  if (!carry_gain) return;
  for (int b = 0; b < 2 * L; b++) {
    PCA_PAR(tid, PCA_THREADS) {
      float acc = 0.f;
      for (int e = tid; e < A * H; e += PCA_THREADS) {
        const int a = e / H, j = e % H;
        float t = Cm[(int64_t)a * W + b * H + j];
        if (carry_scale) t = t * carry_scale[b * H + j];
        acc = fmaf(t, t, acc);
      }
      s_red[tid] = acc;
    }
    PCA_SYNC();
    wg_tree<1>(s_red);
    PCA_PAR(tid, PCA_THREADS) {
      if (tid == 0) carry_gain[pos * 2 * L + b] = s_red[0];
    }
    PCA_SYNC();
  }
}

// ----------------------------------------------------------------------------------------------- the carry sums over the rows
// Elements 256 eb .. of the E = A W elements of the rows [i0, i1) of the pass, added in float64 in row order.  out: [E] float64 of this group.
PCA_WG void lsj_carry_sum_rows_wg(const float *cj, int64_t E, int i0, int i1, int eb, double *out) {
  PCA_PAR(tid, PCA_THREADS) {
    const int64_t e = (int64_t)eb * PCA_THREADS + tid;
    if (e < E) {
      double acc = 0.0;
      for (int i = i0; i < i1; i++) acc += (double)cj[(int64_t)i * E + e];
      out[e] = acc;
    }
  }
}
