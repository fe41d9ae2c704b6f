// csrc/lstm_tangent_core.h — the bodies the LSTM decoder's recurrent dynamics add to those of csrc/lstm_jacobian_core.h and csrc/jacobian_core.h
// (DESIGN.md "LSTM decoder dynamics"; include/tmjx.h: tmjx_lstm_tangent_step, tmjx_lstm_lyapunov): the tangent cell, which pushes tangent rows of
// the carry through one layer of the carry-to-carry map, the per-sequence QR that re-orthonormalises them at every step, and the small kernels
// around them (the order of the sequences by length, the first basis).  The forward that gives the six coefficients of a unit is lsj_cell_fwd_wg,
// the products are jac_gemm_wg<true, .>.  Written with the PCA_WG / PCA_PAR / PCA_SYNC / PCA_PRIVATE discipline, so that they also compile on the
// host (tests/hostemu/lstm_dynamics_emu.cpp).  Every number is one chain of float32 operations in a stated order; no atomics; the bits of a row
// or of a sequence depend neither on what else the call holds nor on where it stands.
//
// The carry space has W = 2 L H columns: the h blocks of every layer, then the c blocks (the layout of carry_jac).  A tangent is a row [W].
//
// The order of the tangent map, per layer k = 0 .. L - 1 and unit j, with the kept coefficients ka, ki, kf, kg, ko, gf of the row's forward:
//   dpre_q = dxp_q + dhp_q  for the gates q = i, f, g, o, with dxp = the chain fmaf(dh'_(k-1) [u], W_ih[k][.][u], .) from 0 in ascending u and dhp = the
//     chain fmaf(dh_k [u], W_hh[k][.][u], .) likewise: the input product first, the recurrent product added to it (as the forward joins them).  At
//     k = 0 the input row is held as recorded (dx_0 = 0): dpre_q = dhp_q, no sum;
//   dc' = fmaf(kg, dpre_g, fmaf(kf, dpre_f, fmaf(ki, dpre_i, gf dc))): the rounded product gf dc, then the gates i, f, g one fmaf each;
//   dh' = fmaf(ka, dc', ko dpre_o): the rounded product ko dpre_o, then one fmaf.
#pragma once
#include <float.h>

#include "lstm_jacobian_core.h"

#define LST_MAX_K 32            // tangents of a sequence
#define LST_TM 128              // tangent rows of a product tile (jac_gemm_wg<true, 8>)

static_assert(LST_MAX_K * 2 * LSJ_MAX_LAYERS <= PCA_THREADS, "one thread per local exponent and per batch of energy sums");

// ----------------------------------------------------------------------------------------------- the tangent cell
// Units 256 blk .. of the M tangent rows of one layer (unit e: tangent row m = e / H, which belongs to row m / K of the pass; hidden unit j = e % H).
// dxp (null at layer 0), dhp [M][4H]: the two products, gate rows i | f | g | o;  keep [rows][LSJ_KEEP][H]: the forward's coefficients;  dc_src: this
// layer's c block of the tangents entering (row stride ld_src).  out_h, out_c: this layer's h and c block of the tangents leaving (row stride
// ld_out); out_c may be dc_src (a unit reads its dc before it writes).  The order is the file's.
PCA_WG void lst_cell_wg(const float *dxp, const float *dhp, const float *keep, const float *dc_src, int64_t ld_src, int64_t M, int K, int H, int blk, float *out_h,
                        float *out_c, int64_t ld_out) {
  PCA_PAR(tid, PCA_THREADS) {
    const int64_t e = (int64_t)blk * PCA_THREADS + tid;
    if (e < M * H) {
      const int64_t m = e / H;
      const int j = (int)(e % H);
      const float *kp = keep + (m / K) * LSJ_KEEP * H + j, *hr = dhp + m * 4 * H + j;
      float di = hr[0], df = hr[H], dg = hr[2 * H], dq = hr[3 * H];
      if (dxp) {
        const float *xr = dxp + m * 4 * H + j;
        di = xr[0] + di;
        df = xr[H] + df;
        dg = xr[2 * H] + dg;
        dq = xr[3 * H] + dq;
      }
      float t = kp[5 * H] * dc_src[m * ld_src + j];
      t = fmaf(kp[H], di, t);
      t = fmaf(kp[2 * H], df, t);
      t = fmaf(kp[3 * H], dg, t);
      const float u = kp[4 * H] * dq;
      out_c[m * ld_out + j] = t;
      out_h[m * ld_out + j] = fmaf(kp[0], t, u);
    }
  }
}

// ----------------------------------------------------------------------------------------------- the trees
// `cnt` interleaved sums s_red[k * PCA_THREADS + tid], each in the fixed binary tree of wg_tree (the pairs i, i + half for half = 128 .. 1), the
// additions of a level shared among all the threads; the totals are s_red[k * PCA_THREADS].  The caller's barrier stands between its stores and this.
PCA_WG void lst_tree(float *s_red, int cnt) {
  for (int half = PCA_THREADS / 2; half >= 1; half >>= 1) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int w = tid; w < cnt * half; w += PCA_THREADS) {
        const int k = w / half, i = w % half;
        s_red[k * PCA_THREADS + i] += s_red[k * PCA_THREADS + i + half];
      }
    }
    PCA_SYNC();
  }
}

// ----------------------------------------------------------------------------------------------- the QR of one sequence at one step
// v [K][W]: the tangents of one sequence behind the step's map, in place -> the rows of Q'.  V = Q' R by modified Gram-Schmidt, twice: two sweeps,
// each over the columns j = 0 .. K - 1 in order (a "column" of the factorisation is a row of v):
//   r = sqrtf(the squared norm of v_j: thread `tid` folds the elements e = tid, tid + 256, ... into the chain fmaf(v_e, v_e, .) from 0, the 256 sums
//     meet in the tree);  the column is DEAD where !(r >= FLT_MIN) (zero, subnormal or not a number): q_j = 0; otherwise q_j = v_j / r, element by element;
//   then for every later column i > j:  d = q_j . v_i (the same chains, fmaf(q_e, v_e, .), and tree),  v_i = fmaf(-d, q_j, v_i) element by element.
// Column j reads no later column, and the second sweep orthogonalises every column against the final earlier ones again.  With r1, r2 the norms of
// the two sweeps, R_jj = r1 r2 and the local exponent is  logf(r1) + logf(r2),  -inf for a column dead in either sweep (a dead column is zero, so
// it is dead at every later step).
// Outputs of thread j < K: local_row [K] (optional);  sums_row [K] float64 (null where the row is not counted): += the local exponent;  status: set to 1
// where a column is dead;  energy_row [K][2 L] (optional): the squared norm of q_j inside each block of H columns (the chain fmaf(q_e, q_e, .) of the
// thread's elements of the block, and the tree; 32 / (2 L) columns a batch);  q_out_row [K][W] (optional): a copy of Q'.
// s_red: [LST_MAX_K][PCA_THREADS] floats of LDS;  s_r: [2 LST_MAX_K] floats.
PCA_WG void lst_qr_wg(float *v, int K, int L, int H, float *local_row, double *sums_row, int32_t *status, float *energy_row, float *q_out_row, float *s_red,
                      float *s_r) {
  const int W = 2 * L * H;
  for (int sweep = 0; sweep < 2; sweep++)
    for (int j = 0; j < K; j++) {
      float *vj = v + (int64_t)j * W;
      PCA_PAR(tid, PCA_THREADS) {
        float acc = 0.f;
        for (int e = tid; e < W; e += PCA_THREADS) acc = fmaf(vj[e], vj[e], acc);
        s_red[tid] = acc;
      }
      PCA_SYNC();
      lst_tree(s_red, 1);
      const float r = sqrtf(s_red[0]);
      const bool dead = !(r >= FLT_MIN);
      PCA_SYNC();
      const int cnt = K - 1 - j;
      PCA_PAR(tid, PCA_THREADS) {
        if (tid == 0) s_r[sweep * LST_MAX_K + j] = dead ? 0.f : r;
        for (int e = tid; e < W; e += PCA_THREADS) vj[e] = dead ? 0.f : vj[e] / r;
        for (int c = 0; c < cnt; c++) {
          const float *vi = vj + (int64_t)(c + 1) * W;
          float acc = 0.f;
          for (int e = tid; e < W; e += PCA_THREADS) acc = fmaf(vj[e], vi[e], acc);
          s_red[c * PCA_THREADS + tid] = acc;
        }
      }
      PCA_SYNC();
      if (cnt > 0) {
        lst_tree(s_red, cnt);
        PCA_PAR(tid, PCA_THREADS) {
          for (int c = 0; c < cnt; c++) {
            float *vi = vj + (int64_t)(c + 1) * W;
            const float d = s_red[c * PCA_THREADS];
            for (int e = tid; e < W; e += PCA_THREADS) vi[e] = fmaf(-d, vj[e], vi[e]);
          }
        }
        PCA_SYNC();
      }
    }
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < K) {
      const float r1 = s_r[tid], r2 = s_r[LST_MAX_K + tid];
      const float le = r1 > 0.f && r2 > 0.f ? logf(r1) + logf(r2) : -INFINITY;
      if (local_row) local_row[tid] = le;
      if (sums_row) sums_row[tid] += (double)le;
    }
    if (tid == 0) {
      bool any = false;
      for (int j = 0; j < K; j++) any = any || !(s_r[j] > 0.f && s_r[LST_MAX_K + j] > 0.f);
      if (any && status) *status = 1;
    }
    if (q_out_row)
      for (int e = tid; e < K * W; e += PCA_THREADS) q_out_row[e] = v[e];
  }
  if (!energy_row) return;
  const int B = 2 * L, per = LST_MAX_K / B;
  for (int j0 = 0; j0 < K; j0 += per) {
    const int nb = K - j0 < per ? K - j0 : per;
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      for (int c = 0; c < nb * B; c++) s_red[c * PCA_THREADS + tid] = 0.f;
      for (int c = 0; c < nb; c++) {
        const float *q = v + (int64_t)(j0 + c) * W;
        for (int e = tid; e < W; e += PCA_THREADS) {
          float *slot = s_red + (c * B + e / H) * PCA_THREADS + tid;
          *slot = fmaf(q[e], q[e], *slot);
        }
      }
    }
    PCA_SYNC();
    lst_tree(s_red, nb * B);
    PCA_PAR(tid, PCA_THREADS) {
      if (tid < nb * B) energy_row[j0 * B + tid] = s_red[tid * PCA_THREADS];
    }
  }
}

// ----------------------------------------------------------------------------------------------- the order of the sequences
// Sequence s = 256 blk + tid of seq_start [S + 1]: its slot is the number of sequences that are longer, or as long and earlier (descending length,
// ties in the order given: the active sequences of a step are then the first slots).  ord [3][S]: the first row, the sequence and the length of
// every slot.
PCA_WG void lst_order_wg(const int32_t *seq_start, int S, int blk, int32_t *ord) {
  PCA_PAR(tid, PCA_THREADS) {
    const int s = blk * PCA_THREADS + tid;
    if (s < S) {
      const int len = seq_start[s + 1] - seq_start[s];
      int slot = 0;
      for (int o = 0; o < S; o++) {
        const int lo = seq_start[o + 1] - seq_start[o];
        slot += lo > len || (lo == len && o < s) ? 1 : 0;
      }
      ord[slot] = seq_start[s];
      ord[S + slot] = s;
      ord[2 * S + slot] = len;
    }
  }
}

// Elements 256 blk .. of the first basis q [S][K W] by slot: that of the slot's sequence in q0 (of the one basis without q0_per_seq).  The threads
// of the first K S elements also clear sums [S][K]; those of the first S status [S] (where there is one).
PCA_WG void lst_init_wg(const float *q0, int q0_per_seq, const int32_t *ord, int S, int K, int W, int blk, float *q, double *sums, int32_t *status) {
  PCA_PAR(tid, PCA_THREADS) {
    const int64_t e = (int64_t)blk * PCA_THREADS + tid, KW = (int64_t)K * W;
    if (e < S * KW) {
      const int slot = (int)(e / KW);
      q[e] = q0[(q0_per_seq ? (int64_t)ord[S + slot] * KW : 0) + e % KW];
      if (e < (int64_t)S * K) sums[e] = 0.0;
      if (status && e < S) status[e] = 0;
    }
  }
}
