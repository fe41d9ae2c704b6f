// csrc/lstm_decoder_act.h — the LSTM decoder policy of a high-level env as ONE launch (include/tmjx.h: tmjx_lstm_decoder_act; the decoder half of
// the LSTM roll-out step, agent/lstm.py LSTMIntentionPolicy.step, driven with latents as environment/wrappers.py HighLevelWrapper does):
//
//   x_0 = [latents | (obs[ref_w:] - mean) / std]
//   layer k = 0 .. L-1:  (h_k, c_k) zeroed where reset != 0;  gates = x_k W_i,k^T + h_k W_h,k^T + b_h,k  (i | f | g | o);
//                        c_k' = sig(f) c_k + sig(i) tanh(g);  h_k' = sig(o) tanh(c_k');  x_{k+1} = h_k'
//   logits = x_L W_p^T + b_p;  action = tanh(logits[0..A))  ->  action_t [A][n]  (+ ctrl [n][A], logits [n][2A] on request)
//
// Qualifying shapes: H = 128, 1 <= L <= 4, Z + obs_w - ref_w <= 320, 2A <= 128, weight rows 16-byte aligned, any n >= 1 (tmjx_lstm_decoder_act_ok).
// Written: action_t, the carry h / c [n][ld >= L H] in place (columns [k H, (k + 1) H) of layer k, rows < n only), and ctrl / logits where given (their
// first A / 2A columns of rows < n).  Nothing else reaches global memory: the input x_0, the gates, the layers' inputs and the cell state in flight stay
// on the CU.
//
// Tile: 32 rows per workgroup of 256 threads (4 waves) — 128 / 256 workgroups at 4 096 / 8 192 envs, decoder_act.h's reasoning.  The contractions run on
// v_mfma_f32_16x16x4_f32 with the weight fragment as the FIRST operand (mlp_chain.h's transposed tiles): register r of a 16 x 16 tile is
// C[row 16 a + li][column 4 kq + r] for lane (li, kq).
//
// Gate mapping — by the wave-to-column mapping, NOT by repacked weights: wave w owns hidden units [32 w, 32 w + 32) of ALL FOUR gates, i.e. the eight
// 16-column tiles (g, b) = weight rows g H + 32 w + 16 b + [0, 16) of the unmodified [4H][K] matrices.  A lane then holds i, f, g and o of the same four
// units of a row in acc[a][2 g + b][r]: the cell update needs no exchange.  32 x 512 gates = 64 accumulator registers per thread.
//
// LDS (122 880 B, one workgroup per CU):
//   X image [32][320]   the layer's input rows, 16-byte chunks XOR-swizzled by (row & 15); layer 0: built on the CU (decoder_io.h: dec_build_ximg);
//                       layer k > 0: h_{k-1}' in its first 128 columns, written from the cell update's registers
//   H image [32][128]   the layer's carried h_k (zero where reset), same swizzle
//   two weight stages [512][16]: K slabs of 16 of all 512 gate rows (chunk ^ 3 for rows with bit 3 set: each ds_read_b128 lane group of MI355X hits
//                       16 distinct 16-byte slots), global -> registers -> LDS, the next slab requested before the current one's MFMAs
// c_k is read from global memory into the registers of the lane that updates it; only the final carry is stored.
//
// Math: sig = lstm_sigmoid and tanh = tanhf, the expressions of lstm_kernels.h (not the fast forms of silu_math.h).  One accumulator chain per gate
// element runs over the input columns and then the hidden columns, the bias is added last: the gates are within rounding of, not bit-identical to, the
// layer-by-layer path's (x W_i^T + b) + h W_h^T.
#pragma once
#include "decoder_io.h"
#include "lstm_kernels.h"

#define LDA_NT 256
#define LDA_BM 32
#define LDA_H 128
#define LDA_WSTAGE (512 * 16)
#define LDA_MAX_LAYERS 4
#define LDA_LDS_FLOATS (LDA_BM * DEC_XLD + LDA_BM * LDA_H + 2 * LDA_WSTAGE)

struct LstmDecLayer { const float *Wi, *Wh, *bh; int ldwi, ldwh; };
struct LstmDecAct {
  DecoderIn in;
  const float *reset;
  int L;
  LstmDecLayer l[LDA_MAX_LAYERS];
  const float *Wp, *bp; int ldwp;
  float *h, *c; int ld;
  DecoderOut out;
};

// acc[a][j] += A[32 rows][K] . W[n][K]^T for the wave's NJ column tiles: tile j covers weight rows (j >> 1) * 128 + 32 wave + 16 (j & 1) + [0, 16).
// aimg: the swizzled LDS image of A (ald floats per row, zeros from column K on up to the next multiple of 16).  Rows n >= N and columns k >= K of W
// are read as exact zeros.  The first barrier also publishes what the caller wrote to the images; the last one leaves images and stages dead.
template <int NJ>
__device__ __forceinline__ void lda_gemm(df4 (&acc)[2][NJ], const float *aimg, int ald, const float *W, int ldw, int N, int K, float *wst,
                                         int t, int wave, int li, int kq) {
  constexpr int NP = 64 * NJ * 4 / LDA_NT;          // float4 per thread per slab (64 NJ weight rows of 16 floats)
  df4 rg[NP];
  auto gload = [&](int k0) {
#pragma unroll
    for (int p = 0; p < NP; p++) {
      const int f = t + LDA_NT * p, n = f >> 2, k = k0 + 4 * (f & 3);
      df4 v = {0.f, 0.f, 0.f, 0.f};
      if (n < N && k < K) {                          // (ldw is a multiple of 4 and >= K: the four floats are inside the row)
        v = *reinterpret_cast<const df4 *>(W + (long long)n * ldw + k);
        if (k + 3 >= K) {
#pragma unroll
          for (int j = 1; j < 4; j++) if (k + j >= K) v[j] = 0.f;
        }
      }
      rg[p] = v;
    }
  };
  auto swrite = [&](int stage) {
    float *sb = wst + stage * LDA_WSTAGE;
#pragma unroll
    for (int p = 0; p < NP; p++) {
      const int f = t + LDA_NT * p, n = f >> 2, ch = f & 3;
      *reinterpret_cast<df4 *>(sb + n * 16 + ((ch ^ (((n >> 3) & 1) * 3)) << 2)) = rg[p];
    }
  };
  const int nk = (K + 15) >> 4;
  gload(0); swrite(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt++) {
    const bool more = kt + 1 < nk;                   // (uniform)
    if (more) gload(16 * (kt + 1));
    const float *sb = wst + (kt & 1) * LDA_WSTAGE;
    df4 fa[2], fb[NJ];
#pragma unroll
    for (int a = 0; a < 2; a++) fa[a] = *reinterpret_cast<const df4 *>(aimg + (16 * a + li) * ald + (((4 * kt + kq) ^ li) << 2));
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const int n = (j >> 1) * 128 + 32 * wave + 16 * (j & 1) + li;
      fb[j] = *reinterpret_cast<const df4 *>(sb + n * 16 + ((kq ^ (((li >> 3) & 1) * 3)) << 2));
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[j][e], fa[a][e], acc[a][j], 0, 0, 0);
    if (more) swrite((kt + 1) & 1);                  // (the other stage: its readers passed the previous barrier)
    __syncthreads();
  }
}

__global__ __launch_bounds__(LDA_NT) void k_lstm_decoder_act(const LstmDecAct P) {
  constexpr int BM = LDA_BM, H = LDA_H;
  extern __shared__ __attribute__((aligned(16))) float lda_lds[];
  float *ximg = lda_lds, *himg = ximg + BM * DEC_XLD, *wst = himg + BM * H;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.x * BM, M = P.in.M, K1 = P.in.Z + P.in.prop;
  const int ld = P.ld;
  dec_build_ximg<BM, LDA_NT>(ximg, P.in, m0, t);            // the X image of layer 0
  bool rs[2];                                              // the row's carry starts from zero
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const int row = m0 + 16 * a + li;
    rs[a] = row < M && P.reset && P.reset[row] != 0.f;
  }
  const bool vec = !(ld & 3) && !((uintptr_t)P.h & 15) && !((uintptr_t)P.c & 15);
  for (int k = 0; k < P.L; k++) {
    const LstmDecLayer &Y = P.l[k];
    // ---- the H image: the carried h_k (the previous layer's last barrier left it dead)
    for (int it = t; it < BM * (H / 4); it += LDA_NT) {
      const int r = it >> 5, c4 = it & 31, row = m0 + r;
      df4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < M && !(P.reset && P.reset[row] != 0.f)) {
        const float *src = P.h + (long long)row * ld + k * H + 4 * c4;
        if (vec) v = *reinterpret_cast<const df4 *>(src);
        else { v[0] = src[0]; v[1] = src[1]; v[2] = src[2]; v[3] = src[3]; }
      }
      *reinterpret_cast<df4 *>(himg + r * H + ((c4 ^ (r & 15)) << 2)) = v;
    }
    df4 acc[2][8];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int j = 0; j < 8; j++) acc[a][j] = df4{0.f, 0.f, 0.f, 0.f};
    lda_gemm<8>(acc, ximg, DEC_XLD, Y.Wi, Y.ldwi, 4 * H, k == 0 ? K1 : H, wst, t, wave, li, kq);
    lda_gemm<8>(acc, himg, H, Y.Wh, Y.ldwh, 4 * H, H, wst, t, wave, li, kq);
    // ---- the cell: lane (li, kq) of wave `wave` holds the four gates of units 32 wave + 16 b + 4 kq + r of rows 16 a + li
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const int u0 = 32 * wave + 16 * b + 4 * kq;
      float bi[4], bf[4], bg[4], bo[4];
#pragma unroll
      for (int r = 0; r < 4; r++) { bi[r] = Y.bh[u0 + r]; bf[r] = Y.bh[H + u0 + r]; bg[r] = Y.bh[2 * H + u0 + r]; bo[r] = Y.bh[3 * H + u0 + r]; }
#pragma unroll
      for (int a = 0; a < 2; a++) {
        const int row = m0 + 16 * a + li;
        const long long off = (long long)row * ld + k * H + u0;
        df4 cp = {0.f, 0.f, 0.f, 0.f};
        if (row < M && !rs[a]) {
          if (vec) cp = *reinterpret_cast<const df4 *>(P.c + off);
          else { cp[0] = P.c[off]; cp[1] = P.c[off + 1]; cp[2] = P.c[off + 2]; cp[3] = P.c[off + 3]; }
        }
        df4 hn, cn;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float gi = lstm_sigmoid(acc[a][b][r] + bi[r]), gf = lstm_sigmoid(acc[a][2 + b][r] + bf[r]);
          const float gg = tanhf(acc[a][4 + b][r] + bg[r]), go = lstm_sigmoid(acc[a][6 + b][r] + bo[r]);
          cn[r] = gf * cp[r] + gi * gg;
          hn[r] = go * tanhf(cn[r]);
        }
        if (row < M) {
          if (vec) { *reinterpret_cast<df4 *>(P.h + off) = hn; *reinterpret_cast<df4 *>(P.c + off) = cn; }
          else {
#pragma unroll
            for (int r = 0; r < 4; r++) { P.h[off + r] = hn[r]; P.c[off + r] = cn[r]; }
          }
        }
        // h_k' is the next layer's (or the head's) A operand: chunk u0 / 4 of row 16 a + li of the X image (every reader of it passed the last barrier)
        *reinterpret_cast<df4 *>(ximg + (16 * a + li) * DEC_XLD + (((u0 >> 2) ^ li) << 2)) = hn;
      }
    }
  }
  // ---- the projection and the tail: wave w owns logits columns [32 w, 32 w + 32), two 16-column tiles
  df4 accf[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) accf[a][b] = df4{0.f, 0.f, 0.f, 0.f};
  const int Nf = 2 * P.out.A;
  lda_gemm<2>(accf, ximg, DEC_XLD, P.Wp, P.ldwp, Nf, H, wst, t, wave, li, kq);
#pragma unroll
  for (int b = 0; b < 2; b++) {
    const int col = 32 * wave + 16 * b + 4 * kq;
    const df4 bv = dec_head_bias(P.bp, col, Nf);
#pragma unroll
    for (int a = 0; a < 2; a++) dec_tail(P.out, M, accf[a][b], bv, m0 + 16 * a + li, col);
  }
}
