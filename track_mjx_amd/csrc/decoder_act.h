// csrc/decoder_act.h — the decoder policy of a high-level env as ONE launch (include/tmjx.h: tmjx_decoder_act; reference:
// track_mjx/agent/mlp_ppo/intention_network.py:194-222 make_decoder_policy, environment/wrappers.py:384-412 HighLevelWrapper):
//
//   x = [latents | (obs[ref_w:] - mean) / std]  ->  Dense -> SiLU -> LayerNorm blocks (256 wide)  ->  action head  ->  tanh  ->  action_t [A][n]
//
// It is the INFERENCE form of the forward chain of mlp_chain.h: the same ChainGemm K loops (k-ordered MFMA chains) and the same EPI 1 epilogue
// expressions, so the logits are bit-identical to tmjx_latent_concat_det -> tmjx_chain_fwd and the actions to tmjx_action_mode of them — but
//   front   the first GEMM's A operand is the X image built on the CU (decoder_io.h: dec_build_ximg), the first weight tiles travelling meanwhile;
//   middle  a hidden layer's output lives in the LDS Y image only: no z, no y, no row statistics leave the CU (the K loops run without the
//           image-to-global transit of the training chain, kstep<.., TR = 0>);
//   tail    from the head's accumulators, one 16-column tile per wave (decoder_io.h: dec_tail): action_t [A][n], optionally ctrl [n][A] and logits.
//
// Row tile: 32 rows (MT = 2).  The launch sits between two physics steps, alone on the device, and the batch is a roll-out's (4 096 .. 8 192 envs): 32-row
// tiles make 128 / 256 workgroups for the 256 CUs where 80-row tiles make 52 / 103 — the row-tile cost model of the layer-by-layer GEMMs (gemm_mt:
// 2.2 against 5.0 per wave of workgroups) picks the same tile for every M <= 8 192.  LDS: the X image (32 x 320 floats, the Y image [32][256] aliases
// its front once the first K loop is done) + two weight stages + the reduction scratch = 111 616 B, one workgroup per CU.
#pragma once
#include "decoder_io.h"
#include "mlp_chain.h"

#define DEC_MT 2
struct DecoderBlock { const float *W, *bias, *gamma, *beta; int ldw; };
struct DecoderAct {
  DecoderIn in;
  int nh;
  DecoderBlock h[CHAIN_MAX_HIDDEN];
  const float *Wf, *bf; int ldwf;
  float eps;
  DecoderOut out;
};
template <int MT> struct DecoderLds {
  static constexpr int BM = 16 * MT, XIMG = BM * DEC_XLD, TOTAL = XIMG + 2 * CH_WSTAGE + 4 * BM * 8;
  static_assert(DEC_XLD >= 256 && DEC_XLD % 64 == 0, "the Y image aliases the X image; whole swizzle groups per row");
};

template <int MT>
__global__ __launch_bounds__(CH_NT) void k_decoder_act(const DecoderAct P) {
  using LD = DecoderLds<MT>;
  constexpr int BM = LD::BM, NW = 8;
  extern __shared__ __attribute__((aligned(16))) float gemm_lds[];
  float *ximg = gemm_lds, *yimg = gemm_lds, *wst = gemm_lds + LD::XIMG, *red1 = wst + 2 * CH_WSTAGE, *red2 = red1 + BM * NW;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4, nw = wave * 32;
  const int m0 = blockIdx.x * BM, M = P.in.M;
  const int K1 = P.in.Z + P.in.prop;
  gf4 acc[MT][2];
  auto zero = [&]() {
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) acc[a][b] = gf4{0.f, 0.f, 0.f, 0.f};
  };
  zero();
  {
    // ---- first block's GEMM: A = the X image, K = Z + prop (masked weight loads in the last partial tile, as ChainGemm's global-A form)
    ChainGemm<MT, 2, true, true, DEC_XLD> G0;
    G0.init(nullptr, 0, M, m0, P.h[0].W, P.h[0].ldw, 256, K1, ximg, wst);
    G0.gload(G0.R0, 0); G0.gload(G0.R1, GEMM_BK);        // the first weight tiles travel while the image is built
    dec_build_ximg<BM, CH_NT>(ximg, P.in, m0, t);
    G0.template swrite<true>(G0.R0, 0); G0.gload(G0.R0, 2 * GEMM_BK);
    __syncthreads();
    G0.fread(G0.F0, 0, 0, 0);
    const int nk = (K1 + GEMM_BK - 1) / GEMM_BK;
    int kt = 0;
    const int nfast = (K1 % GEMM_BK) == 0 ? nk : max(0, (nk - 4) & ~1);
    for (; kt + 1 < nfast; kt += 2) { G0.template kstep<true>(acc, G0.R1, 0, kt); G0.template kstep<true>(acc, G0.R0, 1, kt + 1); }
    if (kt < nfast) { G0.template kstep<true>(acc, G0.R1, 0, kt); kt = nk; }
    for (; kt + 1 < nk; kt += 2) { G0.template kstep<false>(acc, G0.R1, 0, kt); G0.template kstep<false>(acc, G0.R0, 1, kt + 1); }
    if (kt < nk) G0.template kstep<false>(acc, G0.R1, 0, kt);
  }
  ChainGemm<MT, 2, true, true> G;
  ChainGemm<MT, 1, true, true> Gf;
  for (int l = 0;; l++) {
    const DecoderBlock &H = P.h[l];
    const bool more = l + 1 < P.nh;         // (uniform)
    if (more) { G.init(nullptr, 0, M, m0, P.h[l + 1].W, P.h[l + 1].ldw, 256, 256, yimg, wst); G.early(); }
    else { Gf.init(nullptr, 0, M, m0, P.Wf, P.ldwf, 2 * P.out.A, 256, yimg, wst); Gf.early(); }
    // ---- block l's epilogue: k_chain_fwd's EPI 1, expression for expression, without the z / stats stores
    gf4 bv[2], gv[2], bev[2];
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const int col = nw + 16 * b + 4 * kq;
      bv[b] = *reinterpret_cast<const gf4 *>(H.bias + col);
      gv[b] = *reinterpret_cast<const gf4 *>(H.gamma + col); bev[b] = *reinterpret_cast<const gf4 *>(H.beta + col);
    }
    float stat[MT];
#pragma unroll
    for (int a = 0; a < MT; a++) {
      float p = 0.f;
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) { const float v = acc[a][b][r] + bv[b][r]; acc[a][b][r] = tm_silu(v); p += acc[a][b][r]; }
      p += __shfl_xor(p, 16); stat[a] = p + __shfl_xor(p, 32);
    }
    __syncthreads();                   // every wave has read its last fragments (the images and the stages are dead)
    auto exchange = [&](float *red) {  // stat[a] <- sum over the waves
      if (kq == 0) {
#pragma unroll
        for (int a = 0; a < MT; a++) red[(16 * a + li) * NW + wave] = stat[a];
      }
      __syncthreads();
#pragma unroll
      for (int a = 0; a < MT; a++) {
        const gf4 *q = reinterpret_cast<const gf4 *>(red + (16 * a + li) * NW);
        float m = 0.f;
#pragma unroll
        for (int w4 = 0; w4 < NW / 4; w4++) { const gf4 v = q[w4]; m += (v.x + v.y) + (v.z + v.w); }
        stat[a] = m;
      }
    };
    exchange(red1);
    const float inv_n = 1.f / 256.f;
#pragma unroll
    for (int a = 0; a < MT; a++) {
      const float mean = stat[a] * inv_n;
      float q = 0.f;
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) { acc[a][b][r] -= mean; q += acc[a][b][r] * acc[a][b][r]; }
      q += __shfl_xor(q, 16);
      stat[a] = q + __shfl_xor(q, 32);
    }
    exchange(red2);
#pragma unroll
    for (int a = 0; a < MT; a++) {
      const float rstd = rsqrtf(stat[a] * inv_n + P.eps);
#pragma unroll
      for (int b = 0; b < 2; b++) acc[a][b] = acc[a][b] * rstd * gv[b] + bev[b];
    }
    chain_y_to_lds<MT>(yimg, acc, li, kq, nw);
    if (!more) break;
    zero();
    G.late();
    for (int kt = 0; kt < 8; kt += 2) { G.template kstep<true, 0>(acc, G.R1, 0, kt); G.template kstep<true, 0>(acc, G.R0, 1, kt + 1); }
  }
  // ---- the action head and the tail
  gf4 accf[MT][1];
#pragma unroll
  for (int a = 0; a < MT; a++) accf[a][0] = gf4{0.f, 0.f, 0.f, 0.f};
  Gf.late();
  for (int kt = 0; kt < 8; kt += 2) { Gf.template kstep<true, 0>(accf, Gf.R1, 0, kt); Gf.template kstep<true, 0>(accf, Gf.R0, 1, kt + 1); }
  const int col = wave * 16 + 4 * kq;
  const df4 bvf = dec_head_bias(P.bf, col, 2 * P.out.A);
#pragma unroll
  for (int a = 0; a < MT; a++) dec_tail(P.out, M, accf[a][0], bvf, m0 + 16 * a + li, col);
}
