// csrc/decoder_io.h — what the two decoder-policy launches (decoder_act.h: MLP blocks, lstm_decoder_act.h: LSTM layers) share: how the decoder's input
// reaches the CU, how the action leaves it, and the argument checks of both descriptors (include/tmjx.h: tmjx_decoder_act_t, tmjx_lstm_decoder_act_t).
//
//   front  the first contraction's A operand is built ON THE CU: an LDS image [BM][DEC_XLD] (16-byte chunks XOR-swizzled by row & 15, the scheme of
//          mlp_chain.h's Y image) filled from the latents (row-major) and from the env's raw [obs][n_env] observation buffer (read along the env axis:
//          coalesced), normalised with k_latent_concat_det's expression, zeros from column Z + prop on — nobody writes a row-major image of x to global
//          memory;
//   tail   per 16 x 16 accumulator tile of the head (register r of lane (li, kq) = C[row][col + r], col = the tile's first column + 4 kq): bias, the
//          logits [n][ldl] on request, tanh (tmjx_action_mode's expression) of the first A columns stored transposed as action_t [A][n] (what tmjx_step
//          takes) and, on request, as ctrl [n][A].
#pragma once
#include <stdint.h>

typedef float __attribute__((ext_vector_type(4))) df4;

#define DEC_XLD 320          // floats per row of the X image: Z + prop <= 320 (a multiple of 64: the swizzle permutes chunks inside groups of 16)

struct DecoderIn {
  const float *lat; int ldz;
  const float *obs; long long s0, s1;
  const float *mean, *stdv;
  int ref_w, Z, prop, M;
};
struct DecoderOut { float *action_t, *ctrl, *logits; int ldl, A; };

__device__ __forceinline__ float *dec_xslot(float *ximg, int r, int c) { return ximg + r * DEC_XLD + ((((c >> 2) ^ (r & 15)) << 2) | (c & 3)); }

// rows [m0, m0 + BM) of x = [latents | (obs[ref_w:] - mean) / std] into the X image, by a workgroup of NT threads (t = threadIdx.x)
template <int BM, int NT>
__device__ __forceinline__ void dec_build_ximg(float *ximg, const DecoderIn &I, int m0, int t) {
  const int M = I.M, Z = I.Z, K1 = Z + I.prop;
  for (int it = t; it < BM * Z; it += NT) {                // latents: row-major, lanes along the columns
    const int r = it / Z, c = it - r * Z;
    *dec_xslot(ximg, r, c) = m0 + r < M ? I.lat[(long long)(m0 + r) * I.ldz + c] : 0.f;
  }
  for (int it = t; it < BM * (DEC_XLD - Z); it += NT) {    // proprioception: lanes along the env axis; zeros from column K1 on
    const int r = it % BM, c = Z + it / BM;
    float v = 0.f;
    if (c < K1 && m0 + r < M) {
      const int oc = I.ref_w + c - Z;
      v = I.obs[(long long)(m0 + r) * I.s0 + (long long)oc * I.s1];
      if (I.mean) v = (v - I.mean[oc]) / I.stdv[oc];
    }
    *dec_xslot(ximg, r, c) = v;
  }
}

// the head's bias for the lane's four columns col .. col + 3 of 2A (zeros past them, or without a bias)
__device__ __forceinline__ df4 dec_head_bias(const float *bias, int col, int Nf) {
  df4 bv = {0.f, 0.f, 0.f, 0.f};
  if (bias) {
#pragma unroll
    for (int r = 0; r < 4; r++) bv[r] = col + r < Nf ? bias[col + r] : 0.f;
  }
  return bv;
}
// one accumulator tile of the head: acc + bv are the logits of row `row`, columns col .. col + 3
__device__ __forceinline__ void dec_tail(const DecoderOut &O, int M, df4 acc, df4 bv, int row, int col) {
  const int Nf = 2 * O.A, A = O.A;
  const bool vec = O.logits && !(O.ldl & 3) && !((uintptr_t)O.logits & 15);
  const df4 v = acc + bv;
  if (row >= M) return;
  if (O.logits) {
    float *o = O.logits + (long long)row * O.ldl + col;
    if (vec && col + 3 < Nf) *reinterpret_cast<df4 *>(o) = v;
    else {
#pragma unroll
      for (int r = 0; r < 4; r++) if (col + r < Nf) o[r] = v[r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (col + r < A) {
      const float act = tanhf(v[r]);
      O.action_t[(long long)(col + r) * M + row] = act;
      if (O.ctrl) O.ctrl[(long long)row * A + col + r] = act;
    }
  }
}

// ---- host side: the part of the argument check and of the kernel parameters that both descriptors spell with the same field names
#include "host_launch.h"          // al4: the one alignment predicate of every argument check

template <class D>
static const char *decoder_io_why(const D *c) {
  if (!c->mean != !c->std) return "mean and std together";
  if (c->n < 1) return "n >= 1";
  if (c->Z < 1 || c->ldz < c->Z) return "Z >= 1 and ldz >= Z";
  if (c->ref_w < 0 || c->obs_w < c->ref_w) return "obs_w >= ref_w >= 0";
  if ((long long)c->Z + c->obs_w - c->ref_w > DEC_XLD) return "the decoder's input (Z + obs_w - ref_w) is at most 320 columns wide";
  if (c->A < 1 || 2 * c->A > 128) return "the action head has 2A <= 128 columns (A >= 1)";
  for (const void *p : {(const void *)c->latents, (const void *)c->obs, (const void *)c->mean, (const void *)c->std, (const void *)c->action_t, (const void *)c->ctrl,
                        (const void *)c->logits})
    if (!al4(p)) return "float pointers must be 4-byte aligned";
  if (c->logits && c->ldl < 2 * c->A) return "ldl >= 2A";
  return nullptr;
}
template <class D>
static DecoderIn decoder_in(const D *c) {
  return DecoderIn{c->latents, c->ldz, c->obs, c->obs_s0, c->obs_s1, c->mean, c->std, c->ref_w, c->Z, c->obs_w - c->ref_w, c->n};
}
template <class D>
static DecoderOut decoder_out(const D *c) { return DecoderOut{c->action_t, c->ctrl, c->logits, c->ldl, c->A}; }
