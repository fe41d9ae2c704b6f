// csrc/act_shared.h — the expressions of the acting policy's epilogues, ONE definition each for the kernels that launch them one by one
// (k_silu_ln_fwd, k_latent_concat, k_sample_action: csrc/ppo_kernels.h) and for the kernel that runs the whole policy in one launch (k_policy_act,
// csrc/policy_act.h): the two paths agree to the bit because they evaluate the same functions on the same lane layout, and cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "silu_math.h"

__device__ __forceinline__ float ppo_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float ppo_fldj(float x) { return 2.f * (0.69314718055994531f - x - ppo_softplus(-2.f * x)); }
// PPO_G = 8 lanes share one (t, b) / one env: lane s takes the elements s, s + 8, ...
#define PPO_G 8
__device__ __forceinline__ float ppo_group_sum(float x) { x += __shfl_xor(x, 4); x += __shfl_xor(x, 2); x += __shfl_xor(x, 1); return x; }
__device__ __forceinline__ float wave_sum(float x) { for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off); return x; }

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants)
__device__ __forceinline__ void tm_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned *out) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// four N(0, 1) draws for elements 4 q .. 4 q + 3 of stream `sid` at draw counter `ctr` (Box-Muller on 24-bit uniforms in (0, 1]: from 2^23 up + 0.5f rounds to even, the top value gives 1.0 and a radius of 0)
__device__ __forceinline__ void tm_normal4(unsigned long long seed, unsigned long long ctr, unsigned sid, unsigned q, float *n) {
  unsigned x[4];
  tm_philox4x32_10(q, sid, (unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)seed, (unsigned)(seed >> 32), x);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float u1 = ((float)(x[2 * h] >> 8) + 0.5f) * (1.f / 16777216.f), u2 = ((float)(x[2 * h + 1] >> 8) + 0.5f) * (1.f / 16777216.f);
    const float r = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincospif(2.f * u2, &sn, &cs);
    n[2 * h] = r * cs; n[2 * h + 1] = r * sn;
  }
}
// element `idx` of the N(0, 1) array a caller supplies, or of stream `sid` at draw counter `ctr`
__device__ __forceinline__ float tm_normal_at(const float *__restrict__ given, unsigned long long seed, unsigned long long ctr, unsigned sid, size_t idx) {
  if (given) return given[idx];
  float v4[4];
  tm_normal4(seed, ctr, sid, (unsigned)(idx >> 2), v4);
  return v4[idx & 3];
}

// ---- Dense -> SiLU -> LayerNorm block epilogue, one row held by one wave: a[k] = z of the lane's VPT columns on entry, y on return
// (two-pass variance; the row sums by wave shuffles)
template <int VPT>
__device__ __forceinline__ void silu_ln_row(float (&a)[VPT], const float (&b)[VPT], const float (&g)[VPT], const float (&be)[VPT], float eps, float &mean, float &rstd) {
  constexpr int H = VPT * 64;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; k++) { float v = a[k] + b[k]; a[k] = tm_silu(v); s += a[k]; }
  mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; k++) { float d = a[k] - mean; q += d * d; }
  rstd = rsqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
  for (int k = 0; k < VPT; k++) a[k] = (a[k] - mean) * rstd * g[k] + be[k];
}

// ---- latent sample (reparameterize, intention_network.py:78-88) and the proprioceptive columns of the decoder input
// (written as the fused multiply-add it compiles to: the encoder chain's latent tail, csrc/mlp_chain.h, forms the same)
__device__ __forceinline__ float tm_latent_sample(float ep, float logvar, float mean) { return fmaf(ep, expf(0.5f * logvar), mean); }
// (a division, not a product with 1 / std: a near-constant column has std = 1e-6)
__device__ __forceinline__ float tm_obs_normalised(float v, float mean, float stdv) { return (v - mean) / stdv; }

// ---- action sample, tanh post-processing and log-prob (make_inference_fn, ppo_networks.py:46-96): lane `sub` of an env's group of PPO_G takes the
// actions sub, sub + 8, ... of env e, writes raw [n][A] and action_t [A][n] and returns its share of the log-prob (ppo_group_sum adds the shares).
// lg: the env's logits row [loc (A) | raw scale (A)]
__device__ __forceinline__ float sample_action_lane(const float *lg, const float *__restrict__ noise, float *__restrict__ raw, float *__restrict__ action_t,
                                                    int n, int A, size_t e, int sub, unsigned long long seed, unsigned long long ctr) {
  float lp = 0.f;
  for (int a = sub; a < A; a += PPO_G) {
    const float nz = tm_normal_at(noise, seed, ctr, 3u, e * A + a);
    float loc = lg[a], scale = ppo_softplus(lg[A + a]) + 0.001f, x = loc + scale * nz, d = (x - loc) / scale;
    raw[e * A + a] = x;
    action_t[(size_t)a * n + e] = tanhf(x);          // [A][n]: the env-minor layout tmjx_step takes
    lp += -0.5f * d * d - logf(scale) - 0.91893853320467274f - ppo_fldj(x);
  }
  return lp;
}
