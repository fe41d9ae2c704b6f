// csrc/policy_act.h — the whole acting policy of an env group as ONE launch with a small footprint (k_policy_act): encoder blocks -> fc2 -> latent
// sample and decoder input -> decoder blocks -> head -> action sample, tanh, log-prob (make_inference_fn, ppo_networks.py:46-96; the intention
// network, intention_network.py:32-44,68-88).  It replaces the launch sequence k_linear_act / k_silu_ln_fwd / k_latent_concat / k_sample_action
// (csrc/ppo_kernels.h) and computes the same bits: every output element is the same k-ordered MFMA chain (k_linear_act's fragment mapping: lane
// (li, kq) supplies k = 16 c + 4 kq + e to the e-th MFMA of chunk c) and the epilogues are the shared functions of csrc/act_shared.h on the same
// lane layouts.
//
// Footprint: it runs between two physics launches of its env group NEXT TO the other groups' physics waves (twelve resident envs per CU, three waves
// of 136 registers per SIMD), so it lives under k_linear_act's limits (csrc/ppo_kernels.h): 256 threads = one wave per SIMD, <= 96 registers, <= 20 480
// bytes of LDS.  Nothing waits between workgroups; the only cross-workgroup operation is k_sample_action's relaxed ticket for the draw counter.
//
// Mapping: a workgroup owns PA_ROWS = 16 rows (envs) through the whole policy.  LDS holds ONE activation image [16][288] (row stride 296 floats:
// the b128 A-fragment reads of 16 rows x 4 k-quads hit 16 distinct 4-bank slots).  Wave w owns columns 64 w .. 64 w + 63 of a 256-wide layer (four
// accumulator tiles of v_mfma_f32_16x16x4_f32); fc2's and the head's 16-column tiles are dealt to the waves round-robin.  Weight fragments come
// straight from global memory / L2, one float4 per lane and column tile (with 16 rows per workgroup a weight word is used by exactly one wave:
// LDS staging would buy no reuse), the next two K chunks' loads in flight while this one's 16 MFMAs per wave issue (the code object waits with
// vmcnt(11) .. vmcnt(8) before a chunk's MFMAs).  The first layer's operand — the raw observation, wider than the image — is
// staged through the image 288 columns at a time, normalised with k_linear_act<true>'s expression (a - mean[k]) * inv_std[k]; its accumulators run
// through the passes, so the k order is unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include "act_shared.h"
#include "tm_common.h"

#define PA_ROWS 16
#define PA_W 288               // image columns: the widest operand kept whole (the decoder input, Z + proprioception, padded to a multiple of 4)
#define PA_LD 296              // floats per image row: 296 = 40 (mod 64) banks
#define PA_H 256               // every hidden layer's width
#define PA_MAX_BLOCKS 4        // CHAIN_MAX_HIDDEN (csrc/mlp_chain.h)
#define PA_STAGES_WIDE 3        // register stages of weight fragments with four column tiles per wave (16 registers each): two chunks of loads in flight behind the one
                               // being multiplied is what 96 registers hold
#define PA_STAGES_NARROW 3      // ... with one or two column tiles per wave (fc2, the head); a fourth stage costs a spill
#define PA_MAX_LD (1 << 20)     // largest leading dimension of a weight matrix: 4 bytes x 255 rows x ld + a row's bytes stay below 2^32 (the host check)
#define PA_CHUNK 16            // k per pipeline stage: one float4 per lane of A and of every column tile, four MFMAs per tile

struct PolicyActBlock { const float *W, *bias, *gamma, *beta; int ldw; };
struct PolicyAct {
  const float *obs; long long ldo;          // raw observation, row-major [M][ldo]
  const float *mean, *inv_std;              // the first layer's normaliser [K0] (both or neither)
  const float *nmean, *nstd;                // the whole observation's normaliser [obs_w] for the proprioceptive columns (both or neither)
  int M, K0, Z, obs_w, ref_w, A, ne, nd;
  PolicyActBlock enc[PA_MAX_BLOCKS], dec[PA_MAX_BLOCKS];
  const float *W2, *b2; int ldw2;           // fc2 [2Z][ldw2]
  const float *Wh, *bh; int ldwh;           // head [2A][ldwh]
  float ln_eps;
  const float *eps, *noise;                 // the caller's N(0, 1) draws [M][Z] / [M][A], or both null: Philox streams 2 / 3 of (seed, rng_state[0])
  unsigned long long seed; long long *rng_state;
  float *fc2, *logits, *raw, *action_t, *logp;
};

typedef float __attribute__((ext_vector_type(4))) pa_f4;

// acc[j] += A[16 rows][k] W_j[16 columns][k]^T over the chunks c0 .. c0 + nch - 1 of the layer (k = 16 c ..), A from the image (chunk c0 at
// afrag = image + li * PA_LD + 4 kq), W_j from W[j] + pw[j]: a wave-uniform base (scalar registers) and the 32-bit byte offset of the lane's weight row from it (one address
// register per tile, ONE for all tiles where the offsets are equal).  k >= K (the last chunk of a K that is no multiple of 16): k_linear_act stages zeros for both operands; here the
// image holds the zeros and the weight fragment is the row's LAST float4 (readable, finite): 0 x w adds nothing to the chain, the same bits without
// a select per register.  S - 1 chunks of weight loads in flight behind the one being multiplied; loads behind the last chunk are clamped to it.
template <int NT, int S>
__device__ __forceinline__ void pa_gemm(pa_f4 (&acc)[NT], const float *afrag, const float *const (&W)[NT], const unsigned (&pw)[NT], int c0, int nch, int K, int kq) {
  const int cl = c0 + nch - 1;
  auto load = [&](pa_f4 (&w)[NT], int c) {
    c = min(c, cl);
    const unsigned off = min(4u * (16 * c + 4 * kq), 4u * K - 16u);        // K % 4 == 0; k >= K: the row's LAST float4 (readable, finite) against the image's zeros
#pragma unroll
    for (int j = 0; j < NT; j++) w[j] = *reinterpret_cast<const pa_f4 *>(reinterpret_cast<const char *>(W[j]) + (pw[j] + off));
  };
  auto frag = [&](int c) { return *reinterpret_cast<const pa_f4 *>(afrag + 16 * (min(c, cl) - c0)); };
  auto mma = [&](const pa_f4 &a, const pa_f4 (&w)[NT]) {
#pragma unroll
    for (int e = 0; e < 4; e++)
#pragma unroll
      for (int j = 0; j < NT; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], w[j][e], acc[j], 0, 0, 0);
  };
  pa_f4 w[S][NT];
#pragma unroll
  for (int s = 0; s < S - 1; s++) load(w[s], c0 + s);
  // whole groups of S chunks without a branch inside (a guarded step makes the compiler drain every outstanding load at the loop's head), then the
  // at most S - 1 chunks left, whose fragments are already in flight
  int c = c0;
#pragma unroll 1                                        // (unrolled whole, a 256-deep layer's 64 loads are hoisted in front of its MFMAs: spills)
  for (; c + S - 1 <= cl; c += S) {
#pragma unroll
    for (int s = 0; s < S; s++) {
      // (the scheduling barriers keep each chunk's loads IN FRONT of the MFMAs of the chunk two behind it: left alone, the scheduler sinks the loads
      // to one chunk before their use, which saves registers and halves the bytes in flight)
      load(w[(s + S - 1) % S], c + s + S - 1);
      __builtin_amdgcn_sched_barrier(0);
      mma(frag(c + s), w[s]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int s = 0; s < S - 1; s++)
    if (c + s <= cl) mma(frag(c + s), w[s]);
}

// a 256-wide layer: wave w takes the column tiles 4 w .. 4 w + 3
__device__ __forceinline__ void pa_layer256(pa_f4 (&acc)[4], const float *afrag, const float *W, int ldw, int c0, int nch, int K, int wave, int li, int kq) {
  const float *Wj[4];
  unsigned pw[4];
  const int uw = __builtin_amdgcn_readfirstlane(wave);             // (wave-uniform: the tiles' bases live in scalar registers)
#pragma unroll
  for (int j = 0; j < 4; j++) { Wj[j] = W + (size_t)(64 * uw + 16 * j) * ldw; pw[j] = 4u * (unsigned)li * ldw; }
  pa_gemm<4, PA_STAGES_WIDE>(acc, afrag, Wj, pw, c0, nch, K, kq);
}

// Dense -> SiLU -> LayerNorm epilogue of a block: the accumulators go to the image as z (no bias), then every wave runs k_silu_ln_fwd<4>'s row body
// on four rows and writes y back in place.  Enters with every wave possibly still reading A fragments; leaves with the image readable by all.
__device__ __forceinline__ void pa_block_epilogue(float *img, const pa_f4 (&acc)[4], const PolicyActBlock &B, float eps, int wave, int lane, int li, int kq) {
  __syncthreads();                                      // every wave has read its last A fragment
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int r = 0; r < 4; r++) img[(4 * kq + r) * PA_LD + 64 * wave + 16 * j + li] = acc[j][r];      // register r of lane l: C[4 (l / 16) + r][l % 16]
  float b[4], g[4], be[4];
  {
    const float4 qb = *reinterpret_cast<const float4 *>(B.bias + 4 * lane), qg = *reinterpret_cast<const float4 *>(B.gamma + 4 * lane),
                 qe = *reinterpret_cast<const float4 *>(B.beta + 4 * lane);
    b[0] = qb.x; b[1] = qb.y; b[2] = qb.z; b[3] = qb.w; g[0] = qg.x; g[1] = qg.y; g[2] = qg.z; g[3] = qg.w; be[0] = qe.x; be[1] = qe.y; be[2] = qe.z; be[3] = qe.w;
  }
  __syncthreads();
#pragma unroll
  for (int rr = 0; rr < 4; rr++) {
    float *row = img + (4 * wave + rr) * PA_LD + 4 * lane;
    const float4 q = *reinterpret_cast<const float4 *>(row);
    float a[4] = {q.x, q.y, q.z, q.w}, mean, rstd;
    silu_ln_row<4>(a, b, g, be, eps, mean, rstd);
    *reinterpret_cast<float4 *>(row) = float4{a[0], a[1], a[2], a[3]};
  }
  __syncthreads();
}

// A narrow last layer of a stack (fc2: N = 2 Z, the head: N = 2 A; K = 256 from the image): out[row][c] = acc + bias to global memory ([M][N]) and to
// the image's columns [0, N).  NT column tiles per wave, tile w + 4 j for wave w; columns >= N are clamped on load and never stored.
template <int NT>
__device__ __forceinline__ void pa_narrow(float *img, const float *afrag, const float *W, int ldw, const float *bias, float *out, int N, int M, int row0, int wave, int li,
                                          int kq) {
  pa_f4 acc[NT];
  const float *Wj[NT];
  unsigned pw[NT];
#pragma unroll
  for (int j = 0; j < NT; j++) {
    acc[j] = pa_f4{0.f, 0.f, 0.f, 0.f};
    Wj[j] = W;
    pw[j] = 4u * (unsigned)min(16 * (wave + 4 * j) + li, N - 1) * ldw;
  }
  pa_gemm<NT, (NT > 2 ? PA_STAGES_WIDE : PA_STAGES_NARROW)>(acc, afrag, Wj, pw, 0, PA_H / PA_CHUNK, PA_H, kq);
  __syncthreads();                                      // every wave has read its last A fragment
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const int c = 16 * (wave + 4 * j) + li;
    if (c < N) {
      const float bv = bias ? bias[c] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rl = 4 * kq + r;
        const float v = acc[j][r] + bv;
        img[rl * PA_LD + c] = v;
        if (row0 + rl < M) out[(size_t)(row0 + rl) * N + c] = v;
      }
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void pa_narrow_any(float *img, const float *afrag, const float *W, int ldw, const float *bias, float *out, int N, int M, int row0, int wave,
                                              int li, int kq) {
  const int per_wave = ((N + 15) / 16 + 3) / 4;         // N <= 256: 1 .. 4 tiles per wave
  if (per_wave == 1) pa_narrow<1>(img, afrag, W, ldw, bias, out, N, M, row0, wave, li, kq);
  else if (per_wave == 2) pa_narrow<2>(img, afrag, W, ldw, bias, out, N, M, row0, wave, li, kq);
  else pa_narrow<4>(img, afrag, W, ldw, bias, out, N, M, row0, wave, li, kq);
}

__global__ __launch_bounds__(256, 5) void k_policy_act(PolicyAct P) {
  TM_PRIO_ACTING();
  __shared__ __attribute__((aligned(16))) float img[PA_ROWS * PA_LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kq = lane >> 4;
  const int row0 = blockIdx.x * PA_ROWS, M = P.M;
  // the draw counter is read where it is used (not held in registers through the GEMMs), always before this workgroup's ticket: the advance is made
  // by the workgroup that takes the LAST ticket (below), so no workgroup can see it advanced
  auto draw_counter = [&]() { return P.rng_state ? (unsigned long long)__hip_atomic_load(P.rng_state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull; };
  const float *afrag = img + li * PA_LD + 4 * kq;
  pa_f4 acc[4];

  // ---- encoder blocks; the first reads the raw observation through the image, PA_W columns per pass (rows >= M: clamped, never stored)
  for (int l = 0; l < P.ne; l++) {
    const PolicyActBlock &B = P.enc[l];
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = pa_f4{0.f, 0.f, 0.f, 0.f};
    if (l == 0) {
      for (int k0 = 0; k0 < P.K0; k0 += PA_W) {
        if (k0) __syncthreads();                        // every wave has read the previous pass
#pragma unroll 1
        for (int i = t; i < PA_ROWS * (PA_W / 4); i += 256) {
          const int r = i / (PA_W / 4), c = 4 * (i % (PA_W / 4)), k = k0 + c;
          pa_f4 a = pa_f4{0.f, 0.f, 0.f, 0.f};
          if (k < P.K0) {                               // K0 % 4 == 0: a float4 lies inside or outside as a whole
            a = *reinterpret_cast<const pa_f4 *>(P.obs + (long long)min(row0 + r, M - 1) * P.ldo + k);
            if (P.mean) {
              const pa_f4 mu = *reinterpret_cast<const pa_f4 *>(P.mean + k), is = *reinterpret_cast<const pa_f4 *>(P.inv_std + k);
              a = (a - mu) * is;
            }
          }
          *reinterpret_cast<pa_f4 *>(img + r * PA_LD + c) = a;
        }
        __syncthreads();
        const int left = P.K0 - k0, nch = left >= PA_W ? PA_W / PA_CHUNK : (left + PA_CHUNK - 1) / PA_CHUNK;
        pa_layer256(acc, afrag, B.W, B.ldw, k0 / PA_CHUNK, nch, P.K0, wave, li, kq);
      }
    } else {
      pa_layer256(acc, afrag, B.W, B.ldw, 0, PA_H / PA_CHUNK, PA_H, wave, li, kq);
    }
    pa_block_epilogue(img, acc, B, P.ln_eps, wave, lane, li, kq);
  }

  // ---- fc2 = [latent mean | latent logvar]: an output, and the image's columns [0, 2 Z)
  const int Z = P.Z;
  pa_narrow_any(img, afrag, P.W2, P.ldw2, P.b2, P.fc2, 2 * Z, M, row0, wave, li, kq);

  // ---- decoder input in the image: [ mean + eps exp(logvar / 2) | normalised proprioception | 0 .. ] (k_latent_concat's expressions).  The latent
  // samples wait in registers until every thread has read its logvar: the proprioceptive columns overwrite them.
  {
    const int Wd = Z + P.obs_w - P.ref_w;
    const unsigned long long ctr = draw_counter();
    float lat[PA_ROWS * (PA_H / 2) / 256];              // 2 Z <= 256: at most 8 latent elements per thread
#pragma unroll
    for (int q = 0; q < PA_ROWS * (PA_H / 2) / 256; q++) {
      const int i = t + 256 * q;
      lat[q] = 0.f;
      if (i < PA_ROWS * Z) {
        const int r = i / Z, c = i % Z;
        const size_t e = (size_t)min(row0 + r, M - 1);
        lat[q] = tm_latent_sample(tm_normal_at(P.eps, P.seed, ctr, 2u, e * Z + c), img[r * PA_LD + Z + c], img[r * PA_LD + c]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PA_ROWS * (PA_H / 2) / 256; q++) {
      const int i = t + 256 * q;
      if (i < PA_ROWS * Z) img[(i / Z) * PA_LD + i % Z] = lat[q];
    }
    const int rest = PA_W - Z;
#pragma unroll 1
    for (int i = t; i < PA_ROWS * rest; i += 256) {
      const int r = i / rest, c = Z + i % rest;
      float v = 0.f;
      if (c < Wd) {
        const int k = P.ref_w + c - Z;
        v = P.obs[(long long)min(row0 + r, M - 1) * P.ldo + k];
        if (P.nmean) v = tm_obs_normalised(v, P.nmean[k], P.nstd[k]);
      }
      img[r * PA_LD + c] = v;
    }
    __syncthreads();

    // ---- decoder blocks: the first takes the decoder input (its width rounded up to 4, as the padded weight rows)
    for (int l = 0; l < P.nd; l++) {
      const PolicyActBlock &B = P.dec[l];
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = pa_f4{0.f, 0.f, 0.f, 0.f};
      const int K = l == 0 ? (Wd + 3) & ~3 : PA_H;
      pa_layer256(acc, afrag, B.W, B.ldw, 0, (K + PA_CHUNK - 1) / PA_CHUNK, K, wave, li, kq);
      pa_block_epilogue(img, acc, B, P.ln_eps, wave, lane, li, kq);
    }
  }

  // ---- head: logits = [loc | raw scale], an output, and the image's columns [0, 2 A)
  const int A = P.A;
  pa_narrow_any(img, afrag, P.Wh, P.ldwh, P.bh, P.logits, 2 * A, M, row0, wave, li, kq);

  // ---- action sample, tanh, log-prob: k_sample_action's body, PPO_G lanes per env (the first 128 threads = two whole waves)
  if (t < PA_ROWS * PPO_G) {
    const int rl = t / PPO_G, sub = t % PPO_G, e = row0 + rl;
    const unsigned long long ctr = draw_counter();
    float lp = 0.f;
    if (e < M) lp = sample_action_lane(img + rl * PA_LD, P.noise, P.raw, P.action_t, M, A, (size_t)e, sub, P.seed, ctr);
    lp = ppo_group_sum(lp);
    if (e < M && sub == 0) P.logp[e] = lp;
  }
  // the workgroup that takes the last ticket advances the draw counter for the next inference (every workgroup has read it by then: the barrier
  // lies between its threads' reads and its ticket); relaxed, no fence, no spin
  if (P.rng_state && !P.noise) {
    __syncthreads();
    if (t == 0) {
    unsigned long long *st = (unsigned long long *)P.rng_state;
    if (__hip_atomic_fetch_add(st + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned long long)gridDim.x - 1ull) {
      __hip_atomic_store(st + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      P.rng_state[0] += 1;
    }
    }
  }
}
