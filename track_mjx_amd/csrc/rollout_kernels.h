// csrc/rollout_kernels.h — device code of the checkpoint roll-out (include/tmjx.h "Roll-out recorder"): the recorder that copies one control
// step's state and activations into clip-major records, and the two small kernels of the deterministic policy step.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/tmjx.h"

#define REC_ENVS 32         // envs per workgroup (one x-block of the grid)
#define REC_ROWS 64         // SoA source rows per LDS chunk: the tile is REC_ROWS x (REC_ENVS + 1) floats = 8.4 KB
#define REC_NT 256

// grid (ceil(n_env / REC_ENVS), k): workgroup (bx, s) copies row t of stream s for envs [bx * 32, bx * 32 + 32).  Every branch below depends
// on the stream's descriptor only (uniform across the workgroup), never on the env count: a clip's record does not depend on its batch.
__global__ __launch_bounds__(REC_NT) void k_record_step(const tmjx_record_stream_t *__restrict__ tab, int n_env, int t) {
  __shared__ float tile[REC_ROWS][REC_ENVS + 1];     // (+1: the column reads of the store phase hit 32 different banks)
  const tmjx_record_stream_t *S = tab + blockIdx.y;
  const int e0 = blockIdx.x * REC_ENVS;
  const int ne = min(REC_ENVS, n_env - e0);
  const int w = S->w, ld = S->ld, n_idx = S->n_idx;
  const float *__restrict__ src = S->src;
  const long long env_stride = (long long)S->T * w;
  float *__restrict__ dst = S->dst + (long long)(S->t0 + t) * w + (long long)e0 * env_stride;
  const int tid = threadIdx.x;
  if (S->layout == TMJX_RECORD_SOA) {
    for (int r0 = 0; r0 < w; r0 += REC_ROWS) {
      const int nr = min(REC_ROWS, w - r0);
      // load: 32 consecutive envs of one source row per half-wave (128-byte runs along the env index)
      for (int i = tid; i < nr * REC_ENVS; i += REC_NT) {
        const int r = i / REC_ENVS, e = i % REC_ENVS;
        if (e < ne) {
          const int sr = n_idx ? S->idx[r0 + r] : r0 + r;
          tile[r][e] = src[(long long)sr * ld + e0 + e];
        }
      }
      __syncthreads();
      // store: each env's nr floats as one run (consecutive lanes = consecutive floats of one env's record row)
      for (int i = tid; i < nr * ne; i += REC_NT) {
        const int e = i / nr, r = i % nr;
        dst[(long long)e * env_stride + r0 + r] = tile[r][e];
      }
      __syncthreads();
    }
    return;
  }
  // row-major source [n_env][ld]: each env's w floats are contiguous in the source and in the record
  const float *__restrict__ srow = src + (long long)e0 * ld;
  const bool vec = !n_idx && !(w & 3) && !(ld & 3) && !((uintptr_t)src & 15) && !((uintptr_t)S->dst & 15);
  if (vec) {
    const int n4 = w >> 2;
    for (int i = tid; i < ne * n4; i += REC_NT) {
      const int e = i / n4, c = i % n4;
      const float4 v = reinterpret_cast<const float4 *>(srow + (long long)e * ld)[c];
      reinterpret_cast<float4 *>(dst + (long long)e * env_stride)[c] = v;
    }
  } else {
    for (int i = tid; i < ne * w; i += REC_NT) {
      const int e = i / w, c = i % w;
      dst[(long long)e * env_stride + c] = srow[(long long)e * ld + (n_idx ? S->idx[c] : c)];
    }
  }
}

// x = [fc2[:, :Z] | normalised proprioception | 0 ...] ([n][ldx]) and, optionally, traj = the normalised reference half ([n][ldt]).
// One thread per output element; (v - mean) / std with the correctly rounded division (what torch / numpy compute in float32).
__global__ __launch_bounds__(256) void k_latent_concat_det(const float *__restrict__ fc2, int ldf, const float *__restrict__ obs, long long s0, long long s1,
                                                           const float *__restrict__ mean, const float *__restrict__ stdv, float *__restrict__ x, int ldx,
                                                           float *__restrict__ traj, int ldt, int n, int Z, int obs_w, int ref_w) {
  const long long nx = (long long)n * ldx, total = nx + (traj ? (long long)n * ldt : 0);
  const int prop = obs_w - ref_w;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
    if (k < nx) {
      const int i = (int)(k / ldx), c = (int)(k % ldx);
      float v = 0.f;
      if (c < Z) {
        v = fc2[(long long)i * ldf + c];
      } else if (c < Z + prop) {
        const int oc = ref_w + c - Z;
        v = obs[(long long)i * s0 + (long long)oc * s1];
        if (mean) v = (v - mean[oc]) / stdv[oc];
      }
      x[k] = v;
    } else {
      const long long q = k - nx;
      const int i = (int)(q / ldt), c = (int)(q % ldt);
      float v = 0.f;
      if (c < ref_w) {
        v = obs[(long long)i * s0 + (long long)c * s1];
        if (mean) v = (v - mean[c]) / stdv[c];
      }
      traj[q] = v;
    }
  }
}

// ctrl[i][j] = action_t[j][i] = tanh(logits[i][j]), j < A.  Thread k -> (i, j) with j fastest: the ctrl stores are coalesced, the transposed
// ones are 38 scattered words per env (the same as tmjx_sample_action's)
__global__ __launch_bounds__(256) void k_action_mode(const float *__restrict__ logits, int ldl, float *__restrict__ ctrl, float *__restrict__ action_t, int n,
                                                     int A) {
  const long long total = (long long)n * A;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(k / A), j = (int)(k % A);
    const float a = tanhf(logits[(long long)i * ldl + j]);
    ctrl[k] = a;
    action_t[(long long)j * n + i] = a;
  }
}
