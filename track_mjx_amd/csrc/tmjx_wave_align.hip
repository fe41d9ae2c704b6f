// csrc/tmjx_wave_align.hip — a translation unit of libtmjx_hip.so of its own: k_align_wave, the ALIGN done-policy of the step epilogue
// (csrc/wave_align.h; include/tmjx.h: tmjx_set_done_policy).  It takes the place k_autoreset has under the auto-reset policy — the last launch
// of tmjx_step / tmjx_step_sensors, behind k_post, which decides `done` — so a handle under TM_DONE_NONE or TM_DONE_RESET launches exactly what
// it launched before this unit existed, and csrc/tmjx_wave.hip stays as it is.
//
// One 64-lane workgroup per env, the physics kernel's LDS image (the position stage runs on it).  A wave whose env is not done returns at
// once; terminations are rare, so nearly every wave of the launch is that one load and branch.
#include <hip/hip_runtime.h>

#include "../../include/tmjx.h"
#include "wave_align.h"

template <bool STATIC>
__global__ __launch_bounds__(64) void k_align_wave(const DModel *__restrict__ mp, float *st, const int *is, float *obs, const float *done, int n) {
  extern __shared__ float tmw_lds[];
  const int e = blockIdx.x;
  if (e >= n || done[e] == 0.f) return;
  WCtx c{(TmwModel *)mp, tmw_lds, st, n, e, (int)threadIdx.x, nullptr, 0ull, nullptr};
  c.rs = 0;
  c.mspill = nullptr;
  c.action = nullptr;
  constexpr WLayout ks(TMW_RODENT_DIMS, 1);
  const WLayout kd = STATIC ? ks : WLayout(mp->nbody, mp->njnt, mp->nq, mp->nv, mp->nu, mp->ncon, mp->nlim, mp->nnz, mp->ngroup,
                                           mp->nround_body, mp->nround_dof);
  const WLayout &K = STATIC ? ks : kd;
  tmw_align(c, K, *mp, is, obs);
}

extern "C" void tmjx_internal_launch_align_wave(int rodent, size_t lds, hipStream_t stream, const DModel *mp, float *st, const int *is, float *obs,
                                                const float *done, int n) {
  if (rodent) hipLaunchKernelGGL(k_align_wave<true>, dim3(n), dim3(64), lds, stream, mp, st, is, obs, done, n);
  else hipLaunchKernelGGL(k_align_wave<false>, dim3(n), dim3(64), lds, stream, mp, st, is, obs, done, n);
}
