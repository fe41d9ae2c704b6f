// csrc/tmjx_wave_sensors.hip — fourth translation unit of libtmjx_hip.so: the RECORDING physics kernel of checkpoint roll-outs,
// k_physics_wave_sensors — K2 (csrc/tmjx_wave.hip) with the sensor stage (wave_physics.h: tmw_sensor_stage) between the solve and Euler of the
// control step's last substep, writing sensordata [nsensordata][n_env] and cfrc_ext [nbody * 6][n_env].
//
// Its own unit, with the product unit's flag (track_mjx_amd/hip.py SOURCE_FLAGS: -mllvm -disable-machine-licm), so that csrc/tmjx_wave.hip
// stays as it is: k_physics_wave<bool> does not call the stage and disassembles to the same instructions as before the stage existed.  The
// substep loop below is the product's, with the stage as a template parameter (SENS = false would be the product loop); the stage only READS
// the product's LDS image and writes LDS behind it (wave_physics.h: TmwSens), so state, observation and reward come out bit for bit as from
// k_physics_wave (tests/test_gpu_sensors.py).  Roll-outs run at most a few thousand envs, so the extra LDS (10 KB per env for the rodent:
// 24.5 KB in all) and the residency it costs do not matter there: 704 against 670 us per launch at 1024 envs.
#include <hip/hip_runtime.h>

#include "../../include/tmjx.h"
#include "wave_physics.h"

#ifndef TMW_WAVES_PER_SIMD
#define TMW_WAVES_PER_SIMD 3
#endif
template <bool STATIC, bool SENS>
__global__ __launch_bounds__(64, TMW_WAVES_PER_SIMD) void k_physics_wave_sensors(const DModel *__restrict__ mp, float *st, const float *action, int nsub,
                                                             int do_euler, float *ws_dump, int n, int e0, int rs, float *spill, int spill_stride,
                                                             float *sensordata, float *cfrc_ext) {
  extern __shared__ float tmw_lds[];
  WCtx c{(TmwModel *)mp, tmw_lds, st, n, (int)blockIdx.x + e0, (int)threadIdx.x, nullptr, 0ull, nullptr};
  c.rs = rs;
  c.mspill = spill ? spill + 64 + (size_t)(blockIdx.x + e0) * (size_t)spill_stride : nullptr;
  c.action = action;
  c.dump = ws_dump;
  constexpr WLayout ks(TMW_RODENT_DIMS, 1);
  const WLayout kd = STATIC ? ks : WLayout(mp->nbody, mp->njnt, mp->nq, mp->nv, mp->nu, mp->ncon, mp->nlim, mp->nnz, mp->ngroup,
                                           mp->nround_body, mp->nround_dof);
  const WLayout &K = STATIC ? ks : kd;
  float time = tmw_load_state(c, K, action);
  for (int f = 0; f < nsub; f++) {
    // (the product kernel's opaque per-substep copies of the lane id and the model pointer: csrc/tmjx_wave.hip says why)
    { int l; asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l)); c.lane = l;
      TmwModel *q = (TmwModel *)mp; asm volatile("" : "+s"(q)); c.mp = q; }
    tmw_forward(c, K, f == nsub - 1);
    if (SENS && f == nsub - 1) tmw_sensor_stage(c, K, sensordata, cfrc_ext);
    if (do_euler) time = tmw_euler(c, K, time);
  }
  if (ws_dump) tmw_dump(c, K, ws_dump);
  tmw_store_state(c, K, time);
}

extern "C" void tmjx_internal_launch_physics_wave_sensors(int rodent, int cnt, size_t lds, hipStream_t stream, const DModel *mp, float *st,
                                                          const float *action, int nsub, int do_euler, float *ws_dump, int n, int e0, int rs,
                                                          float *spill, int spill_stride, float *sensordata, float *cfrc_ext) {
  if (rodent) hipLaunchKernelGGL((k_physics_wave_sensors<true, true>), dim3(cnt), dim3(64), lds, stream, mp, st, action, nsub, do_euler, ws_dump, n, e0, rs,
                                 spill, spill_stride, sensordata, cfrc_ext);
  else hipLaunchKernelGGL((k_physics_wave_sensors<false, true>), dim3(cnt), dim3(64), lds, stream, mp, st, action, nsub, do_euler, ws_dump, n, e0, rs,
                          spill, spill_stride, sensordata, cfrc_ext);
}
