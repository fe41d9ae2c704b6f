// csrc/tmjx_wave_rand.hip — translation unit of libtmjx_hip.so: the physics kernel with PER-ENV DOMAIN RANDOMISATION, k_physics_wave_rand — K2
// (csrc/tmjx_wave.hip) with this env's friction, actuator and damping scale applied to the model constants (wave_physics.h: TMW_RAND, TMW_SCALE)
// and this env's gravity vector in place of the model's (TMW_GRAV).
//
// Its own unit, with the product unit's flag (track_mjx_amd/hip.py SOURCE_FLAGS: -mllvm -disable-machine-licm), as the recording kernel is
// (csrc/tmjx_wave_sensors.hip): this file alone defines TMW_RAND in front of wave_physics.h, every other unit compiles the body without the
// switch — the tokens it compiled before — and a handle without scales launches the product kernel (tmjx_hip.hip: launch_wave).
//
// One wavefront integrates one env, so a per-env SCALAR is wave-uniform: the three scales of env e0 + workgroup are read with scalar loads from
// env_scales [3][scales_n] (row 0 friction, 1 actuator, 2 damping; constant address space: never written while a launch reads it) once, in front
// of the substep loop, and live in SGPRs — nothing is added to the lanes' register budget, nothing to LDS.  The env's gravity is three more
// wave-uniform floats, read the same way from env_gravity [3][gravity_n] (rows gx, gy, gz; world frame).  Either table may be null: no scales =
// (1, 1, 1) (x * 1.0f is exact), no gravity table = the model's gravity, read here once — one kernel serves scales only, gravity only, or both.
// Per-env VECTORS (masses, per-geom tables, a whole model) would need registers and LDS, and are not built.
#include <hip/hip_runtime.h>

#include "../../include/tmjx.h"
#define TMW_RAND 1
#include "wave_physics.h"

#ifndef TMW_WAVES_PER_SIMD
#define TMW_WAVES_PER_SIMD 3
#endif
template <bool STATIC>
__global__ __launch_bounds__(64, TMW_WAVES_PER_SIMD) void k_physics_wave_rand(const DModel *__restrict__ mp, float *st, const float *action, int nsub,
                                                          int do_euler, float *ws_dump, int n, int e0, int rs, float *spill, int spill_stride,
                                                          const float *__restrict__ env_scales, int scales_n,
                                                          const float *__restrict__ env_gravity, int gravity_n) {
  extern __shared__ float tmw_lds[];
  WCtx c{(TmwModel *)mp, tmw_lds, st, n, (int)blockIdx.x + e0, (int)threadIdx.x, nullptr, 0ull, nullptr};
  c.rs = rs;
  c.mspill = spill ? spill + 64 + (size_t)(blockIdx.x + e0) * (size_t)spill_stride : nullptr;
  c.action = action;
  c.dump = ws_dump;
  {   // the GLOBAL env id indexes both tables (a split launch passes e0); the host has checked e0 + gridDim.x <= scales_n and <= gravity_n
    const __attribute__((address_space(4))) float *sc = (const __attribute__((address_space(4))) float *)env_scales;
    const __attribute__((address_space(4))) float *gv = (const __attribute__((address_space(4))) float *)env_gravity;
    const size_t e = (size_t)((int)blockIdx.x + e0);
    c.s_f = c.s_a = c.s_d = 1.f;
    if (sc) { c.s_f = sc[e]; c.s_a = sc[(size_t)scales_n + e]; c.s_d = sc[2 * (size_t)scales_n + e]; }
    c.has_g = 1;
    if (gv) { c.g[0] = gv[e]; c.g[1] = gv[(size_t)gravity_n + e]; c.g[2] = gv[2 * (size_t)gravity_n + e]; }
    else { TmwModel *q = (TmwModel *)mp; c.g[0] = q->gravity[0]; c.g[1] = q->gravity[1]; c.g[2] = q->gravity[2]; }
  }
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
    if (do_euler) time = tmw_euler(c, K, time);
  }
  if (ws_dump) tmw_dump(c, K, ws_dump);
  tmw_store_state(c, K, time);
}

extern "C" void tmjx_internal_launch_physics_wave_rand(int rodent, int cnt, size_t lds, hipStream_t stream, const DModel *mp, float *st,
                                                       const float *action, int nsub, int do_euler, float *ws_dump, int n, int e0, int rs,
                                                       float *spill, int spill_stride, const float *env_scales, int scales_n,
                                                       const float *env_gravity, int gravity_n) {
  if (rodent) hipLaunchKernelGGL(k_physics_wave_rand<true>, dim3(cnt), dim3(64), lds, stream, mp, st, action, nsub, do_euler, ws_dump, n, e0, rs, spill,
                                 spill_stride, env_scales, scales_n, env_gravity, gravity_n);
  else hipLaunchKernelGGL(k_physics_wave_rand<false>, dim3(cnt), dim3(64), lds, stream, mp, st, action, nsub, do_euler, ws_dump, n, e0, rs, spill,
                          spill_stride, env_scales, scales_n, env_gravity, gravity_n);
}
