// csrc/tmjx_intervene.hip — the activation intervention (include/tmjx.h: tmjx_intervene_ok, tmjx_intervene; DESIGN.md "Interventions").  The
// arithmetic is csrc/intervene_core.h (it also compiles on the host), the argument checks csrc/intervene_host.h.
//   k_intervene<SUBSPACE>  one wave per row: the row in 16 registers per lane, one direction at a time (read once from global memory: its dot product
//                          and its term of the edit use the same registers), butterfly reduction by lane shuffles
//   k_intervene<UNITS>     one wave per row, element-wise
// Workgroups of 4 waves = 4 rows that share nothing: no LDS, no barrier, no atomics.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "intervene_host.h"

template <int MODE>
__global__ __launch_bounds__(IV_LANES *IV_ROWS_PER_WG) void k_intervene(const tmjx_intervene_t d, const int t) {
  const int lane = threadIdx.x & (IV_LANES - 1);
  const int r = blockIdx.x * IV_ROWS_PER_WG + (threadIdx.x >> 6);
  if (r >= d.n) return;                                     // (wave-uniform)
  const float dose = d.dose[r];
  const bool on = iv_on(t, d.t_on[r], d.t_off[r], dose);
  if (!on && (MODE == TMJX_INTERVENE_UNITS || !d.proj)) return;
  float *row = d.h + (int64_t)r * d.ld;
  const int w = d.w;
  float hr[IV_PER_LANE], xc[IV_PER_LANE];
#pragma unroll
  for (int i = 0; i < IV_PER_LANE; i++) {
    const int j = lane + IV_LANES * i;
    hr[i] = j < w ? row[j] : 0.f;
    xc[i] = j < w ? iv_centred(hr[i], d.center, j) : 0.f;
  }
  if (MODE == TMJX_INTERVENE_UNITS) {
#pragma unroll
    for (int i = 0; i < IV_PER_LANE; i++) {
      const int j = lane + IV_LANES * i;
      if (j < w) row[j] = iv_unit(hr[i], xc[i], d.gain[j], d.offset[j], dose);
    }
    return;
  }
  float e[IV_PER_LANE];
#pragma unroll
  for (int i = 0; i < IV_PER_LANE; i++) e[i] = 0.f;
  for (int k = 0; k < d.K; k++) {
    const float *v = d.dirs + (int64_t)k * d.ldv;
    float vk[IV_PER_LANE], p = 0.f;
#pragma unroll
    for (int i = 0; i < IV_PER_LANE; i++) {
      const int j = lane + IV_LANES * i;
      vk[i] = j < w ? v[j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < IV_PER_LANE; i++)
      if (lane + IV_LANES * i < w) p = iv_dot_term(xc[i], vk[i], p);
#pragma unroll
    for (int off = IV_LANES / 2; off >= 1; off >>= 1) p = iv_tree_step(p, __shfl_xor(p, off, IV_LANES));
    if (d.proj && lane == 0) d.proj[(int64_t)r * d.ldp + k] = p;
    const float coef = iv_coef(d.gain[k], p, d.offset[k]);
#pragma unroll
    for (int i = 0; i < IV_PER_LANE; i++) e[i] = iv_edit_term(coef, vk[i], e[i]);
  }
  if (!on) return;
#pragma unroll
  for (int i = 0; i < IV_PER_LANE; i++) {
    const int j = lane + IV_LANES * i;
    if (j < w) row[j] = iv_apply(hr[i], dose, e[i]);
  }
}

extern "C" {

int tmjx_intervene_ok(const tmjx_intervene_t *d) {
  const std::string e = tmjx_host::intervene_check(d);
  if (e.empty()) return 1;
  tmjx_internal_fail(TMJX_EINVAL, ("tmjx_intervene: " + e).c_str());
  return 0;
}

int tmjx_intervene(const tmjx_intervene_t *d, int t, void *stream) {
  const std::string e = tmjx_host::intervene_check(d);
  if (!e.empty()) return tmjx_internal_fail(TMJX_EINVAL, ("tmjx_intervene: " + e).c_str());
  const dim3 grid((d->n + IV_ROWS_PER_WG - 1) / IV_ROWS_PER_WG), block(IV_LANES * IV_ROWS_PER_WG);
  if (d->mode == TMJX_INTERVENE_SUBSPACE)
    hipLaunchKernelGGL(k_intervene<TMJX_INTERVENE_SUBSPACE>, grid, block, 0, (hipStream_t)stream, *d, t);
  else
    hipLaunchKernelGGL(k_intervene<TMJX_INTERVENE_UNITS>, grid, block, 0, (hipStream_t)stream, *d, t);
  return check_launch("k_intervene");
}

}  // extern "C"
