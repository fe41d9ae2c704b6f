// tests/hostemu/rand_emu.cpp — TEST-ONLY host emulation of the DOMAIN-RANDOMISATION physics kernel (csrc/tmjx_wave_rand.hip): the wave-per-env
// kernel body of csrc/wave_physics.h compiled with TMW_RAND, one emulated 64-lane wavefront and an LDS image per env, each env with its own
// friction / actuator / damping scale from a [3][n] table.  Built next to hostemu.cpp (same headers; TMW_RAND is this file's alone, as it is
// the kernel unit's alone); nothing in track_mjx_amd/ loads it.
#define TM_HOST_EMU 1
#define TM_DEV static inline
#define TMW_RAND 1
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../track_mjx_amd/csrc/env_core.h"
#include "../../track_mjx_amd/csrc/model_host.h"
#include "../../track_mjx_amd/csrc/wave_physics.h"

struct RandEmuModel { DModel h; };
static std::string g_err;

extern "C" {
const char *rand_last_error() { return g_err.c_str(); }
RandEmuModel *rand_model_create(const void *blob, size_t n) {
  RandEmuModel *m = new RandEmuModel();
  if (!tmjx_host::build_dmodel(blob, n, m->h, g_err)) { delete m; return nullptr; }
  return m;
}
void rand_model_destroy(RandEmuModel *m) { delete m; }
// k_physics_wave_rand's loop; `scales` [3][scales_n] (friction | actuator | damping), env e of the launch reads column e0 + e
void rand_physics_wave(RandEmuModel *mm, float *st, const float *action, int nsub, int do_euler, float *ws_dump, int n, const float *scales, int scales_n,
                       int e0, int chains) {
  const WLayout K = tmjx_host::make_wave_layout(mm->h, chains != 0);
  std::vector<float> lds(K.lds_floats + 64);
  for (int e = 0; e < n; e++) {
    std::fill(lds.begin(), lds.end(), 0.f);
    WCtx c{&mm->h, lds.data(), st, n, e, 0, nullptr, 0ull, ws_dump};
    std::vector<float> spill(mm->h.nnz + mm->h.nv + 64, 0.f);
    c.mspill = spill.data() + 64;
    c.action = action;
    c.s_f = scales[e0 + e]; c.s_a = scales[(size_t)scales_n + e0 + e]; c.s_d = scales[2 * (size_t)scales_n + e0 + e];
    float time = tmw_load_state(c, K, action);
    for (int f = 0; f < nsub; f++) { tmw_forward(c, K, f == nsub - 1); if (do_euler) time = tmw_euler(c, K, time); }
    if (ws_dump) tmw_dump(c, K, ws_dump);
    tmw_store_state(c, K, time);
  }
}
}
