// tests/hostemu/grav_emu.cpp — TEST-ONLY host emulation of the DOMAIN-RANDOMISATION physics kernel with BOTH of its tables
// (csrc/tmjx_wave_rand.hip): the wave-per-env kernel body of csrc/wave_physics.h compiled with TMW_RAND, one emulated 64-lane wavefront and an
// LDS image per env, each env with its own friction / actuator / damping scales from a [3][n] table and its own gravity vector from a second
// [3][n] table.  Either table may be null, as in the kernel: no scales = (1, 1, 1), no gravity table = the model's gravity.  Built next to
// hostemu.cpp (same headers; TMW_RAND is this file's, as it is the kernel unit's); nothing in track_mjx_amd/ loads it.
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

struct GravEmuModel { DModel h; };
static std::string g_err;

extern "C" {
const char *grav_last_error() { return g_err.c_str(); }
GravEmuModel *grav_model_create(const void *blob, size_t n) {
  GravEmuModel *m = new GravEmuModel();
  if (!tmjx_host::build_dmodel(blob, n, m->h, g_err)) { delete m; return nullptr; }
  return m;
}
void grav_model_destroy(GravEmuModel *m) { delete m; }
// k_physics_wave_rand's loop; `scales` [3][scales_n] (friction | actuator | damping) or null, `gravity` [3][gravity_n] (gx | gy | gz) or null; env e
// of the launch reads column e0 + e of each.  TMJX_EMU_POISON as in hostemu.cpp: what the wave finds in LDS, registers and scratch.
void grav_physics_wave(GravEmuModel *mm, float *st, const float *action, int nsub, int do_euler, float *ws_dump, int n, const float *scales,
                       int scales_n, const float *gravity, int gravity_n, int e0, int chains) {
  const WLayout K = tmjx_host::make_wave_layout(mm->h, chains != 0);
  std::vector<float> lds(K.lds_floats + 64);
  const char *poison_s = getenv("TMJX_EMU_POISON");
  const float poison = poison_s ? (!strcmp(poison_s, "nan") ? NAN : (float)atof(poison_s)) : 0.f;
  for (int e = 0; e < n; e++) {
    std::fill(lds.begin(), lds.end(), poison);
    WCtx c{&mm->h, lds.data(), st, n, e, 0, nullptr, 0ull, ws_dump};
    if (poison_s) {
      for (int l = 0; l < TMW_NL; l++) {
        c.qfs0[l] = c.qfs1[l] = c.dg0[l] = c.dg1[l] = c.wp0[l] = c.wp1[l] = poison;
        c.qa0[l] = c.qa1[l] = c.ma0[l] = c.ma1[l] = poison;
      }
    }
    std::vector<float> spill(mm->h.nnz + mm->h.nv + 64, poison);
    c.mspill = spill.data() + 64;
    c.action = action;
    c.s_f = c.s_a = c.s_d = 1.f;
    if (scales) { c.s_f = scales[e0 + e]; c.s_a = scales[(size_t)scales_n + e0 + e]; c.s_d = scales[2 * (size_t)scales_n + e0 + e]; }
    c.has_g = 0;                     // (no table: the body reads the model's gravity, the path aggregate initialisation selects)
    if (gravity) { c.has_g = 1; for (int k = 0; k < 3; k++) c.g[k] = gravity[(size_t)k * gravity_n + e0 + e]; }
    float time = tmw_load_state(c, K, action);
    for (int f = 0; f < nsub; f++) { tmw_forward(c, K, f == nsub - 1); if (do_euler) time = tmw_euler(c, K, time); }
    if (ws_dump) tmw_dump(c, K, ws_dump);
    tmw_store_state(c, K, time);
  }
}
}
