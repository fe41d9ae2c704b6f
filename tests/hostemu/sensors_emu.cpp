// tests/hostemu/sensors_emu.cpp — TEST-ONLY host emulation of the RECORDING physics kernel (csrc/tmjx_wave_sensors.hip): the wave-per-env
// kernel body of csrc/wave_physics.h with the sensor stage (tmw_sensor_stage) on the last substep, one emulated 64-lane wavefront and an LDS
// image per env that includes the stage's scratch behind the product image.  Built next to hostemu.cpp (same headers, same defines); nothing in
// track_mjx_amd/ loads it.
#define TM_HOST_EMU 1
#define TM_DEV static inline
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

struct SensEmuModel { DModel h; };
static std::string g_err;

extern "C" {
const char *sens_last_error() { return g_err.c_str(); }
SensEmuModel *sens_model_create(const void *blob, size_t n) {
  SensEmuModel *m = new SensEmuModel();
  if (!tmjx_host::build_dmodel(blob, n, m->h, g_err)) { delete m; return nullptr; }
  return m;
}
void sens_model_destroy(SensEmuModel *m) { delete m; }
void sens_info(const SensEmuModel *m, int *out) { out[0] = m->h.nsensordata; out[1] = m->h.nbody; out[2] = m->h.nsensor; }
// LDS floats of the recording kernel (chain layout if `chains` and the model has it, else the generic layout)
int sens_lds_floats(const SensEmuModel *m, int chains) { return tmw_sens_layout(tmjx_host::make_wave_layout(m->h, chains != 0)).end; }
// `sensors` = 0: the product loop (k_physics_wave), 1: the recording loop (k_physics_wave_sensors); sd / cf as in tmjx_physics_sensors
void sens_physics_wave(SensEmuModel *mm, float *st, const float *action, int nsub, int do_euler, float *ws_dump, int n, int sensors, float *sd, float *cf,
                       int chains) {
  const WLayout K = tmjx_host::make_wave_layout(mm->h, chains != 0);
  std::vector<float> lds(tmw_sens_layout(K).end + 64);
  for (int e = 0; e < n; e++) {
    std::fill(lds.begin(), lds.end(), 0.f);
    WCtx c{&mm->h, lds.data(), st, n, e, 0, nullptr, 0ull, ws_dump};
    std::vector<float> spill(mm->h.nnz + mm->h.nv + 64, 0.f);
    c.mspill = spill.data() + 64;
    c.action = action;
    float time = tmw_load_state(c, K, action);
    for (int f = 0; f < nsub; f++) {
      tmw_forward(c, K, f == nsub - 1);
      if (sensors && f == nsub - 1) tmw_sensor_stage(c, K, sd, cf);
      if (do_euler) time = tmw_euler(c, K, time);
    }
    if (ws_dump) tmw_dump(c, K, ws_dump);
    tmw_store_state(c, K, time);
  }
}
}
