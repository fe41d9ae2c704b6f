// tests/hostemu/align_emu.cpp — TEST-ONLY host emulation of tmjx_step under a done-policy (include/tmjx.h: tmjx_set_done_policy): per action
// repeat the wave-per-env physics (csrc/wave_physics.h, one emulated 64-lane wavefront and an LDS image per env) and K3 (csrc/env_core.h), then,
// under TM_DONE_ALIGN, the align epilogue (csrc/wave_align.h: tmw_align) on the done envs — the source k_align_wave compiles, on an LDS image and
// lane registers of its own that start from TMJX_EMU_POISON (nan or a number; default zeros), like hostemu.cpp's.  Built next to hostemu.cpp (same
// headers, same defines); nothing in track_mjx_amd/ loads it.
#define TM_HOST_EMU 1
#define TM_DEV static inline
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../track_mjx_amd/csrc/model_host.h"
#include "../../track_mjx_amd/csrc/wave_align.h"

struct AlignEmuModel { DModel h; std::vector<float> clips[7]; };
static std::string g_err;

static void poison_ctx(WCtx &c, float poison) {
  for (int l = 0; l < TMW_NL; l++) {
    c.qfs0[l] = c.qfs1[l] = c.dg0[l] = c.dg1[l] = c.wp0[l] = c.wp1[l] = poison;
    c.qa0[l] = c.qa1[l] = c.ma0[l] = c.ma1[l] = poison;
  }
}

extern "C" {
const char *align_last_error() { return g_err.c_str(); }
AlignEmuModel *align_model_create(const void *blob, size_t n) {
  AlignEmuModel *m = new AlignEmuModel();
  if (!tmjx_host::build_dmodel(blob, n, m->h, g_err)) { delete m; return nullptr; }
  return m;
}
void align_model_destroy(AlignEmuModel *m) { delete m; }
// the five leaves of tmjx_clips_upload, then the two of tmjx_clips_upload_velocities (both null: a table without velocities)
void align_clips(AlignEmuModel *m, const float *p, const float *q, const float *j, const float *b, const float *a, const float *v, const float *jv, int nc, int nf) {
  size_t cf = (size_t)nc * nf, w[7] = {3, 4, (size_t)(m->h.nq - 7), (size_t)(m->h.nbody - 1) * 3, 3, 3, (size_t)(m->h.nv - 6)};
  const float *src[7] = {p, q, j, b, a, v, jv};
  for (int i = 0; i < 7; i++) { m->clips[i].clear(); if (src[i]) m->clips[i].assign(src[i], src[i] + cf * w[i]); }
  m->h.clip_pos = m->clips[0].data(); m->h.clip_quat = m->clips[1].data(); m->h.clip_joints = m->clips[2].data(); m->h.clip_bodypos = m->clips[3].data();
  m->h.clip_angvel = m->clips[4].data();
  m->h.clip_vel = v ? m->clips[5].data() : nullptr; m->h.clip_jvel = jv ? m->clips[6].data() : nullptr;
  m->h.n_clips = nc; m->h.n_frames_clip = nf;
}
// tmjx_set_wrappers + tmjx_set_done_policy; returns -1 (with a message) where the C-ABI refuses
int align_set_policy(AlignEmuModel *m, int episode_length, int policy) {
  if (policy != TM_DONE_NONE && policy != TM_DONE_RESET && policy != TM_DONE_ALIGN) { g_err = "unknown done policy"; return -1; }
  if (policy == TM_DONE_ALIGN && (!m->h.clip_vel || !m->h.clip_jvel)) { g_err = "the align done-policy needs the clips' velocities"; return -1; }
  m->h.episode_length = episode_length; m->h.done_policy = policy; m->h.auto_reset = policy == TM_DONE_RESET;
  return 0;
}
// tmjx_step with action_repeat R on [row][n] buffers; `ws`: the lane-per-env workspace (unused rows stay untouched); returns the number of aligned envs
int align_step(AlignEmuModel *mm, float *st, int *is, const float *action, float *obs, float *rew, float *done, float *trunc, float *metrics, int n, int R) {
  const DModel &m = mm->h;
  const WLayout K = tmjx_host::make_wave_layout(m, true);
  std::vector<float> lds(std::max(K.lds_floats, tmjx_host::make_wave_layout(m, false).lds_floats) + 64);
  const char *poison_s = getenv("TMJX_EMU_POISON");
  const float poison = poison_s ? (!strcmp(poison_s, "nan") ? NAN : (float)atof(poison_s)) : 0.f;
  int aligned = 0;
  for (int e = 0; e < n; e++) {
    EnvRef r{st, nullptr, n, e};
    for (int k = 0; k < R; k++) {
      if (k == 0) tm_step_prologue(m, r);
      std::fill(lds.begin(), lds.end(), poison);
      WCtx c{&mm->h, lds.data(), st, n, e, 0, nullptr, 0ull, nullptr};
      if (poison_s) poison_ctx(c, poison);
      std::vector<float> spill(m.nnz + m.nv + 64, poison);
      c.mspill = spill.data() + 64;
      c.action = action;
      float time = tmw_load_state(c, K, action);
      for (int f = 0; f < m.n_frames; f++) { tmw_forward(c, K, f == m.n_frames - 1); time = tmw_euler(c, K, time); }
      tmw_store_state(c, K, time);
      tm_step_post(m, r, is, action, obs, rew, done, trunc, metrics, nullptr, false, nullptr, TM_REP(R, k == 0, k == R - 1));
    }
    if (m.done_policy == TM_DONE_ALIGN && done[e] != 0.f) {      // k_align_wave
      std::fill(lds.begin(), lds.end(), poison);
      WCtx c{&mm->h, lds.data(), st, n, e, 0, nullptr, 0ull, nullptr};
      if (poison_s) poison_ctx(c, poison);
      c.rs = 0; c.mspill = nullptr; c.action = nullptr;
      tmw_align(c, K, m, is, obs);
      aligned++;
    }
  }
  return aligned;
}
}
