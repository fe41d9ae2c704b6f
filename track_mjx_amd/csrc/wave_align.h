// csrc/wave_align.h — the ALIGN done-policy of the step epilogue (TM_DONE_ALIGN, include/tmjx.h: tmjx_set_done_policy), one wavefront per env.
//
// Replaces AutoAlignWrapperTracking.step after the inner env's step (reference track_mjx/environment/wrappers.py:328-381): an env whose step
// ended with done set is not thrown back to its first state; it is put onto the reference pose of the clip frame it has reached, and goes on:
//   qpos <- position | quaternion | joints,  qvel <- velocity | angular_velocity | joints_velocity  of the frame the step just computed its
//   reward against (tm_cur_frame(time, start_frame): time is NOT rewound, so the frame keeps advancing through the clip across alignments; past
//   the clip's last frame tm_clip_row CLAMPS the index to the last frame, like the reference's gather), no noise;
//   smooth.kinematics on that state: xpos and the torso's xmat (all K3 and the observation read of it);
//   the observation rebuilt from the aligned state and the unchanged info (same clip, same start frame, same frame).
// act, qacc_warmstart, time, qfrc_actuator, prev_ctrl, the action ring buffer and its index, reward, done, truncation and the metrics stay those
// of the terminated step (unlike auto-reset, which restores prev_ctrl).  The stored quaternion is the clip's, not the normalised copy the
// kinematics work on: the next step's position stage normalises it as it does every stored quaternion.
//
// The kinematics are the physics kernel's own position stage (wave_physics.h: tmw_position, pointer jumping in LDS) on a freshly zeroed LDS image,
// so the next step's physics re-derives the very same xpos from the aligned qpos.  The observation is env_core.h's tm_get_obs in its part form,
// one lane per part, as k_step_parts runs it for every env.  Envs that are not done are not touched: the kernel returns before its first store.
// Single source for the GPU (csrc/tmjx_wave_align.hip) and the TEST-ONLY host emulation (tests/hostemu/align_emu.cpp).
#pragma once
#include "env_core.h"
#include "wave_physics.h"

// global stores of one block of lane code -> global loads of the next one by OTHER lanes of the wave (xpos written by the position stage, read by
// the observation parts): a workgroup barrier with its memory fence on the GPU (one wave per workgroup), nothing in the lane-serial emulation
#ifdef TM_HOST_EMU
#define TMW_GLOBAL_SYNC() do { } while (0)
#else
#define TMW_GLOBAL_SYNC() __syncthreads()
#endif

// element i of the aligned [qpos | qvel] (nq + nv words) from row `row` of the clip table
TM_DEV float tm_align_word(const DModel &m, size_t row, int i) {
  const int nj = m.nq - 7;
  if (i < 3) return m.clip_pos[row * 3 + i];
  if (i < 7) return m.clip_quat[row * 4 + (i - 3)];
  if (i < m.nq) return m.clip_joints[row * (size_t)nj + (i - 7)];
  i -= m.nq;
  if (i < 3) return m.clip_vel[row * 3 + i];
  if (i < 6) return m.clip_angvel[row * 3 + (i - 3)];
  return m.clip_jvel[row * (size_t)(m.nv - 6) + (i - 6)];
}

// `md`: the same model as c.mp through a plain pointer (env_core.h's functions take one); c.rs must be 0 (the [row][n_env] state).
// The caller has checked that this env is done.
TM_DEV void tmw_align(WCtx &c, const WLayout &K, const DModel &md, const int *is, float *obs) {
  TmwModel &m = *c.mp; float *L = c.L;
  const int clip = is[(size_t)md.i_clip_idx * c.n + c.e], start = is[(size_t)md.i_start_frame * c.n + c.e];
  (void)tmw_load_state(c, K, nullptr);       // zeroed LDS image, the kernel's per-launch tables; the terminated qpos / qvel it loads are replaced below
  TMW_LANE_DECL
  const int frame = tm_cur_frame(md, WST(m.s_time, 0), start);
  const size_t row = tm_clip_row(md, clip, frame);
  TMW_FOR {
    for (int i = lane; i < K.nq + K.nv; i += 64) {
      const float v = tm_align_word(md, row, i);
      L[K.l_qpos + i] = v;
      WST(m.s_qpos, i) = v;                  // (qvel follows qpos in the state rows, as tmw_load_state reads them)
    }
  }
  TMW_SYNC();
  tmw_position(c, K, true);                  // emit: xpos and the torso's xmat into the state rows
  TMW_GLOBAL_SYNC();
  TMW_FOR {
    EnvRef r{c.st, nullptr, c.n, c.e};
    for (int part = lane; part < TM_OBS_PARTS(md.traj_length); part += 64) tm_get_obs(md, r, clip, frame, obs, true, part);
  }
}
