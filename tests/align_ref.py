"""Expected values of the align done-policy (AutoAlignWrapperTracking), built from the oracle's existing primitives plus numpy — shared by
tests/test_align_cpu.py and tests/test_gpu_align.py (test infrastructure; the oracle itself is not changed).

The oracle has no entry that re-derives positions and the observation after env_set without also re-running the reward bookkeeping.  What it
has is env_reset: reset at start_frame = f with zero qpos noise and qvel "noise" = the clip's qvel row puts a scratch env onto exactly the
aligned state (qpos, qvel <- the clip at frame f), runs the forward pass, and builds the observation for cur_frame = floor(0 * hz + f) = f with
the same clip.  The only observation entries that read something a reset changes are the nv actuator forces (qfrc_actuator: the aligned env keeps
the terminated step's); they are patched in from the stepped env, through the observation's nan_to_num."""
from __future__ import annotations

import numpy as np


def clip_qpos(clips: dict, c: int, f: int) -> np.ndarray:
    """float32 [nq]: position | quaternion | joints of frame f (clamped to the clip's last frame) of clip c."""
    f = min(max(int(f), 0), clips["position"].shape[1] - 1)
    return np.concatenate([clips[k][c, f] for k in ("position", "quaternion", "joints")]).astype(np.float32)


def clip_qvel(clips: dict, c: int, f: int) -> np.ndarray:
    """float32 [nv]: velocity | angular_velocity | joints_velocity of the same frame."""
    f = min(max(int(f), 0), clips["position"].shape[1] - 1)
    return np.concatenate([clips[k][c, f] for k in ("velocity", "angular_velocity", "joints_velocity")]).astype(np.float32)


def actuator_force_columns(nq: int, nv: int, n_joint_idx: int, n_body_idx: int, traj_length: int) -> slice:
    """The observation columns that hold qfrc_actuator (csrc/env_core.h: tm_get_obs)."""
    o0 = traj_length * (7 + n_joint_idx + 3 * n_body_idx) + (nq - 7) + (nv - 6)
    return slice(o0, o0 + nv)


def nan_to_num32(x):
    return np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=np.finfo(np.float32).max, neginf=-np.finfo(np.float32).max)


def oracle_align(O, envs, i: int, clips: dict, scratch, force_cols: slice):
    """Apply the align policy to oracle env i (which has just stepped with done set): returns (qpos, qvel, expected obs) and leaves env i on the
    aligned state, ready for its next step."""
    c, f = int(O.env_get(envs, i, "clip_idx")[0]), int(O.env_get(envs, i, "cur_frame")[0])
    qpos, qvel = clip_qpos(clips, c, f), clip_qvel(clips, c, f)
    qfrc = O.env_get(envs, i, "qfrc_actuator")
    O.env_reset(scratch, 0, c, min(max(f, 0), clips["position"].shape[1] - 1), np.zeros(qpos.size), qvel.astype(np.float64))
    obs = O.env_get(scratch, 0, "obs").copy()
    obs[force_cols] = nan_to_num32(qfrc)
    O.env_set(envs, i, "qpos", qpos.astype(np.float64))
    O.env_set(envs, i, "qvel", qvel.astype(np.float64))
    return qpos, qvel, obs


def violent_actions(rng, nu: int, n: int, scales=(0.02, 0.1, 0.3)) -> np.ndarray:
    """[nu][n] float32 actions; env e draws at scales[e % len(scales)] of the control range.  At a third of the range the imitation terminations (bad
    pose, too far, fall) occur within a few steps of tracking, and again after an alignment, while fewer than 5 % of the envs go NaN (full-scale
    actions under action_repeat = 2 drove 8 % there on the CPU emulation); the quiet third survives to its truncation."""
    sc = np.asarray(scales, np.float64)[np.arange(n) % len(scales)]
    return np.clip(rng.normal(size=(nu, n)) * sc[None, :], -1, 1).astype(np.float32)
