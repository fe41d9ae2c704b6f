"""wrappers.wrap mirror (reference: track_mjx/environment/wrappers.py:18-56).

In the reference `wrap` stacks brax's EpisodeWrapper and VmapWrapper and then the
(LSTM)AutoResetWrapperTracking.  Here batching is native and the episode / auto-reset logic runs
inside the K3 kernel (csrc/env_core.h: tm_step_prologue / tm_step_post), so `wrap` only switches
those semantics on for the env's handle and returns the env itself.  `action_repeat` is brax EpisodeWrapper's: the env's own step
runs that many times per `step` with the same action, rewards summed, the step counter advanced by `action_repeat`
(include/tmjx.h: tmjx_set_action_repeat).

AutoAlignWrapperTracking (wrappers.py:328-381) and EvalClipWrapperTracking (wrappers.py:313-325) are the evaluation-side wrappers: the first
switches the handle to the align done-policy (include/tmjx.h: tmjx_set_done_policy; csrc/wave_align.h), the second pins reset to a clip's frame 0.
"""
from __future__ import annotations

from .task import MultiClipTracking


def wrap(env: MultiClipTracking, episode_length: int = 1000, action_repeat: int = 1, randomization_fn=None,
         use_lstm: bool = True, hidden_state_dim: int = 128, hidden_layer_num: int = 2) -> MultiClipTracking:
    """Episode (steps/truncation) + auto-reset semantics (wrappers.py:104-144, brax EpisodeWrapper).

    `use_lstm`, `hidden_state_dim`, `hidden_layer_num` are accepted for signature parity: the LSTM
    auto-reset wrapper differs from the plain one only by an unused `info["hidden_state"]`
    (wrappers.py:59-144 vs 278-310), which is not materialised."""
    if randomization_fn is not None:
        # brax's DomainRandomizationVmapWrapper steps every env with its own copy of the mjx.Model; the physics kernel reads ONE model
        # from constant memory (csrc/dmodel.h), and no reference config or call site passes a randomization_fn (ppo.py:466-474)
        raise NotImplementedError("domain randomisation (a per-env model) is not supported: the device model is one constant per handle")
    env.configure_wrappers(int(episode_length), auto_reset=True, action_repeat=int(action_repeat))
    return env


def AutoAlignWrapperTracking(env: MultiClipTracking, episode_length: int = 1000, action_repeat: int = 1) -> MultiClipTracking:
    """Align-on-failure tracking (wrappers.py:328-381) with brax EpisodeWrapper's step counter / truncation underneath it, in the style of `wrap`:
    the handle is switched to the align done-policy and the env itself is returned.  An env whose step ends with done set (terminated or truncated
    at `episode_length`) is put onto the reference pose and velocities of the clip frame it has reached — kinematics and a fresh observation
    included, inside the same `step` — and tracking goes on; `state.done` of that step counts one re-alignment.  time is not rewound and
    prev_ctrl is not restored.  With `action_repeat` > 1 the alignment follows the last inner step.  Needs the clip set's velocity and
    joints_velocity (a ValueError / TmjxError otherwise)."""
    if not isinstance(env, MultiClipTracking):
        raise TypeError(f"AutoAlignWrapperTracking wraps a MultiClipTracking env, not {type(env).__name__}")
    if int(episode_length) < 1:
        raise ValueError("episode_length must be >= 1")
    if int(action_repeat) < 1:
        raise ValueError("action_repeat must be >= 1")
    env.configure_wrappers(int(episode_length), auto_reset=False, action_repeat=int(action_repeat), done_policy="align")
    return env


class EvalClipWrapperTracking:
    """reset at frame 0 of a given clip (wrappers.py:313-325: reset_from_clip(rng, {clip_idx, start_frame: 0}, noise=False)); everything else is
    the wrapped env's.  As in the reference, noise=False zeroes the qvel noise ONLY: the qpos noise U(-reset_noise_scale, +reset_noise_scale) is
    still drawn and added (single_clip_tracking.py:153-161)."""

    def __init__(self, env: MultiClipTracking):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, rng=None, clip_idx=None):
        import torch
        e = self.env
        n = e.num_envs
        if clip_idx is None:
            raise ValueError("EvalClipWrapperTracking.reset needs clip_idx (an int for every env, or one per env)")
        ci = torch.as_tensor(clip_idx, dtype=torch.int32).reshape(-1)
        if ci.numel() == 1:
            ci = ci.expand(n).contiguous()
        if ci.numel() != n:
            raise ValueError(f"clip_idx must be one int or {n} of them")
        if int(ci.min()) < 0 or int(ci.max()) >= max(e._n_clips, 1):
            raise IndexError(f"clip_idx outside the table's {e._n_clips} clips")
        return e.reset(rng, ci, start_frame=torch.zeros(n, dtype=torch.int32), qvel_noise=torch.zeros((int(e.layout.nv), n)))
