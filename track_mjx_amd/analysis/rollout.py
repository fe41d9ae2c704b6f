"""Checkpoint roll-outs that record the network's activations — mirror of track_mjx/analysis/rollout.py (create_environment :25-70,
create_rollout_generator / generate_rollout :73-269) with the reset of RenderRolloutWrapperMulticlipTracking (environment/wrappers.py:251-275).

generate_rollout(clip_idx, seed) tracks whole clips from frame 0 with the deterministic policy.  A batch of clips is rolled out at once, one
env per clip (the reference notebook's jit(vmap(generate_rollout)): every clip gets the same seed, hence the same reset noise).  One control
step is a fixed sequence of launches on preallocated buffers, with no torch operation in the loop:

    staging copy of the observation (tmjx_record_step, T = 1)  ->  encoder: tmjx_linear_nolds_norm / tmjx_linear_nolds + tmjx_silu_ln_fwd  ->
    fc2 (tmjx_linear_nolds)  ->  tmjx_latent_concat_det  ->  decoder blocks / LSTM layers (tmjx_linear_nolds [+ tmjx_lstm_seq_fwd, T = 1])  ->
    head  ->  tmjx_action_mode  ->  tmjx_step (tmjx_step_sensors with log_sensor_data)  ->  tmjx_record_step
    (with an intervention, analysis/intervene.py: one tmjx_intervene directly behind the launch that produces its target; without one, exactly these)

Every dense layer is the matrix-core variant of tmjx_linear_nolds (row-major operands with 16-byte aligned rows, K padded to a multiple of 4):
its per-row arithmetic does not depend on the number of rows, so a clip's record is the same bits alone or in any batch.  The recorder
writes each step into device-resident records [clip][T][w]; they are copied to the host once per batch.

A checkpoint trained with mlp_gemm_inputs=bf16 is rolled out on these fp32 kernels (its weights are fp32; only the training GEMMs rounded
their inputs).

log_sensor_data (rollout.py:72-210): the env steps through the recording physics kernel (tmjx_step_sensors: K2 with a sensor stage on the
last substep, the same state / reward bits), whose sensordata and cfrc_ext rows ([rows][n], device buffers at fixed addresses) two more
TMJX_RECORD_SOA streams record: `sensor_readings` [T-1, nsensordata] and `joint_forces` [T-1, nbody, 6] (pipeline_state.sensordata / cfrc_ext
of the reference; values of the last substep's forward, like the reference's).  The roll-out env has no auto-reset; on an auto-reset handle
the values would be those of the physics that ran, before K3 restores a done env.

align_on_fail (AutoAlignWrapperTracking, environment/wrappers.py:328-381): the env steps under the align done-policy (tmjx_set_done_policy), so
a clip is tracked from frame 0 to its end whatever happens on the way: an env that terminates (fell, too far, bad pose, NaN) is put onto the
reference pose of the frame it has reached, inside the same tmjx_step, and goes on.  The record gains `aligned` [T-1] (bool: step t ended with a
re-alignment, so qposes_rollout[t + 1] is the clip's pose) and `n_alignments` (their count: the clip's failure count); the LSTM policy's carry is
zeroed where an alignment happened (tmjx_lstm_seq_fwd's reset flags = the env's done buffer).  Off by default: without it the records are what
they were.

CLI:  python -m track_mjx_amd.analysis.rollout checkpoint=<run dir | step dir> [data_path=...] [clips=all|a:b|i,j,k] [seed=42] [out=<dir>]
      [log_activations=true] [log_metrics=true] [log_sensor_data=false] [log_decoder_input=false] [align_on_fail=false]
      ->  <out>/clip_<idx>.h5 (save_to_h5py layout + a `meta` group)
      log_decoder_input=true: an LSTM roll-out also records activations/egocentric_obs, the normalised proprioceptive columns of the decoder's input
      row (an MLP roll-out always does), which analysis.jacobian needs to place the LSTM decoder's Jacobian at the recorded steps.
      replay_latents=<dir of clip_<i>.h5> [latent_scale=1.0] [path=auto|fused|layers]: instead of running the encoder, re-run the clips of those files
      through a HighLevelWrapper env (environment/wrappers.py: the checkpoint's decoder inside the env) fed their recorded activations/intention
      (times latent_scale), and write the same clip_<i>.h5 layout (activations: the intention that was fed).
      intervene_pca=<pca.h5> [intervene_components=a:b] | intervene_readout=<readout.h5> [intervene_columns=a:b] | intervene_centroids=<clusters.h5> [intervene_columns=a:b] | intervene_units=<target>:i,j,k
      [intervene_mean=<pca.h5>], with [intervene_gain=0] [intervene_offset=0] [intervene_window=a:b] [intervene_dose=<d | d0,d1,..>]: the roll-out (or the
      replay) runs with that edit of one activation (analysis/intervene.py) and every clip_<i>.h5 gains the group `intervention`.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Callable, Sequence

import numpy as np
import torch

from .. import hip as _hip
from .. import jax_random as _jr
from ..agent.launch_list import LaunchList, ceil4 as _ceil4, ptr as _p
from ..environment.task import METRIC_NAMES

# logging_config.rollout_metrics of rodent-full-clips.yaml:97-113 (the default when a config has no logging_config)
ROLLOUT_METRICS = ("pos_reward", "quat_reward", "joint_reward", "angvel_reward", "bodypos_reward", "endeff_reward", "summed_pos_distance",
                   "joint_distance", "quat_distance", "ctrl_cost", "ctrl_diff_cost", "energy_cost", "too_far", "bad_pose", "bad_quat", "fall")
CLIPS_PER_BATCH = 1024


# ---------------------------------------------------------------------------------------------------------------- environment
def create_environment(cfg: dict, num_envs: int = 1, device: str | torch.device = "cuda"):
    """The env of the checkpoint's config on ALL clips of `data_path` (rollout.py:25-70); "synthetic" rebuilds the training run's synthetic
    table (n_synthetic_clips, clip seed 0).  No Episode / AutoReset wrapper: the env keeps stepping after done."""
    from .. import clips as _clips
    from ..train import build_env
    from ..walker import Rodent
    path = cfg.get("data_path", "synthetic")
    if path == "synthetic":
        table = _clips.make_synthetic_clips(Rodent(**cfg["walker_config"]).model, int(cfg.get("n_synthetic_clips", 64)),
                                            n_frames=cfg["reference_config"]["clip_length"], seed=0, mocap_hz=cfg["env_config"]["env_args"]["mocap_hz"])
    else:
        from ..io import load
        table = load.load_data(path)
    return build_env(cfg, int(num_envs), device, reference_clip=table)


def _sibling_env(env, n: int):
    """An env of `n` envs with `env`'s model and configuration that reads `env`'s resident clip table."""
    from ..environment.task import MultiClipTracking
    return MultiClipTracking(env._reference_clips, env.walker, env._reward_config, physics_steps_per_control_step=env._n_frames,
                             reset_noise_scale=env._reset_noise_scale, iterations=env._opts["iterations"], ls_iterations=env._opts["ls_iterations"],
                             mj_model_timestep=env._opts["timestep"], mocap_hz=env._mocap_hz, clip_length=env._clip_length,
                             random_init_range=env._random_init_range, traj_length=env._ref_len, num_envs=n, device=env.device,
                             share_clips_with=env if env._clip_owner is None else env._clip_owner)


# ---------------------------------------------------------------------------------------------------------------- key plumbing
def reset_inputs(seed: int, n_clips: int, nq: int, nv: int, noise_scale: float, clip_idx: int | None = None):
    """(clip_idx, qpos_noise [nq], qvel_noise [nv]) of generate_rollout(clip_idx, seed): key = PRNGKey(seed); _, reset_rng, act_rng = split(key, 3)
    (rollout.py:133-134); RenderRolloutWrapperMulticlipTracking.reset: _, clip_rng, rng = split(reset_rng, 3), clip_idx = randint(clip_rng, (), 0,
    n_clips) when None, start_frame = 0 (wrappers.py:266-271); reset_from_clip: _, rng1, _ = split(rng, 3), both noises from rng1
    (single_clip_tracking.py:134-161)."""
    reset_rng = _jr.split(_jr.PRNGKey(int(seed)), 3)[1]
    _, clip_rng, rng = _jr.split(reset_rng, 3)
    if clip_idx is None:
        clip_idx = int(_jr.randint(clip_rng, (), 0, int(n_clips)))
    rng1 = _jr.split(rng, 3)[1]
    s = float(noise_scale)
    return int(clip_idx), _jr.uniform(rng1, (int(nq),), -s, s), _jr.uniform(rng1, (int(nv),), -s, s)


# ---------------------------------------------------------------------------------------------------------------- inference fn
class RolloutPolicy:
    """The deterministic inference function of a checkpoint (checkpointing.load_inference_fn): the policy module with fp32 weights on the
    device and the normaliser's mean / std.  create_rollout_generator runs it on the HIP kernels; calling it acts on a batch of observations."""

    def __init__(self, policy, mean: torch.Tensor | None, std: torch.Tensor | None, model: str, get_activation: bool = True,
                 trained_gemm_inputs: str = "f32"):
        self.policy, self.mean, self.std, self.model = policy, mean, std, model
        self.get_activation, self.trained_gemm_inputs = bool(get_activation), trained_gemm_inputs
        self.device = policy.fc2.weight.device
        self.action_size = int(policy.action_size)

    @torch.no_grad()
    def __call__(self, obs: torch.Tensor, key=None, hidden_state=None, intervention=None, t: int = 0):
        """obs [n, W] (raw) -> (ctrl [n, nu], {"activations": ...}) (+ the new (h, c) [n, L, H] for the LSTM policy, from `hidden_state` or zeros).
        `intervention` (analysis.intervene.Intervention): the step runs with its edit, gated as at control step `t` (its window / dose: one value,
        or one per row of obs); the activations are what the rest of the network saw."""
        obs = obs.to(device=self.device, dtype=torch.float32)
        n = obs.shape[0]
        step = _PolicyStep(self, n, obs.t().contiguous(), record=False, intervention=intervention,
                           gates=None if intervention is None else intervention.per_clip(n))
        if self.model == "lstm" and hidden_state is not None:
            step.h.copy_(hidden_state[0]); step.c.copy_(hidden_state[1])
        step.launch(t)
        torch.cuda.current_stream(self.device).synchronize()
        ctrl = step.ctrl.clone()
        extras = {"activations": {k: v.clone() for k, v in step.activation_views().items()}} if self.get_activation else {}
        if self.model == "lstm":
            return ctrl, extras, (step.h.clone(), step.c.clone())
        return ctrl, extras


class _PolicyStep:
    """Preallocated buffers and the launch sequence of one deterministic policy step for `n` envs reading the env's raw observation
    buffer obs_soa [W][n]."""

    def __init__(self, rp: RolloutPolicy, n: int, obs_soa: torch.Tensor, record: bool = True, carry_reset: torch.Tensor | None = None,
                 intervention=None, gates=None, decoder_input: bool = False):
        """`carry_reset` [n] float32 (LSTM policy): where it is non-zero when the step is launched, the row's (h, c) are zeroed first.
        `decoder_input` (LSTM policy): the normalised proprioceptive columns of the decoder's input row are an activation, egocentric_obs, as they
        always are for the MLP policy.
        `intervention` (analysis.intervene.Intervention) with `gates` = (window [n, 2], dose [n]): one tmjx_intervene call directly behind the
        launch that produces its target; without one the list is what it always was."""
        pol, dev = rp.policy, rp.device
        self.rp, self.n, self.obs_soa = rp, int(n), obs_soa
        self.L = _hip.lib()
        f32 = dict(dtype=torch.float32, device=dev)
        W = obs_soa.shape[0]
        ref, Z, A = pol.reference_obs_size, pol.latents, pol.action_size
        if W % 4:
            raise ValueError(f"roll-out: the observation width {W} must be a multiple of 4 (row-major staging with 16-byte aligned rows)")
        self.W, self.ref, self.Z, self.A = W, ref, Z, A
        self.stage = torch.zeros((n, W), **f32)
        # normaliser: mean / std of the whole observation (tmjx_latent_concat_det), mean / 1 / std of the reference part padded with zeros
        # to the first layer's padded K (tmjx_linear_nolds_norm; the pad columns of the weight are zero)
        Kp = _ceil4(ref)
        self.mean, self.std = (rp.mean.contiguous(), rp.std.contiguous()) if rp.mean is not None else (None, None)
        self.fold_mean, self.fold_inv = torch.zeros(Kp, **f32), torch.zeros(Kp, **f32)
        if self.mean is not None:
            self.fold_mean[:ref].copy_(self.mean[:ref])
            torch.reciprocal(self.std[:ref], out=self.fold_inv[:ref])
        else:
            self.fold_inv[:ref].fill_(1.0)
        ll = self.ll = LaunchList(n, dev)      # the step's calls in launch order (agent/launch_list.py: the decoder half is HighLevelWrapper's too)
        self.acts = {"encoder": {}}         # activation name -> (buffer, column offset, width, leading dimension)
        h = None
        for i, blk in enumerate(pol.encoder):
            h = ll.block(self.stage, W, blk, fold=(self.fold_mean, self.fold_inv)) if i == 0 else ll.block(h, h.shape[1], blk)
            self.acts["encoder"][f"layer_{i}"] = (h, 0, h.shape[1], h.shape[1])
        self.fc2 = ll.linear(h, h.shape[1], pol.fc2.weight, pol.fc2.bias)
        self.acts["encoder"]["mean"] = (self.fc2, 0, Z, 2 * Z)
        self.acts["encoder"]["logvar"] = (self.fc2, Z, Z, 2 * Z)
        prop = W - ref
        self.x = torch.zeros((n, _ceil4(Z + prop)), **f32)
        self.traj = torch.zeros((n, Kp), **f32)
        ll.call("tmjx_latent_concat_det", _p(self.fc2), 2 * Z, _p(self.stage), W, 1, _p(self.mean), _p(self.std), _p(self.x), self.x.shape[1],
                _p(self.traj), self.traj.shape[1], n, Z, W, ref)
        if rp.model == "lstm":
            Lk, H = pol.hidden_layer_num, pol.hidden_state_size
            self.h, self.c = torch.zeros((n, Lk, H), **f32), torch.zeros((n, Lk, H), **f32)
            _, self.logits, self.ctrl, self.action_t = ll.decoder(self.x, (), pol.projection.weight, pol.projection.bias,
                                                                  lstm=(pol.w_ih, pol.w_hh, pol.b_hh, self.h, self.c, carry_reset))
            self.acts["decoder"] = {"lstm_projection": (self.logits, 0, 2 * A, 2 * A)}
            if decoder_input:
                self.acts["egocentric_obs"] = (self.x, Z, prop, self.x.shape[1])
        else:
            ys, self.logits, self.ctrl, self.action_t = ll.decoder(self.x, pol.decoder, pol.head.weight, pol.head.bias)
            self.acts["decoder"] = {f"layer_{i}": (y, 0, y.shape[1], y.shape[1]) for i, y in enumerate(ys)}
            self.acts["egocentric_obs"] = (self.x, Z, prop, self.x.shape[1])
            self.acts["traj_obs"] = (self.traj, 0, ref, self.traj.shape[1])
        self.acts["intention"] = (self.x, 0, Z, self.x.shape[1])
        # the staging copy of the observation: one SoA stream into a [n][1][W] record
        st = _hip.RecordStream(_p(obs_soa), _p(self.stage), _hip.RECORD_SOA, n, W, W, 1, 0, 0)
        self.stage_table = _upload_table([st], n, 1, dev)
        # (a list built on the host, to be inspected and never launched, has no stream)
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if torch.device(dev).type == "cuda" else None
        self.iv_entry = self.iv = None
        if intervention is not None:
            layers = {f"{part}/{k}": v[0] for part in ("encoder", "decoder") for k, v in self.acts[part].items() if k.startswith("layer_")}
            self.iv_entry, self.iv = ll.place_intervention(intervention, gates[0], gates[1], self.x, Z, layers, self.h if rp.model == "lstm" else None)

    def launch(self, t: int = 0) -> None:
        """The policy step's launches on the current stream (ctypes calls only: no torch operation); `t`: the control-step index an
        intervention's gate sees."""
        if self.iv_entry is not None:
            self.iv_entry[1][1] = t
        _hip.check(self.L.tmjx_record_step(self.stage_table.data_ptr(), 1, self.n, 0, 1, self.stream), "tmjx_record_step")
        self.ll.run(self.stream)

    def activation_views(self) -> dict:
        out = {}
        for k, v in self.acts.items():
            if isinstance(v, dict):
                for k2, (buf, c0, w, _) in v.items():
                    out[f"{k}/{k2}"] = buf[:, c0:c0 + w]
            else:
                buf, c0, w, _ = v
                out[k] = buf[:, c0:c0 + w]
        if self.rp.model == "lstm":
            out["hidden_state/h"], out["hidden_state/c"] = self.h, self.c
        return out


def _upload_table(streams: Sequence, n: int, T: int, dev) -> torch.Tensor:
    """Validate a recorder stream table on the host (tmjx_record_check) and copy it to the device once (16-byte aligned)."""
    k = len(streams)
    tab = (_hip.RecordStream * k)(*streams)
    _hip.check(_hip.lib().tmjx_record_check(tab, k, int(n), int(T)), "tmjx_record_check")
    raw = np.frombuffer(bytes(tab), dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(dev)


# ---------------------------------------------------------------------------------------------------------------- generator
def create_rollout_generator(cfg: dict, environment, inference_fn: Callable, model: str = "mlp", log_activations: bool = False,
                             log_metrics: bool = False, log_sensor_data: bool = False, clips_per_batch: int = CLIPS_PER_BATCH,
                             align_on_fail: bool = False, friction_scale=None, actuator_scale=None, damping_scale=None,
                             gravity_scale=None, slope_deg=None, intervention=None, log_decoder_input: bool = False):
    """rollout.py:73-269.  Returns generate_rollout(clip_idx=None, seed=42): one clip (int / None) -> dict of arrays; a sequence of clips -> the
    same dict with a leading [N] axis (batches larger than `clips_per_batch` run in chunks).

    `friction_scale` / `actuator_scale` / `damping_scale` (the perturbation experiment): one float for every clip, or one per clip of a
    generate_rollout call — each roll-out env then runs with its clip's scales of the model's sliding friction, actuator force and dof damping
    (environment.DomainRandomization), and the result carries them as `domain_scales` [3].  All None: the env as it was given.

    `gravity_scale` / `slope_deg` (one float, or one per clip, likewise): the clip's env runs with the gravity vector slope_gravity(|g|, s, a) =
    s |g| (sin a, 0, -cos a), |g| the magnitude of the model's gravity — s < 1 is body-weight support, a > 0 a floor inclined so that +x is
    downhill — and the result carries it as `gravity` [3].

    `intervention` (analysis.intervene.Intervention): the policy step runs with its edit of one activation (one more launch, tmjx_intervene, behind
    the one that produces the target); its window and dose are one value, or one per clip of a generate_rollout call (a clip may be repeated in
    clip_idx with different doses).  The result gains the group `intervention` (target, mode, directions | units, center, gain, offset, window [2],
    dose and, in subspace mode, projection [T - 1, K]: the pre-edit coordinates of every step, ON or OFF), and the recorded activation of the
    target is its value after the edit.

    `log_decoder_input`: with log_activations, an LSTM roll-out also records activations/egocentric_obs [T - 1, prop], the normalised proprioceptive
    columns of the decoder's input row, which an MLP roll-out always records (analysis.jacobian places the LSTM decoder's Jacobian there).  On an
    MLP policy it changes nothing."""
    if intervention is not None:
        from .intervene import Intervention
        if not isinstance(intervention, Intervention):
            raise TypeError(f"intervention must be an analysis.intervene.Intervention, got {type(intervention).__name__}")
    iv_gates: dict = {}
    given_scales = {k: v for k, v in (("friction", friction_scale), ("actuator", actuator_scale), ("damping", damping_scale)) if v is not None}
    if given_scales and not hasattr(environment, "set_domain_randomization"):
        raise NotImplementedError(f"friction_scale / actuator_scale / damping_scale: {type(environment).__name__} has no per-env scales "
                                  "(MultiClipTracking.set_domain_randomization)")
    if given_scales and log_sensor_data:
        raise NotImplementedError("log_sensor_data cannot be combined with friction_scale / actuator_scale / damping_scale: the recording physics "
                                  "kernel that produces sensor_readings and joint_forces has no domain-randomisation build; run the perturbed "
                                  "roll-out without log_sensor_data, or the sensor roll-out without scales")
    given_gravity = {k: v for k, v in (("gravity_scale", gravity_scale), ("slope_deg", slope_deg)) if v is not None}
    if given_gravity and not hasattr(environment, "set_domain_randomization"):
        raise NotImplementedError(f"gravity_scale / slope_deg: {type(environment).__name__} has no per-env gravity "
                                  "(MultiClipTracking.set_domain_randomization)")
    if given_gravity and log_sensor_data:
        raise NotImplementedError("log_sensor_data cannot be combined with gravity_scale / slope_deg: the recording physics kernel that produces "
                                  "sensor_readings and joint_forces reads the model's gravity and has no per-env build; run the perturbed "
                                  "roll-out without log_sensor_data, or the sensor roll-out without them")
    if log_sensor_data and not hasattr(environment, "sensor_buffers"):
        raise NotImplementedError("log_sensor_data: cfrc_ext and sensordata are not computed by the physics kernel of this environment: they "
                                  "come from MultiClipTracking's recording kernel (tmjx_step_sensors), and the environment given is "
                                  f"{type(environment).__name__}")
    if not isinstance(inference_fn, RolloutPolicy):
        raise TypeError("create_rollout_generator: inference_fn must be the deterministic inference function made by "
                        "track_mjx_amd.agent.checkpoint.load_inference_fn (the roll-out runs it on the HIP kernels); got "
                        f"{type(inference_fn).__name__}")
    if model not in ("mlp", "lstm"):
        raise ValueError("model must be 'mlp' or 'lstm'")
    if model != inference_fn.model:
        raise ValueError(f"model={model!r} but the inference function holds the {inference_fn.model} policy")
    metrics = tuple((cfg.get("logging_config") or {}).get("rollout_metrics", ROLLOUT_METRICS))
    bad = [m for m in metrics if m not in METRIC_NAMES]
    if bad:
        raise ValueError(f"logging_config.rollout_metrics: unknown metrics {bad} (known: {METRIC_NAMES})")
    if log_metrics and len(metrics) > _hip.RECORD_MAX_IDX:
        raise ValueError(f"at most {_hip.RECORD_MAX_IDX} rollout metrics")
    env0 = environment
    spf = float(env0._steps_for_cur_frame)
    T = int(int(cfg["reference_config"]["clip_length"]) * spf)
    if T < 2:
        raise ValueError("a roll-out needs clip_length * steps_for_cur_frame >= 2")
    envs: dict = {}

    policy = "align" if align_on_fail else "none"
    if align_on_fail and not hasattr(env0, "configure_wrappers"):
        raise NotImplementedError(f"align_on_fail: {type(env0).__name__} has no done-policy to switch (MultiClipTracking.configure_wrappers)")

    def with_policy(env):
        # align_on_fail: the handle under the align done-policy, no episode limit; otherwise the env as it was given — except one that an
        # earlier align_on_fail generator left aligning, which goes back to stepping on after done
        if getattr(env, "_done_policy", "none") != policy and (align_on_fail or env._done_policy == "align"):
            env.configure_wrappers(env._episode_length if not align_on_fail else (1 << 30), auto_reset=False,
                                   action_repeat=getattr(env, "_action_repeat", 1), done_policy=policy)
        return env

    def env_of(n):
        if n == env0.num_envs:
            return with_policy(env0)
        if n not in envs:
            envs.clear()                    # (one cached sibling: the buffers of a batch size are not kept around)
            envs[n] = _sibling_env(env0, n)
        return with_policy(envs[n])

    def scales_of(n: int, offset: int, total: int):
        """[3][n] scales of clips offset .. offset + n of a call of `total` clips, or None."""
        if not given_scales:
            return None
        tab = np.ones((3, n), np.float32)
        for r, name in enumerate(("friction", "actuator", "damping")):
            if name not in given_scales:
                continue
            v = np.atleast_1d(np.asarray(given_scales[name], dtype=np.float64)).ravel()
            if v.size not in (1, total):
                raise ValueError(f"{name}_scale: {v.size} values for {total} clips (one value, or one per clip)")
            tab[r] = v[0] if v.size == 1 else v[offset:offset + n]
        return tab

    def gravity_of(n: int, offset: int, total: int):
        """[n, 3] gravity vectors of clips offset .. offset + n of a call of `total` clips, or None."""
        if not given_gravity:
            return None
        per = {}
        for name, default in (("gravity_scale", 1.0), ("slope_deg", 0.0)):
            v = np.atleast_1d(np.asarray(given_gravity.get(name, default), dtype=np.float64)).ravel()
            if v.size not in (1, total):
                raise ValueError(f"{name}: {v.size} values for {total} clips (one value, or one per clip)")
            per[name] = np.full(n, v[0]) if v.size == 1 else v[offset:offset + n]
        return slope_gravity(model_gravity_magnitude(env0), per["gravity_scale"], per["slope_deg"])

    def run_batch(clips: list, seed: int, scales=None, gravity=None, gates=None) -> dict:
        n = len(clips)
        env = env_of(n)
        if scales is not None or gravity is not None:
            from ..environment import DomainRandomization
            sc = (None, None, None) if scales is None else (scales[0], scales[1], scales[2])
            env.set_domain_randomization(DomainRandomization(*sc, num_envs=n, gravity=gravity))
        dev, Lay = env.device, env.layout
        nq, nv = int(Lay.nq), int(Lay.nv)
        qn, vn = np.empty((nq, n), np.float32), np.empty((nv, n), np.float32)
        for j, c in enumerate(clips):
            _, qn[:, j], vn[:, j] = reset_inputs(seed, env._n_clips, nq, nv, env._reset_noise_scale, c)
        with torch.cuda.device(dev):
            env.reset(None, torch.tensor(clips, dtype=torch.int32), start_frame=torch.zeros(n, dtype=torch.int32),
                      qpos_noise=torch.from_numpy(qn), qvel_noise=torch.from_numpy(vn))
            # align_on_fail: the LSTM carry of an env is zeroed in the policy step that follows its alignment (done_buf is 0 after reset)
            step = _PolicyStep(inference_fn, n, env.obs_buf, carry_reset=env.done_buf if align_on_fail and inference_fn.model == "lstm" else None,
                               intervention=intervention, gates=gates, decoder_input=bool(log_decoder_input))
            f32 = dict(dtype=torch.float32, device=dev)
            rec: dict = {}
            state_streams, step_streams = [], []

            def add(name, buf_ptr, layout, ld, w, extent, rows, t0, idx=()):
                dst = torch.empty((n, rows, w), **f32)
                rec[name] = dst
                s = _hip.RecordStream(buf_ptr, _p(dst), layout, ld, w, extent, rows, t0, len(idx))
                for i, v in enumerate(idx):
                    s.idx[i] = v
                return s

            sb = env.state_buf
            state = [("qposes_rollout", sb.data_ptr() + 4 * Lay.qpos * n, _hip.RECORD_SOA, n, nq, nq, ()),
                     ("state_rewards", _p(env.reward_buf), _hip.RECORD_SOA, n, 1, 1, ())]
            if log_metrics:
                state.append(("rollout_metrics", _p(env.metrics_buf), _hip.RECORD_SOA, n, len(metrics), len(METRIC_NAMES),
                              tuple(METRIC_NAMES.index(m) for m in metrics)))
            for name, ptr, lay, ld, w, ext, idx in state:
                state_streams.append(add(name, ptr, lay, ld, w, ext, T, 1, idx))
            init_streams = []
            for (name, ptr, lay, ld, w, ext, idx), s in zip(state, state_streams):
                s0 = _hip.RecordStream.from_buffer_copy(s)
                s0.t0 = 0
                init_streams.append(s0)
            step_streams.append(add("ctrl", _p(step.ctrl), _hip.RECORD_ROWMAJOR, inference_fn.action_size, inference_fn.action_size,
                                    inference_fn.action_size, T - 1, 0))
            if log_activations:
                for name, v in step.acts.items():
                    items = v.items() if isinstance(v, dict) else [(None, v)]
                    for k2, (buf, c0, w, ld) in items:
                        key = name if k2 is None else f"{name}/{k2}"
                        step_streams.append(add("act:" + key, buf.data_ptr() + 4 * c0, _hip.RECORD_ROWMAJOR, ld, w, w, T - 1, 0))
                if inference_fn.model == "lstm":
                    LH = step.h.shape[1] * step.h.shape[2]
                    step_streams.append(add("act:hidden_state/h", _p(step.h), _hip.RECORD_ROWMAJOR, LH, LH, LH, T - 1, 0))
                    step_streams.append(add("act:hidden_state/c", _p(step.c), _hip.RECORD_ROWMAJOR, LH, LH, LH, T - 1, 0))
            if log_sensor_data:
                sd_buf, cf_buf = env.sensor_buffers()
                nsd, nb6 = (0 if sd_buf is None else sd_buf.shape[0]), cf_buf.shape[0]
                if nsd:
                    step_streams.append(add("sensor_readings", _p(sd_buf), _hip.RECORD_SOA, n, nsd, nsd, T - 1, 0))
                step_streams.append(add("joint_forces", _p(cf_buf), _hip.RECORD_SOA, n, nb6, nb6, T - 1, 0))
            if align_on_fail:
                step_streams.append(add("aligned", _p(env.done_buf), _hip.RECORD_SOA, n, 1, 1, T - 1, 0))
            if step.iv is not None and step.iv.proj is not None:
                K = step.iv.K
                step_streams.append(add("intervention:projection", _p(step.iv.proj), _hip.RECORD_ROWMAJOR, K, K, K, T - 1, 0))
            init_tab = _upload_table(init_streams, n, 1, dev)
            state_tab = _upload_table(state_streams, n, T - 1, dev)
            step_tab = _upload_table(step_streams, n, T - 1, dev)
            L, s = _hip.lib(), step.stream
            hdl = env._handle
            env_args = [_p(env.state_buf), _p(env.istate_buf), _p(step.action_t), _p(env.obs_buf), _p(env.reward_buf), _p(env.done_buf),
                        _p(env.trunc_buf), _p(env.metrics_buf), _p(env.workspace), n]
            step_fn = "tmjx_step"
            if log_sensor_data:       # tmjx_step_sensors: tmjx_step's arguments with the two output buffers in front of n_env
                env._check_sensor_bufs(sd_buf, cf_buf)
                env_args[-1:-1] = [_p(sd_buf), _p(cf_buf)]
                step_fn = "tmjx_step_sensors"
            ks, kp = len(state_streams), len(step_streams)
            _hip.check(L.tmjx_record_step(init_tab.data_ptr(), ks, n, 0, 1, s), "tmjx_record_step")
            _step_loop(step, L, s, hdl, env_args, state_tab.data_ptr(), ks, step_tab.data_ptr(), kp, n, T, step_fn)
            host = {k: v.cpu().numpy() for k, v in rec.items()}          # one device-to-host copy per record, once per batch
        out = {"qposes_rollout": host["qposes_rollout"], "ctrl": host["ctrl"], "state_rewards": host["state_rewards"][:, :, 0]}
        ref = env._reference_clips
        rows = [np.repeat(np.hstack([np.asarray(ref.position[c], np.float32), np.asarray(ref.quaternion[c], np.float32),
                                     np.asarray(ref.joints[c], np.float32)]), int(spf), axis=0) for c in clips]
        out["qposes_ref"] = np.stack(rows)
        if scales is not None:
            out["domain_scales"] = np.ascontiguousarray(scales.T)          # [n, 3]: friction, actuator, damping of each clip's env
        if gravity is not None:
            out["gravity"] = np.ascontiguousarray(gravity, dtype=np.float32)        # [n, 3]: each clip's env's gravity vector (world frame)
        if align_on_fail:
            out["aligned"] = host["aligned"][:, :, 0] != 0
            out["n_alignments"] = out["aligned"].sum(axis=1).astype(np.int64)
        if intervention is not None:
            out["intervention"] = intervention.record(gates[0], gates[1], host.get("intervention:projection"))
        if log_sensor_data:
            out["joint_forces"] = host["joint_forces"].reshape(n, T - 1, -1, 6)
            out["sensor_readings"] = host["sensor_readings"] if "sensor_readings" in host else np.zeros((n, T - 1, 0), np.float32)
        if log_metrics:
            m = host["rollout_metrics"]
            out["rollout_metrics"] = {f"{name}s": np.ascontiguousarray(m[:, :, j]) for j, name in enumerate(metrics)}
        if log_activations:
            acts: dict = {}
            for k, v in host.items():
                if not k.startswith("act:"):
                    continue
                parts = k[4:].split("/")
                node = acts
                for p_ in parts[:-1]:
                    node = node.setdefault(p_, {})
                node[parts[-1]] = v
            if "hidden_state" in acts:
                Lk, H = step.h.shape[1], step.h.shape[2]
                hs = acts.pop("hidden_state")
                acts["hidden_state"] = (hs["h"].reshape(n, T - 1, Lk, H), hs["c"].reshape(n, T - 1, Lk, H))
            out["activations"] = acts
        return out

    def generate_rollout(clip_idx: int | Sequence[int] | None = None, seed: int = 42, scales: dict | None = None, gravity: dict | None = None,
                         gates: dict | None = None) -> dict:
        """`scales`: {"friction" | "actuator" | "damping": float or one per clip} for THIS call, in place of the generator's own (a generator made
        without scales takes none: its sensor / env checks were made for the plain env).  `gravity`: {"gravity_scale" | "slope_deg": ...}, likewise.
        `gates`: {"window" | "dose": one value or one per clip} of the generator's intervention for THIS call, in place of the intervention's own."""
        if gates is not None:
            if intervention is None:
                raise ValueError("generate_rollout(gates=...): the generator was created without an intervention")
            iv_gates.clear(); iv_gates.update({k: v for k, v in gates.items() if v is not None})
        if gravity is not None:
            if not given_gravity:
                raise ValueError("generate_rollout(gravity=...): the generator was created without gravity_scale / slope_deg")
            given_gravity.clear(); given_gravity.update({k: v for k, v in gravity.items() if v is not None})
        if scales is not None:
            if not given_scales:
                raise ValueError("generate_rollout(scales=...): the generator was created without friction_scale / actuator_scale / damping_scale")
            given_scales.clear(); given_scales.update({k: v for k, v in scales.items() if v is not None})
        batched = clip_idx is not None and not isinstance(clip_idx, (int, np.integer))
        if batched:
            clips = [int(c) for c in clip_idx]
        else:
            clips = [reset_inputs(seed, env0._n_clips, int(env0.layout.nq), int(env0.layout.nv), env0._reset_noise_scale,
                                  None if clip_idx is None else int(clip_idx))[0]]
        if not clips:
            raise ValueError("generate_rollout: no clips")
        bad = [c for c in clips if not 0 <= c < env0._n_clips]
        if bad:
            raise IndexError(f"clip indices {bad[:5]} outside the table's {env0._n_clips} clips")
        win = dose = None
        if intervention is not None:
            win, dose = intervention.per_clip(len(clips), iv_gates.get("window"), iv_gates.get("dose"))
        parts = [run_batch(clips[i:i + clips_per_batch], seed, scales_of(len(clips[i:i + clips_per_batch]), i, len(clips)),
                           gravity_of(len(clips[i:i + clips_per_batch]), i, len(clips)),
                           None if intervention is None else (win[i:i + clips_per_batch], dose[i:i + clips_per_batch]))
                 for i in range(0, len(clips), int(clips_per_batch))]
        out = _concat(parts) if len(parts) > 1 else parts[0]
        return out if batched else _index0(out)

    generate_rollout.T = T
    generate_rollout.metrics = metrics
    generate_rollout.done_policy = policy
    return generate_rollout


def _step_loop(step: _PolicyStep, L, s, hdl, env_args, state_tab: int, ks: int, step_tab: int, kp: int, n: int, T: int,
               step_fn: str = "tmjx_step") -> None:
    """The T - 1 control steps: policy launches, tmjx_action_mode (inside step.launch), tmjx_step (or tmjx_step_sensors), tmjx_record_step x 2."""
    env_step = getattr(L, step_fn)
    for t in range(T - 1):
        step.launch(t)
        _hip.check(env_step(hdl, *env_args, s), step_fn)
        _hip.check(L.tmjx_record_step(step_tab, kp, n, t, T - 1, s), "tmjx_record_step")
        _hip.check(L.tmjx_record_step(state_tab, ks, n, t, T - 1, s), "tmjx_record_step")


def _concat(parts: list):
    a = parts[0]
    if isinstance(a, dict):
        return {k: _concat([p[k] for p in parts]) for k in a}
    if isinstance(a, tuple):
        return tuple(_concat([p[i] for p in parts]) for i in range(len(a)))
    return np.concatenate(parts, axis=0)


def _index0(tree):
    if isinstance(tree, dict):
        return {k: _index0(v) for k, v in tree.items()}
    if isinstance(tree, tuple):
        return tuple(_index0(v) for v in tree)
    return tree[0]


# ---------------------------------------------------------------------------------------------------------------- CLI
def _parse_clips(spec: str, n_clips: int) -> list:
    spec = str(spec).strip()
    if spec in ("", "all"):
        return list(range(n_clips))
    if ":" in spec:
        a, _, b = spec.partition(":")
        return list(range(int(a or 0), int(b) if b else n_clips))
    return [int(c) for c in spec.split(",") if c.strip()]


CLI_OPTIONS = ("checkpoint", "clips", "seed", "out", "log_activations", "log_metrics", "log_sensor_data", "log_decoder_input", "align_on_fail", "step",
               "replay_latents", "latent_scale", "path", "friction_scale", "actuator_scale", "damping_scale", "gravity_scale", "slope_deg",
               "intervene_pca", "intervene_components", "intervene_readout", "intervene_centroids", "intervene_columns", "intervene_units", "intervene_mean", "intervene_gain",
               "intervene_offset", "intervene_window", "intervene_dose")


def slope_gravity(magnitude: float, gravity_scale=1.0, slope_deg=0.0) -> np.ndarray:
    """[..., 3] float32: s |g| (sin a, 0, -cos a) — gravity of magnitude s |g| in a world whose floor is inclined by a degrees about the y axis,
    +x downhill for a > 0 (the floor stays the plane z = 0: the gravity vector is tilted instead).  Formed in float64."""
    s, a = np.broadcast_arrays(np.asarray(gravity_scale, dtype=np.float64), np.deg2rad(np.asarray(slope_deg, dtype=np.float64)))
    if not (np.isfinite(s).all() and np.isfinite(a).all()) or (s <= 0).any() or (np.abs(a) >= np.pi / 2).any():
        raise ValueError("gravity_scale must be > 0 and |slope_deg| < 90")
    return (s[..., None] * float(magnitude) * np.stack([np.sin(a), np.zeros_like(a), -np.cos(a)], -1)).astype(np.float32)


def model_gravity_magnitude(env) -> float:
    """|gravity| of the env's model (its blob entry `gravity`)."""
    from .. import blob as _blob
    return float(np.linalg.norm(np.asarray(_blob.unpack(env._blob)["gravity"], dtype=np.float64)))


def parse_per_clip(name: str, text, n_clips: int):
    """A command-line value `v` or `v0,v1,..`: a list of one float, or of one per clip (anything else is a ValueError)."""
    v = [float(x) for x in str(text).split(",") if x.strip() != ""]
    if len(v) not in (1, int(n_clips)):
        raise ValueError(f"{name}: {len(v)} values for {n_clips} clips (one value, or one per clip)")
    return v


def replay_latents(cfg: dict, decoder_policy, clips: Sequence[int], latents: np.ndarray, seed: int = 42, path: str = "auto", metrics=ROLLOUT_METRICS,
                   intervention=None) -> dict:
    """Step a HighLevelWrapper env (the decoder inside the env) from generate_rollout's reset of `clips` with latents [n, T - 1, Z]: the roll-out
    dict ([n] leading axis) with qposes_rollout, ctrl, state_rewards, qposes_ref, rollout_metrics and activations/intention (what was fed).
    `intervention` (analysis.intervene.Intervention on intention, decoder/layer_<i> or hidden_state/h:<k>; window / dose: one value, or one per
    clip): the decoder runs with its edit on the "layers" path (path="fused" raises), and the dict gains the group `intervention`."""
    from ..environment.wrappers import HighLevelWrapper
    n, T = len(clips), latents.shape[1] + 1
    env = create_environment(cfg, n, decoder_policy.device)
    from ..agent.checkpoint import LSTMDecoderPolicy
    # (an LSTM decoder's carry starts from zero at the reset and is never reset afterwards, as in a plain roll-out)
    kw = dict(reset_carry_on_done=False) if isinstance(decoder_policy, LSTMDecoderPolicy) else {}
    hl = HighLevelWrapper(env, decoder_policy, decoder_policy.reference_obs_size, path=path, intervention=intervention, **kw)
    gates = None if intervention is None else intervention.per_clip(n)
    nq, nv = int(env.layout.nq), int(env.layout.nv)
    qn, vn = np.empty((nq, n), np.float32), np.empty((nv, n), np.float32)
    for j, c in enumerate(clips):
        _, qn[:, j], vn[:, j] = reset_inputs(seed, env._n_clips, nq, nv, env._reset_noise_scale, int(c))
    with torch.cuda.device(env.device):
        st = hl.reset(None, torch.tensor([int(c) for c in clips], dtype=torch.int32), start_frame=torch.zeros(n, dtype=torch.int32),
                      qpos_noise=torch.from_numpy(qn), qvel_noise=torch.from_numpy(vn))
        lat = torch.from_numpy(np.ascontiguousarray(latents, dtype=np.float32)).to(env.device)
        f32 = dict(dtype=torch.float32, device=env.device)
        qpos, rew = torch.empty((T, n, nq), **f32), torch.empty((T, n), **f32)
        met, ctrl = torch.empty((T, len(METRIC_NAMES), n), **f32), torch.empty((T - 1, n, decoder_policy.action_size), **f32)
        proj = torch.empty((T - 1, n, intervention.K), **f32) if intervention is not None and intervention.mode == "subspace" else None
        qpos[0].copy_(st.pipeline_state["qpos"]); rew[0].copy_(st.reward); met[0].copy_(env.metrics_buf)
        for t in range(T - 1):
            st = hl.step(st, lat[:, t], t)
            qpos[t + 1].copy_(st.pipeline_state["qpos"]); rew[t + 1].copy_(st.reward); met[t + 1].copy_(env.metrics_buf); ctrl[t].copy_(hl.last_ctrl)
            if proj is not None:
                proj[t].copy_(hl.intervention_projection)
        qpos, rew, met, ctrl = (v.cpu().numpy() for v in (qpos, rew, met, ctrl))
    spf = int(env._steps_for_cur_frame)
    ref = env._reference_clips
    rows = [np.repeat(np.hstack([np.asarray(ref.position[c], np.float32), np.asarray(ref.quaternion[c], np.float32),
                                 np.asarray(ref.joints[c], np.float32)]), spf, axis=0) for c in clips]
    return {"qposes_rollout": np.ascontiguousarray(qpos.transpose(1, 0, 2)), "ctrl": np.ascontiguousarray(ctrl.transpose(1, 0, 2)),
            "state_rewards": np.ascontiguousarray(rew.T), "qposes_ref": np.stack(rows),
            "rollout_metrics": {f"{m}s": np.ascontiguousarray(met[:, METRIC_NAMES.index(m)].T) for m in metrics},
            "activations": {"intention": np.ascontiguousarray(latents, dtype=np.float32)}, "path": hl.path,
            **({} if intervention is None else {"intervention": intervention.record(
                gates[0], gates[1], None if proj is None else np.ascontiguousarray(proj.cpu().numpy().transpose(1, 0, 2)))})}


def _main_replay(opts: dict, cfg: dict, step_dir: str, intervention=None) -> int:
    import re
    from ..agent import checkpoint as ckpt
    from .utils import load_from_h5py, save_to_h5py
    src = opts["replay_latents"]
    found = sorted(int(m.group(1)) for m in (re.fullmatch(r"clip_(\d+)\.h5", f) for f in os.listdir(src)) if m)
    if "clips" in opts and opts["clips"] not in ("", "all"):
        want = set(_parse_clips(opts["clips"], max(found, default=-1) + 1))
        found = [c for c in found if c in want]
    if not found:
        print(f"[rollout] replay_latents: no clip_<i>.h5 in {src}", file=sys.stderr)
        return 2
    scale = float(opts.get("latent_scale", 1.0))
    use_lstm = "lstm_decoder" in ckpt.load_policy(step_dir)[1].get("params", {})
    dp = (ckpt.make_lstm_decoder_policy_fn if use_lstm else ckpt.make_decoder_policy_fn)(step_dir, device="cuda")
    metrics = tuple((cfg.get("logging_config") or {}).get("rollout_metrics", ROLLOUT_METRICS))
    out_dir = opts.get("out", os.path.join(step_dir, "replays"))
    os.makedirs(out_dir, exist_ok=True)
    for i in range(0, len(found), CLIPS_PER_BATCH):
        chunk = found[i:i + CLIPS_PER_BATCH]
        recs = [load_from_h5py(os.path.join(src, f"clip_{c}.h5")) for c in chunk]
        for c, r in zip(chunk, recs):
            if "activations" not in r or "intention" not in r["activations"]:
                raise ValueError(f"replay_latents: {src}/clip_{c}.h5 has no activations/intention (roll it out with log_activations=true)")
        seed = int(opts["seed"]) if "seed" in opts else int(recs[0]["meta"]["seed"])
        lat = np.stack([np.asarray(r["activations"]["intention"], np.float32) for r in recs])
        if scale != 1.0:
            lat = lat * np.float32(scale)
        iv = intervention
        if iv is not None:      # (this chunk's doses of a per-clip list)
            import copy
            iv = copy.copy(intervention)
            iv.dose = intervention.per_clip(len(found))[1][i:i + len(chunk)]
        res = replay_latents(cfg, dp, chunk, lat, seed=seed, path=opts.get("path", "auto"), metrics=metrics, intervention=iv)
        used = res.pop("path")
        for j, c in enumerate(chunk):
            one = _index_j(res, j)
            one["meta"] = {"seed": np.int64(seed), "clip_idx": np.int64(c), "checkpoint": str(step_dir), "model": "lstm" if use_lstm else "mlp", "replay_latents": str(src),
                           "latent_scale": np.float64(scale), "decoder_path": used, "rollout_gemm_inputs": "f32",
                           "trained_gemm_inputs": dp.trained_gemm_inputs}
            save_to_h5py(os.path.join(out_dir, f"clip_{c}.h5"), one)
    print(f"[rollout] replayed the recorded intentions of {len(found)} clips (x {scale}) through the {used} decoder path; wrote {out_dir}", flush=True)
    return 0


def _split_argv(argv) -> tuple:
    """(the roll-out's own key=value options, everything else: config overrides in train's syntax)."""
    from . import cli
    return cli.split(argv, CLI_OPTIONS)


def main(argv=None) -> int:
    from .. import config as _config
    from ..agent import checkpoint as ckpt
    from .utils import save_to_h5py
    argv = list(sys.argv[1:] if argv is None else argv)
    opts, rest = _split_argv(argv)
    if "checkpoint" not in opts:
        print("usage: python -m track_mjx_amd.analysis.rollout checkpoint=<run dir | step dir> [data_path=...] [clips=all|a:b|i,j,k] [seed=42] "
              "[out=<dir>] [log_activations=true] [log_metrics=true] [log_sensor_data=false] [log_decoder_input=false] [align_on_fail=false] "
              "[friction_scale=<s | s0,s1,..>] [actuator_scale=..] [damping_scale=..] [gravity_scale=<s | s0,s1,..>] [slope_deg=<a | a0,a1,..>] "
              "[replay_latents=<dir of clip_<i>.h5> [latent_scale=1.0] [path=auto|fused|layers]] "
              "[intervene_pca=<pca.h5> [intervene_components=a:b] | intervene_readout=<readout.h5> [intervene_columns=a:b] | intervene_centroids=<clusters.h5> [intervene_columns=a:b] | "
              "intervene_units=<target>:i,j,k [intervene_mean=<pca.h5>]] [intervene_gain=0] [intervene_offset=0] [intervene_window=a:b] "
              "[intervene_dose=<d | d0,d1,..>] [key=value config overrides ...]", file=sys.stderr)
        return 2
    yes = lambda v: str(v).lower() in ("1", "true", "yes")     # noqa: E731
    path = opts["checkpoint"]
    step_no = int(opts["step"]) if "step" in opts else None
    cfg = ckpt.load_config_from_checkpoint(path, step_no)
    cfg = _config._deep_update(_config.default_config(), cfg or {})
    for ov in rest:                                   # the same key=value parsing as train
        key, _, val = ov.partition("=")
        node = cfg
        for part in key.split(".")[:-1]:
            node = node.setdefault(part, {})
        import yaml
        node[key.split(".")[-1]] = yaml.safe_load(val)
    step_dir = ckpt.resolve_step_dir(path, step_no)
    from . import intervene as _iv
    try:
        intervention = _iv.from_cli(opts)
        if intervention is not None and "replay_latents" in opts and opts.get("path") == "fused":
            raise ValueError("path=fused cannot run an intervention (the fused decoder launch has no seam between its layers): path=layers or auto")
    except ValueError as e:
        print(f"[rollout] {e}", file=sys.stderr)
        return 2
    if "replay_latents" in opts:
        try:
            return _main_replay(opts, cfg, step_dir, intervention)
        except ValueError as e:
            if intervention is None:
                raise
            print(f"[rollout] {e}", file=sys.stderr)
            return 2
    if "latent_scale" in opts or "path" in opts:
        print("[rollout] latent_scale / path go with replay_latents=<dir>", file=sys.stderr)
        return 2
    policy = ckpt.load_policy(step_dir, cfg)
    fn = ckpt.load_inference_fn(cfg, policy, deterministic=True, get_activation=True)
    env = create_environment(cfg, 1, "cuda")
    seed = int(opts.get("seed", 42))
    log_act, log_met = yes(opts.get("log_activations", "true")), yes(opts.get("log_metrics", "true"))
    log_sens = yes(opts.get("log_sensor_data", "false"))
    align = yes(opts.get("align_on_fail", "false"))
    log_dec_in = yes(opts.get("log_decoder_input", "false"))
    clips = _parse_clips(opts.get("clips", "all"), env._n_clips)

    def scale_opt(name):          # one float, or a comma list with one value per clip
        if name not in opts:
            return None
        v = [float(x) for x in str(opts[name]).split(",") if x.strip() != ""]
        if len(v) not in (1, len(clips)):
            raise ValueError(f"{name}: {len(v)} values for {len(clips)} clips (one value, or one per clip)")
        return v
    scale_lists = {k: scale_opt(k) for k in ("friction_scale", "actuator_scale", "damping_scale")}
    gravity_lists = {k: parse_per_clip(k, opts[k], len(clips)) for k in ("gravity_scale", "slope_deg") if k in opts}
    if intervention is not None:
        try:
            _, iv_dose = intervention.per_clip(len(clips))
        except ValueError as e:
            print(f"[rollout] intervene_{e}", file=sys.stderr)
            return 2
    gen = create_rollout_generator(cfg, env, fn, model=fn.model, log_activations=log_act, log_metrics=log_met, log_sensor_data=log_sens,
                                   align_on_fail=align, **{k: (None if v is None else 1.0) for k, v in scale_lists.items()},
                                   **{k: (1.0 if k == "gravity_scale" else 0.0) for k in gravity_lists}, intervention=intervention,
                                   log_decoder_input=log_dec_in)
    print(f"[rollout] done-policy: {gen.done_policy}" + (" (a done env is re-aligned to the clip frame it has reached; `aligned` / `n_alignments` "
                                                        "are recorded)" if align else " (the env keeps stepping after done)"), flush=True)
    out_dir = opts.get("out", os.path.join(step_dir, "rollouts"))
    os.makedirs(out_dir, exist_ok=True)
    meta_common = {"seed": np.int64(seed), "checkpoint_step": np.int64(int(os.path.basename(os.path.normpath(step_dir)))
                                                                        if os.path.basename(os.path.normpath(step_dir)).isdigit() else -1),
                   "checkpoint": str(step_dir), "model": fn.model, "trained_gemm_inputs": fn.trained_gemm_inputs,
                   "rollout_gemm_inputs": "f32"}
    if align:
        meta_common["done_policy"] = "align"
    if log_sens:
        table = env.walker.sensor_table()
        meta_common.update(sensor_names=",".join(t[0] for t in table), sensor_adr=np.array([t[1] for t in table], np.int64),
                           sensor_dim=np.array([t[2] for t in table], np.int64),
                           joint_forces_convention="cfrc_ext: per body [torque(3), force(3)] of the contact forces, world frame, about "
                                                   "subtree_com[body_rootid] (mj_rnePostConstraint); values of the control step's last substep")
    for i in range(0, len(clips), CLIPS_PER_BATCH):
        chunk = clips[i:i + CLIPS_PER_BATCH]
        sc = {k.split("_")[0]: (v[0] if len(v) == 1 else v[i:i + len(chunk)]) for k, v in scale_lists.items() if v is not None}
        gr = {k: (v[0] if len(v) == 1 else v[i:i + len(chunk)]) for k, v in gravity_lists.items()}
        try:
            res = gen(chunk, seed=seed, **({"scales": sc} if sc else {}), **({"gravity": gr} if gr else {}),
                      **({"gates": {"dose": iv_dose[i:i + len(chunk)]}} if intervention is not None else {}))
        except ValueError as e:      # an intervention the policy step refuses (a target it does not have, a width that does not match)
            if intervention is None:
                raise
            print(f"[rollout] {e}", file=sys.stderr)
            return 2
        for j, c in enumerate(chunk):
            one = _index_j(res, j)
            one["meta"] = dict(meta_common, clip_idx=np.int64(c))
            save_to_h5py(os.path.join(out_dir, f"clip_{c}.h5"), one)
    print(f"[rollout] wrote {len(clips)} clip files to {out_dir} (T={gen.T}, seed={seed}, model={fn.model})", flush=True)
    return 0


def _index_j(tree, j):
    if isinstance(tree, dict):
        return {k: _index_j(v, j) for k, v in tree.items()}
    if isinstance(tree, tuple):
        return tuple(_index_j(v, j) for v in tree)
    return tree[j]


if __name__ == "__main__":
    # (run as a script this file is `__main__`: use the package module, whose RolloutPolicy class load_inference_fn returns)
    from track_mjx_amd.analysis.rollout import main as _main
    sys.exit(_main())
