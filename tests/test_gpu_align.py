"""GPU: the align done-policy (AutoAlignWrapperTracking: include/tmjx.h tmjx_set_done_policy, csrc/wave_align.h, k_align_wave) and whole-clip
roll-outs under it (analysis/rollout.py: align_on_fail).  Expected values come from the oracle's existing primitives plus numpy
(tests/align_ref.py); the same bit-identity claims run without a GPU under the host emulation in tests/test_align_cpu.py.

Measured on an MI355X (test_aligned_observation_against_the_oracle, 320 envs, one step): aligned envs' observation relative error 4.8e-08
(80 envs) against 7.1e-05 for the 240 not-done envs of the same step (bound: twice the latter)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import align_ref as AR
from tests.common import default_walker, make_oracle, rel_err
from track_mjx_amd import clips as _clips
from track_mjx_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ENV, N_CLIPS, EPISODE = 320, 4, 3


def _env(cl, n=N_ENV, share=None):
    from track_mjx_amd.environment import MultiClipTracking, RewardConfig
    w, cfg = default_walker()
    return MultiClipTracking(cl, w, RewardConfig(**cfg["env_config"]["reward_weights"]), **cfg["env_config"]["env_args"], **cfg["reference_config"],
                             num_envs=n, device=DEV, share_clips_with=share), w, cfg


@pytest.fixture(scope="module")
def table():
    w, _ = default_walker()
    return _clips.make_synthetic_clips(w.model, N_CLIPS, seed=0)


def _reset_inputs(n, rng, far=False):
    qn = rng.uniform(-1e-3, 1e-3, (74, n)).astype(np.float32); vn = rng.uniform(-1e-3, 1e-3, (73, n)).astype(np.float32)
    if far:
        qn[0, 1::4] += 0.3
    return (np.arange(n) % N_CLIPS).astype(np.int32), ((7 * np.arange(n)) % 44).astype(np.int32), qn, vn


def _reset(env, ci, sf, qn, vn):
    env.reset(None, torch.from_numpy(ci), start_frame=torch.from_numpy(sf), qpos_noise=torch.from_numpy(qn), qvel_noise=torch.from_numpy(vn))


BUFS = ("state_buf", "istate_buf", "workspace", "obs_buf", "reward_buf", "done_buf", "trunc_buf", "metrics_buf")


@pytest.mark.parametrize("action_repeat", [1, 2])
def test_align_semantics_against_a_twin_under_policy_none(table, action_repeat):
    """Per step, against a second env stepped under policy "none" from the same state.  Not-done envs: obs, every state row, reward, metrics
    bit-identical.  Done envs: qpos / qvel rows bit-identical to the float32 clip arrays at the current frame — the frame of the time AFTER the
    last inner step, so with action_repeat = 2 this is one alignment per outer step, after the second inner step; every state row the alignment
    does not write (act, qacc_warmstart, time, qfrc_actuator, prev_ctrl, the action buffer, done, steps, the reset snapshot) and the int state
    equal to the twin's; steps zeroed on the following step.  reward, done, truncation, metrics equal for all envs.  The align env READS THE
    TWIN'S clip table (tmjx_clips_share), velocities included."""
    from track_mjx_amd.environment import AutoAlignWrapperTracking
    clips = table.as_dict()
    N, _, _ = _env(table)
    N.configure_wrappers(EPISODE * action_repeat, auto_reset=False, action_repeat=action_repeat)
    A, _, _ = _env(table, share=N)
    assert AutoAlignWrapperTracking(A, episode_length=EPISODE * action_repeat, action_repeat=action_repeat) is A and A._done_policy == "align"
    n, L = N_ENV, A.layout
    rng = np.random.default_rng(3)
    ci, sf, qn, vn = _reset_inputs(n, rng)
    _reset(A, ci, sf, qn, vn)
    written = np.zeros(L.state_rows, bool)
    for r0, cnt in ((L.qpos, L.nq), (L.qvel, L.nv), (L.xpos, 3 * L.nbody), (L.xmat_torso, 9)):
        written[r0:r0 + cnt] = True
    seen_term = seen_trunc = n_nan = 0
    n_aligned, prev_done = np.zeros(n, int), np.zeros(n, bool)
    for t in range(8):
        a = torch.from_numpy(AR.violent_actions(rng, 38, n)).to(DEV)
        for b in BUFS:
            getattr(N, b).copy_(getattr(A, b))
        A.step(None, a); N.step(None, a)
        torch.cuda.synchronize()
        g = {b: getattr(A, b).cpu().numpy() for b in BUFS}; h = {b: getattr(N, b).cpu().numpy() for b in BUFS}
        for b in ("reward_buf", "done_buf", "trunc_buf", "metrics_buf", "istate_buf"):
            assert np.array_equal(g[b], h[b], equal_nan=True), (t, b)
        done = h["done_buf"] != 0
        for b in ("state_buf", "obs_buf"):
            assert np.array_equal(g[b][:, ~done], h[b][:, ~done], equal_nan=True), (t, b)
        assert np.array_equal(g["state_buf"][~written][:, done], h["state_buf"][~written][:, done], equal_nan=True), t
        st = g["state_buf"]
        for e in np.nonzero(done)[0]:
            f = int(np.floor(np.float32(np.float32(st[L.time, e]) * np.float32(50)) + np.float32(sf[e])))
            assert np.array_equal(st[L.qpos:L.qpos + L.nq, e], AR.clip_qpos(clips, ci[e], f)), (t, e)
            assert np.array_equal(st[L.qvel:L.qvel + L.nv, e], AR.clip_qvel(clips, ci[e], f)), (t, e)
        # (an env that went NaN keeps its NaN act / qacc_warmstart / qfrc_actuator, as in the reference: only what the alignment writes is finite)
        assert np.isfinite(st[written][:, done]).all() and np.isfinite(g["obs_buf"][:, done]).all(), t
        assert np.all(st[L.steps_f, prev_done] == action_repeat), t
        nan_now = int((h["metrics_buf"][14] != 0).sum())
        assert nan_now <= 0.05 * n, (t, nan_now)
        n_nan += nan_now
        seen_term += int((done & (h["trunc_buf"] == 0)).sum()); seen_trunc += int((h["trunc_buf"] != 0).sum())
        n_aligned += done
        prev_done = done
    print(f"action_repeat {action_repeat}: {seen_term} terminations, {seen_trunc} truncations, {n_nan} NaN env-steps, most alignments of one env {n_aligned.max()}")
    assert seen_term > 0 and seen_trunc > 0 and n_aligned.max() >= 2


def test_aligned_observation_against_the_oracle(table):
    """The done envs of the first step that has any (every fourth env starts 0.3 m off its reference: too_far on step 0, far from the threshold):
    observation relative error against the expectation built from the oracle's primitives, no worse than twice the same quantity of the
    not-done envs of the same step (the existing path).  Both numbers are printed; DESIGN.md §7 records them."""
    from track_mjx_amd.environment import AutoAlignWrapperTracking
    clips = table.as_dict()
    A, w, cfg = _env(table)
    AutoAlignWrapperTracking(A, episode_length=EPISODE)
    n = N_ENV
    O = make_oracle(A._blob, table)
    envs, scratch = O.new_envs(n), O.new_envs(1)
    rng = np.random.default_rng(3)
    ci, sf, qn, vn = _reset_inputs(n, rng, far=True)
    _reset(A, ci, sf, qn, vn)
    for e in range(n):
        O.env_reset(envs, e, ci[e], sf[e], qn[:, e], vn[:, e])
    a = AR.violent_actions(rng, 38, n, scales=(0.1,))
    A.step(None, torch.from_numpy(a).to(DEV))
    torch.cuda.synchronize()
    for e in range(n):
        O.env_step(envs, e, a[:, e])
    done_o = np.array([O.env_get(envs, e, "done")[0] for e in range(n)]) != 0
    assert np.array_equal(done_o, A.done_buf.cpu().numpy() != 0) and np.array_equal(done_o, np.arange(n) % 4 == 1)
    cols = AR.actuator_force_columns(74, 73, len(w.joint_idxs), len(w.body_idxs), cfg["reference_config"]["traj_length"])
    exp = np.stack([AR.oracle_align(O, envs, e, clips, scratch, cols)[2] if done_o[e] else AR.nan_to_num32(O.env_get(envs, e, "obs")) for e in range(n)], 1)
    obs = A.obs_buf.cpu().numpy()
    err_aligned, err_kept = rel_err(obs[:, done_o], exp[:, done_o]), rel_err(obs[:, ~done_o], exp[:, ~done_o])
    print(f"aligned obs rel err {err_aligned:.3e} ({done_o.sum()} envs), not-done obs rel err {err_kept:.3e} ({(~done_o).sum()} envs)")
    assert err_aligned <= 2 * err_kept


def test_errors(table):
    from track_mjx_amd.environment import AutoAlignWrapperTracking
    bare = dataclasses.replace(table, velocity=None, joints_velocity=None)
    env, _, _ = _env(bare, n=8)
    with pytest.raises(hip.TmjxError, match="velocity"):
        AutoAlignWrapperTracking(env, episode_length=10)
    L = hip.lib()
    assert L.tmjx_set_done_policy(env._handle, 7) == -22 and b"unknown done policy 7" in L.tmjx_last_error()
    with pytest.raises(ValueError, match="done_policy"):
        env.configure_wrappers(10, False, done_policy="realign")
    # a handle that shares a table without velocities is refused too; one that has them takes the policy, and K3 as one kernel refuses it
    sharer, _, _ = _env(bare, n=8, share=env)
    with pytest.raises(hip.TmjxError, match="velocity"):
        AutoAlignWrapperTracking(sharer, episode_length=10)
    ok, _, _ = _env(table, n=8)
    AutoAlignWrapperTracking(ok, episode_length=10)
    ok.reset(0)
    p = lambda t: t.data_ptr()      # noqa: E731
    a = torch.zeros((38, 8), device=DEV)
    rc = L.tmjx_reward_obs(ok._handle, p(ok.state_buf), p(ok.istate_buf), p(a), p(ok.obs_buf), p(ok.reward_buf), p(ok.done_buf), p(ok.trunc_buf),
                           p(ok.metrics_buf), None, 8, None)
    assert rc == -22 and b"align" in L.tmjx_last_error()


# ---------------------------------------------------------------------------------------------------------------- roll-outs
def _cfg(overrides=()):
    from track_mjx_amd import config as _config
    return _config.load_config(None, ["n_synthetic_clips=6", *overrides])


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """A small MLP checkpoint with random weights, written here: its controls are wild enough that the walker fails within a clip."""
    from tests.common import StubEnv
    from track_mjx_amd.agent.checkpoint import save_step_dir
    from track_mjx_amd.agent.ppo import PPOLearner
    ln = PPOLearner(StubEnv(512), encoder_layers=[256, 256], decoder_layers=[256, 256], critic_layers=[64, 64], latents=60, unroll_length=4,
                    batch_size=256, num_minibatches=8, num_updates_per_batch=1, use_graph=False, seed=3)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for prm in ln.policy.parameters():
            prm.add_((torch.randn(prm.shape, generator=g) * 0.05).to(prm.device))
    d = tmp_path_factory.mktemp("align_ckpt")
    save_step_dir(d, 0, ln, config=_cfg())
    return str(d)


def _frames_after_steps(cfg, T):
    """The clip frame an env that started at frame 0 has reached after control step t = 0 .. T - 2 — floor(time * mocap_hz) in float32, time
    being the float32 sum of the substeps' timesteps (single_clip_tracking.py:452-454): it is t + 1 or, where the product rounds just below
    the integer, t.  (One control step per frame in this configuration.)"""
    ea = cfg["env_config"]["env_args"]
    dt, nsub, hz = np.float32(ea["mj_model_timestep"]), int(ea["physics_steps_per_control_step"]), np.float32(ea["mocap_hz"])
    assert round(1.0 / (float(hz) * float(dt))) == nsub
    time, out = np.float32(0), []
    for _ in range(T - 1):
        for _ in range(nsub):
            time = np.float32(time + dt)
        out.append(int(np.floor(np.float32(time * hz))))
    return np.array(out)


def test_rollout_align_on_fail(ckpt, tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import create_environment, create_rollout_generator
    from track_mjx_amd.analysis.utils import load_from_h5py
    cfg = ck.load_config_from_checkpoint(ckpt)
    fn = ck.load_inference_fn(cfg, ck.load_policy(ckpt, cfg))
    plain = create_rollout_generator(cfg, create_environment(cfg, 1, DEV), fn, model=fn.model, log_metrics=True)
    gen = create_rollout_generator(cfg, create_environment(cfg, 1, DEV), fn, model=fn.model, log_metrics=True, align_on_fail=True)
    assert gen.done_policy == "align" and plain.done_policy == "none"
    clips = [0, 3, 5]
    r, r0 = gen(clips), plain(clips)
    T = gen.T
    assert set(r) == set(r0) | {"aligned", "n_alignments"} and "aligned" not in r0 and "n_alignments" not in r0
    assert r["aligned"].shape == (3, T - 1) and r["aligned"].dtype == np.bool_ and r["qposes_rollout"].shape[:2] == (3, T)      # one record per clip, to the clip's end
    assert np.array_equal(r["aligned"].sum(1), r["n_alignments"]) and r["n_alignments"].sum() > 0
    print("alignments per clip:", r["n_alignments"].tolist())
    assert np.isfinite(r["qposes_rollout"]).all()
    frames = _frames_after_steps(cfg, T)
    assert np.abs(frames - np.arange(1, T)).max() <= 1 and (frames != np.arange(1, T)).any()       # float32 floor: frame t + 1 or the one before
    for j in range(3):
        for t in np.nonzero(r["aligned"][j])[0]:
            assert np.array_equal(r["qposes_rollout"][j, t + 1], r["qposes_ref"][j, frames[t]]), (j, t)
    # up to the first alignment of a clip the two roll-outs are the same bits
    for j in range(3):
        first = int(np.argmax(r["aligned"][j])) if r["aligned"][j].any() else T - 1
        assert np.array_equal(r["qposes_rollout"][j, :first + 1], r0["qposes_rollout"][j, :first + 1], equal_nan=True)
    # CLI: files with and without the flag
    env_ = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.environ.get("PYTHONPATH", "")]))
    names = {}
    for flag in ("true", "false"):
        out = tmp_path / flag
        res = subprocess.run([sys.executable, "-m", "track_mjx_amd.analysis.rollout", f"checkpoint={ckpt}", "clips=3", f"out={out}", "log_activations=false",
                              f"align_on_fail={flag}"], capture_output=True, text=True, env=env_, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        assert f"[rollout] done-policy: {'align' if flag == 'true' else 'none'}" in res.stdout.splitlines()[0]
        names[flag] = load_from_h5py(out / "clip_3.h5")
    assert set(names["true"]) == set(names["false"]) | {"aligned", "n_alignments"}
    assert set(names["false"]) == {"qposes_ref", "qposes_rollout", "ctrl", "state_rewards", "rollout_metrics", "meta"}
    assert int(names["true"]["n_alignments"]) == int(r["n_alignments"][1]) and np.array_equal(names["true"]["aligned"] != 0, r["aligned"][1])
    assert np.array_equal(names["false"]["qposes_rollout"], r0["qposes_rollout"][1], equal_nan=True)


def test_rollout_align_on_fail_lstm(tmp_path_factory):
    """The LSTM policy under align_on_fail: runs to the clip's end, and its carry is zeroed where an alignment happened — the recorded (h, c) of the
    step after an aligned one are those of a step from a zero carry, i.e. what the same policy returns for that step's inputs from hidden_state=0."""
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.agent.checkpoint import save_step_dir
    from track_mjx_amd.agent.lstm import LSTMPPOLearner
    from track_mjx_amd.analysis.rollout import create_environment, create_rollout_generator
    cfg = _cfg(["train_setup.train_config.use_lstm=true"])
    env = create_environment(cfg, 64, DEV)
    ln = LSTMPPOLearner(env, encoder_layers=(256, 256), decoder_layers=(256, 256), critic_layers=(64, 64), latents=60, unroll_length=4, batch_size=64,
                        num_minibatches=4, num_updates_per_batch=1, seed=0, hidden_state_size=128, hidden_layer_num=2)
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for prm in ln.policy.parameters():
            prm.add_((torch.randn(prm.shape, generator=g) * 0.05).to(prm.device))
    d = tmp_path_factory.mktemp("align_lstm_ckpt")
    save_step_dir(d, 0, ln, config=cfg)
    cfg = ck.load_config_from_checkpoint(str(d))
    fn = ck.load_inference_fn(cfg, ck.load_policy(str(d), cfg))
    gen = create_rollout_generator(cfg, create_environment(cfg, 1, DEV), fn, model="lstm", log_activations=True, align_on_fail=True)
    r = gen([1, 4])
    assert np.array_equal(r["aligned"].sum(1), r["n_alignments"]) and r["n_alignments"].sum() > 0 and np.isfinite(r["qposes_rollout"]).all()
    h, c = r["activations"]["hidden_state"]
    frames = _frames_after_steps(cfg, gen.T)
    # |c| of a step from a zero carry is bounded by the input gate alone: |c_t| = |i * g| < 1 in every unit; carried on, |c| grows past that
    for j in range(2):
        for t in np.nonzero(r["aligned"][j][:-1])[0]:
            assert np.abs(c[j, t + 1]).max() < 1.0, (j, t)
            assert np.array_equal(r["qposes_rollout"][j, t + 1], r["qposes_ref"][j, frames[t]])
