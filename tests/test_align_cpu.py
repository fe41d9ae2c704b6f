"""CPU: the align done-policy (AutoAlignWrapperTracking; include/tmjx.h: tmjx_set_done_policy, csrc/wave_align.h) without a GPU — the Python
wrappers' argument checking, the clip-velocity packing, the roll-out CLI, the C-ABI's refusals that need no device, and the kernel source itself
under the TEST-ONLY host emulation (tests/hostemu/align_emu.cpp) with TMJX_EMU_POISON=nan: the same bit-identity claims tests/test_gpu_align.py
makes on the GPU, with every LDS word and lane register of the align wave starting from NaN."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent / "hostemu"))
from emu import Emu  # noqa: E402
from align_emu import DONE_ALIGN, DONE_NONE, AlignEmu  # noqa: E402

from tests import align_ref as AR  # noqa: E402
from tests.common import default_blob, default_walker, make_oracle, rel_err  # noqa: E402
from track_mjx_amd import clips as _clips  # noqa: E402
from track_mjx_amd import hip  # noqa: E402

EPISODE = 3


@pytest.fixture(scope="module")
def setup():
    w, cfg = default_walker()
    blob = default_blob(w, cfg, episode_length=EPISODE, auto_reset=False)
    clip = _clips.make_synthetic_clips(w.model, 4, seed=0)
    return w, cfg, blob, clip.as_dict()


def _reset(E, n, rng, far=False):
    qn = rng.uniform(-1e-3, 1e-3, (74, n)).astype(np.float32); vn = rng.uniform(-1e-3, 1e-3, (73, n)).astype(np.float32)
    if far:
        qn[0, 1::4] += 0.3
    ci, sf = (np.arange(n) % 4).astype(np.int32), ((7 * np.arange(n)) % 44).astype(np.int32)
    E.reset(ci, sf, qn, vn)
    return ci, sf, qn, vn


def _copy(dst, src):
    for k in ("st", "ist", "ws", "obs", "reward", "done", "trunc", "metrics"):
        getattr(dst, k)[...] = getattr(src, k)


@pytest.mark.parametrize("action_repeat", [1, 2])
def test_emulated_align_step_bit_identity_under_nan_poison(setup, monkeypatch, action_repeat):
    """Per step, against a twin stepped under policy "none" from the same state: not-done envs bit-identical everywhere; done envs on the clip's
    float32 qpos / qvel rows exactly, everything a step does not restore equal to the twin's; steps zeroed by the next prologue; with
    action_repeat = 2 one alignment per outer step, after the second inner step."""
    monkeypatch.setenv("TMJX_EMU_POISON", "nan")
    w, cfg, blob, clips = setup
    n, steps = 24, 8
    E, N = Emu(blob, n), Emu(blob, n)
    E.set_clips(clips)
    A = AlignEmu(blob, clips); A.set_policy(EPISODE * action_repeat, DONE_ALIGN)
    B = AlignEmu(blob, clips); B.set_policy(EPISODE * action_repeat, DONE_NONE)
    rng = np.random.default_rng(3)
    ci, sf, _, _ = _reset(E, n, rng)
    untouched = np.ones(E.s_rows, bool)
    for name in ("qpos", "qvel", "xpos", "xmat_torso"):
        r0 = (E.rows(name).ctypes.data - E.st.ctypes.data) // (4 * n)
        untouched[r0:r0 + E.rows(name).shape[0]] = False
    seen_term = seen_trunc = 0
    n_aligned = np.zeros(n, int)
    prev_done = np.zeros(n, bool)
    for t in range(steps):
        a = AR.violent_actions(rng, 38, n)
        _copy(N, E)
        k = A.step(E, a, action_repeat)
        assert B.step(N, a, action_repeat) == 0
        done = N.done != 0
        assert k == done.sum()
        for name in ("reward", "done", "trunc", "metrics"):
            assert np.array_equal(getattr(E, name), getattr(N, name), equal_nan=True), (t, name)
        keep = ~done
        assert np.array_equal(E.st[:, keep], N.st[:, keep], equal_nan=True) and np.array_equal(E.obs[:, keep], N.obs[:, keep], equal_nan=True), t
        assert np.array_equal(E.ist, N.ist)
        time_row = E.rows("time")[0]
        for e in np.nonzero(done)[0]:
            f = int(np.floor(np.float32(np.float32(time_row[e]) * np.float32(50)) + np.float32(sf[e])))
            assert np.array_equal(E.rows("qpos")[:, e], AR.clip_qpos(clips, ci[e], f)), (t, e)
            assert np.array_equal(E.rows("qvel")[:, e], AR.clip_qvel(clips, ci[e], f)), (t, e)
            for name in ("act", "qacc_warmstart", "time", "qfrc_actuator", "steps"):
                assert np.array_equal(E.rows(name)[:, e], N.rows(name)[:, e], equal_nan=True), (t, e, name)
            # ... and every other state row but the four the alignment writes (prev_ctrl, the action buffer, done, the reset snapshot)
            assert np.array_equal(E.st[untouched, e], N.st[untouched, e], equal_nan=True), (t, e)
            assert np.isfinite(E.obs[:, e]).all() and np.isfinite(E.rows("xpos")[:, e]).all(), (t, e)      # nothing of the poison got through
            assert not np.array_equal(E.obs[:, e], N.obs[:, e])
        # the step counter of an env aligned on the previous step was zeroed by this step's prologue: it now holds this step's repeats only
        assert np.all(E.rows("steps")[0, prev_done] == action_repeat), t
        seen_term += int(((N.done != 0) & (N.trunc == 0)).sum()); seen_trunc += int((N.trunc != 0).sum())
        n_aligned += done
        prev_done = done
    assert seen_term > 0 and seen_trunc > 0 and n_aligned.max() >= 2, (seen_term, seen_trunc, n_aligned)


def test_emulated_aligned_observation_against_the_oracle(setup, monkeypatch):
    """The aligned envs' observation of the first step that has any, against the expectation built from the oracle (tests/align_ref.py): no
    worse than twice the not-done envs' error of the same step against the oracle (the existing path)."""
    monkeypatch.setenv("TMJX_EMU_POISON", "nan")
    w, cfg, blob, clips = setup
    n = 24
    E = Emu(blob, n)
    E.set_clips(clips)
    A = AlignEmu(blob, clips); A.set_policy(EPISODE, DONE_ALIGN)
    O = make_oracle(blob, None); O.set_clips(clips)
    envs, scratch = O.new_envs(n), O.new_envs(1)
    rng = np.random.default_rng(3)
    ci, sf, qn, vn = _reset(E, n, rng, far=True)
    for e in range(n):
        O.env_reset(envs, e, ci[e], sf[e], qn[:, e], vn[:, e])
    cols = AR.actuator_force_columns(74, 73, len(w.joint_idxs), len(w.body_idxs), cfg["reference_config"]["traj_length"])
    # one step from a common state: every fourth env starts 0.3 m off its reference (too_far, far from the threshold, so the oracle and the
    # kernel agree on who is done), the actions are moderate
    a = AR.violent_actions(rng, 38, n, scales=(0.1,))
    A.step(E, a)
    for e in range(n):
        O.env_step(envs, e, a[:, e])
    done_o = np.array([O.env_get(envs, e, "done")[0] for e in range(n)]) != 0
    assert np.array_equal(done_o, E.done != 0) and np.array_equal(done_o, np.arange(n) % 4 == 1)
    assert done_o.any() and not done_o.all()
    exp = np.stack([AR.oracle_align(O, envs, e, clips, scratch, cols)[2] if done_o[e] else AR.nan_to_num32(O.env_get(envs, e, "obs")) for e in range(n)], 1)
    err_aligned, err_kept = rel_err(E.obs[:, done_o], exp[:, done_o]), rel_err(E.obs[:, ~done_o], exp[:, ~done_o])
    print(f"aligned obs rel err {err_aligned:.3e} ({done_o.sum()} envs), not-done obs rel err {err_kept:.3e} ({(~done_o).sum()} envs)")
    assert err_aligned <= 2 * err_kept


def test_emulation_refuses_align_without_velocities_and_unknown_policies(setup):
    w, cfg, blob, clips = setup
    with pytest.raises(ValueError, match="velocities"):
        AlignEmu(blob, clips, velocities=False).set_policy(EPISODE, DONE_ALIGN)
    with pytest.raises(ValueError, match="unknown done policy"):
        AlignEmu(blob, clips).set_policy(EPISODE, 7)


def test_c_abi_refusals_without_gpu():
    L = hip.lib()
    assert {"tmjx_set_done_policy", "tmjx_clips_upload_velocities"} <= set(hip.EXPORTS)
    assert L.tmjx_set_done_policy(None, 7) == -22 and b"unknown done policy 7" in L.tmjx_last_error()
    assert L.tmjx_set_done_policy(None, hip.DONE_ALIGN) == -22 and b"null argument" in L.tmjx_last_error()
    assert L.tmjx_clips_upload_velocities(None, None, None, 1, 1) == -22
    assert (hip.DONE_NONE, hip.DONE_RESET, hip.DONE_ALIGN) == (0, 1, 2)
    header = (Path(__file__).parents[1] / "include" / "tmjx.h").read_text()
    for k, v in (("TMJX_DONE_NONE", 0), ("TMJX_DONE_RESET", 1), ("TMJX_DONE_ALIGN", 2)):
        assert f"#define {k} {v}" in header


def test_clip_velocity_packing(setup):
    """qpos = position | quaternion | joints, qvel = velocity | angular_velocity | joints_velocity of ONE frame, frame index clamped."""
    w, cfg, blob, clips = setup
    q, v = AR.clip_qpos(clips, 2, 17), AR.clip_qvel(clips, 2, 17)
    assert q.shape == (74,) and v.shape == (73,) and q.dtype == v.dtype == np.float32
    assert np.array_equal(q[3:7], clips["quaternion"][2, 17]) and np.array_equal(v[:3], clips["velocity"][2, 17])
    assert np.array_equal(v[3:6], clips["angular_velocity"][2, 17]) and np.array_equal(v[6:], clips["joints_velocity"][2, 17])
    last = clips["position"].shape[1] - 1
    assert np.array_equal(AR.clip_qpos(clips, 1, last + 40), AR.clip_qpos(clips, 1, last))


class _Recorder:
    """Stands in for MultiClipTracking.configure_wrappers (which talks to the device)."""
    def __init__(self):
        self.calls = []

    def __call__(self, env, *a, **kw):
        self.calls.append((a, kw))


def test_wrapper_construction_and_argument_checking(monkeypatch):
    from track_mjx_amd.environment import AutoAlignWrapperTracking, EvalClipWrapperTracking, MultiClipTracking
    from track_mjx_amd.environment.task import DONE_POLICIES
    assert DONE_POLICIES == {"none": 0, "reset": 1, "align": 2}
    rec = _Recorder()
    monkeypatch.setattr(MultiClipTracking, "configure_wrappers", lambda self, *a, **kw: rec(self, *a, **kw))
    env = object.__new__(MultiClipTracking)
    env._handle = None
    assert AutoAlignWrapperTracking(env, episode_length=150, action_repeat=2) is env
    assert rec.calls == [((150,), dict(auto_reset=False, action_repeat=2, done_policy="align"))]
    with pytest.raises(TypeError):
        AutoAlignWrapperTracking(object())
    with pytest.raises(ValueError):
        AutoAlignWrapperTracking(env, episode_length=0)
    with pytest.raises(ValueError):
        AutoAlignWrapperTracking(env, action_repeat=0)
    monkeypatch.undo()
    # configure_wrappers itself: the policy is checked before anything touches the device
    with pytest.raises(ValueError, match="done_policy"):
        MultiClipTracking.configure_wrappers(env, 100, False, done_policy="realign")
    with pytest.raises(ValueError, match="contradicts"):
        MultiClipTracking.configure_wrappers(env, 100, True, done_policy="align")
    # EvalClipWrapperTracking: frame 0 of the given clip, zero qvel noise, the qpos noise left to the env's own draw
    class Stub:
        num_envs, _n_clips = 3, 4
        class layout:
            nv = 73
        def reset(self, rng, clip_idx, **kw):
            self.got = (rng, clip_idx, kw)
            return "state"
    stub = Stub()
    ev = EvalClipWrapperTracking(stub)
    assert ev.reset(5, clip_idx=2) == "state" and ev.num_envs == 3
    rng, ci, kw = stub.got
    assert rng == 5 and ci.tolist() == [2, 2, 2] and kw["start_frame"].tolist() == [0, 0, 0]
    assert kw["qvel_noise"].shape == (73, 3) and not kw["qvel_noise"].any() and "qpos_noise" not in kw
    with pytest.raises(ValueError):
        ev.reset(5)
    with pytest.raises(IndexError):
        ev.reset(5, clip_idx=4)


def test_cli_parsing_and_generator_refusal():
    from track_mjx_amd import config as _config
    from track_mjx_amd.analysis import rollout as R
    opts, rest = R._split_argv(["checkpoint=/x", "align_on_fail=true", "env_config.env_args.mocap_hz=50", "clips=0:2"])
    assert opts == {"checkpoint": "/x", "align_on_fail": "true", "clips": "0:2"} and rest == ["env_config.env_args.mocap_hz=50"]
    assert "align_on_fail" in R.CLI_OPTIONS and R.main([]) == 2
    import inspect
    assert inspect.signature(R.create_rollout_generator).parameters["align_on_fail"].default is False
    cfg = _config.load_config(None, [])
    with pytest.raises(TypeError, match="load_inference_fn"):
        R.create_rollout_generator(cfg, None, lambda obs, key: obs, align_on_fail=True)
