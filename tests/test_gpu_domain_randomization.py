"""GPU: per-env domain randomisation — k_physics_wave_rand (csrc/tmjx_wave_rand.hip) behind tmjx_set_env_scales, and the Python surface on top
of it (MultiClipTracking.set_domain_randomization, wrap / ppo.train randomization_fn, the roll-out's perturbation scales).

The expectation for an env with the scale triple (friction, actuator, damping) is a handle — the oracle's, or this library's plain kernel —
created from the model blob with con_friction[:, 0], act_gain (and the affine bias pair) and dof_damping scaled on the host
(tests/domain_rand_ref.py).  The same kernel source runs under the host emulation in tests/test_domain_randomization_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.common import default_walker, make_oracle, rel_err
from tests.domain_rand_ref import TRIPLES_G1, scaled_blob, scales_table
from track_mjx_amd import clips as _clips
from track_mjx_amd import hip
from track_mjx_amd.environment import DomainRandomization, uniform_randomization_fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PHYS = ("qpos", "qvel", "act", "qacc_warmstart", "time")
BUFS = ("state_buf", "istate_buf", "obs_buf", "reward_buf", "done_buf", "trunc_buf", "metrics_buf")


def _table(config="rodent-full-clips", n_clips=4):
    w, cfg = default_walker(config)
    return _clips.make_synthetic_clips(w.model, n_clips, seed=0), w, cfg


class _PrescaledWalker:
    """A walker whose blob entries were scaled on the host: what MultiClipTracking builds its handle from (walker.build_blob reads
    `walker.model`), everything else the wrapped walker's."""

    def __init__(self, w, triple):
        from track_mjx_amd import blob as _blob
        self._w = w
        self.model = _blob.unpack(scaled_blob(_blob.pack(w.model), *triple))

    def __getattr__(self, name):
        return getattr(self._w, name)


def _env(cl, w, cfg, n, triple=None, share=None):
    from track_mjx_amd.environment import MultiClipTracking, RewardConfig
    return MultiClipTracking(cl, w if triple is None else _PrescaledWalker(w, triple), RewardConfig(**cfg["env_config"]["reward_weights"]),
                             **cfg["env_config"]["env_args"], **cfg["reference_config"], num_envs=n, device=DEV, share_clips_with=share)


def _dr(table):
    return DomainRandomization(table[0], table[1], table[2])


def _reset(env, seed=0):
    n = env.num_envs
    g = torch.Generator().manual_seed(seed)
    clip = torch.randint(0, 4, (n,), generator=g, dtype=torch.int32); start = torch.randint(0, 44, (n,), generator=g, dtype=torch.int32)
    qn = (torch.rand((74, n), generator=g) * 2 - 1) * 1e-3; vn = (torch.rand((73, n), generator=g) * 2 - 1) * 1e-3
    env.reset(None, clip, start_frame=start, qpos_noise=qn, qvel_noise=vn)
    return clip, start, qn, vn


def _snap(env):
    torch.cuda.synchronize()
    return {b: getattr(env, b).cpu().numpy().copy() for b in BUFS}


def _same(a, b, cols=slice(None), what=""):
    for k in BUFS:
        x, y = (a[k][..., cols], b[k][..., cols])
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), (what, k)


def initial_states(cl, n, rng, sink=0.001):
    """test_substep_teacher_forced's initial states (tests/test_gpu_parity.py: _init_states)."""
    qpos = np.zeros((n, 74)); qvel = rng.uniform(-1e-3, 1e-3, size=(n, 73))
    for e in range(n):
        c, f = e % cl.position.shape[0], (7 * e) % 44
        qpos[e] = np.concatenate([cl.position[c, f], cl.quaternion[c, f], cl.joints[c, f]]) + rng.uniform(-1e-3, 1e-3, 74)
        qpos[e, 2] -= sink * (e % 5)
    return qpos, qvel


def run_teacher_forced(blob, cl, physics, n=64, warmup=0, substeps=40, seed=1):
    """test_substep_teacher_forced's protocol and states with one oracle pair per scale triple.  That test's trajectory (40 substeps from the clip
    poses, actions N(0, 0.03)) reaches the floor near its end; the float64 oracles run its first `warmup` substeps on their own, and the
    comparison covers the rest — the part where the paws are on the floor and sliding, the activations have built up and the joints move, so
    that friction, actuator strength and damping all act.  Every compared substep starts all parties from the float64 oracles' state;
    `physics(state rows dict, action [nu][n] float32) -> {"qpos", "qvel"} [rows][n]` is the implementation under test with
    scales_table(TRIPLES_G1, n // 4).  Asserts that test's bounds for every group, over the group's n // 4 x `substeps` env-substeps (16 envs
    are too few for a per-substep 0.9-quantile: the plain kernel on a pre-scaled model misses that by chance), and the sensitivity condition
    spelled out below."""
    per = n // len(TRIPLES_G1)
    O32 = [make_oracle(scaled_blob(blob, *t), cl, "f32") for t in TRIPLES_G1]
    O64 = [make_oracle(scaled_blob(blob, *t), cl, "f64") for t in TRIPLES_G1]
    plain = O64[0]
    assert TRIPLES_G1[0] == (1.0, 1.0, 1.0)
    rng = np.random.default_rng(seed)
    qpos, qvel = initial_states(cl, n, rng)
    grp = lambda e: e // per          # noqa: E731
    d32 = [O32[grp(e)].new_data(qpos[e], qvel[e]) for e in range(n)]
    d64 = [O64[grp(e)].new_data(qpos[e], qvel[e]) for e in range(n)]
    dpl = [plain.new_data(qpos[e], qvel[e]) for e in range(n)]
    for _ in range(warmup):
        a = np.clip(rng.normal(size=(n, 38)) * 0.03, -1, 1)
        for e in range(n):
            O64[grp(e)].step(d64[e], a[e])
    ncon = 0
    pooled = {(g, k): ([], []) for g in range(len(TRIPLES_G1)) for k in ("qpos", "qvel")}
    moved, parity = {}, {}
    for sub in range(substeps):
        a = np.clip(rng.normal(size=(n, 38)) * 0.03, -1, 1)
        st = {k: np.stack([O64[grp(e)].get(d64[e], k) for e in range(n)], 1) for k in PHYS}
        for e in range(n):
            for k, v in st.items():
                O32[grp(e)].set(d32[e], k, v[:, e]); plain.set(dpl[e], k, v[:, e])
        got = physics(st, a.T.astype(np.float32).copy())
        for e in range(n):
            O32[grp(e)].step(d32[e], a[e]); O64[grp(e)].step(d64[e], a[e]); plain.step(dpl[e], a[e])
        ref = {k: np.stack([O64[grp(e)].get(d64[e], k) for e in range(n)], 1) for k in ("qpos", "qvel")}
        r32 = {k: np.stack([O32[grp(e)].get(d32[e], k) for e in range(n)], 1) for k in ("qpos", "qvel")}
        unscaled = np.stack([plain.get(dpl[e], "qvel") for e in range(n)], 1)
        ncon += sum((O64[grp(e)].get(d64[e], "con_dist") < 0).sum() for e in range(n))
        for g, t in enumerate(TRIPLES_G1):
            sl = slice(g * per, (g + 1) * per)
            for k in ("qpos", "qvel"):
                pooled[g, k][0].append(rel_err(got[k][:, sl], ref[k][:, sl], axis=0)); pooled[g, k][1].append(rel_err(r32[k][:, sl], ref[k][:, sl], axis=0))
            if sum(s != 1.0 for s in t) == 1:
                moved.setdefault(g, []).append(rel_err(got["qvel"][:, sl], unscaled[:, sl], axis=0))
                parity.setdefault(g, []).append(rel_err(ref["qvel"][:, sl], unscaled[:, sl], axis=0))      # (the ORACLE's own sensitivity)
    assert ncon > 0, "the states must be in contact"
    for (g, k), (eg, e32) in pooled.items():
        eg, e32 = np.concatenate(eg), np.concatenate(e32)
        print(f"group {TRIPLES_G1[g]} {k}: {len(eg)} env-substeps, median {np.median(eg):.2e}, q90 {np.quantile(eg, 0.9):.2e}; float32 oracle median "
              f"{np.median(e32):.2e}, q90 {np.quantile(e32, 0.9):.2e}")
    for (g, k), (eg, e32) in pooled.items():
        eg, e32 = np.concatenate(eg), np.concatenate(e32)
        assert np.median(eg) <= 1e-5, (TRIPLES_G1[g], k, np.median(eg))
        assert np.quantile(eg, 0.9) <= 2 * np.quantile(e32, 0.9) + 1e-5, (TRIPLES_G1[g], k, np.quantile(eg, 0.9), np.quantile(e32, 0.9))
    # sensitivity, for the groups with ONE scale off 1.  P = the group's parity error on qvel (the 0.9-quantile the bound above is about), P32 the
    # float32 oracle's.  The env-substeps on which the float64 oracle ITSELF is sensitive to the scale — its scaled and unscaled results more than
    # 100 P32 apart, far outside its own arithmetic: paws sliding on the floor for friction, activations built up for the actuators — must be
    # plenty (the states are chosen for that), and on at least 9 of 10 of them the result must be further than 10 P from the unscaled oracle's.
    # A kernel that ignores the scale computes the unscaled result: 0 of 10.
    for g in moved:
        mv, osens = np.concatenate(moved[g]), np.concatenate(parity[g])
        P, P32 = np.quantile(np.concatenate(pooled[g, "qvel"][0]), 0.9), np.quantile(np.concatenate(pooled[g, "qvel"][1]), 0.9)
        S = osens > 100 * P32
        frac = float((mv[S] > 10 * P).mean()) if S.any() else 0.0
        print(f"group {TRIPLES_G1[g]}: oracle sensitive on {S.sum()} of {len(S)} env-substeps (median {np.median(osens[S]) if S.any() else 0:.2e}); "
              f"result > 10 x parity error ({P:.2e}) from the unscaled oracle on {100 * frac:.1f} % of them")
        assert S.sum() >= len(S) // 4, (TRIPLES_G1[g], int(S.sum()))
        assert frac >= 0.9, (TRIPLES_G1[g], frac)
    return pooled


# ------------------------------------------------------------------------------------------------ G1
@pytest.mark.parametrize("config", ["rodent-full-clips", "rodent-sps-per-actor"])
def test_parity_against_the_oracle_per_scale_triple(config):
    """64 envs, 16 for each of (1, 1, 1), (0.6, 1, 1), (1, 0.7, 1), (1.3, 1.2, 1.8), one substep at a time from the float64 oracles' states: per
    group median relative error <= 1e-5 on qpos and qvel, 0.9-quantile <= 2 x the float32 oracle's own + 1e-5 (test_substep_teacher_forced's
    bounds and trajectory: run_teacher_forced), and the single-scale groups further than 10 x their parity error from the unscaled oracle: a
    kernel that ignores a scale fails."""
    cl, w, cfg = _table(config)
    n = 64
    env = _env(cl, w, cfg, n)
    table = scales_table(TRIPLES_G1, n // 4)
    env.set_domain_randomization(_dr(table))
    assert np.array_equal(env.domain_randomization.table(), table)

    def physics(st, a):
        for k, v in st.items():
            env.rows(k).copy_(torch.from_numpy(v.astype(np.float32)))
        env.physics(torch.from_numpy(a).to(DEV), 1)
        torch.cuda.synchronize()
        return {k: env.rows(k).cpu().numpy() for k in ("qpos", "qvel")}
    run_teacher_forced(env._blob, cl, physics, n=n)


# ------------------------------------------------------------------------------------------------ G2
def test_unit_scales_are_the_plain_kernel_bit_for_bit():
    """256 envs, 3 control steps: a handle with all scales 1 gives state, obs, reward, done and metrics bit-identical to the same handle without
    scales (scaled constants x 1 are the constants; the contact weight re-formed from mu is the host's expression, operation by operation)."""
    cl, w, cfg = _table()
    n = 256
    A = _env(cl, w, cfg, n); B = _env(cl, w, cfg, n, share=A)
    for e in (A, B):
        e.configure_wrappers(195, auto_reset=True)
    B.set_domain_randomization(DomainRandomization(num_envs=n))
    _reset(A); _reset(B)
    _same(_snap(A), _snap(B), what="reset")
    g = torch.Generator().manual_seed(4)
    for t in range(3):
        a = (torch.randn((38, n), generator=g) * 0.3).clamp(-1, 1).to(DEV)
        A.step(None, a); B.step(None, a)
        sa, sb = _snap(A), _snap(B)
        assert np.isfinite(sa["obs_buf"]).all()
        _same(sa, sb, what=f"step {t}")


# ------------------------------------------------------------------------------------------------ G3
def test_power_of_two_scales_equal_prescaled_handles():
    """128 envs with triples from {0.5, 1, 2}^3 (all 27, cycled): after 2 control steps every env is bit-identical to the plain kernel on a
    handle whose blob was scaled by that env's triple — "scale the constant first" and the per-env indexing."""
    cl, w, cfg = _table()
    n = 128
    triples = [(f, a, d) for f in (0.5, 1.0, 2.0) for a in (0.5, 1.0, 2.0) for d in (0.5, 1.0, 2.0)]
    idx = (np.arange(n) * 5) % 27                   # (5 and 27 coprime: every triple, no period that lines up with the launch)
    table = np.ascontiguousarray(np.asarray(triples, np.float32)[idx].T)
    R = _env(cl, w, cfg, n)
    R.configure_wrappers(195, auto_reset=True)
    R.set_domain_randomization(_dr(table))
    inputs = _reset(R, seed=2)
    g = torch.Generator().manual_seed(5)
    acts = [(torch.randn((38, n), generator=g) * 0.3).clamp(-1, 1).to(DEV) for _ in range(2)]
    for a in acts:
        R.step(None, a)
    got = _snap(R)
    plain = None
    for k, t in enumerate(triples):
        P = _env(cl, w, cfg, n, triple=t, share=R)
        P.configure_wrappers(195, auto_reset=True)
        P.reset(None, inputs[0], start_frame=inputs[1], qpos_noise=inputs[2], qvel_noise=inputs[3])
        for a in acts:
            P.step(None, a)
        want = _snap(P)
        cols = np.nonzero(idx == k)[0]
        assert len(cols) >= 4
        _same(got, want, cols=cols, what=t)
        if t == (1.0, 1.0, 1.0):
            plain = want
    # every env whose actuator or damping scale is off 1 differs from the unscaled handle (a friction scale alone acts only once a paw is down)
    L = R.layout
    qv = slice(L.qvel, L.qvel + L.nv)
    for e in range(n):
        if triples[idx[e]][1:] != (1.0, 1.0):
            assert not np.array_equal(got["state_buf"][qv, e], plain["state_buf"][qv, e]), (e, triples[idx[e]])


# ------------------------------------------------------------------------------------------------ G4
def test_env_groups_take_their_slice_of_the_scales():
    """The pipelined roll-out's three-group split (48, 44, 36: test_pipelined_rollout_env_groups) with a different scale in every env: each
    group's handle with its slice of the table is bit-identical to the single launch of all 128 envs — in one launch the global env id indexes
    the table (TMJX_SPLIT_LAUNCH would pass e0), across groups the slices do."""
    cl, w, cfg = _table()
    sizes, n = (48, 44, 36), 128
    rng = np.random.default_rng(6)
    table = rng.uniform(0.5, 1.5, size=(3, n)).astype(np.float32)
    full = _env(cl, w, cfg, n)
    full.configure_wrappers(195, auto_reset=True)
    full.set_domain_randomization(_dr(table))
    inputs = _reset(full, seed=3)
    g = torch.Generator().manual_seed(6)
    acts = [(torch.randn((38, n), generator=g) * 0.3).clamp(-1, 1) for _ in range(2)]
    for a in acts:
        full.step(None, a.to(DEV))
    want = _snap(full)
    lo = 0
    for sz in sizes:
        sl = slice(lo, lo + sz)
        G = _env(cl, w, cfg, sz, share=full)
        G.configure_wrappers(195, auto_reset=True)
        G.set_domain_randomization(_dr(table).shard(lo, lo + sz))
        G.reset(None, inputs[0][sl], start_frame=inputs[1][sl], qpos_noise=inputs[2][:, sl].contiguous(), qvel_noise=inputs[3][:, sl].contiguous())
        for a in acts:
            G.step(None, a[:, sl].contiguous().to(DEV))
        got = _snap(G)
        for k in BUFS:
            assert np.array_equal(got[k], want[k][..., sl], equal_nan=True), (lo, k)
        lo += sz


def test_split_launch_passes_the_global_env_id(monkeypatch):
    """TMJX_SPLIT_LAUNCH=4: one call's envs go out as four launches with e0 = 0, 32, 64, 96; the result is the single launch's, bit for bit."""
    cl, w, cfg = _table()
    n = 128
    table = np.random.default_rng(8).uniform(0.5, 1.5, size=(3, n)).astype(np.float32)
    a = (torch.randn((38, n), generator=torch.Generator().manual_seed(8)) * 0.3).clamp(-1, 1).to(DEV)
    snaps = []
    for split in (None, "4"):
        if split:
            monkeypatch.setenv("TMJX_SPLIT_LAUNCH", split)
        E = _env(cl, w, cfg, n)
        E.set_domain_randomization(_dr(table))
        _reset(E, seed=4)
        E.step(None, a)
        snaps.append(_snap(E))
    _same(snaps[0], snaps[1], what="split launch")


# ------------------------------------------------------------------------------------------------ G5
def test_refusals_and_clearing():
    cl, w, cfg = _table()
    n = 64
    E = _env(cl, w, cfg, n)
    fresh = _env(cl, w, cfg, n, share=E)
    table = scales_table(TRIPLES_G1, n // 4)
    E.set_domain_randomization(_dr(table))
    _reset(E); _reset(fresh)
    a = (torch.randn((38, n), generator=torch.Generator().manual_seed(1)) * 0.3).clamp(-1, 1).to(DEV)
    # the recording kernel has no RAND build: refused, by name, with nothing launched
    before = _snap(E)
    sd, cf = E.sensor_buffers()
    with pytest.raises(hip.TmjxError, match="tmjx_step_sensors.*tmjx_set_env_scales"):
        E.step_sensors(a, sd, cf)
    with pytest.raises(hip.TmjxError, match="tmjx_physics_sensors.*tmjx_set_env_scales"):
        E.physics_sensors(a, 1, sd, cf)
    _same(before, _snap(E), what="refused call")
    # scales shorter than the launch
    L = E._L
    short = torch.ones((3, n - 1), dtype=torch.float32, device=DEV)
    hip.check(L.tmjx_set_env_scales(E._handle, C.c_void_p(short.data_ptr()), n - 1), "tmjx_set_env_scales")
    with pytest.raises(hip.TmjxError, match=f"launch of {n} envs.*scales for {n - 1}"):
        E.step(None, a)
    with pytest.raises(hip.TmjxError, match="scales for"):
        E.physics(a, 1)
    _same(before, _snap(E), what="refused launch")
    assert L.tmjx_set_env_scales(E._handle, C.c_void_p(short.data_ptr()), 0) != 0 and L.tmjx_set_env_scales(None, None, 0) != 0
    with pytest.raises(ValueError):
        E.set_domain_randomization(DomainRandomization(num_envs=n + 1))
    with pytest.raises(TypeError):
        E.set_domain_randomization(table)
    # NULL clears: the plain launch again, bit-identical to a handle that never had scales
    E.set_domain_randomization(None)
    assert E.domain_randomization is None
    _reset(E)                                  # (the first reset ran its forward pass with the scales: qfrc_actuator, the warm start)
    E.step(None, a); fresh.step(None, a)
    _same(_snap(E), _snap(fresh), what="cleared")
    E.step_sensors(a, sd, cf); fresh.step(None, a)          # ... and the recording kernel takes the handle again
    _same(_snap(E), _snap(fresh), what="cleared, sensors")


def test_wrap_applies_the_scales_and_refuses_models():
    from track_mjx_amd.environment import AutoAlignWrapperTracking, wrap
    cl, w, cfg = _table()
    E = _env(cl, w, cfg, 8)
    dr = DomainRandomization(friction=np.linspace(0.5, 1.2, 8))
    assert wrap(E, episode_length=10, randomization_fn=lambda m: dr) is E and E.domain_randomization == dr
    for ret in (lambda m: m, lambda m: (m, None)):
        with pytest.raises(NotImplementedError, match="per-env model"):
            wrap(E, episode_length=10, randomization_fn=ret)
    dr2 = DomainRandomization(damping=np.linspace(0.5, 2.0, 8))
    assert AutoAlignWrapperTracking(E, episode_length=10, randomization_fn=lambda m: dr2) is E and E.domain_randomization == dr2


# ------------------------------------------------------------------------------------------------ G6
def test_align_policy_with_scales():
    """64 envs with scales set (two triples, 32 envs each) under the align done-policy: the aligned envs' observation meets
    tests/test_gpu_align.py::test_aligned_observation_against_the_oracle's bound — relative error against the expectation built from the
    oracle's primitives no worse than twice that of the not-done envs of the same step.  The alignment is kinematics: it reads no scale."""
    from tests import align_ref as AR
    from track_mjx_amd.environment import AutoAlignWrapperTracking
    cl, w, cfg = _table()
    clips = cl.as_dict()
    n, triples = 64, ((0.6, 0.7, 1.8), (1.3, 1.2, 0.5))
    A = _env(cl, w, cfg, n)
    table = scales_table(triples, n // 2)
    AutoAlignWrapperTracking(A, episode_length=3, randomization_fn=lambda m: _dr(table))
    Os = [make_oracle(scaled_blob(A._blob, *t), cl) for t in triples]
    envs, scratch = [O.new_envs(n) for O in Os], [O.new_envs(1) for O in Os]
    rng = np.random.default_rng(3)
    qn = rng.uniform(-1e-3, 1e-3, (74, n)).astype(np.float32); vn = rng.uniform(-1e-3, 1e-3, (73, n)).astype(np.float32)
    qn[0, 1::4] += 0.3                                   # every fourth env starts 0.3 m off its reference: too_far on step 0
    ci, sf = (np.arange(n) % 4).astype(np.int32), ((7 * np.arange(n)) % 44).astype(np.int32)
    A.reset(None, torch.from_numpy(ci), start_frame=torch.from_numpy(sf), qpos_noise=torch.from_numpy(qn), qvel_noise=torch.from_numpy(vn))
    og = lambda e: e // (n // 2)          # noqa: E731
    for e in range(n):
        Os[og(e)].env_reset(envs[og(e)], e, ci[e], sf[e], qn[:, e], vn[:, e])
    a = AR.violent_actions(rng, 38, n, scales=(0.1,))
    A.step(None, torch.from_numpy(a).to(DEV))
    torch.cuda.synchronize()
    for e in range(n):
        Os[og(e)].env_step(envs[og(e)], e, a[:, e])
    done_o = np.array([Os[og(e)].env_get(envs[og(e)], e, "done")[0] for e in range(n)]) != 0
    assert np.array_equal(done_o, A.done_buf.cpu().numpy() != 0) and np.array_equal(done_o, np.arange(n) % 4 == 1)
    cols = AR.actuator_force_columns(74, 73, len(w.joint_idxs), len(w.body_idxs), cfg["reference_config"]["traj_length"])
    exp = np.stack([AR.oracle_align(Os[og(e)], envs[og(e)], e, clips, scratch[og(e)], cols)[2] if done_o[e]
                    else AR.nan_to_num32(Os[og(e)].env_get(envs[og(e)], e, "obs")) for e in range(n)], 1)
    obs = A.obs_buf.cpu().numpy()
    err_aligned, err_kept = rel_err(obs[:, done_o], exp[:, done_o]), rel_err(obs[:, ~done_o], exp[:, ~done_o])
    print(f"aligned obs rel err {err_aligned:.3e} ({done_o.sum()} envs), not-done obs rel err {err_kept:.3e} ({(~done_o).sum()} envs)")
    assert err_aligned <= 2 * err_kept


# ------------------------------------------------------------------------------------------------ G7
RANGES = dict(friction=(0.5, 1.5), actuator=(0.7, 1.3), damping=(0.5, 2.0))


@pytest.mark.parametrize("use_lstm", [False, True], ids=["mlp", "lstm"])
def test_training_smoke_with_randomization_fn(use_lstm, tmp_path):
    """ppo.train(randomization_fn=) for 2 training steps, 256 envs in two env groups, 64-wide nets: finite metrics; the training envs' scales are
    the groups' slices of uniform_scales(256, key_env), the evaluator's a different draw (eval_key); a run resumed from the checkpoint has the same."""
    from track_mjx_amd.agent import ppo
    from track_mjx_amd.environment import uniform_scales
    from track_mjx_amd.environment.randomization import randomization_keys
    cl, w, cfg = _table()
    fn = uniform_randomization_fn(**RANGES)
    seed = 5
    key_env, eval_key = randomization_keys(seed)
    want = uniform_scales(256, key_env, **RANGES)

    def run(**kw):
        e0 = _env(cl, w, cfg, 128)
        envs = [e0, _env(cl, w, cfg, 128, share=e0)]
        ev = _env(cl, w, cfg, 64, share=e0)
        seen = []
        _, params, metrics = ppo.train(envs, num_timesteps=2 * 256 * 5, episode_length=50, num_evals=2, num_resets_per_eval=1, seed=seed, unroll_length=5,
                                       batch_size=64, num_minibatches=4, num_updates_per_batch=1, encoder_hidden_layer_sizes=(64, 64),
                                       decoder_hidden_layer_sizes=(64, 64), value_hidden_layer_sizes=(64, 64), max_training_steps=2, eval_env=ev,
                                       num_eval_envs=64, use_lstm=use_lstm, hidden_state_size=128, hidden_layer_num=2, randomization_fn=fn,
                                       checkpoint_path=str(tmp_path / "ck"), progress_fn=lambda s, m: seen.append(m), **kw)
        torch.cuda.synchronize()
        return envs, ev, params, seen
    envs, ev, params, seen = run()
    # (the evaluator's per-term episode metrics of an untrained policy carry the NaNs of envs that blew up, with or without scales: the training
    # metrics and the parameters are what two training steps must leave finite)
    train_metrics = {k: v for m in seen for k, v in m.items() if k.startswith("training/")}
    assert train_metrics and all(np.isfinite(v) for v in train_metrics.values()), train_metrics
    assert all(bool(torch.isfinite(v).all()) for tree in params for v in tree.values())
    assert np.array_equal(np.concatenate([e.domain_randomization.table() for e in envs], 1), want.table())
    assert ev.domain_randomization == uniform_scales(64, eval_key, **RANGES)
    assert not np.array_equal(ev.domain_randomization.table(), want.table()[:, :64])
    envs2, ev2, _, _ = run(restore_from=str(tmp_path / "ck"))
    assert np.array_equal(np.concatenate([e.domain_randomization.table() for e in envs2], 1), want.table()) and ev2.domain_randomization == ev.domain_randomization


def test_rollout_command_line_perturbation(tmp_path, capsys):
    """`rollout friction_scale=0.5` writes domain_scales [3] into the clip file, and its qpos differs from the unperturbed roll-out of the same
    clip and seed; with log_sensor_data=true the combination is refused in words a user can act on."""
    from tests.common import StubEnv
    from track_mjx_amd import config as _config
    from track_mjx_amd.agent.checkpoint import save_step_dir
    from track_mjx_amd.agent.ppo import PPOLearner
    from track_mjx_amd.analysis import rollout
    from track_mjx_amd.analysis.utils import load_from_h5py
    cfg = _config.load_config(None, ["n_synthetic_clips=4", "network_config.encoder_layer_sizes=[64,64]", "network_config.decoder_layer_sizes=[64,64]",
                                     "network_config.critic_layer_sizes=[64,64]"])
    ln = PPOLearner(StubEnv(256), encoder_layers=[64, 64], decoder_layers=[64, 64], critic_layers=[64, 64], latents=60, unroll_length=4,
                    batch_size=64, num_minibatches=4, num_updates_per_batch=1, use_graph=False, seed=3)
    with torch.no_grad():
        ln.policy.head.weight.mul_(0.05)       # gentle controls: a roll-out never resets, and an untrained policy at full scale blows the walker up in a few steps
    d = tmp_path / "ck"
    save_step_dir(d, 0, ln, config=cfg)
    assert rollout.main([f"checkpoint={d}", "clips=1,2", "seed=7", f"out={tmp_path / 'plain'}", "log_activations=false"]) == 0
    assert rollout.main([f"checkpoint={d}", "clips=1,2", "seed=7", f"out={tmp_path / 'slip'}", "log_activations=false", "friction_scale=0.5",
                         "damping_scale=1.0,2.0"]) == 0
    for j, c in enumerate((1, 2)):
        plain, slip = load_from_h5py(tmp_path / "plain" / f"clip_{c}.h5"), load_from_h5py(tmp_path / "slip" / f"clip_{c}.h5")
        assert "domain_scales" not in plain
        assert np.asarray(slip["domain_scales"]).tolist() == [0.5, 1.0, (1.0, 2.0)[j]]
        qs, qp = slip["qposes_rollout"], plain["qposes_rollout"]
        assert qs.shape == qp.shape and np.array_equal(qs[0], qp[0])          # the same reset
        both = np.isfinite(qs).all(axis=1) & np.isfinite(qp).all(axis=1)      # (a roll-out never resets: an untrained policy may blow an env up late)
        assert both.sum() >= 10 and (qs[both] != qp[both]).any()
    with pytest.raises(NotImplementedError, match="log_sensor_data cannot be combined with friction_scale"):
        rollout.main([f"checkpoint={d}", "clips=1", f"out={tmp_path / 'bad'}", "friction_scale=0.5", "log_sensor_data=true"])
