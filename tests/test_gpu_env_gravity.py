"""GPU: per-env gravity — the second table of k_physics_wave_rand (csrc/tmjx_wave_rand.hip) behind tmjx_set_env_gravity, and the Python surface
on top of it (DomainRandomization(gravity=), uniform_scales(gravity_scale=, gravity_tilt_deg=), the roll-out's gravity_scale= / slope_deg=).

The expectation for an env with gravity g is exact: a handle — the oracle's, or this library's plain kernel — created from the model blob with
its `gravity` entry set to g (tests/gravity_ref.py: gravity_blob).  The physics reads gravity in one place and no derived model constant
depends on it, so the comparison with the plain kernel is bit for bit for ANY float32 vector.  The same kernel source runs under the host
emulation in tests/test_env_gravity_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.common import default_walker, make_oracle, rel_err
from tests.domain_rand_ref import TRIPLES_G1, scaled_blob, scales_table
from tests.gravity_ref import gravity_blob, gravity_set, gravity_table, model_gravity, tilted
from track_mjx_amd import blob as _blob
from track_mjx_amd import clips as _clips
from track_mjx_amd import hip
from track_mjx_amd.environment import DomainRandomization, uniform_scales

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PHYS = ("qpos", "qvel", "act", "qacc_warmstart", "time")
BUFS = ("state_buf", "istate_buf", "obs_buf", "reward_buf", "done_buf", "trunc_buf", "metrics_buf")


def _table(config="rodent-full-clips", n_clips=4):
    w, cfg = default_walker(config)
    return _clips.make_synthetic_clips(w.model, n_clips, seed=0), w, cfg


class _BlobWalker:
    """A walker whose blob entries were changed on the host by `fn(blob) -> blob`: what MultiClipTracking builds its handle from
    (walker.build_blob reads `walker.model`), everything else the wrapped walker's."""

    def __init__(self, w, fn):
        self._w = w
        self.model = _blob.unpack(fn(_blob.pack(w.model)))

    def __getattr__(self, name):
        return getattr(self._w, name)


def _env(cl, w, cfg, n, blob_fn=None, share=None):
    from track_mjx_amd.environment import MultiClipTracking, RewardConfig
    return MultiClipTracking(cl, w if blob_fn is None else _BlobWalker(w, blob_fn), RewardConfig(**cfg["env_config"]["reward_weights"]),
                             **cfg["env_config"]["env_args"], **cfg["reference_config"], num_envs=n, device=DEV, share_clips_with=share)


def _g0(w):
    return model_gravity(_blob.pack(w.model))


def _dr_g(gtab, stab=None):
    sc = (None, None, None) if stab is None else (stab[0], stab[1], stab[2])
    return DomainRandomization(*sc, gravity=np.ascontiguousarray(gtab.T))


def _inputs(n, seed=0, sink=0.002):
    """Reset inputs from a seed; env e starts sunk by sink * (e % 5) below its clip pose (tests/test_gpu_domain_randomization.py:
    initial_states), so that the paws are in the floor from the first substep on."""
    g = torch.Generator().manual_seed(seed)
    clip = torch.randint(0, 4, (n,), generator=g, dtype=torch.int32); start = torch.randint(0, 44, (n,), generator=g, dtype=torch.int32)
    qn = (torch.rand((74, n), generator=g) * 2 - 1) * 1e-3; vn = (torch.rand((73, n), generator=g) * 2 - 1) * 1e-3
    qn[2] -= sink * (torch.arange(n) % 5)
    return clip, start, qn, vn


def _reset(env, inputs, sl=slice(None)):
    env.reset(None, inputs[0][sl], start_frame=inputs[1][sl], qpos_noise=inputs[2][:, sl].contiguous(), qvel_noise=inputs[3][:, sl].contiguous())


def _snap(env):
    torch.cuda.synchronize()
    return {b: getattr(env, b).cpu().numpy().copy() for b in BUFS}


def _bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def _same(a, b, cols_a=slice(None), cols_b=slice(None), what=""):
    for k in BUFS:
        assert np.array_equal(_bits(a[k][..., cols_a]), _bits(b[k][..., cols_b])), (what, k)


def _acts(n, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((38, n), generator=g) * 0.3).clamp(-1, 1) for _ in range(steps)]


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("config", ["rodent-full-clips", "rodent-sps-per-actor"])
def test_every_gravity_equals_the_handle_built_from_its_blob(config):
    """96 envs, 16 consecutive envs per member of the gravity set, reset from a common seed (sunk into the floor) and stepped 3 control steps:
    state, istate, obs, reward, done, truncation and metrics are bit-identical to six plain handles, each created from gravity_blob(., g) and
    stepping the same 16 envs.  Then the same with scales set too: TRIPLES_G1's four (friction, actuator, damping) patterns with the
    power-of-two values {0.5, 1, 2} (a scaled constant is exact only then), crossed with two gravities, against scaled_blob(gravity_blob(..))."""
    cl, w, cfg = _table(config)
    G = gravity_set(_g0(w))
    per, n = 16, 96
    R = _env(cl, w, cfg, n)
    R.configure_wrappers(195, auto_reset=True)
    R.set_domain_randomization(_dr_g(gravity_table(G, per)))
    inputs, acts = _inputs(n, seed=11), _acts(n, 3, seed=12)
    _reset(R, inputs)
    for a in acts:
        R.step(None, a.to(DEV))
    got = _snap(R)
    assert np.isfinite(got["obs_buf"]).all()
    R.physics(acts[0].to(DEV), 1)                 # (one more substep with the dump: the run is on the floor)
    torch.cuda.synchronize()
    assert int((R.rows("con_dist") < 0).sum()) > 0, "the run must pass through floor contact"
    L = R.layout
    qv = slice(L.qvel, L.qvel + L.nv)
    Q = _env(cl, w, cfg, n, share=R)              # the same envs under the model's gravity: every other gravity must have moved every env
    Q.configure_wrappers(195, auto_reset=True)
    _reset(Q, inputs)
    for a in acts:
        Q.step(None, a.to(DEV))
    plain = _snap(Q)
    for k, g in enumerate(G):
        sl = slice(k * per, (k + 1) * per)
        P = _env(cl, w, cfg, per, blob_fn=lambda b, g=g: gravity_blob(b, g), share=R)
        P.configure_wrappers(195, auto_reset=True)
        _reset(P, inputs, sl)
        for a in acts:
            P.step(None, a[:, sl].contiguous().to(DEV))
        want = _snap(P)
        _same(got, want, cols_a=sl, what=g.tolist())
        # ... and another gravity moved the env.  (An env whose last step ended with done set was auto-reset onto its stored first state, which
        # is the same under every gravity: only the envs still running in both runs are asked, and they must be at least half of the group.)
        running = [e for e in range(k * per, (k + 1) * per) if got["done_buf"][e] == 0 and plain["done_buf"][e] == 0]
        moved = [not np.array_equal(plain["state_buf"][qv, e], got["state_buf"][qv, e]) for e in running]
        assert len(running) >= per // 2, (g.tolist(), running)
        assert (all(moved) if k else not any(moved)), (g.tolist(), running, moved)
    # scales and gravity together
    pow2 = [tuple({0.6: 0.5, 0.7: 0.5, 1.0: 1.0, 1.3: 2.0, 1.2: 2.0, 1.8: 2.0}[s] for s in t) for t in TRIPLES_G1]
    combos = [(t, g) for g in (G[3], G[5]) for t in pow2]
    per, n = 8, 64
    R = _env(cl, w, cfg, n)
    R.configure_wrappers(195, auto_reset=True)
    R.set_domain_randomization(_dr_g(gravity_table([g for _, g in combos], per), scales_table([t for t, _ in combos], per)))
    inputs, acts = _inputs(n, seed=13), _acts(n, 3, seed=14)
    _reset(R, inputs)
    for a in acts:
        R.step(None, a.to(DEV))
    got = _snap(R)
    for k, (t, g) in enumerate(combos):
        sl = slice(k * per, (k + 1) * per)
        P = _env(cl, w, cfg, per, blob_fn=lambda b, t=t, g=g: scaled_blob(gravity_blob(b, g), *t), share=R)
        P.configure_wrappers(195, auto_reset=True)
        _reset(P, inputs, sl)
        for a in acts:
            P.step(None, a[:, sl].contiguous().to(DEV))
        _same(got, _snap(P), cols_a=sl, what=(t, g.tolist()))


# ------------------------------------------------------------------------------------------------ 2
def test_model_gravity_table_and_clearing():
    """128 envs, 3 control steps: a table holding the model's gravity for every env (the RAND kernel, gravity only) is bit-identical to the
    handle without a table; after set(None) the handle launches the product kernel again and equals a fresh handle."""
    cl, w, cfg = _table()
    n = 128
    A = _env(cl, w, cfg, n); B = _env(cl, w, cfg, n, share=A)
    for e in (A, B):
        e.configure_wrappers(195, auto_reset=True)
    g0 = _g0(w)
    B.set_domain_randomization(_dr_g(gravity_table([g0], n)))
    assert B.domain_randomization.gravity.shape == (n, 3) and B._scales_dev is None and B._gravity_dev is not None      # gravity only
    inputs, acts = _inputs(n, seed=21), _acts(n, 3, seed=22)
    _reset(A, inputs); _reset(B, inputs)
    _same(_snap(A), _snap(B), what="reset")
    for t, a in enumerate(acts):
        A.step(None, a.to(DEV)); B.step(None, a.to(DEV))
        sa = _snap(A)
        assert np.isfinite(sa["obs_buf"]).all()
        _same(sa, _snap(B), what=f"step {t}")
    # a real table, then cleared
    B.set_domain_randomization(_dr_g(gravity_table([0.5 * g0], n)))
    _reset(B, inputs)
    B.step(None, acts[0].to(DEV))
    B.set_domain_randomization(None)
    assert B.domain_randomization is None and B._gravity_dev is None
    fresh = _env(cl, w, cfg, n, share=A)
    fresh.configure_wrappers(195, auto_reset=True)
    _reset(B, inputs); _reset(fresh, inputs)
    for a in acts[:2]:
        B.step(None, a.to(DEV)); fresh.step(None, a.to(DEV))
    _same(_snap(B), _snap(fresh), what="cleared")
    sd, cf = B.sensor_buffers()
    B.step_sensors(acts[2].to(DEV), sd, cf); fresh.step(None, acts[2].to(DEV))      # ... and the recording kernel takes the handle again
    _same(_snap(B), _snap(fresh), what="cleared, sensors")


# ------------------------------------------------------------------------------------------------ 3
def test_env_groups_and_split_launches_take_their_slice_of_the_table(monkeypatch):
    """Three env groups (48, 44, 36) with their slices of one table — a different gravity in every env — are bit-identical to the single launch
    of all 128 envs, and so is the single call sent out as four launches with e0 = 0, 32, 64, 96 (TMJX_SPLIT_LAUNCH=4)."""
    cl, w, cfg = _table()
    sizes, n = (48, 44, 36), 128
    g0 = _g0(w)
    rng = np.random.default_rng(6)
    gt = np.stack([tilted(g0, rng.uniform(0.4, 1.5), rng.uniform(0, 20), (np.cos(az), np.sin(az))) for az in rng.uniform(0, 2 * np.pi, n)])
    dr = DomainRandomization(gravity=gt)
    full = _env(cl, w, cfg, n)
    full.configure_wrappers(195, auto_reset=True)
    full.set_domain_randomization(dr)
    inputs, acts = _inputs(n, seed=31), _acts(n, 2, seed=32)
    _reset(full, inputs)
    for a in acts:
        full.step(None, a.to(DEV))
    want = _snap(full)
    lo = 0
    for sz in sizes:
        sl = slice(lo, lo + sz)
        Gp = _env(cl, w, cfg, sz, share=full)
        Gp.configure_wrappers(195, auto_reset=True)
        Gp.set_domain_randomization(dr.shard(lo, lo + sz))
        _reset(Gp, inputs, sl)
        for a in acts:
            Gp.step(None, a[:, sl].contiguous().to(DEV))
        _same(_snap(Gp), want, cols_b=sl, what=f"group at {lo}")
        lo += sz
    monkeypatch.setenv("TMJX_SPLIT_LAUNCH", "4")
    S = _env(cl, w, cfg, n, share=full)
    S.configure_wrappers(195, auto_reset=True)
    S.set_domain_randomization(dr)
    _reset(S, inputs)
    for a in acts:
        S.step(None, a.to(DEV))
    _same(_snap(S), want, what="split launch")


# ------------------------------------------------------------------------------------------------ 4
def parity_groups(g0):
    """The oracle-parity groups: g0, 0.5 g0, |g0| tilted 10 deg toward +x, |g0| tilted 20 deg toward -y."""
    G = gravity_set(g0)
    return [G[0], G[1], G[3], G[4]]


def run_teacher_forced_gravity(blob, cl, physics, groups, n=64, substeps=40, seed=1):
    """tests/test_gpu_domain_randomization.py: run_teacher_forced's protocol — test_substep_teacher_forced's states (clip poses sunk into the
    floor) and actions N(0, 0.03), every substep started by all parties from the float64 oracles' state — with one float64 / float32 oracle
    pair per GRAVITY, built from gravity_blob.  `physics(state rows dict, action [nu][n] float32) -> {"qpos", "qvel"} [rows][n]` is the
    implementation under test with gravity_table(groups, n // len(groups)).  Bounds (that test's, per group over its env-substeps): median
    relative error <= 1e-5, 0.9-quantile <= 2 x the float32 oracle's own + 1e-5, on qpos and qvel.  Sensitivity, for every group whose gravity
    is not the model's: the float64 oracle's qvel with that gravity differs from the plain float64 oracle's, stepped from the same states, by
    more than 10 x the group's implementation-vs-oracle median (median over the env-substeps, both) — and so does the implementation's own
    result: one that ignored the table would sit on the plain oracle's."""
    from tests.test_gpu_domain_randomization import initial_states
    per = n // len(groups)
    O32 = [make_oracle(gravity_blob(blob, g), cl, "f32") for g in groups]
    O64 = [make_oracle(gravity_blob(blob, g), cl, "f64") for g in groups]
    plain = make_oracle(blob, cl, "f64")
    rng = np.random.default_rng(seed)
    qpos, qvel = initial_states(cl, n, rng)
    grp = lambda e: e // per          # noqa: E731
    d32 = [O32[grp(e)].new_data(qpos[e], qvel[e]) for e in range(n)]
    d64 = [O64[grp(e)].new_data(qpos[e], qvel[e]) for e in range(n)]
    dpl = [plain.new_data(qpos[e], qvel[e]) for e in range(n)]
    ncon = 0
    pooled = {(g, k): ([], []) for g in range(len(groups)) for k in ("qpos", "qvel")}
    osens, moved = {}, {}
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
        unpert = np.stack([plain.get(dpl[e], "qvel") for e in range(n)], 1)
        ncon += sum((O64[grp(e)].get(d64[e], "con_dist") < 0).sum() for e in range(n))
        for g in range(len(groups)):
            sl = slice(g * per, (g + 1) * per)
            for k in ("qpos", "qvel"):
                pooled[g, k][0].append(rel_err(got[k][:, sl], ref[k][:, sl], axis=0)); pooled[g, k][1].append(rel_err(r32[k][:, sl], ref[k][:, sl], axis=0))
            osens.setdefault(g, []).append(rel_err(ref["qvel"][:, sl], unpert[:, sl], axis=0))
            moved.setdefault(g, []).append(rel_err(got["qvel"][:, sl], unpert[:, sl], axis=0))
    assert ncon > 0, "the states must be in contact"
    g0 = model_gravity(blob)
    out = {}
    for (g, k), (eg, e32) in pooled.items():
        eg, e32 = np.concatenate(eg), np.concatenate(e32)
        out[g, k] = (np.median(eg), np.quantile(eg, 0.9), np.median(e32), np.quantile(e32, 0.9))
        print(f"group {np.round(groups[g], 4).tolist()} {k}: {len(eg)} env-substeps, median {np.median(eg):.2e}, q90 {np.quantile(eg, 0.9):.2e}; float32 oracle "
              f"median {np.median(e32):.2e}, q90 {np.quantile(e32, 0.9):.2e}")
    for g in range(len(groups)):
        print(f"group {np.round(groups[g], 4).tolist()}: float64 oracle vs the plain oracle, qvel median {np.median(np.concatenate(osens[g])):.2e}; "
              f"implementation vs the plain oracle {np.median(np.concatenate(moved[g])):.2e}")
    for (g, k), (med, q90, _, q90_32) in out.items():
        assert med <= 1e-5, (groups[g].tolist(), k, med)
        assert q90 <= 2 * q90_32 + 1e-5, (groups[g].tolist(), k, q90, q90_32)
    for g in range(len(groups)):
        if np.array_equal(np.asarray(groups[g], np.float32), g0.astype(np.float32)):       # the model's own gravity (as the float32 the kernel reads)
            continue
        med = out[g, "qvel"][0]
        assert np.median(np.concatenate(osens[g])) > 10 * med, (groups[g].tolist(), np.median(np.concatenate(osens[g])), med)
        assert np.median(np.concatenate(moved[g])) > 10 * med, (groups[g].tolist(), np.median(np.concatenate(moved[g])), med)
    return out


@pytest.mark.parametrize("config", ["rodent-full-clips", "rodent-sps-per-actor"])
def test_parity_against_the_oracle_per_gravity(config):
    """64 envs as 4 groups of 16 — g0, 0.5 g0, tilt 10 deg, tilt 20 deg — over the 40 teacher-forced substeps against float64 and float32 oracles
    built from gravity_blob: run_teacher_forced_gravity's bounds and sensitivity condition."""
    cl, w, cfg = _table(config)
    n = 64
    env = _env(cl, w, cfg, n)
    groups = parity_groups(_g0(w))
    env.set_domain_randomization(_dr_g(gravity_table(groups, n // 4)))

    def physics(st, a):
        for k, v in st.items():
            env.rows(k).copy_(torch.from_numpy(v.astype(np.float32)))
        env.physics(torch.from_numpy(a).to(DEV), 1)
        torch.cuda.synchronize()
        return {k: env.rows(k).cpu().numpy() for k in ("qpos", "qvel")}
    run_teacher_forced_gravity(env._blob, cl, physics, groups, n=n)


# ------------------------------------------------------------------------------------------------ 5
def test_refusals():
    cl, w, cfg = _table()
    n = 64
    E = _env(cl, w, cfg, n)
    gtab = gravity_table(parity_groups(_g0(w)), n // 4)
    E.set_domain_randomization(_dr_g(gtab))
    inputs = _inputs(n, seed=41)
    _reset(E, inputs)
    a = _acts(n, 1, seed=42)[0].to(DEV)
    # the recording kernel's sensor stage reads the model's gravity: refused, by name, with nothing launched
    before = _snap(E)
    sd, cf = E.sensor_buffers()
    with pytest.raises(hip.TmjxError, match="tmjx_step_sensors.*tmjx_set_env_gravity"):
        E.step_sensors(a, sd, cf)
    with pytest.raises(hip.TmjxError, match="tmjx_physics_sensors.*tmjx_set_env_gravity"):
        E.physics_sensors(a, 1, sd, cf)
    _same(before, _snap(E), what="refused call")
    # a table shorter than the launch: refused before any launch (with and without a long enough scales table beside it)
    L = E._L
    short = torch.from_numpy(gtab[:, :n - 1].copy()).to(DEV)
    ones = torch.ones((3, n), dtype=torch.float32, device=DEV)
    hip.check(L.tmjx_set_env_gravity(E._handle, C.c_void_p(short.data_ptr()), n - 1), "tmjx_set_env_gravity")
    for scales in (None, ones):
        hip.check(L.tmjx_set_env_scales(E._handle, None if scales is None else C.c_void_p(scales.data_ptr()), 0 if scales is None else n), "tmjx_set_env_scales")
        with pytest.raises(hip.TmjxError, match=f"launch of {n} envs.*gravity for {n - 1}.*tmjx_set_env_gravity"):
            E.step(None, a)
        with pytest.raises(hip.TmjxError, match="tmjx_set_env_gravity"):
            E.physics(a, 1)
        with pytest.raises(hip.TmjxError, match="tmjx_set_env_gravity"):
            _reset(E, inputs)
    _same(before, _snap(E), what="refused launch")          # nothing was enqueued: not even reset's first kernel
    assert L.tmjx_set_env_gravity(E._handle, C.c_void_p(short.data_ptr()), 0) != 0 and L.tmjx_set_env_gravity(None, None, 0) != 0
    hip.check(L.tmjx_set_env_gravity(E._handle, None, 0), "tmjx_set_env_gravity")
    with pytest.raises(ValueError):
        E.set_domain_randomization(DomainRandomization(gravity=np.zeros((n + 1, 3))))
    for bad in (np.zeros((n, 2)), np.zeros(n), np.full((n, 3), np.nan)):
        with pytest.raises(ValueError):
            DomainRandomization(gravity=bad)


def test_lane_cross_check_build_refuses_a_gravity_table(monkeypatch):
    """The lane-per-env cross-check implementation has no domain-randomisation path: tmjx_set_env_gravity fails on its handle, by name (the same
    build's wave-per-env handle takes the table)."""
    from pathlib import Path
    from tests.common import default_blob
    so = Path(__file__).resolve().parent / "lane" / "libtmjx_hip_lane.so"
    L = hip.load(so)
    blob = default_blob()
    t = torch.zeros((3, 4), dtype=torch.float32, device=DEV)
    monkeypatch.setenv("TMJX_IMPL", "lane")
    h = C.c_void_p()
    assert L.tmjx_model_create(blob, len(blob), C.byref(h)) == 0, L.tmjx_last_error()
    assert L.tmjx_set_env_gravity(h, C.c_void_p(t.data_ptr()), 4) == -22           # TMJX_EINVAL (include/tmjx.h)
    assert b"tmjx_set_env_gravity" in L.tmjx_last_error() and b"wave-per-env" in L.tmjx_last_error()
    assert L.tmjx_set_env_gravity(h, None, 0) == 0
    L.tmjx_model_destroy(h)
    monkeypatch.delenv("TMJX_IMPL")
    h = C.c_void_p()
    assert L.tmjx_model_create(blob, len(blob), C.byref(h)) == 0, L.tmjx_last_error()
    assert L.tmjx_set_env_gravity(h, C.c_void_p(t.data_ptr()), 4) == 0
    L.tmjx_model_destroy(h)


# ------------------------------------------------------------------------------------------------ 6
def test_wrap_applies_a_gravity_randomization():
    from track_mjx_amd.environment import wrap
    cl, w, cfg = _table()
    E = _env(cl, w, cfg, 8)
    g0 = _g0(w)
    seen = {}

    def fn(model):
        seen["g"] = np.asarray(model["gravity"], np.float64)
        return uniform_scales(model["num_envs"], 5, friction=(0.5, 1.5), gravity_scale=(0.5, 1.5), gravity_tilt_deg=(0.0, 15.0), gravity=model["gravity"])
    assert wrap(E, episode_length=10, randomization_fn=fn) is E
    assert np.array_equal(seen["g"], g0)
    dr = E.domain_randomization
    assert dr == uniform_scales(8, 5, friction=(0.5, 1.5), gravity_scale=(0.5, 1.5), gravity_tilt_deg=(0.0, 15.0), gravity=g0) and dr.gravity.shape == (8, 3)
    assert dr != uniform_scales(8, 5, friction=(0.5, 1.5))
    assert E._scales_dev is not None and np.array_equal(E._gravity_dev.cpu().numpy(), dr.gravity.T)
    st = E.reset(torch.Generator().manual_seed(0))
    st = E.step(st, torch.zeros((38, 8), device=DEV))
    torch.cuda.synchronize()
    assert np.isfinite(st.obs.cpu().numpy()).all()


def test_uniform_scales_gravity_draw():
    g0 = np.array([0.0, 0.0, -9.81])
    n, key = 1000, 9
    kw = dict(friction=(0.5, 1.5), actuator=(0.8, 1.2), damping=(0.5, 2.0))
    a = uniform_scales(n, key, **kw, gravity_scale=(0.4, 1.5), gravity_tilt_deg=(2.0, 20.0), gravity=g0)
    b = uniform_scales(n, key, **kw, gravity_scale=(0.4, 1.5), gravity_tilt_deg=(2.0, 20.0), gravity=g0)
    plain = uniform_scales(n, key, **kw)
    assert a == b and np.array_equal(a.gravity, b.gravity) and a.gravity.dtype == np.float32
    for name in ("friction", "actuator", "damping"):          # the three scales' draws do not depend on whether gravity is drawn
        assert np.array_equal(getattr(a, name), getattr(plain, name)), name
    assert plain.gravity is None
    g = a.gravity.astype(np.float64)
    mag = np.linalg.norm(g, axis=1) / 9.81
    ang = np.degrees(np.arccos(np.clip((g @ g0) / (np.linalg.norm(g, axis=1) * 9.81), -1, 1)))
    tol = 4 * np.finfo(np.float32).eps             # (the vector is built in float64 and stored in float32)
    assert mag.min() >= 0.4 * (1 - tol) and mag.max() <= 1.5 * (1 + tol) and mag.max() - mag.min() > 0.9 * 1.1
    assert ang.min() >= 2.0 - 1e-4 and ang.max() <= 20.0 + 1e-4 and ang.max() - ang.min() > 0.9 * 18
    az = np.arctan2(g[:, 1], g[:, 0])
    assert (np.histogram(az, bins=4, range=(-np.pi, np.pi))[0] > n // 8).all()        # every quadrant
    assert uniform_scales(n, key + 1, gravity_scale=(0.4, 1.5), gravity=g0) != uniform_scales(n, key, gravity_scale=(0.4, 1.5), gravity=g0)
    only_scale = uniform_scales(n, key, gravity_scale=(0.5, 0.5), gravity=g0)
    assert np.allclose(only_scale.gravity, 0.5 * g0, rtol=1e-6) and not only_scale.has_scales


def test_rollout_command_line_slope_and_gravity_scale(tmp_path):
    """`rollout slope_deg=15` writes `gravity` [3] = |g| (sin 15, 0, -cos 15) into the clip files, starts from the plain run's reset and leaves its
    trajectory; `domain_scales` appears only with a scale; with log_sensor_data=true the gravity options are refused before any launch."""
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
    assert rollout.main([f"checkpoint={d}", "clips=1,2", "seed=7", f"out={tmp_path / 'slope'}", "log_activations=false", "slope_deg=15"]) == 0
    w, _ = default_walker()
    mag = np.linalg.norm(_g0(w))
    want = (mag * np.array([np.sin(np.deg2rad(15.0)), 0.0, -np.cos(np.deg2rad(15.0))])).astype(np.float32)
    for c in (1, 2):
        plain, slope = load_from_h5py(tmp_path / "plain" / f"clip_{c}.h5"), load_from_h5py(tmp_path / "slope" / f"clip_{c}.h5")
        assert "gravity" not in plain and "domain_scales" not in slope
        assert np.array_equal(np.asarray(slope["gravity"], np.float32), want)
        qs, qp = slope["qposes_rollout"], plain["qposes_rollout"]
        assert qs.shape == qp.shape and np.array_equal(qs[0], qp[0])          # the same reset
        both = np.isfinite(qs).all(axis=1) & np.isfinite(qp).all(axis=1)      # (a roll-out never resets: an untrained policy may blow an env up late)
        assert both.sum() >= 10 and (qs[both] != qp[both]).any()
    with pytest.raises(NotImplementedError, match="log_sensor_data cannot be combined with gravity_scale / slope_deg"):
        rollout.main([f"checkpoint={d}", "clips=1", f"out={tmp_path / 'bad'}", "gravity_scale=0.5", "log_sensor_data=true"])
    assert not (tmp_path / "bad").exists() or not list((tmp_path / "bad").glob("clip_*.h5"))
