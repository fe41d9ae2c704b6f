"""CPU: per-env gravity (environment/randomization.py, analysis/rollout.py, the RAND build of csrc/wave_physics.h with both of its tables
through tests/hostemu/grav_emu.*).

C1 the emulated RAND body with per-env gravity against the oracle on blobs whose `gravity` entry was set on the host, and against the plain
body built from the same blobs; C2 no gravity table (and unit scales) = the plain body, bit for bit, with every LDS word and register starting
from NaN; C3 host logic — DomainRandomization(gravity=), the draw, the config keys, sharding, the slope formula, the command line's
one-or-per-clip values; C4 the C-ABI entry is exported.  The same kernel source runs on the GPU in tests/test_gpu_env_gravity.py."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent / "hostemu"))
from emu import Emu  # noqa: E402
from grav_emu import GravEmu  # noqa: E402

from tests.common import default_blob, default_walker, make_oracle, rel_err  # noqa: E402
from tests.gravity_ref import gravity_blob, gravity_set, gravity_table, model_gravity  # noqa: E402
from track_mjx_amd import clips as _clips  # noqa: E402
from track_mjx_amd import jax_random as jr  # noqa: E402
from track_mjx_amd.environment import DomainRandomization, shard_scales, uniform_randomization_fn, uniform_scales  # noqa: E402
from track_mjx_amd.environment import randomization as _rand  # noqa: E402

PHYS = ("qpos", "qvel", "act", "qacc_warmstart", "time")
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def setup():
    w, cfg = default_walker()
    blob = default_blob(w, cfg)
    clip = _clips.make_synthetic_clips(w.model, 4, seed=0)
    return w, blob, clip


def _states(blob, clip, n, rng, pen):
    """tests/test_domain_randomization_cpu.py's states: clip poses lowered until the nearest paw contacts penetrate the floor by `pen` .. 3 `pen`,
    with joint and root velocities and non-zero activations."""
    O = make_oracle(blob, clip, "f64")
    qpos = np.zeros((n, 74)); qvel = rng.uniform(-0.5, 0.5, size=(n, 73))
    for e in range(n):
        c, f = e % 4, (7 * e) % 44
        qpos[e] = np.concatenate([clip.position[c, f], clip.quaternion[c, f], clip.joints[c, f]]) + rng.uniform(-1e-3, 1e-3, 74)
        d = O.new_data(qpos[e], np.zeros(73)); O.forward(d)
        qpos[e, 2] -= O.get(d, "con_dist").min() + pen * (1 + e % 3)
    qvel[:, :2] = rng.uniform(0.1, 0.3, size=(n, 2))
    act = rng.uniform(-0.3, 0.3, size=(n, 38))
    return qpos, qvel, act


def _fill(E, qpos, qvel, act):
    E.rows("qpos")[:] = qpos.T; E.rows("qvel")[:] = qvel.T; E.rows("act")[:] = act.T


# ------------------------------------------------------------------------------------------------ C1
@pytest.mark.parametrize("chains", [True, False], ids=["chain-layout", "generic-layout"])
def test_grav_emu_against_the_oracle_on_gravity_blobs(setup, chains):
    """8 envs, 4 gravities (two envs each: g0, 0.5 g0, |g0| tilted 10 deg toward +x, 0.38 |g0| tilted 5 deg toward (+x, +y)), 2 teacher-forced
    substeps: the emulated RAND body with the per-env gravity table against the float64 oracle created from gravity_blob, under the bounds of
    tests/test_domain_randomization_cpu.py::test_rand_emu_against_the_oracle_on_scaled_blobs (no scales table: unit scales)."""
    w, blob, clip = setup
    n, per = 8, 2
    G = gravity_set(model_gravity(blob))
    groups = [G[0], G[1], G[3], G[5]]
    gtab = gravity_table(groups, per)
    E, R = Emu(blob, n), GravEmu(blob)
    blobs = [gravity_blob(blob, g) for g in groups]
    O32 = [make_oracle(b, clip, "f32") for b in blobs]
    O64 = [make_oracle(b, clip, "f64") for b in blobs]
    plain = make_oracle(blob, clip, "f64")
    rng = np.random.default_rng(1)
    qpos, qvel, act = _states(blob, clip, n, rng, 0.002)
    d32, d64, dpl = [], [], []
    for e in range(n):
        for O, ds in ((O32[e // per], d32), (O64[e // per], d64), (plain, dpl)):
            d = O.new_data(qpos[e], qvel[e]); O.set(d, "act", act[e]); ds.append(d)
    acc = {k: ([], []) for k in ("qpos", "qvel")}
    sens = []
    for sub in range(2):
        a = np.clip(rng.normal(size=(n, 38)) * 0.3, -1, 1)
        for k in PHYS:
            v = np.stack([O64[e // per].get(d64[e], k) for e in range(n)], 1)
            E.rows(k)[:] = v
            for e in range(n):
                O32[e // per].set(d32[e], k, v[:, e]); plain.set(dpl[e], k, v[:, e])
        R.physics(E, a.T.astype(np.float32).copy(), 1, None, gtab, dump=False, chains=chains)
        for e in range(n):
            O32[e // per].step(d32[e], a[e]); O64[e // per].step(d64[e], a[e]); plain.step(dpl[e], a[e])
        for k in ("qpos", "qvel"):
            ref = np.stack([O64[e // per].get(d64[e], k) for e in range(n)], 1)
            r32 = np.stack([O32[e // per].get(d32[e], k) for e in range(n)], 1)
            e_emu, e_32 = rel_err(E.rows(k), ref, axis=0), rel_err(r32, ref, axis=0)
            acc[k][0].append(e_emu); acc[k][1].append(e_32)
            print(f"substep {sub} {k}: emu {e_emu}, f32 oracle {e_32}")
            assert np.median(e_emu) <= 1e-5, (sub, k, e_emu)
        sens.append(rel_err(E.rows("qvel"), np.stack([plain.get(dpl[e], "qvel") for e in range(n)], 1), axis=0))
    for k in ("qpos", "qvel"):
        g, f = np.concatenate(acc[k][0]), np.concatenate(acc[k][1])
        print(f"{k}: median {np.median(g):.3e} / {np.median(f):.3e}, q90 {np.quantile(g, 0.9):.3e} / {np.quantile(f, 0.9):.3e}, max {g.max():.3e} / {f.max():.3e}")
        assert np.median(g) <= (1.25 if chains else 4.0) * np.median(f) + 1e-7, (k, np.median(g), np.median(f))
        assert np.quantile(g, 0.9) <= (2.0 if chains else 4.0) * np.quantile(f, 0.9) + 1e-5, (k, np.quantile(g, 0.9), np.quantile(f, 0.9))
        assert g.max() <= 4 * f.max() + (1e-4 if k == "qvel" else 2e-5), (k, g.max(), f.max())
    assert sum((O64[e // per].get(d64[e], "con_dist") < 0).sum() for e in range(n)) > 0, "the states must reach contact"
    # gravity acts (the GPU test's sensitivity condition): per group with another gravity, the result's distance from the PLAIN float64 oracle's,
    # stepped from the same states, is more than 10 x the group's parity median (medians over the group's env-substeps)
    dist, par = np.stack(sens), np.stack(acc["qvel"][0])
    for g in range(1, len(groups)):
        sl = slice(g * per, (g + 1) * per)
        print(f"group {groups[g].tolist()}: distance from the plain oracle median {np.median(dist[:, sl]):.3e}, parity median {np.median(par[:, sl]):.3e}")
        assert np.median(dist[:, sl]) > 10 * np.median(par[:, sl]), (groups[g].tolist(), dist[:, sl], par[:, sl])


@pytest.mark.parametrize("chains", [True, False], ids=["chain-layout", "generic-layout"])
def test_grav_emu_equals_the_plain_body_on_the_gravity_blob(setup, chains, monkeypatch):
    """The six gravities of the set (one env each, read at an e0 offset from a longer table whose other columns must not be read): the RAND body
    with the table is bit-identical — every state row — to the plain body built from gravity_blob(., g)."""
    w, blob, clip = setup
    if not chains:
        monkeypatch.setenv("TMJX_EMU_GENERIC", "1")
    G = gravity_set(model_gravity(blob))
    n, e0 = len(G), 3
    gtab = np.full((3, e0 + n + 2), 123.0, np.float32)
    gtab[:, e0:e0 + n] = gravity_table(G, 1)
    rng = np.random.default_rng(3)
    qpos, qvel, act = _states(blob, clip, n, rng, 0.002)
    a = np.clip(rng.normal(size=(38, n)) * 0.3, -1, 1).astype(np.float32)
    B, R = Emu(blob, n), GravEmu(blob)
    _fill(B, qpos, qvel, act)
    R.physics(B, a, 2, None, gtab, e0=e0, dump=False, chains=chains)
    P = Emu(blob, n)
    _fill(P, qpos, qvel, act)
    P.physics_wave(a, 2, True, dump=False)
    for e, g in enumerate(G):
        A = Emu(gravity_blob(blob, g), 1)
        _fill(A, qpos[e:e + 1], qvel[e:e + 1], act[e:e + 1])
        A.physics_wave(a[:, e:e + 1].copy(), 2, True, dump=False)
        for k in PHYS:
            assert np.array_equal(A.rows(k)[:, 0].view(np.uint32), B.rows(k)[:, e].view(np.uint32)), (e, g.tolist(), k)
        assert np.array_equal(P.rows("qvel")[:, e], B.rows("qvel")[:, e]) == (e == 0), (e, g.tolist())


# ------------------------------------------------------------------------------------------------ C2
@pytest.mark.parametrize("chains", [True, False], ids=["chain-layout", "generic-layout"])
def test_no_gravity_table_and_unit_scales_are_the_plain_body(setup, chains, monkeypatch):
    """Null gravity table with unit scales, null scales with the model's gravity as a table, and both null: each bit-identical to hostemu's
    plain body — state and every dumped intermediate — with LDS, registers and scratch starting from NaN (TMJX_EMU_POISON=nan)."""
    w, blob, clip = setup
    monkeypatch.setenv("TMJX_EMU_POISON", "nan")
    if not chains:
        monkeypatch.setenv("TMJX_EMU_GENERIC", "1")
    n = 8
    rng = np.random.default_rng(2)
    qpos, qvel, act = _states(blob, clip, n, rng, 0.002)
    a = np.clip(rng.normal(size=(38, n)) * 0.3, -1, 1).astype(np.float32)
    A, R = Emu(blob, n), GravEmu(blob)
    _fill(A, qpos, qvel, act)
    A.physics_wave(a, 2, True, dump=True)
    assert (A.rows("con_dist") < 0).sum() > 0 and np.isfinite(A.rows("qvel")).all()
    g0 = gravity_table([model_gravity(blob)], n)
    for scales, grav in ((np.ones((3, n), np.float32), None), (None, g0), (None, None), (np.ones((3, n), np.float32), g0)):
        B = Emu(blob, n)
        _fill(B, qpos, qvel, act)
        R.physics(B, a, 2, scales, grav, dump=True, chains=chains)
        assert np.array_equal(A.st.view(np.uint32), B.st.view(np.uint32)), (scales is None, grav is None)
        assert np.array_equal(A.ws.view(np.uint32), B.ws.view(np.uint32)), (scales is None, grav is None)


# ------------------------------------------------------------------------------------------------ C3
def test_domain_randomization_gravity_field():
    g = np.array([[0.0, 0.0, -9.81], [1.0, 0.0, -9.0], [0.0, -2.0, -4.0]])
    d = DomainRandomization(gravity=g)
    assert d.num_envs == 3 and d.gravity.dtype == np.float32 and np.array_equal(d.gravity, g.astype(np.float32)) and not d.has_scales
    assert d.gravity_table().shape == (3, 3) and np.array_equal(d.gravity_table(), g.astype(np.float32).T) and d.gravity_table().flags.c_contiguous
    assert d.table().tolist() == np.ones((3, 3)).tolist()                       # the scales' table is what it was
    assert DomainRandomization(friction=[0.5, 1.0, 2.0]).gravity is None and DomainRandomization(num_envs=2).gravity_table() is None
    # three positional arguments still are the three scales; equality of gravity-free instances is the tables'
    p = DomainRandomization([0.5, 1.0], [1.0, 1.5], [2.0, 1.0])
    assert p == DomainRandomization(friction=[0.5, 1.0], actuator=[1.0, 1.5], damping=[2.0, 1.0]) and p.gravity is None and p.has_scales
    assert DomainRandomization(num_envs=3) != d and d == DomainRandomization(gravity=g) and d != DomainRandomization(gravity=g * 0.5)
    both = DomainRandomization(friction=[0.5, 1.0, 2.0], gravity=g)
    assert both.has_scales and both != d and both != DomainRandomization(friction=[0.5, 1.0, 2.0])
    s = both.shard(1, 3)
    assert s.num_envs == 2 and np.array_equal(s.gravity, g[1:].astype(np.float32)) and s.friction.tolist() == [1.0, 2.0]
    assert not d.shard(0, 2).has_scales
    for bad in (np.zeros((3, 2)), np.zeros(3), np.zeros((0, 3)), np.full((3, 3), np.nan), np.full((3, 3), 1e60)):
        with pytest.raises(ValueError):
            DomainRandomization(gravity=bad)
    with pytest.raises(ValueError):
        DomainRandomization(friction=[1.0, 1.0], gravity=g)                    # lengths disagree
    with pytest.raises(ValueError):
        DomainRandomization(gravity=g, num_envs=4)
    with pytest.raises((ValueError, AttributeError)):
        d.gravity[0, 0] = 3.0                                                   # read-only
    assert "gravity" in repr(d) and "gravity" not in repr(p)


def test_uniform_scales_gravity_draw_is_behind_the_three_scales():
    key = jr.PRNGKey(7)
    g0 = np.array([0.0, 0.0, -9.81])
    kw = dict(friction=(0.5, 1.5), actuator=(0.8, 1.2), damping=(0.5, 2.0))
    a = uniform_scales(500, key, **kw, gravity_scale=(0.5, 1.5), gravity_tilt_deg=(0.0, 20.0), gravity=g0)
    plain = uniform_scales(500, key, **kw)
    assert np.array_equal(a.table(), plain.table()) and plain.gravity is None
    assert a == uniform_scales(500, np.array(key), **kw, gravity_scale=(0.5, 1.5), gravity_tilt_deg=(0.0, 20.0), gravity=g0)
    g = a.gravity.astype(np.float64)
    mag = np.linalg.norm(g, axis=1) / 9.81
    ang = np.degrees(np.arccos(np.clip(-g[:, 2] / np.linalg.norm(g, axis=1), -1, 1)))
    assert mag.min() >= 0.5 - 1e-6 and mag.max() <= 1.5 + 1e-6 and ang.max() <= 20.0 + 1e-4 and ang.max() - ang.min() > 15
    # the sub-keys: fold_in(key, 3) split in three — scale, tilt, azimuth
    ks, kt, ka = jr.split(jr.fold_in(key, 3), 3)
    want = _rand.gravity_vectors(g0, jr.uniform(ks, (500,), 0.5, 1.5), jr.uniform(kt, (500,), 0.0, 20.0), jr.uniform(ka, (500,), 0.0, 2 * np.pi))
    assert np.array_equal(a.gravity, want)
    # a tilt about a gravity that is not along -z keeps the angle to THAT vector
    gm = np.array([1.0, 2.0, -9.0])
    t = uniform_scales(200, key, gravity_tilt_deg=(10.0, 10.0), gravity=gm).gravity.astype(np.float64)
    cosang = (t @ gm) / (np.linalg.norm(t, axis=1) * np.linalg.norm(gm))
    assert np.allclose(np.degrees(np.arccos(cosang)), 10.0, atol=1e-3) and np.allclose(np.linalg.norm(t, axis=1), np.linalg.norm(gm), rtol=1e-6)
    for bad in dict(gravity_scale=(0.0, 1.0)), dict(gravity_scale=(2.0, 1.0)), dict(gravity_tilt_deg=(-1.0, 5.0)), dict(gravity_tilt_deg=(5.0, 1.0)), \
            dict(gravity_tilt_deg=(0.0, 120.0)), dict(gravity_scale="ab"), dict(gravity_tilt_deg=(1.0,)), dict(gravity_scale=(0.5, 1.5), gravity=(0, 0, 0)):
        with pytest.raises(ValueError):
            uniform_scales(4, key, **bad)


def test_train_config_parses_the_gravity_ranges(capsys):
    from track_mjx_amd import config as _config
    from track_mjx_amd import train as _train
    cfg = _config.load_config(None, [])
    dr = cfg["env_config"]["domain_randomization"]
    assert dr.get("gravity_scale_range") is None and dr.get("gravity_tilt_range") is None and _train.randomization_options(cfg) == {}
    cfg = _config.load_config(None, ["env_config.domain_randomization.gravity_scale_range=[0.5, 1.5]", "env_config.domain_randomization.gravity_tilt_range=[0, 15]"])
    fn = _train.randomization_options(cfg)["randomization_fn"]
    assert fn.ranges == {"friction": None, "actuator": None, "damping": None, "gravity_scale": (0.5, 1.5), "gravity_tilt_deg": (0.0, 15.0)}
    key = jr.PRNGKey(5)
    g0 = np.array([0.0, 0.0, -9.81])
    d = fn({"num_envs": 12, "gravity": g0}, key)
    assert d == uniform_scales(12, key, gravity_scale=(0.5, 1.5), gravity_tilt_deg=(0.0, 15.0), gravity=g0) and d.gravity.shape == (12, 3) and not d.has_scales
    with pytest.raises(ValueError, match="gravity"):
        fn({"num_envs": 12}, key)
    only = _train.randomization_options(_config.load_config(None, ["env_config.domain_randomization.gravity_tilt_range=[5, 5]"]))["randomization_fn"]
    assert only.ranges["gravity_tilt_deg"] == (5.0, 5.0) and "gravity_scale" not in only.ranges
    for key_, bad in (("gravity_scale_range", "[1.5, 0.5]"), ("gravity_scale_range", "[0, 1]"), ("gravity_scale_range", "3"),
                      ("gravity_tilt_range", "[-5, 5]"), ("gravity_tilt_range", "[10, 5]"), ("gravity_tilt_range", "[0, 100]")):
        with pytest.raises(ValueError):
            _train.randomization_options(_config.load_config(None, [f"env_config.domain_randomization.{key_}={bad}"]))
    with pytest.raises(ValueError, match="unknown keys"):
        _train.randomization_options(_config.load_config(None, ["env_config.domain_randomization.gravity_range=[0.5, 1.5]"]))

    def runner(cmd, env=None):
        return 0
    _train.main(["num_gpus=2", "env_config.domain_randomization.gravity_scale_range=[0.5,1.5]", "env_config.domain_randomization.gravity_tilt_range=[0,15]"], runner=runner)
    first = capsys.readouterr().out.splitlines()[0]
    assert first.startswith("[train] config=") and "gravity_scale=[0.5, 1.5]" in first and "gravity_tilt_deg=[0.0, 15.0]" in first


def test_shards_and_env_groups_carry_the_gravity():
    from track_mjx_amd.agent import ppo
    key_env, _ = _rand.randomization_keys(3)
    fn = uniform_randomization_fn(friction=(0.5, 1.5), gravity_scale=(0.5, 1.5), gravity_tilt_deg=(0.0, 20.0))
    total, world = 48, 4
    full = fn({"num_envs": total, "gravity": (0.0, 0.0, -9.81)}, key_env)
    for rank in range(world):
        lo, hi = ppo.shard_range(total, rank, world)
        sh = shard_scales(full, rank, world)
        assert np.array_equal(sh.gravity, full.gravity[lo:hi]) and np.array_equal(sh.table(), full.table()[:, lo:hi])
        assert np.array_equal(sh.gravity_table(), full.gravity_table()[:, lo:hi])
    local = shard_scales(full, 1, world)
    lo = 0
    for sz in ppo.group_sizes(local.num_envs, 3):
        assert np.array_equal(local.shard(lo, lo + sz).gravity, full.gravity[12 + lo:12 + lo + sz])
        lo += sz


def test_slope_formula_and_per_clip_values():
    from track_mjx_amd.analysis import rollout
    mag = 9.81
    g = rollout.slope_gravity(mag, 1.0, 0.0)
    assert g.dtype == np.float32 and g.tolist() == [0.0, 0.0, np.float32(-9.81)]
    g = rollout.slope_gravity(mag, [1.0, 0.5, 0.38], [15.0, 0.0, -10.0]).astype(np.float64)
    for row, (s, a) in zip(g, ((1.0, 15.0), (0.5, 0.0), (0.38, -10.0))):
        want = s * mag * np.array([np.sin(np.deg2rad(a)), 0.0, -np.cos(np.deg2rad(a))])
        assert np.array_equal(row, want.astype(np.float32).astype(np.float64))
        assert abs(np.linalg.norm(row) - s * mag) < 1e-5 and row[1] == 0 and row[2] < 0
        assert np.sign(row[0]) == np.sign(a)                 # a positive slope: +x is downhill (gravity has a +x component)
    for s, a in ((0.0, 0.0), (-1.0, 0.0), (1.0, 90.0), (1.0, float("nan"))):
        with pytest.raises(ValueError):
            rollout.slope_gravity(mag, s, a)
    assert rollout.parse_per_clip("slope_deg", "15", 3) == [15.0] and rollout.parse_per_clip("gravity_scale", "0.5,1,1.5", 3) == [0.5, 1.0, 1.5]
    assert rollout.parse_per_clip("slope_deg", "-5", 1) == [-5.0]
    for bad in ("1,2", "1,2,3,4", ""):
        with pytest.raises(ValueError, match="one value, or one per clip"):
            rollout.parse_per_clip("slope_deg", bad, 3)
    with pytest.raises(ValueError):
        rollout.parse_per_clip("slope_deg", "a", 1)
    assert {"gravity_scale", "slope_deg"} <= set(rollout.CLI_OPTIONS)


class _NoRand:
    """An environment without set_domain_randomization (what create_rollout_generator looks at before anything else)."""


def test_rollout_generator_refuses_before_any_launch():
    from track_mjx_amd.analysis import rollout

    class _Env:
        def set_domain_randomization(self, dr):
            raise AssertionError("nothing may be set")
    for kw in (dict(gravity_scale=0.5), dict(slope_deg=10.0), dict(gravity_scale=0.5, slope_deg=10.0)):
        with pytest.raises(NotImplementedError, match="log_sensor_data cannot be combined with gravity_scale / slope_deg"):
            rollout.create_rollout_generator({}, _Env(), None, log_sensor_data=True, **kw)
        with pytest.raises(NotImplementedError, match="no per-env gravity"):
            rollout.create_rollout_generator({}, _NoRand(), None, **kw)
    with pytest.raises(NotImplementedError, match="log_sensor_data cannot be combined with friction_scale"):          # (the scales' refusal keeps its words)
        rollout.create_rollout_generator({}, _Env(), None, log_sensor_data=True, friction_scale=0.5, gravity_scale=0.5)


# ------------------------------------------------------------------------------------------------ C4
def test_the_library_exports_tmjx_set_env_gravity():
    from track_mjx_amd import hip
    assert "tmjx_set_env_gravity" in hip.EXPORTS
    so = Path(hip.SO_PATH)
    assert so.exists(), f"{so} is not built"
    syms = subprocess.run(["nm", "-D", "--defined-only", str(so)], check=True, capture_output=True, text=True).stdout
    assert any(line.split()[-1] == "tmjx_set_env_gravity" for line in syms.splitlines() if line.strip())
    assert "int tmjx_set_env_gravity(tmjx_model *m, const float *gravity_dev, int n_env);" in (ROOT / "include" / "tmjx.h").read_text()
