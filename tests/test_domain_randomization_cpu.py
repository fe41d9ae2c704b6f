"""CPU: per-env domain randomisation (environment/randomization.py, the RAND build of csrc/wave_physics.h through tests/hostemu/rand_emu.*).

C1 validation of DomainRandomization / uniform_scales / the wrap dispatch; C2 the emulated RAND body against the oracle on blobs scaled on the
host; C3 unit scales = the plain body, bit for bit; C4 config plumbing and sharding of the global draw.  The same kernel source runs on the GPU
in tests/test_gpu_domain_randomization.py."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent / "hostemu"))
from emu import Emu  # noqa: E402
from rand_emu import RandEmu  # noqa: E402

from tests.common import default_blob, default_walker, make_oracle, rel_err  # noqa: E402
from tests.domain_rand_ref import TRIPLES_G1, scaled_blob, scales_table  # noqa: E402
from track_mjx_amd import clips as _clips  # noqa: E402
from track_mjx_amd import jax_random as jr  # noqa: E402
from track_mjx_amd.environment import DomainRandomization, shard_scales, uniform_randomization_fn, uniform_scales  # noqa: E402
from track_mjx_amd.environment import randomization as _rand  # noqa: E402

PHYS = ("qpos", "qvel", "act", "qacc_warmstart", "time")


@pytest.fixture(scope="module")
def setup():
    w, cfg = default_walker()
    blob = default_blob(w, cfg)
    clip = _clips.make_synthetic_clips(w.model, 4, seed=0)
    return w, blob, clip


_PLAIN_ORACLE = {}


def _states(clip, n, rng, pen):
    """Clip poses lowered until the nearest paw contacts penetrate the floor by `pen` .. 3 `pen` (the float64 oracle's con_dist says by how
    much), with joint and root velocities and non-zero activations: states on which friction, actuator strength and damping all act."""
    if "O" not in _PLAIN_ORACLE:
        w, cfg = default_walker()
        _PLAIN_ORACLE["O"] = make_oracle(default_blob(w, cfg), clip, "f64")
    O = _PLAIN_ORACLE["O"]
    qpos = np.zeros((n, 74)); qvel = rng.uniform(-0.5, 0.5, size=(n, 73))
    for e in range(n):
        c, f = e % 4, (7 * e) % 44
        qpos[e] = np.concatenate([clip.position[c, f], clip.quaternion[c, f], clip.joints[c, f]]) + rng.uniform(-1e-3, 1e-3, 74)
        d = O.new_data(qpos[e], np.zeros(73)); O.forward(d)
        qpos[e, 2] -= O.get(d, "con_dist").min() + pen * (1 + e % 3)
    qvel[:, :2] = rng.uniform(0.1, 0.3, size=(n, 2))          # tangential velocity of the paws on the floor
    act = rng.uniform(-0.3, 0.3, size=(n, 38))
    return qpos, qvel, act


# ------------------------------------------------------------------------------------------------ C1
def test_domain_randomization_validation():
    d = DomainRandomization(friction=[0.5, 1.0, 2.0])
    assert d.num_envs == 3 and d.table().shape == (3, 3) and d.table().dtype == np.float32
    assert np.array_equal(d.table()[1:], np.ones((2, 3), np.float32))
    assert DomainRandomization(num_envs=4).table().tolist() == np.ones((3, 4)).tolist()
    for bad in ([1.0, 0.0], [1.0, -0.5], [1.0, float("nan")], [1.0, float("inf")], [[1.0, 1.0]], []):
        for name in ("friction", "actuator", "damping"):
            with pytest.raises(ValueError):
                DomainRandomization(**{name: bad})
    with pytest.raises(ValueError):
        DomainRandomization(friction=[1.0, 1.0], damping=[1.0, 1.0, 1.0])       # lengths disagree
    with pytest.raises(ValueError):
        DomainRandomization(friction=[1.0, 1.0], num_envs=3)
    with pytest.raises(ValueError):
        DomainRandomization()
    with pytest.raises(ValueError):
        DomainRandomization(friction=[1e-60, 1.0])           # underflows float32 to 0
    with pytest.raises((ValueError, AttributeError)):
        d.friction[0] = 3.0                                   # read-only


def test_uniform_scales_reproducible_and_in_range():
    key = jr.PRNGKey(7)
    a = uniform_scales(1000, key, friction=(0.5, 1.5), actuator=(0.8, 1.2), damping=(0.5, 2.0))
    b = uniform_scales(1000, np.array(key), friction=(0.5, 1.5), actuator=(0.8, 1.2), damping=(0.5, 2.0))
    assert a == b and np.array_equal(a.table(), b.table())
    for row, (lo, hi) in zip(a.table(), ((0.5, 1.5), (0.8, 1.2), (0.5, 2.0))):
        assert row.min() >= np.float32(lo) and row.max() <= np.float32(hi)
        assert row.max() - row.min() > 0.9 * (hi - lo)        # a thousand draws fill the range
    assert uniform_scales(1000, jr.PRNGKey(8), friction=(0.5, 1.5)) != uniform_scales(1000, key, friction=(0.5, 1.5))
    # a scale that is not drawn stays 1 and does not move the others' draws
    f_only = uniform_scales(1000, key, friction=(0.5, 1.5))
    assert np.array_equal(f_only.friction, a.friction) and (f_only.actuator == 1).all() and (f_only.damping == 1).all()
    # the draw is jax.random.uniform of the sub-key
    assert np.array_equal(a.damping, jr.uniform(jr.split(key, 3)[2], (1000,), 0.5, 2.0))
    assert uniform_scales(5, 3, damping=(2.0, 2.0)).damping.tolist() == [2.0] * 5
    for bad in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0, float("inf")), (1.0,), "ab"):
        with pytest.raises(ValueError):
            uniform_scales(4, key, friction=bad)
    with pytest.raises(ValueError):
        uniform_scales(0, key, friction=(0.5, 1.5))


class _FakeEnv:
    """What wrap's dispatch touches of an env (no GPU): the blob, num_envs, set_domain_randomization."""

    def __init__(self, blob, n):
        self._blob, self.num_envs, self.applied = blob, n, None

    def set_domain_randomization(self, dr):
        self.applied = dr


def test_wrap_dispatch(setup):
    _, blob, _ = setup
    env = _FakeEnv(blob, 6)
    seen = {}

    def fn(model):
        seen["model"] = model
        return DomainRandomization(friction=np.full(model["num_envs"], 0.5))
    _rand.apply_randomization_fn(env, fn)
    assert env.applied.num_envs == 6 and (env.applied.friction == 0.5).all()
    m = seen["model"]
    assert m["num_envs"] == 6 and {"con_friction", "act_gain", "dof_damping"} <= set(m)
    with pytest.raises(TypeError):
        m["num_envs"] = 7                                   # read-only mapping
    with pytest.raises(ValueError):
        m["dof_damping"][0] = 1.0
    for ret in (lambda m: m, lambda m: (m, None), lambda m: None, lambda m: np.ones((3, 6))):
        env.applied = None
        with pytest.raises(NotImplementedError, match="per-env model.*SCALES"):
            _rand.apply_randomization_fn(env, ret)
        assert env.applied is None


# ------------------------------------------------------------------------------------------------ C2
@pytest.mark.parametrize("chains", [True, False], ids=["chain-layout", "generic-layout"])
def test_rand_emu_against_the_oracle_on_scaled_blobs(setup, chains):
    """8 envs, 4 distinct triples (two envs each, (1, 1, 1) among them), 2 teacher-forced substeps: the emulated RAND body with per-env scales
    against the float64 oracle created from the blob scaled on the host, under the bounds tests/test_hostemu_parity.py::test_substeps_teacher_forced
    holds the plain emulated body to (its "wave" bounds for the chain layout, its "wave-generic" bounds for the generic one)."""
    w, blob, clip = setup
    n, per = 8, 2
    table = scales_table(TRIPLES_G1, per)
    E, R = Emu(blob, n), RandEmu(blob)
    O32 = [make_oracle(scaled_blob(blob, *t), clip, "f32") for t in TRIPLES_G1]
    O64 = [make_oracle(scaled_blob(blob, *t), clip, "f64") for t in TRIPLES_G1]
    rng = np.random.default_rng(1)
    qpos, qvel, act = _states(clip, n, rng, 0.002)
    d32, d64 = [], []
    for e in range(n):
        for O, ds in ((O32[e // per], d32), (O64[e // per], d64)):
            d = O.new_data(qpos[e], qvel[e]); O.set(d, "act", act[e]); ds.append(d)
    acc = {k: ([], []) for k in ("qpos", "qvel")}
    for sub in range(2):
        a = np.clip(rng.normal(size=(n, 38)) * 0.3, -1, 1)
        for k in PHYS:
            v = np.stack([O64[e // per].get(d64[e], k) for e in range(n)], 1)
            E.rows(k)[:] = v
            for e in range(n):
                O32[e // per].set(d32[e], k, v[:, e])
        R.physics(E, a.T.astype(np.float32).copy(), 1, table, dump=False, chains=chains)
        for e in range(n):
            O32[e // per].step(d32[e], a[e]); O64[e // per].step(d64[e], a[e])
        for k in ("qpos", "qvel"):
            ref = np.stack([O64[e // per].get(d64[e], k) for e in range(n)], 1)
            r32 = np.stack([O32[e // per].get(d32[e], k) for e in range(n)], 1)
            e_emu, e_32 = rel_err(E.rows(k), ref, axis=0), rel_err(r32, ref, axis=0)
            acc[k][0].append(e_emu); acc[k][1].append(e_32)
            print(f"substep {sub} {k}: emu {e_emu}, f32 oracle {e_32}")
            assert np.median(e_emu) <= 1e-5, (sub, k, e_emu)
    for k in ("qpos", "qvel"):
        g, f = np.concatenate(acc[k][0]), np.concatenate(acc[k][1])
        print(f"{k}: median {np.median(g):.3e} / {np.median(f):.3e}, q90 {np.quantile(g, 0.9):.3e} / {np.quantile(f, 0.9):.3e}, max {g.max():.3e} / {f.max():.3e}")
        assert np.median(g) <= (1.25 if chains else 4.0) * np.median(f) + 1e-7, (k, np.median(g), np.median(f))
        assert np.quantile(g, 0.9) <= (2.0 if chains else 4.0) * np.quantile(f, 0.9) + 1e-5, (k, np.quantile(g, 0.9), np.quantile(f, 0.9))
        assert g.max() <= 4 * f.max() + (1e-4 if k == "qvel" else 2e-5), (k, g.max(), f.max())
    assert sum((O64[e // per].get(d64[e], "con_dist") < 0).sum() for e in range(n)) > 0, "the states must reach contact"


# ------------------------------------------------------------------------------------------------ C3
@pytest.mark.parametrize("chains", [True, False], ids=["chain-layout", "generic-layout"])
def test_rand_emu_at_unit_scale_is_the_plain_body(setup, chains, monkeypatch):
    w, blob, clip = setup
    if not chains:
        monkeypatch.setenv("TMJX_EMU_GENERIC", "1")
    n = 8
    A, B, R = Emu(blob, n), Emu(blob, n), RandEmu(blob)
    rng = np.random.default_rng(2)
    qpos, qvel, act = _states(clip, n, rng, 0.002)
    for X in (A, B):
        X.rows("qpos")[:] = qpos.T; X.rows("qvel")[:] = qvel.T; X.rows("act")[:] = act.T
    a = np.clip(rng.normal(size=(38, n)) * 0.3, -1, 1).astype(np.float32)
    A.physics_wave(a, 2, True, dump=True)
    R.physics(B, a, 2, np.ones((3, n), np.float32), dump=True, chains=chains)
    assert (A.rows("con_dist") < 0).sum() > 0
    assert np.array_equal(A.st.view(np.uint32), B.st.view(np.uint32))
    assert np.array_equal(A.ws.view(np.uint32), B.ws.view(np.uint32))      # every dumped intermediate too (efc_D: the re-formed contact weight)


@pytest.mark.parametrize("chains", [True, False], ids=["chain-layout", "generic-layout"])
def test_rand_emu_power_of_two_scales_equal_the_prescaled_model(setup, chains, monkeypatch):
    """"Scale the constant first": with scales from {0.5, 1, 2} every scaled constant is exact, and the RAND body reproduces, bit for bit, the
    plain body on a model whose blob was scaled on the host — per env, so the per-env indexing (with an e0 offset into a longer table) is
    checked with it.  Each scale moves the result."""
    w, blob, clip = setup
    if not chains:
        monkeypatch.setenv("TMJX_EMU_GENERIC", "1")
    triples = [(0.5, 1, 1), (1, 2, 1), (1, 1, 0.5), (2, 0.5, 2), (0.5, 0.5, 0.5), (2, 2, 2), (1, 0.5, 2), (2, 1, 0.5)]
    n, e0 = len(triples), 3
    table = np.full((3, e0 + n + 2), 7.0, np.float32)          # (the columns outside e0 .. e0 + n must not be read)
    table[:, e0:e0 + n] = np.asarray(triples, np.float32).T
    rng = np.random.default_rng(3)
    qpos, qvel, act = _states(clip, n, rng, 0.002)
    a = np.clip(rng.normal(size=(38, n)) * 0.3, -1, 1).astype(np.float32)
    B, R = Emu(blob, n), RandEmu(blob)
    B.rows("qpos")[:] = qpos.T; B.rows("qvel")[:] = qvel.T; B.rows("act")[:] = act.T
    R.physics(B, a, 2, table, e0=e0, dump=False, chains=chains)
    P = Emu(blob, n)
    P.rows("qpos")[:] = qpos.T; P.rows("qvel")[:] = qvel.T; P.rows("act")[:] = act.T
    P.physics_wave(a, 2, True, dump=False)
    for e, t in enumerate(triples):
        A = Emu(scaled_blob(blob, *t), 1)
        A.rows("qpos")[:, 0] = qpos[e]; A.rows("qvel")[:, 0] = qvel[e]; A.rows("act")[:, 0] = act[e]
        A.physics_wave(a[:, e:e + 1].copy(), 2, True, dump=False)
        for k in PHYS:
            assert np.array_equal(A.rows(k)[:, 0].view(np.uint32), B.rows(k)[:, e].view(np.uint32)), (e, t, k)
        assert not np.array_equal(P.rows("qvel")[:, e], B.rows("qvel")[:, e]), (e, t)


def test_each_scale_alone_moves_the_emulated_result(setup):
    """Friction, actuator and damping each change qvel on states with sliding contacts, activations and joint velocities (a body that ignored one
    of them would pass the parity tests of the groups it does honour)."""
    w, blob, clip = setup
    n = 4
    rng = np.random.default_rng(4)
    qpos, qvel, act = _states(clip, n, rng, 0.002)
    a = np.clip(rng.normal(size=(38, n)) * 0.3, -1, 1).astype(np.float32)
    R = RandEmu(blob)
    out = []
    for t in ((1, 1, 1), (0.6, 1, 1), (1, 0.7, 1), (1, 1, 1.8)):
        E = Emu(blob, n)
        E.rows("qpos")[:] = qpos.T; E.rows("qvel")[:] = qvel.T; E.rows("act")[:] = act.T
        R.physics(E, a, 1, scales_table([t], n), dump=False)
        out.append(E.rows("qvel").copy())
    for k in (1, 2, 3):
        assert rel_err(out[k], out[0]) > 1e-4, k


# ------------------------------------------------------------------------------------------------ C4
def test_train_config_parses_the_ranges():
    from track_mjx_amd import config as _config
    from track_mjx_amd import train as _train
    cfg = _config.load_config(None, [])
    assert cfg["env_config"]["domain_randomization"] == {"friction_range": None, "actuator_range": None, "damping_range": None}
    assert _train.randomization_options(cfg) == {}
    cfg = _config.load_config(None, ["env_config.domain_randomization.friction_range=[0.5, 1.5]", "env_config.domain_randomization.damping_range=[1.0, 2.0]"])
    fn = _train.randomization_options(cfg)["randomization_fn"]
    assert fn.ranges == {"friction": (0.5, 1.5), "actuator": None, "damping": (1.0, 2.0)}
    key = jr.PRNGKey(5)
    d = fn({"num_envs": 12}, key)
    assert d == uniform_scales(12, key, friction=(0.5, 1.5), damping=(1.0, 2.0)) and (d.actuator == 1).all()
    for bad in ("[1.5, 0.5]", "[0, 1]", "3"):
        with pytest.raises(ValueError):
            _train.randomization_options(_config.load_config(None, [f"env_config.domain_randomization.actuator_range={bad}"]))
    with pytest.raises(ValueError, match="unknown keys"):
        _train.randomization_options(_config.load_config(None, ["env_config.domain_randomization.mass_range=[0.5, 1.5]"]))


def test_train_first_log_line_prints_the_ranges(capsys):
    from track_mjx_amd import train as _train

    def runner(cmd, env=None):          # num_gpus=2 on this box: main() prints its first lines, then hands the ranks to the runner
        return 0
    _train.main(["num_gpus=2", "env_config.domain_randomization.friction_range=[0.5,1.5]"], runner=runner)
    first = capsys.readouterr().out.splitlines()[0]
    assert first.startswith("[train] config=") and "domain_randomization friction=[0.5, 1.5] actuator=off damping=off" in first
    _train.main(["num_gpus=2"], runner=runner)
    assert "domain_randomization" not in capsys.readouterr().out.splitlines()[0]


def test_a_rank_takes_its_shard_of_the_one_global_draw():
    from track_mjx_amd.agent import ppo
    key_env, eval_key = _rand.randomization_keys(3)
    assert not np.array_equal(key_env, eval_key)
    assert all(np.array_equal(a, b) for a, b in zip(_rand.randomization_keys(3), (key_env, eval_key)))         # from the seed alone: resume, every rank
    assert not np.array_equal(_rand.randomization_keys(4)[0], key_env)
    fn = uniform_randomization_fn(friction=(0.5, 1.5), actuator=(0.7, 1.3), damping=(0.5, 2.0))
    total, world = 48, 4
    full = fn({"num_envs": total}, key_env)
    for rank in range(world):
        lo, hi = ppo.shard_range(total, rank, world)
        assert np.array_equal(shard_scales(full, rank, world).table(), full.table()[:, lo:hi])
    # ... and an env group its slice of the rank's shard
    local = shard_scales(full, 1, world)
    sizes = ppo.group_sizes(local.num_envs, 3)
    lo = 0
    for sz in sizes:
        assert np.array_equal(local.shard(lo, lo + sz).table(), full.table()[:, 12 + lo:12 + lo + sz])
        lo += sz
    with pytest.raises(ValueError):
        shard_scales(full, 0, 5)
    assert shard_scales(None, 0, 2) is None
