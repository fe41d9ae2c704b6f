"""CPU: the position-actuator, 0.8-scale rodent of the reference's rodent-sps-per-actor.yaml (walker_config.torque_actuators: False,
rescale_factor: 0.8) — model compiler (affine-bias mode), committed blob, walker table, configuration, and the product kernel body
(csrc/wave_physics.h, host emulation) against the unmodified float64 oracle with the bias substituted into the activation
(tests/affine_bias.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests" / "hostemu"))
import compile_model as cm  # noqa: E402
from emu import Emu  # noqa: E402

from tests.affine_bias import Actuation, collect, oracle_substep, position_config, position_walker  # noqa: E402
from tests.common import PHYS_ROWS, assert_substep_sample_bounds, default_blob, make_oracle, rel_err  # noqa: E402
from tests.test_model_compiler import TOY  # noqa: E402
from track_mjx_amd import blob as _blob  # noqa: E402
from track_mjx_amd import clips as _clips  # noqa: E402
from track_mjx_amd import walker as _walker  # noqa: E402

ASSETS = ROOT / "track_mjx_amd" / "assets"
XML = Path(cm.DEFAULT_XML)
needs_xml = pytest.mark.skipif(not XML.exists(), reason="the reference's rodent.xml is not present")


@pytest.fixture(scope="module")
def toy_xml(tmp_path_factory):
    p = tmp_path_factory.mktemp("toy_affine") / "toy.xml"
    p.write_text(TOY)
    return p


# ------------------------------------------------------------------------------------------------ compiler
def test_compiler_affine_mode_on_the_toy(toy_xml):
    s = 0.8
    m = cm.compile_model(str(toy_xml), torque_actuators=False, rescale_factor=s, affine_bias=True)
    np.testing.assert_array_equal(m["act_gain"], [3.0, 1.0])                       # gainprm[0] as written
    np.testing.assert_array_equal(m["act_bias"], [[0, -3, 0], [0, -1, 0]])         # biasprm[0:3]
    nz = [(a, d, v) for a in range(2) for d, v in enumerate(m["act_moment"][a]) if v]
    assert [(a, d) for a, d, _ in nz] == [(0, 6), (1, 7)]
    np.testing.assert_allclose([v for *_, v in nz], [2 * s * s, 1.5 * s * s], rtol=1e-15)   # gear x s^2
    e = cm.to_blob(m)
    assert "act_bias" in e and e["act_bias"].shape == (6,)


def test_compiler_torque_mode_has_no_bias_and_plain_no_torque_still_refused(toy_xml):
    m = cm.compile_model(str(toy_xml), torque_actuators=True, rescale_factor=1.0)
    assert "act_bias" not in m and "act_bias" not in cm.to_blob(m)
    with pytest.raises(AssertionError):
        cm.compile_model(str(toy_xml), torque_actuators=False, rescale_factor=1.0)


@pytest.mark.parametrize("edit", [('biasprm="0 -3 0"', 'biasprm="0 -3 0.5"'), ('gainprm="3"', 'gainprm="3 0.1"')],
                         ids=["biasprm2", "gainprm1"])
def test_compiler_refuses_what_the_bias_path_does_not_compute(tmp_path, edit):
    p = tmp_path / "toy.xml"
    p.write_text(TOY.replace(*edit))
    with pytest.raises(AssertionError):
        cm.compile_model(str(p), torque_actuators=False, rescale_factor=1.0, affine_bias=True)


def test_compiler_refuses_a_moment_on_the_free_joint(tmp_path):
    p = tmp_path / "toy.xml"
    p.write_text(TOY.replace('joint="elbow" gear="2"', 'joint="root" gear="2"'))
    with pytest.raises(AssertionError):
        cm.compile_model(str(p), torque_actuators=False, rescale_factor=1.0, affine_bias=True)


@needs_xml
@pytest.mark.parametrize("fname,args", [("rodent_model.tmjx", []),
                                        ("rodent_model_pos080.tmjx.txt", ["--no-torque", "--rescale", "0.8", "--affine-bias"])])
def test_committed_blobs_regenerate_byte_identically(tmp_path, fname, args):
    import subprocess
    out = tmp_path / fname
    subprocess.run([sys.executable, str(ROOT / "tools" / "compile_model.py"), "--out", str(out), *args], check=True, capture_output=True)
    stem = _blob.stem(fname)
    for name in (fname, f"{stem}.names.txt", f"{stem}_dump.txt"):
        assert (tmp_path / name).read_bytes() == (ASSETS / name).read_bytes(), name


@needs_xml
def test_text_blob_packs_to_the_compilers_binary_blob(tmp_path):
    """The committed text form of the 0.8 blob is lossless: packed, it is byte for byte the binary blob the compiler writes."""
    import subprocess
    out = tmp_path / "pos080.tmjx"
    subprocess.run([sys.executable, str(ROOT / "tools" / "compile_model.py"), "--out", str(out), "--no-torque", "--rescale", "0.8", "--affine-bias"],
                   check=True, capture_output=True)
    assert _blob.pack(_blob.load(ASSETS / "rodent_model_pos080.tmjx.txt")) == out.read_bytes()


def test_text_blob_round_trip():
    e = _blob.load(ASSETS / "rodent_model.tmjx")
    back = _blob.from_text(_blob.to_text(e))
    assert list(back) == list(e) and _blob.pack(back) == _blob.pack(e)
    assert _blob.stem("a/b/rodent_model_pos080.tmjx.txt") == "rodent_model_pos080" and _blob.stem("rodent_model.tmjx") == "rodent_model"


@needs_xml
def test_pos080_blob_actuators_against_the_xml():
    """gainprm / biasprm / gear of every actuator as rodent.xml writes them (tests/golden/rodent_xml_actuators.npz, read with ElementTree by
    tests/golden/make_rodent_xml_actuators.py), against the committed 0.8 blob; body positions below `walker` are 0.8 x the XML's."""
    X = np.load(ROOT / "tests" / "golden" / "rodent_xml_actuators.npz")
    w, _ = position_walker()
    A = Actuation(w.model)
    assert [n for n, _ in sorted(w.names["actuator"].items(), key=lambda t: t[1])] == X["actuator_name"].tolist()
    assert (X["actuator_biastype"] == "affine").all()
    np.testing.assert_array_equal(A.gain, X["actuator_gainprm"][:, 0])
    assert not X["actuator_gainprm"][:, 1:].any()
    np.testing.assert_array_equal(np.stack([A.b0, A.b1, A.b2], 1), X["actuator_biasprm"])
    s2 = 0.8 * 0.8
    for a, (tgt, ten) in enumerate(zip(X["actuator_target"], X["actuator_is_tendon"])):
        if not ten:
            d = int(np.asarray(w.model["jnt_dofadr"])[w.names["joint"][tgt]])
            nz = np.nonzero(A.moment[a])[0]
            assert nz.tolist() == [d], (tgt, nz)
            np.testing.assert_allclose(A.moment[a, d], X["actuator_gear"][a] * s2, rtol=1e-15)
        else:
            assert len(np.nonzero(A.moment[a])[0]) >= 2
    # the 0.9 torque blob and the 0.8 position blob share the tendon coefficients: moments differ by the gear scale only
    w9 = _walker.Rodent(**{**position_config()["walker_config"], "torque_actuators": True, "rescale_factor": 0.9})
    np.testing.assert_allclose(A.moment, Actuation(w9.model).moment * (s2 / 0.81), rtol=1e-12)
    Xb = np.load(ROOT / "tests" / "golden" / "rodent_xml.npz")
    pos = dict(zip(Xb["body_name"].tolist(), Xb["body_pos"]))
    bp = np.asarray(w.model["body_pos"]).reshape(-1, 3)
    below = False
    checked = 0
    for name, i in sorted(w.names["body"].items(), key=lambda t: t[1]):
        if name == "walker":
            below = True
            continue
        if below and name in pos:
            np.testing.assert_allclose(bp[i], 0.8 * pos[name], rtol=1e-12, atol=1e-15)
            checked += 1
    assert checked > 60


# ------------------------------------------------------------------------------------------------ walker / configuration
def test_walker_table_and_attributes():
    w, cfg = position_walker()
    assert (w.torque_actuators, w.rescale_factor, w.actuator_mode) == (False, 0.8, "position")
    assert w.blob_path.name == "rodent_model_pos080.tmjx.txt" and "act_bias" in w.model
    assert "position actuators" in w.describe() and "0.8" in w.describe() and "rodent_model_pos080.tmjx.txt" in w.describe()
    w9 = _walker.Rodent(**{**cfg["walker_config"], "torque_actuators": True, "rescale_factor": 0.9})
    assert w9.actuator_mode == "torque" and w9.blob_path.name == "rodent_model.tmjx" and "act_bias" not in w9.model
    for tq, s in ((False, 0.9), (True, 0.8), (False, 1.0)):
        with pytest.raises(NotImplementedError, match="compile_model.py"):
            _walker.Rodent(**{**cfg["walker_config"], "torque_actuators": tq, "rescale_factor": s})


def test_sps_per_actor_config_with_the_walker_overrides():
    cfg = position_config()
    assert cfg["walker_config"]["torque_actuators"] is False and cfg["walker_config"]["rescale_factor"] == 0.8
    assert cfg["env_config"]["env_args"]["physics_steps_per_control_step"] == 5      # the rest of the named configuration is kept
    from track_mjx_amd import config as _config
    assert _config.named_config("rodent-sps-per-actor")["walker_config"]["torque_actuators"] is True     # its default is unchanged


# ------------------------------------------------------------------------------------------------ host loader
def _blob_with(w, cfg, **entries):
    e = dict(_blob.unpack(default_blob(w, cfg)))
    e.update(entries)
    return _blob.pack(e)


def test_loader_rejects_malformed_bias():
    w, cfg = position_walker()
    b = np.asarray(w.model["act_bias"], np.float64).copy()
    with pytest.raises(RuntimeError, match="act_bias"):
        Emu(_blob_with(w, cfg, act_bias=b[:-3]), 1)
    b2 = b.copy(); b2[2] = 0.1
    with pytest.raises(RuntimeError, match="biasprm"):
        Emu(_blob_with(w, cfg, act_bias=b2), 1)
    Emu(default_blob(w, cfg), 1)                                  # the committed blob loads


# ------------------------------------------------------------------------------------------------ kernel body (host emulation)
def _start_states(w, clip, n, rng):
    nq, nv, nu = w.nq, w.nv, w.nu
    qpos = np.zeros((nq, n)); qvel = rng.uniform(-1e-2, 1e-2, size=(nv, n)); act = rng.uniform(-0.3, 0.3, size=(nu, n))
    for e in range(n):
        c, f = e % clip.position.shape[0], (7 * e) % 44
        qpos[:, e] = np.concatenate([clip.position[c, f], clip.quaternion[c, f], clip.joints[c, f]]) + rng.uniform(-1e-3, 1e-3, nq)
        qpos[2, e] -= 0.001 * (e % 5)
    return {"qpos": qpos, "qvel": qvel, "act": act, "qacc_warmstart": np.zeros((nv, n)), "time": np.zeros((1, n))}


@pytest.mark.parametrize("generic", [False, True], ids=["chain", "generic"])
def test_hostemu_substeps_against_the_substituted_oracle(generic, monkeypatch):
    """The product kernel body, teacher-forced one substep at a time at three action scales, against the float64 oracle with the bias
    substituted into act (bounds of assert_substep_sample_bounds); qfrc_actuator against the numpy restatement; act against the filter."""
    if generic:
        monkeypatch.setenv("TMJX_EMU_GENERIC", "1")
    w, cfg = position_walker()
    blob = default_blob(w, cfg)
    A = Actuation(w.model)
    h = cfg["env_config"]["env_args"]["mj_model_timestep"]
    clip = _clips.make_synthetic_clips(w.model, 4, seed=0)
    n = 12
    E = Emu(blob, n); O32 = make_oracle(blob, clip, "f32"); O64 = make_oracle(blob, clip, "f64")
    rng = np.random.default_rng(5)
    errs = {k: ([], []) for k in ("qpos", "qvel")}
    for scale in (0.03, 0.3, 1.0):
        st = _start_states(w, clip, n, rng)
        for k in PHYS_ROWS:
            E.rows(k)[:] = st[k]
        for sub in range(4):
            st = {k: E.rows(k).astype(np.float64) for k in PHYS_ROWS}
            a = np.clip(rng.normal(size=(w.nu, n)) * scale, -1, 1).astype(np.float32)
            E.physics_wave(a, 1, True, dump=False)
            np.testing.assert_allclose(E.rows("qfrc_actuator"), A.qfrc_actuator(st["act"], st["qpos"]), rtol=1e-5,
                                       atol=1e-5 * np.abs(A.qfrc_actuator(st["act"], st["qpos"])).max())
            np.testing.assert_allclose(E.rows("act"), A.next_act(st["act"], a, h), rtol=1e-6, atol=1e-7)
            for e in range(n):
                s1 = {k: v[:, e] for k, v in st.items()}
                collect(errs, {k: E.rows(k)[:, e] for k in ("qpos", "qvel")},
                        oracle_substep(O64, A, s1, a[:, e]), oracle_substep(O32, A, s1, a[:, e]))
    errs = {k: (np.array(v[0]), np.array(v[1])) for k, v in errs.items()}
    if not generic:
        assert_substep_sample_bounds(errs, min_samples=140)
        return
    # the generic path's plain float32 leaf -> root factorisation sits ~3 x above the float32 oracle on the torque walker as well: the
    # generic bounds of tests/test_hostemu_parity.py::test_substeps_teacher_forced
    for k, (g, f) in errs.items():
        assert len(g) >= 140 and np.isfinite(g).all(), k
        assert np.median(g) <= 1e-5 and np.median(g) <= 4.0 * np.median(f) + 1e-7, (k, np.median(g), np.median(f))
        assert np.quantile(g, 0.9) <= 4.0 * np.quantile(f, 0.9) + 1e-5, (k, np.quantile(g, 0.9), np.quantile(f, 0.9))
        assert g.max() <= 4 * f.max() + 1e-4, (k, g.max(), f.max())


def test_substitution_is_needed():
    """The bias is not small: without it the oracle's substep lands far from the kernel's (the check above would catch a missing bias)."""
    w, cfg = position_walker()
    blob = default_blob(w, cfg)
    A = Actuation(w.model)
    clip = _clips.make_synthetic_clips(w.model, 4, seed=0)
    st = _start_states(w, clip, 4, np.random.default_rng(2))
    f_bias, f_plain = A.qfrc_actuator(st["act"], st["qpos"]), A.moment.T @ (A.gain[:, None] * st["act"])
    assert rel_err(f_plain, f_bias) > 0.05
    E = Emu(blob, 4)
    for k in PHYS_ROWS:
        E.rows(k)[:] = st[k]
    E.physics_wave(np.zeros((w.nu, 4), np.float32), 1, True, dump=False)
    assert rel_err(E.rows("qfrc_actuator"), f_plain) > 0.05
