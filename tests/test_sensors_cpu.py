"""CPU: sensor readings and contact forces of checkpoint roll-outs (log_sensor_data) — the model compiler's sensor entries, the recording kernel's
sensor stage (csrc/wave_physics.h: tmw_sensor_stage) under host emulation against a float64 numpy restatement (tests/sensor_ref.py), that the
stage does not perturb the physics, and the at-rest invariants of the readings."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "hostemu"))
sys.path.insert(0, str(ROOT / "tools"))
from emu import Emu  # noqa: E402
from sensors_emu import SensorEmu  # noqa: E402

import compile_model as cm  # noqa: E402
from tests import sensor_ref as SR  # noqa: E402
from tests.common import default_blob, default_walker, make_oracle  # noqa: E402
from track_mjx_amd import blob as _blob  # noqa: E402
from track_mjx_amd import clips as _clips  # noqa: E402

XML = Path(cm.DEFAULT_XML)
needs_xml = pytest.mark.skipif(not XML.exists(), reason="the reference's rodent.xml is not on this machine")

TOY = """<mujoco>
  <compiler angle="radian"/>
  <option gravity="0 0 -9.81"/>
  <default><default class="sensor"><site group="4"/></default></default>
  <worldbody>
    <body name="floor"><geom name="floor" type="plane" size="10 10 0.1" contype="1" conaffinity="1"/></body>
    <body name="walker" pos="0 0 0.2">
      <freejoint name="root"/>
      <body name="torso" pos="0.01 0 0">
        <geom type="sphere" size="0.02" contype="0" conaffinity="0"/>
        <body name="arm" pos="0.03 0.01 0">
          <joint name="j0" axis="0 1 0" range="-1 1"/>
          <geom type="capsule" size="0.005 0.01" pos="0 0 -0.01" contype="0" conaffinity="0"/>
          <site name="tip" class="sensor" pos="0.004 -0.002 0.006" euler="0.3 -0.2 0.5"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <general name="a0" joint="j0" dyntype="filter" dynprm="0.04" gainprm="0.1" ctrllimited="true" ctrlrange="-1 1" forcerange="-0.1 0.1"/>
  </actuator>
  <sensor>
    <velocimeter name="vel" site="tip"/>
    <subtreelinvel name="torso_v" body="torso"/>
    <accelerometer name="acc" site="tip"/>
    <gyro name="gyr" site="tip"/>
  </sensor>
</mujoco>
"""


def _toy(tmp_path, text=TOY):
    p = tmp_path / "toy.xml"
    p.write_text(text)
    return p


def test_compiler_sensor_entries(tmp_path):
    m1 = cm.compile_model(_toy(tmp_path), torque_actuators=True, rescale_factor=1.0)
    m2 = cm.compile_model(_toy(tmp_path), torque_actuators=True, rescale_factor=0.5)
    e = cm.sensor_entries(m2)
    assert not set(e) & set(cm.to_blob(m2)), "the model blob itself carries no sensor entries"
    assert m2["sensor_names"] == ["vel", "torso_v", "acc", "gyr"] and m2["site_names"] == ["tip"]
    arm = m2["body_names"].index("arm")
    assert e["sensor_type"].tolist() == [1, 3, 0, 2]
    assert e["sensor_objid"].tolist() == [0, m2["body_names"].index("torso"), 0, 0]
    assert e["sensor_adr"].tolist() == [0, 3, 6, 9] and m2["nsensordata"] == 12
    assert e["site_bodyid"].tolist() == [arm]
    # rescale scales body positions (dm_scale_spec) but not site positions
    np.testing.assert_allclose(m2["body_pos"][arm], 0.5 * m1["body_pos"][arm], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(e["site_pos"], [0.004, -0.002, 0.006])
    np.testing.assert_allclose(e["site_quat"], cm.euler_to_quat([0.3, -0.2, 0.5]), rtol=0, atol=1e-15)
    assert list(e) == ["site_bodyid", "site_pos", "site_quat", "sensor_type", "sensor_objid", "sensor_adr"]


def test_compiler_writes_the_sensor_side_file(tmp_path):
    """compile_model.py --out <stem>.tmjx writes the model blob without sensor entries and <stem>.sensors.tmjx.txt with them; a model
    without a <sensor> block gets no side file."""
    import subprocess
    xml = _toy(tmp_path)
    subprocess.run([sys.executable, str(ROOT / "tools" / "compile_model.py"), "--xml", str(xml), "--rescale", "1.0", "--out", str(tmp_path / "toy.tmjx")],
                   check=True, capture_output=True)
    side = _blob.load(tmp_path / "toy.sensors.tmjx.txt")
    assert list(side) == ["site_bodyid", "site_pos", "site_quat", "sensor_type", "sensor_objid", "sensor_adr"]
    assert not set(side) & set(_blob.load(tmp_path / "toy.tmjx"))
    names = (tmp_path / "toy.names.txt").read_text().splitlines()
    assert names[-5:] == ["site 0 tip", "sensor 0 vel", "sensor 1 torso_v", "sensor 2 acc", "sensor 3 gyr"]
    bare = tmp_path / "bare"
    bare.mkdir()
    (bare / "toy.xml").write_text(TOY[:TOY.index("  <sensor>")] + "</mujoco>\n")
    subprocess.run([sys.executable, str(ROOT / "tools" / "compile_model.py"), "--xml", str(bare / "toy.xml"), "--rescale", "1.0", "--out",
                    str(bare / "toy.tmjx")], check=True, capture_output=True)
    assert not (bare / "toy.sensors.tmjx.txt").exists()


@pytest.mark.parametrize("bad,match", [('<touch name="t" site="tip"/>', "type touch is not compiled"),
                                       ('<framepos name="f" objtype="site" objname="tip"/>', "type framepos is not compiled"),
                                       ('<gyro name="g2" site="tip" cutoff="2"/>', "non-zero cutoff")])
def test_compiler_refuses_unsupported_sensors(tmp_path, bad, match):
    with pytest.raises(NotImplementedError, match=match):
        cm.compile_model(_toy(tmp_path, TOY.replace("</sensor>", bad + "\n  </sensor>")), torque_actuators=True, rescale_factor=1.0)


@pytest.mark.parametrize("config", ["rodent-full-clips", "rodent-sps-per-actor"])
def test_committed_blobs_carry_the_rodent_sensors(config):
    w, _ = default_walker(config)
    assert w.nsensordata == 12
    assert w.sensor_table() == [("accelerometer", 0, 3), ("velocimeter", 3, 3), ("gyro", 6, 3), ("torso", 9, 3)]
    assert w.names["site"] == {"head": 0}
    assert w.model["site_bodyid"].tolist() == [w.names["body"]["skull"]] == [56]
    assert w.model["sensor_objid"].tolist() == [0, 0, 0, w.names["body"]["torso"]]
    np.testing.assert_array_equal(w.model["site_pos"], 0.0)
    np.testing.assert_array_equal(w.model["site_quat"], [1.0, 0, 0, 0])
    # the side file's entries come behind the blob's own in the walker's model, and so in the blob handed to tmjx_model_create
    assert list(w.model)[-6:] == ["site_bodyid", "site_pos", "site_quat", "sensor_type", "sensor_objid", "sensor_adr"]


@needs_xml
@pytest.mark.parametrize("fname,kw", [("rodent_model.tmjx", dict(torque_actuators=True, rescale_factor=0.9)),
                                      ("rodent_model_pos080.tmjx.txt", dict(torque_actuators=False, rescale_factor=0.8, affine_bias=True))])
def test_committed_blobs_equal_the_compiler(fname, kw):
    m = cm.compile_model(XML, **kw)
    for got, want in ((_blob.load(ROOT / "track_mjx_amd" / "assets" / fname), cm.to_blob(m)),
                      (_blob.load(ROOT / "track_mjx_amd" / "assets" / f"{_blob.stem(fname)}.sensors.tmjx.txt"), cm.sensor_entries(m))):
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype.kind == np.asarray(want[k]).dtype.kind, k
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ---------------------------------------------------------------------------------------------------------------- the sensor stage
@pytest.fixture(scope="module")
def setup():
    w, cfg = default_walker()
    blob = default_blob(w, cfg)
    clip = _clips.make_synthetic_clips(w.model, 4, seed=0)
    return w, blob, clip, SR.model_dict(_blob.unpack(blob))


def _states(clip, n, rng, sink, vel):
    qpos = np.zeros((n, 74))
    qvel = rng.uniform(-vel, vel, size=(n, 73))
    for e in range(n):
        c, f = e % 4, (7 * e) % 44
        qpos[e] = np.concatenate([clip.position[c, f], clip.quaternion[c, f], clip.joints[c, f]]) + rng.uniform(-1e-3, 1e-3, 74)
        qpos[e, 2] -= sink * (e % 5)
    return qpos, qvel


def _per_sensor_err(got, ref):
    """max over envs of |got - ref| / max |ref|, per 3-wide sensor (each sensor against its own scale)."""
    g, r = got.reshape(-1, 4, 3), ref.reshape(-1, 4, 3)
    return np.abs(g - r).max(axis=(0, 2)) / (np.abs(r).max(axis=(0, 2)) + 1e-12)


def test_sensor_stage_vs_float64_restatement(setup):
    """One teacher-forced substep of 20 envs (clip poses sunk into the floor: contacts in most envs, velocities up to 0.5).
    (a) the restatement fed the emulation's own starting state, qacc, efc_force and contact frames (contact points from the float64 oracle):
        isolates the stage's fp32 arithmetic.  Measured: sensors <= 1.4e-6 of each sensor's scale, cfrc_ext <= 5e-8 of its scale — bounds
        1e-4 / 1e-5.
    (b) the restatement fed the float64 oracle's qacc / efc_force / frames: the bound includes the solver's fp32 error.  Measured: sensors
        <= 2.5e-6, cfrc_ext <= 1e-4 — bound 1e-3 (the solver's fp32 error grows with the number of active contacts)."""
    w, blob, clip, M = setup
    n = 20
    E, S, O64 = Emu(blob, n), SensorEmu(blob), make_oracle(blob, clip, "f64")
    rng = np.random.default_rng(0)
    qpos, qvel = _states(clip, n, rng, 0.006, 0.5)
    act = rng.uniform(-0.1, 0.1, size=(n, 38))
    E.rows("qpos")[:] = qpos.T; E.rows("qvel")[:] = qvel.T; E.rows("act")[:] = act.T
    q0, v0 = E.rows("qpos").astype(np.float64).T.copy(), E.rows("qvel").astype(np.float64).T.copy()
    a = np.clip(rng.normal(size=(38, n)) * 0.3, -1, 1).astype(np.float32)
    sd, cf = S.physics(E, a, 1)
    qacc, ef, fr = E.rows("qacc").T.astype(np.float64), E.rows("efc_force").T.astype(np.float64), E.rows("con_frame").T.astype(np.float64)
    refA, refB, cfA, cfB = [], [], [], []
    for e in range(n):
        d = O64.new_data(q0[e], v0[e]); O64.set(d, "act", act[e]); O64.set(d, "qacc_warmstart", np.zeros(73))
        O64.step(d, a[:, e].astype(np.float64))
        cp = O64.get(d, "con_pos")
        s1, c1 = SR.sensors(M, q0[e], v0[e], qacc[e], ef[e], cp, fr[e])
        s2, c2 = SR.sensors(M, q0[e], v0[e], O64.get(d, "qacc"), O64.get(d, "efc_force"), cp, O64.get(d, "con_frame"))
        refA.append(s1); refB.append(s2); cfA.append(c1.ravel()); cfB.append(c2.ravel())
    refA, refB, cfA, cfB = map(np.array, (refA, refB, cfA, cfB))
    in_contact = np.abs(cfA).max(1) > 0
    assert in_contact.sum() >= n // 4, in_contact.sum()
    assert np.isfinite(sd).all() and np.isfinite(cf).all()
    assert np.all(cf[:6] == 0.0), "the world body's row stays 0"
    ea, eb = _per_sensor_err(sd.T, refA), _per_sensor_err(sd.T, refB)
    assert ea.max() < 1e-4, ea
    assert eb.max() < 1e-3, eb
    sc = np.abs(cfA).max()
    assert np.abs(cf.T - cfA).max() / sc < 1e-5, np.abs(cf.T - cfA).max() / sc
    assert np.abs(cf.T - cfB).max() / sc < 1e-3, np.abs(cf.T - cfB).max() / sc
    # reaction: the floor body's row is minus the sum of the rodent's forces
    F = cf.reshape(68, 6, n)
    np.testing.assert_allclose(F[1, 3:], -F[2:, 3:].sum(0), rtol=1e-4, atol=1e-6)


def test_sensor_stage_does_not_perturb_the_physics(setup):
    """N control steps (10 substeps each) with and without the stage: state, observation and reward bit for bit."""
    w, blob, clip, _ = setup
    n = 6
    rng = np.random.default_rng(3)
    qpos, qvel = _states(clip, n, rng, 0.003, 0.2)
    runs = []
    for sensors in (False, True):
        E, S = Emu(blob, n), SensorEmu(blob)
        E.set_clips(clip.as_dict())
        E.reset(np.arange(n) % 4, np.zeros(n), np.zeros((74, n)), np.zeros((73, n)))
        E.rows("qpos")[:] = qpos.T; E.rows("qvel")[:] = qvel.T
        r2 = np.random.default_rng(5)
        for _ in range(4):
            a = np.clip(r2.normal(size=(38, n)) * 0.4, -1, 1).astype(np.float32)
            S.physics(E, a, 10, sensors=sensors, dump=False)
            E.post(a)
        runs.append((E.st.copy(), E.obs.copy(), E.reward.copy()))
    for x, y in zip(*runs):
        assert np.array_equal(x, y, equal_nan=True)


def test_readings_without_motion_or_contact(setup):
    """Raised 0.5 above the floor with qvel = 0: no contact, so cfrc_ext is exactly 0 (the floor's row included); the velocity sensors are
    exactly 0 (every cvel is a sum of cdof * 0).  (A settled at-rest check — accelerometer = R_skull^T g, summed contact force = weight — is
    not made: the torque rodent with zero action is a ragdoll whose light distal joints keep moving; in the emulation max |qvel| stayed
    between 1 and 50 over 10 000 substeps.)"""
    w, blob, clip, M = setup
    n = 3
    E, S = Emu(blob, n), SensorEmu(blob)
    qpos = np.stack([np.concatenate([clip.position[e, 0], clip.quaternion[e, 0], clip.joints[e, 0]]) for e in range(n)])
    qpos[:, 2] += 0.5
    E.rows("qpos")[:] = qpos.T
    E.rows("qvel")[:] = 0.0
    sd, cf = S.physics(E, np.zeros((38, n), np.float32), 1)
    assert np.all(cf == 0.0)
    assert np.all(sd[3:] == 0.0)
    assert np.isfinite(sd[:3]).all()


def test_generator_refusals_with_sensor_logging():
    """log_sensor_data=True needs an environment with the recording kernel's entry (MultiClipTracking.sensor_buffers); with one, the
    generator still refuses an inference function that is not the HIP roll-out policy."""
    from track_mjx_amd import config as _config
    from track_mjx_amd.analysis.rollout import create_rollout_generator
    cfg = _config.load_config(None, [])
    with pytest.raises(NotImplementedError, match="environment given is NoneType"):
        create_rollout_generator(cfg, None, lambda obs, key: obs, log_sensor_data=True)

    class WithSensors:
        def sensor_buffers(self):
            raise AssertionError("not reached")
    with pytest.raises(TypeError, match="load_inference_fn"):
        create_rollout_generator(cfg, WithSensors(), lambda obs, key: obs, log_sensor_data=True)
