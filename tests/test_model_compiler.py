"""CPU: known answers for tools/compile_model.py (the MJCF-subset restatement of MuJoCo's model compiler that every physics
constant of the hot path comes from).

Reference lines the compiler mirrors: track_mjx/environment/walker/spec_utils.py:19-52 (dm_scale_spec: body pos, geom pos / size
x s, gear x s^2), track_mjx/environment/walker/rodent.py:70-78 (torque-actuator rewrite: gainprm[0] = forcerange[1], bias off).
The expected values here are NOT taken from the compiler's own formulas: primitive inertias come from a quasi-Monte-Carlo
integration of the solid and from the hemisphere + cylinder decomposition written out independently; the scaling laws are pure
dimensional analysis (mass ~ s^3, inertia ~ s^5); the contact cases are worked out by hand for axis-aligned poses.
"""
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import compile_model as cm  # noqa: E402

from tests.common import default_blob, default_walker, make_oracle  # noqa: E402


def _qmc_inertia(inside, half_extent, n=1 << 20):
    """Volume and unit-density inertia diag(Ixx, Iyy, Izz) about the origin of the solid {p : inside(p)} by Sobol integration."""
    from scipy.stats import qmc
    p = (qmc.Sobol(3, seed=0).random(n) * 2 - 1) * half_extent
    m = inside(p)
    box = np.prod(2 * np.asarray(half_extent))
    x, y, z = p[m].T
    vol = box * m.mean()
    return vol, box / n * np.array([(y * y + z * z).sum(), (x * x + z * z).sum(), (x * x + y * y).sum()])


PRIMS = [
    ("sphere", cm.GEOM_SPHERE, np.array([0.013, 0, 0]), lambda p: (p ** 2).sum(1) <= 0.013 ** 2, [0.013] * 3),
    ("capsule", cm.GEOM_CAPSULE, np.array([0.004, 0.011, 0]),
     lambda p: (p[:, 0] ** 2 + p[:, 1] ** 2 + np.maximum(np.abs(p[:, 2]) - 0.011, 0) ** 2) <= 0.004 ** 2, [0.004, 0.004, 0.015]),
    ("ellipsoid", cm.GEOM_ELLIPSOID, np.array([0.006, 0.003, 0.002]),
     lambda p: ((p / np.array([0.006, 0.003, 0.002])) ** 2).sum(1) <= 1, [0.006, 0.003, 0.002]),
    ("box", cm.GEOM_BOX, np.array([0.01, 0.02, 0.005]), lambda p: np.ones(len(p), bool), [0.01, 0.02, 0.005]),
    ("cylinder", cm.GEOM_CYLINDER, np.array([0.007, 0.02, 0]), lambda p: p[:, 0] ** 2 + p[:, 1] ** 2 <= 0.007 ** 2, [0.007, 0.007, 0.02]),
]


@pytest.mark.parametrize("name,gtype,size,inside,ext", PRIMS, ids=[p[0] for p in PRIMS])
def test_primitive_volume_and_inertia_against_numerical_integration(name, gtype, size, inside, ext):
    vol, ine = cm.geom_volume_inertia(gtype, size)
    v_ref, i_ref = _qmc_inertia(inside, ext)
    assert abs(vol - v_ref) < 2e-3 * v_ref
    np.testing.assert_allclose(ine, i_ref, rtol=3e-3)


def test_capsule_and_friends_closed_forms():
    # capsule = cylinder (radius r, length h) + two hemispheres (mass m_h each, COM 3r/8 beyond the flat face, own-COM inertia 83/320 m r^2)
    r, hh = 0.004, 0.011
    h = 2 * hh
    m_c, m_h = np.pi * r * r * h, 2.0 / 3.0 * np.pi * r ** 3
    izz = m_c * r * r / 2 + 2 * (2.0 / 5.0 * m_h * r * r)
    ixx = m_c * (3 * r * r + h * h) / 12 + 2 * (83.0 / 320.0 * m_h * r * r + m_h * (hh + 3 * r / 8) ** 2)
    vol, ine = cm.geom_volume_inertia(cm.GEOM_CAPSULE, np.array([r, hh, 0]))
    assert abs(vol - (m_c + 2 * m_h)) < 1e-15
    np.testing.assert_allclose(ine, [ixx, ixx, izz], rtol=1e-12)
    # densities of the rodent XML (rodent.xml default classes): masses are density * volume
    a, b, c = 0.006, 0.003, 0.002
    v, i = cm.geom_volume_inertia(cm.GEOM_ELLIPSOID, np.array([a, b, c]))
    assert abs(1100 * v - 1100 * 4 / 3 * np.pi * a * b * c) < 1e-15
    np.testing.assert_allclose(500 * i, 500 * v / 5 * np.array([b * b + c * c, a * a + c * c, a * a + b * b]), rtol=1e-13)
    v, i = cm.geom_volume_inertia(cm.GEOM_SPHERE, np.array([0.01, 0, 0]))
    np.testing.assert_allclose([v, i[0]], [4 / 3 * np.pi * 1e-6, 2 / 5 * (4 / 3 * np.pi * 1e-6) * 1e-4], rtol=1e-13)
    v, i = cm.geom_volume_inertia(cm.GEOM_BOX, np.array([0.01, 0.02, 0.005]))      # half sizes -> edges 0.02 x 0.04 x 0.01
    np.testing.assert_allclose([v, *i], [8e-6, 8e-6 / 12 * (0.04 ** 2 + 0.01 ** 2), 8e-6 / 12 * (0.02 ** 2 + 0.01 ** 2), 8e-6 / 12 * (0.02 ** 2 + 0.04 ** 2)], rtol=1e-13)


TOY = textwrap.dedent("""
    <mujoco model="toy">
      <compiler angle="radian"/>
      <default>
        <geom density="1100" contype="0" conaffinity="0"/>
        <general ctrllimited="true" ctrlrange="-1 1" dyntype="filter" dynprm="0.04" forcelimited="false"/>
        <default class="paw"><geom contype="1" conaffinity="0" priority="1" friction="1.5 0.005 0.0001" density="500"/></default>
      </default>
      <worldbody>
        <geom name="floor" type="plane" size="1 1 0.1" contype="0" conaffinity="1"/>
        <body name="walker" pos="0 0 0.2">
          <freejoint name="root"/>
          <geom name="trunk" type="capsule" size="0.02 0.05" pos="0.01 0 0"/>
          <body name="arm" pos="0.1 0.02 -0.03">
            <joint name="elbow" type="hinge" axis="0 1 0" range="-1 1" limited="true" damping="0.002" armature="1e-6"/>
            <geom name="upper" type="ellipsoid" size="0.03 0.01 0.005" density="500"/>
            <geom name="ball" type="sphere" size="0.01" pos="0.04 0 0"/>
            <body name="hand" pos="0.08 0 0">
              <joint name="wrist" type="hinge" axis="0 0 1" range="-0.5 0.5" limited="true"/>
              <geom name="palm" type="box" size="0.01 0.008 0.002" density="500"/>
              <geom name="pad" class="paw" type="capsule" size="0.003 0.006" pos="0.01 0 -0.004" quat="0.7071067811865476 0 0.7071067811865476 0"/>
            </body>
          </body>
        </body>
      </worldbody>
      <actuator>
        <general name="elbow_m" joint="elbow" gear="2" gainprm="3" biastype="affine" biasprm="0 -3 0" forcerange="-0.7 0.7"/>
        <general name="wrist_m" joint="wrist" gear="1.5" gainprm="1" biastype="affine" biasprm="0 -1 0" forcerange="-0.2 0.25"/>
      </actuator>
    </mujoco>
""")


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    p = tmp_path_factory.mktemp("toy") / "toy.xml"
    p.write_text(TOY)
    return {s: cm.compile_model(str(p), torque_actuators=True, rescale_factor=s) for s in (1.0, 0.9)}, p


def test_toy_model_masses_coms_and_inertias(toy):
    m = toy[0][1.0]
    assert (m["nbody"], m["njnt"], m["nq"], m["nv"], m["nu"]) == (4, 3, 9, 8, 2)
    names = m["body_names"]
    w, arm, hand = names.index("walker"), names.index("arm"), names.index("hand")
    r, hh = 0.02, 0.05
    v_cap = np.pi * r * r * 2 * hh + 4 / 3 * np.pi * r ** 3
    assert abs(m["body_mass"][w] - 1100 * v_cap) < 1e-12
    np.testing.assert_allclose(m["body_ipos"][w], [0.01, 0, 0], atol=1e-15)
    # arm: ellipsoid (density 500) at the origin + sphere (1100) at x = 0.04: mass, COM and the parallel-axis inertia by hand
    m_e, m_s = 500 * 4 / 3 * np.pi * 0.03 * 0.01 * 0.005, 1100 * 4 / 3 * np.pi * 0.01 ** 3
    com_x = m_s * 0.04 / (m_e + m_s)
    assert abs(m["body_mass"][arm] - (m_e + m_s)) < 1e-12 and abs(m["body_ipos"][arm][0] - com_x) < 1e-15
    i_e = m_e / 5 * np.array([0.01 ** 2 + 0.005 ** 2, 0.03 ** 2 + 0.005 ** 2, 0.03 ** 2 + 0.01 ** 2])
    i_s = 2 / 5 * m_s * 0.01 ** 2 * np.ones(3)
    shift = m_e * com_x ** 2 + m_s * (0.04 - com_x) ** 2
    expect = i_e + i_s + np.array([0, shift, shift])
    np.testing.assert_allclose(np.sort(m["body_inertia"][arm]), np.sort(expect), rtol=1e-12)
    assert (np.diff(m["body_inertia"][arm]) <= 0).all(), "principal inertias in decreasing order (MuJoCo eig3)"
    # hand: box + rotated capsule, total mass
    v_pad = np.pi * 0.003 ** 2 * 0.012 + 4 / 3 * np.pi * 0.003 ** 3
    assert abs(m["body_mass"][hand] - (500 * 8 * 0.01 * 0.008 * 0.002 + 500 * v_pad)) < 1e-12
    # mass matrix at qpos0: total mass on the translational block, symmetric positive definite
    M = m["M0"]
    np.testing.assert_allclose(np.diag(M)[:3], m["body_mass"].sum(), rtol=1e-12)
    assert np.allclose(M, M.T) and np.linalg.eigvalsh(M).min() > 0
    assert abs(m["meaninertia"] - np.trace(M) / 8) < 1e-15


def test_dm_scale_spec_scaling_laws(toy):
    """spec_utils.py:19-52 with scale 0.9: lengths x 0.9 (body pos, geom pos / size) => mass x 0.9^3, inertia x 0.9^5; gear x 0.9^2;
    the free body's own position (the walker root) is NOT scaled by the body loop (it scales the children of `walker`)."""
    a, b = toy[0][1.0], toy[0][0.9]
    s = 0.9
    names = a["body_names"]
    for n in ("arm", "hand"):
        i = names.index(n)
        np.testing.assert_allclose(b["body_pos"][i], a["body_pos"][i] * s, rtol=1e-13)
    np.testing.assert_allclose(b["body_pos"][names.index("walker")], a["body_pos"][names.index("walker")])
    # dm_scale_spec walks `walker.first_body()` onwards: the DESCENDANTS of `walker` are scaled, the walker body's own pos and geoms are
    # not (spec_utils.py:24-35,51) — a quirk of the reference reproduced by the compiler (the rodent's walker body carries no geom)
    wi = names.index("walker")
    scaled = np.array([n not in ("world", "walker") for n in names])
    np.testing.assert_allclose(b["body_mass"][scaled], a["body_mass"][scaled] * s ** 3, rtol=1e-12)
    np.testing.assert_allclose(b["body_inertia"][scaled], a["body_inertia"][scaled] * s ** 5, rtol=1e-10)
    np.testing.assert_allclose(b["body_ipos"][scaled], a["body_ipos"][scaled] * s, rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(b["body_mass"][wi], a["body_mass"][wi], rtol=1e-14)
    for ga, gb in zip(a["geoms"], b["geoms"]):
        f = s if ga["body"] not in (0, wi) else 1.0
        np.testing.assert_allclose(gb["size"], ga["size"] * f, rtol=1e-13)
        np.testing.assert_allclose(gb["pos"], ga["pos"] * f, rtol=1e-13)
    np.testing.assert_allclose(b["act_moment"], a["act_moment"] * s * s, rtol=1e-13)
    assert a["act_moment"][0][a["jnt_dofadr"][a["jnt_names"].index("elbow")]] == 2.0
    np.testing.assert_allclose(b["jnt_range"], a["jnt_range"])           # angles do not scale


def test_torque_actuator_rewrite(toy):
    """rodent.py:70-78: gainprm[0] = forcerange[1], biastype none, biasprm 0 — position servos become torque motors."""
    m = toy[0][1.0]
    np.testing.assert_allclose(m["act_gain"], [0.7, 0.25])
    np.testing.assert_allclose(m["act_tau"], [0.04, 0.04])
    np.testing.assert_allclose(m["act_ctrlrange"], [[-1, 1], [-1, 1]])
    with pytest.raises(AssertionError):       # the affine-bias (position servo) mode is not compiled: the reference config never uses it
        cm.compile_model(str(toy[1]), torque_actuators=False, rescale_factor=1.0)


def test_toy_contact_slots_and_priority_mixing(toy):
    m = toy[0][1.0]
    assert m["ncon"] == 2 and list(m["con_sub"]) == [0, 1] and list(m["con_type"]) == [cm.GEOM_CAPSULE] * 2      # plane-capsule: two slots
    assert m["geoms"][m["con_geom1"][0]]["name"] == "floor" and m["geoms"][m["con_geom2"][0]]["name"] == "pad"
    np.testing.assert_allclose(m["con_friction"][0], [1.5, 0.005, 0.0001])       # the priority-1 paw geom's parameters win


def test_rodent_blob_scaling_against_the_xml():
    """The committed blob (rescale_factor 0.9, torque actuators) against numbers read straight from rodent.xml with ElementTree
    (stored in tests/golden/rodent_xml.npz by tests/golden/make_rodent_xml_fixture.py)."""
    X = np.load(ROOT / "tests" / "golden" / "rodent_xml.npz")
    w, _ = default_walker()
    pos = dict(zip(X["body_name"].tolist(), X["body_pos"]))
    names = [ln.split()[2] for ln in (ROOT / "track_mjx_amd" / "assets" / "rodent_model.names.txt").read_text().splitlines() if ln.startswith("body ")]
    bp = np.asarray(w.model["body_pos"]).reshape(-1, 3)
    checked = 0
    for i, n in enumerate(names):
        if n in pos and n not in ("walker", "floor"):
            np.testing.assert_allclose(bp[i], 0.9 * pos[n], rtol=1e-12, atol=1e-15, err_msg=n)
            checked += 1
    assert checked >= 60
    forcerange = dict(zip(X["actuator_name"].tolist(), X["actuator_forcerange"]))
    anames = [ln.split()[2] for ln in (ROOT / "track_mjx_amd" / "assets" / "rodent_model.names.txt").read_text().splitlines() if ln.startswith("actuator ")]
    gain = np.asarray(w.model["act_gain"])
    for i, n in enumerate(anames):
        fr = forcerange[n]
        if not np.isnan(fr[1]):
            assert abs(gain[i] - fr[1]) < 1e-12, n


def test_plane_capsule_and_plane_ellipsoid_contacts_by_hand():
    """SURVEY Appendix A colliders, hand-worked on the rodent with the root lifted and UNROTATED pose `qpos0`: for every paw slot the
    oracle's contact distance / position / normal must equal the closed form computed here from the geom's world pose
    (horizontal plane at height z0, normal +z): capsule end-sphere centres c +- axis * half_length: dist = z_end - r, pos = end - n (r + dist / 2);
    ellipsoid: support point in direction -n: dist = c_z - sqrt(sum (R^T n)_k^2 s_k^2)."""
    w, cfg = default_walker()
    O = make_oracle(default_blob(w, cfg), None, "f64")
    M = w.model
    for pose in range(2):
        _contacts_by_hand(O, M, pose)


def _contacts_by_hand(O, M, pose):
    qpos = np.asarray(M["qpos0"], dtype=np.float64).copy()
    qpos[2] = -0.006          # low enough that some paw slots penetrate the floor (z0 = -0.005) and others do not
    if pose == 1:             # pitched and rolled root, bent joints: the general-orientation branches of both colliders
        q = cm.quat_mul(cm.axis_angle_quat(np.array([0.0, 1.0, 0.0]), 0.3), cm.axis_angle_quat(np.array([1.0, 0.0, 0.0]), -0.2))
        qpos[3:7] = q / np.linalg.norm(q)
        qpos[7:] += 0.2 * np.sin(np.arange(67))
        qpos[2] = 0.012
    d = O.new_data(qpos, np.zeros(73))
    O.forward(d)
    xpos, xquat = O.get(d, "xpos").reshape(-1, 3), O.get(d, "xquat").reshape(-1, 4)
    dist, cpos, frame = O.get(d, "con_dist"), O.get(d, "con_pos").reshape(-1, 3), O.get(d, "con_frame").reshape(-1, 9)
    ncon = len(dist)
    g2p, g2q, g2s = (np.asarray(M[k], dtype=np.float64).reshape(ncon, -1) for k in ("con_g2_pos", "con_g2_quat", "con_g2_size"))
    body2, sub, typ = np.asarray(M["con_body2"]), np.asarray(M["con_sub"]), np.asarray(M["con_type"])
    g1p, g1q, body1 = np.asarray(M["con_g1_pos"], dtype=np.float64).reshape(ncon, 3), np.asarray(M["con_g1_quat"], dtype=np.float64).reshape(ncon, 4), np.asarray(M["con_body1"])
    n = np.array([0.0, 0.0, 1.0])
    seen = set()
    for c in range(ncon):
        # the floor plane: horizontal, at the height of its body + geom offset (rodent.xml:167-170)
        assert np.allclose(cm.quat_to_mat(xquat[body1[c]]) @ cm.quat_to_mat(g1q[c]) @ n, n)
        z0 = (xpos[body1[c]] + cm.quat_to_mat(xquat[body1[c]]) @ g1p[c])[2]
        R = cm.quat_to_mat(xquat[body2[c]]) @ cm.quat_to_mat(g2q[c])
        centre = xpos[body2[c]] + cm.quat_to_mat(xquat[body2[c]]) @ g2p[c]
        if typ[c] == cm.GEOM_CAPSULE:
            r, hl = g2s[c][0], g2s[c][1]
            end = centre + R[:, 2] * hl * (1.0 if sub[c] == 0 else -1.0)
            dd = end[2] - z0 - r
            pp = end - n * (r + dd / 2)
        else:
            s = g2s[c]
            loc = R.T @ n
            reach = np.sqrt(((loc * s) ** 2).sum())
            dd = centre[2] - z0 - reach
            support = centre - R @ (s * s * loc) / reach
            pp = support - n * dd / 2
        seen.add(int(typ[c]))
        assert abs(dist[c] - dd) < 1e-12, (c, dist[c], dd)
        np.testing.assert_allclose(cpos[c], pp, atol=1e-12, err_msg=f"slot {c}")
        np.testing.assert_allclose(frame[c][:3], n, atol=1e-12)
    assert seen == {cm.GEOM_CAPSULE, cm.GEOM_ELLIPSOID} and (dist < 0).any() and (dist > 0).any()
