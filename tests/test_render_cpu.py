"""The roll-out renderer on the CPU: the compiler's render tables against rodent.xml, the float64 reference's own properties, and the host
emulation of the kernel bodies (tests/hostemu/render_emu.cpp) under the checks tests/test_gpu_render.py applies to the kernels, at the same
shapes; the C-ABI's argument refusals; the command-line tool on a synthetic clip_0.h5."""
from __future__ import annotations

import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import compile_model as cm  # noqa: E402

from tests import render_ref as rr  # noqa: E402
from tests import render_scenes as S  # noqa: E402
from tests.common import default_walker  # noqa: E402
from tests.hostemu import render_emu as E  # noqa: E402
from track_mjx_amd import blob as _blob  # noqa: E402
from track_mjx_amd import hip  # noqa: E402
from track_mjx_amd import walker as _walker  # noqa: E402

CONFIGS = tuple(S.WALKERS)
FIX = np.load(ROOT / "tests" / "golden" / "rodent_xml_render.npz")


@functools.lru_cache(None)
def emu(config="torque090"):
    w, _ = S.make_walker(config)
    return E.RenderEmu(_blob.pack(w.model)), w


def cam_of(d) -> hip.Camera:
    return E.make_camera(d["body"], d["mode"], d["offset"], d["quat"], d["fovy"])


# ------------------------------------------------------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("config", CONFIGS)
def test_render_side_file_against_the_xml(config):
    w, cfg = S.make_walker(config)
    s = w.rescale_factor
    t = w.render_table()
    assert len(t["type"]) == len(FIX["geom_name"]) == 101      # every geom of rodent.xml is in groups 0-2
    codes = np.array([cm.GEOM_TYPES[str(n)] for n in FIX["geom_type"]])
    np.testing.assert_array_equal(t["type"], codes)
    if config == "torque090":
        counts = {k: int((t["type"] == cm.GEOM_TYPES[k]).sum()) for k in ("capsule", "ellipsoid", "sphere", "box", "plane")}
        assert counts == {"capsule": 56, "ellipsoid": 22, "sphere": 15, "box": 7, "plane": 1}
    np.testing.assert_array_equal(t["group"], FIX["geom_group"])
    assert set(t["group"].tolist()) <= {0, 1, 2}
    np.testing.assert_array_equal(t["body"], [w.names["body"][str(b)] if str(b) != "world" else 0 for b in FIX["geom_body"]])
    below = np.array([bool(x) for x in FIX["geom_below_walker"]])      # dm_scale_spec scales what hangs below "walker"
    k = np.where(below, s, 1.0)[:, None]
    np.testing.assert_allclose(t["size"], FIX["geom_size"] * k, rtol=1e-15, atol=0)
    np.testing.assert_allclose(t["pos"], FIX["geom_pos"] * k, rtol=1e-15, atol=0)
    np.testing.assert_allclose(t["rgba"], FIX["geom_rgba"], rtol=0, atol=0)
    for i in range(101):      # orientation attributes resolved: quat as written, euler in the xyz intrinsic order
        kind, v = str(FIX["geom_orient_kind"][i]), FIX["geom_orient"][i]
        want = np.array([1.0, 0, 0, 0]) if kind == "none" else (v[:4] / np.linalg.norm(v[:4]) if kind == "quat" else cm.euler_to_quat(v[:3]))
        assert kind in ("none", "quat", "euler")
        np.testing.assert_allclose(t["quat"][i], want, atol=1e-15)
    cams = w.cameras()
    assert list(cams) == [str(n) for n in FIX["camera_name"]] == ["close_profile", "back", "side", "side_alt", "top", "egocentric"]
    for i, (name, c) in enumerate(cams.items()):
        assert c["mode"] == str(FIX["camera_mode"][i]) and c["fovy"] == FIX["camera_fovy"][i]
        assert c["body"] == w.names["body"][str(FIX["camera_body"][i])]
        np.testing.assert_array_equal(c["pos"], FIX["camera_pos"][i])      # cameras are not rescaled
        R = cm.quat_to_mat(c["quat"])
        kind, v = str(FIX["camera_orient_kind"][i]), FIX["camera_orient"][i]
        if kind == "xyaxes":      # x along the first vector, y in the plane of both, right-handed
            x = v[:3] / np.linalg.norm(v[:3])
            np.testing.assert_allclose(R[:, 0], x, atol=1e-12)
            assert abs(R[:, 1] @ x) < 1e-12 and R[:, 1] @ v[3:6] > 0 and abs(R[:, 2] @ v[3:6]) < 1e-12
        elif kind == "zaxis":
            np.testing.assert_allclose(R[:, 2], v[:3] / np.linalg.norm(v[:3]), atol=1e-12)
        else:
            assert kind == "euler"
            np.testing.assert_allclose(c["quat"], cm.euler_to_quat(v[:3]), atol=1e-15)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
    assert np.isclose(np.linalg.det(cm.quat_to_mat(cams["close_profile"]["quat"])), 1.0)
    # close_profile looks at the torso from (.5, -.5, .5): along -Z
    np.testing.assert_allclose(-cm.quat_to_mat(cams["close_profile"]["quat"])[:, 2], np.array([-1, 1, -1]) / np.sqrt(3), atol=1e-12)


def test_model_blobs_and_entry_order_are_untouched():
    w, _ = default_walker()
    keys = list(w.model)
    assert keys.index("rgeom_body") > keys.index("con_g2_size") and keys[-6:] == ["site_bodyid", "site_pos", "site_quat", "sensor_type", "sensor_objid", "sensor_adr"]
    own = _blob.load(w.blob_path)
    assert not [k for k in own if k.startswith(("rgeom_", "rcam_"))]


def test_compiler_refuses_unrendered_geoms_by_name():
    w, _ = default_walker()
    m = dict(geoms=[dict(name="pipe", body=1, type=cm.GEOM_CYLINDER, size=np.ones(3), pos=np.zeros(3), quat=np.array([1.0, 0, 0, 0]),
                         rgba=np.ones(4), group=0)], cameras=[])
    with pytest.raises(NotImplementedError, match="pipe.*cylinder"):
        cm.render_entries(m)
    m["geoms"][0]["group"] = 3      # invisible: not rendered, not refused
    assert len(cm.render_entries(m)["rgeom_type"]) == 0


# ------------------------------------------------------------------------------------------------------------------ 2. reference
def test_reference_kinematics_are_the_compilers():
    w, m, qpos = S.walker_setup()
    for f in (0, 77):
        a, b = cm.fk(m, qpos[0, f].astype(np.float64)), rr.fk(m, qpos[0, f].astype(np.float64))
        np.testing.assert_allclose(a[0], b[0], rtol=0, atol=1e-15)      # (np.linalg.norm against sqrt(sum): the last bit)
        np.testing.assert_allclose(a[1], b[1], rtol=0, atol=1e-15)
    c = w.cameras()["close_profile"]
    q0 = np.asarray(w.model["qpos0"], np.float64)
    np.testing.assert_allclose(rr.subtree_com(m, q0, c["body"]) + c["off0"], rr.fk(m, q0)[0][c["body"]] + c["pos"], atol=1e-14)


def test_zoo_has_200_interior_pixels_of_every_type():
    counts = S.zoo_interior_counts(S.zoo_reference())
    print(counts)
    assert set(counts) == {rr.SPHERE, rr.CAPSULE, rr.ELLIPSOID, rr.BOX, rr.PLANE} and min(counts.values()) >= 200
    assert S.zoo_reference()["blended"].sum() >= 200


def test_walker_view_is_60_percent_interior_in_every_frame():
    for f, ref in enumerate(S.walker_reference()):
        share, n = S.walker_interior_share(ref)
        print(f"frame {f}: {share:.3f} of {n} walker / ghost pixels are interior")
        assert share >= 0.60 and n > 2000


# ------------------------------------------------------------------------------------------------------------------ 3. emulation
@pytest.mark.parametrize("config", CONFIGS)
def test_emu_pose(config):
    em, w = emu(config)
    p64, (e_c, e_r) = S.pose_reference(config)
    cams, prims = em.pose(S.pose_frames(config), None, em.camera("close_profile"))
    err_c = np.abs(prims[..., 0:3] - p64[..., 0:3]).max()
    err_r = np.abs(prims[..., 3:12] - p64[..., 3:12]).max()
    print(f"{config}: centre err {err_c:.3e} (reference float32 {e_c:.3e}), rotation err {err_r:.3e} (reference float32 {e_r:.3e})")
    assert err_c <= 4 * e_c and err_r <= 4 * e_r
    np.testing.assert_array_equal(prims[..., 12:18], p64[..., 12:18].astype(np.float32))
    np.testing.assert_array_equal(prims[..., 18:20].view(np.int32), rr.pack_prims(p64)[..., 18:20].view(np.int32))
    m = S.walker_setup(config)[1]
    for f, q in enumerate(S.pose_frames(config)):      # the named trackcom camera follows the subtree's centre of mass with its qpos0 offset
        want = rr.camera_record(m, rr.named_camera(w, "close_profile"), q.astype(np.float64))
        np.testing.assert_allclose(cams[f, :13], want[:13], atol=4 * e_c + 1e-7)


@pytest.mark.parametrize("size", S.SIZES)
def test_emu_zoo(size):
    em, _ = emu()
    prims, cam = S.zoo()
    ref = S.zoo_reference(*size)
    rgba, depth, gid = em.prims(rr.pack_prims(prims)[None], cam.astype(np.float32)[None], *size)
    S.check_pixels(ref, rgba[0], depth[0], gid[0], f"zoo {size}")


def test_emu_walker():
    em, w = emu()
    q, g = S.walker_frames()
    rgba, depth, gid = em.render(q, g, cam_of(S.close_camera(w)), S.W, S.H)
    for f, ref in enumerate(S.walker_reference()):
        S.check_pixels(ref, rgba[f], depth[f], gid[f], f"walker frame {f}")


def test_emu_identities():
    em, w = emu()
    q, g = S.walker_frames()
    cam = em.camera("close_profile")
    W, H = 40, 30
    full = em.render(q, g, cam, W, H)
    one = em.render(q[1:2], g[1:2], cam, W, H)
    for a, b in zip(full, one):
        np.testing.assert_array_equal(a[1].view(np.uint8), b[0].view(np.uint8))
    cams, prims = em.pose(q, g, cam)
    for a, b in zip(full, em.prims(prims, cams, W, H)):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    off = em.render(q, None, cam, W, H)
    nvis = em.info(1, True).ngeom
    no_ghost = full[2] < nvis
    assert no_ghost.any() and (~no_ghost).any()
    for a, b in zip(full, off):
        np.testing.assert_array_equal(a[no_ghost].view(np.uint8), b[no_ghost].view(np.uint8))
    byhand = cam_of(rr.named_camera(w, "close_profile"))
    for a, b in zip(full, em.render(q, g, byhand, W, H)):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    ego = em.render(q, g, em.camera("egocentric"), W, H)      # mode fixed, on the skull
    assert (ego[2] >= 0).any()


def test_emu_refusals():
    em, w = emu()
    q, g = S.walker_frames()
    cam = em.camera("close_profile")
    bare = E.RenderEmu(_blob.pack({k: v for k, v in w.model.items() if not k.startswith(("rgeom_", "rcam_"))}))
    for call in (lambda: bare.info(1, False), lambda: bare.camera("close_profile"), lambda: bare.render(q, g, cam, 8, 8)):
        with pytest.raises(ValueError, match="no render tables"):
            call()
    with pytest.raises(ValueError, match="unknown camera 'nose'.*close_profile"):
        em.camera("nose")
    with pytest.raises(ValueError, match="ghost frames: 2 frames against 3"):
        em.render(q, g[:2], cam, 8, 8)
    with pytest.raises(ValueError, match="W and H must be >= 1"):
        em.render(q, g, cam, 0, 8)
    with pytest.raises(ValueError, match="W and H must be >= 1"):
        em.render(q, g, cam, 8, -1)
    with pytest.raises(ValueError, match="F must be >= 1"):
        em.render(q[:0], None, cam, 8, 8)
    track = cam_of(dict(rr.named_camera(w, "close_profile"), mode=rr.MODE_TRACK))
    with pytest.raises(ValueError, match="mode track is not rendered"):
        em.render(q, g, track, 8, 8)
    with pytest.raises(ValueError, match="body 68 is out of range"):
        em.render(q, g, cam_of(dict(rr.named_camera(w, "close_profile"), body=68)), 8, 8)
    bad = dict(w.model)
    bad["rgeom_body"] = np.asarray(bad["rgeom_body"]).copy()
    bad["rgeom_body"][5] = 68
    with pytest.raises(ValueError, match="rgeom_body: body id out of range"):
        E.RenderEmu(_blob.pack(bad))


def test_abi_declares_the_renderer():
    assert {"tmjx_render_info", "tmjx_render_camera", "tmjx_render_pose", "tmjx_render_prims", "tmjx_render"} <= set(hip.EXPORTS)
    header = (ROOT / "include" / "tmjx.h").read_text()
    for name in ("tmjx_render_info", "tmjx_render_camera", "tmjx_render_pose", "tmjx_render_prims", "tmjx_render(", "tmjx_camera_t"):
        assert name in header
    assert any(p.name == "tmjx_render.hip" for p in hip.SOURCES)
    assert C.sizeof(hip.Camera) == 40 and C.sizeof(hip.RenderInfo) == 40


# ------------------------------------------------------------------------------------------------------------------ 4. Python and CLI
class EmuRenderer:
    """analysis.render.Renderer's constructor and .render on the host emulation."""

    def __init__(self, walker, device, height=480, width=640, camera="close_profile", render_ghost=True):
        self.em, self.h, self.w, self.ghost = E.RenderEmu(_blob.pack(walker.model)), height, width, render_ghost
        self.cam = self.em.camera(camera)

    def render(self, q, g=None):
        return self.em.render(q, g if self.ghost else None, self.cam, self.w, self.h)[0][..., :3]


def test_cli_on_a_synthetic_rollout(tmp_path, capsys):
    from track_mjx_amd import config as _config
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import render as R
    w, m, qpos = S.walker_setup()
    (tmp_path / "in").mkdir()
    h5lite.write_tree(tmp_path / "in" / "clip_0.h5", {"qposes_rollout": qpos[0, :6], "qposes_ref": qpos[1, :6]})
    assert R.main([f"rollouts={tmp_path / 'in'}", f"out={tmp_path / 'out'}", "size=24x18", "every=2", "camera=side"], renderer_cls=EmuRenderer) == 0
    with h5lite.File(tmp_path / "out" / "clip_0.frames.h5") as h:
        frames, fps, cam = h["frames"][()], float(h["fps"][()]), h["camera"][()]
    assert frames.shape == (3, 18, 24, 3) and frames.dtype == np.uint8 and bytes(cam).decode() == "side"
    cfg = _config.default_config()
    ea = cfg["env_config"]["env_args"]
    assert fps == pytest.approx(1.0 / ea["mj_model_timestep"] / ea["physics_steps_per_control_step"] / 2)
    want = EmuRenderer(w, "cpu", 18, 24, "side").render(qpos[0, 0:1], qpos[1, 0:1])
    np.testing.assert_array_equal(frames[0], want[0])
    assert R.main(["out=x"]) == 2 and "usage" in capsys.readouterr().err
    # the fps rule and the .get defaults: no pinned default config names either key
    assert "render_fps" not in cfg["env_config"] and "render_camera_name" not in cfg["env_config"]
    assert R.render_fps({"env_config": {"render_fps": 30, "env_args": ea}}) == 30.0
    frames2, fps2 = R.render_rollout(cfg, {"qposes_rollout": qpos[0, :2], "qposes_ref": qpos[1, :2]}, height=18, width=24, renderer_cls=EmuRenderer)
    assert frames2.shape == (2, 18, 24, 3) and fps2 == pytest.approx(2 * fps)
    np.testing.assert_array_equal(frames2[0], EmuRenderer(w, "cpu", 18, 24, "close_profile").render(qpos[0, 0:1], qpos[1, 0:1])[0])


def test_emulation_as_a_stand_alone_program(tmp_path):
    """The emulation's own main (the program sanitizer builds run) renders from every named camera of the shipped blob."""
    import subprocess
    w, _ = default_walker()
    (tmp_path / "m.tmjx").write_bytes(_blob.pack(w.model))
    exe = E.build_main(tmp_path / "render_emu")
    out = subprocess.run([str(exe), str(tmp_path / "m.tmjx")], capture_output=True, text=True)
    assert out.returncode == 0 and "6 cameras, 201 primitives" in out.stdout, out.stdout + out.stderr
