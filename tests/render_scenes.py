"""Scenes, float64 references and the shared checks of the renderer tests (tests/test_render_cpu.py: the host emulation; tests/test_gpu_render.py:
the kernels).  Every reference is computed once per process by tests/render_ref.py and never modified.

Bounds (DESIGN.md "Rendering" records the measured numbers):
  pose   centres and rotations within 4 x the worst error of the reference's own float32 run against its float64 run on the same frames;
  pixels on INTERIOR pixels (the float64 (opaque, ghost) pair is the same at the centre and the four corners): ids equal, depth within 4 x the
         reference's float32-against-float64 worst error on those pixels, colour within 1 level, 2 where a ghost is blended.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import render_ref as rr
from tests.common import default_walker
from track_mjx_amd import walker as _walker
from track_mjx_amd import clips as _clips

W, H = 152, 113
SIZES = ((152, 113), (17, 9), (1, 1))
ZOO_TYPES = {0: rr.SPHERE, 1: rr.CAPSULE, 2: rr.ELLIPSOID, 3: rr.BOX, 4: rr.PLANE}      # opaque id -> type; id 5: the ghost ellipsoid
WALKER_FRAMES = (0, 60, 125)
POSE_FRAMES = (0, 31, 62, 93, 124)


WALKERS = {"torque090": (True, 0.9), "position080": (False, 0.8)}      # the two shipped walkers: (torque_actuators, rescale_factor)


@functools.lru_cache(None)
def make_walker(key="torque090"):
    _, cfg = default_walker()
    tq, s = WALKERS[key]
    return _walker.Rodent(**{**cfg["walker_config"], "torque_actuators": tq, "rescale_factor": s}), cfg


def _look(origin, forward, fovy):
    f = np.asarray(forward, float) / np.linalg.norm(forward)
    x = np.cross(f, [0, 0, 1.0])
    x /= np.linalg.norm(x)
    cam = np.zeros(rr.CAM)
    cam[0:3], cam[3:6], cam[6:9], cam[9:12] = origin, x, np.cross(x, f), -f
    cam[12] = np.tan(np.radians(fovy) / 2)
    return cam


def _rec(typ, idx, centre, euler, size, rgb, ghost=0):
    r = np.zeros(rr.REC)
    r[0:3] = centre
    r[3:12] = rr.cm.quat_to_mat(rr.cm.euler_to_quat(np.asarray(euler, float))).ravel()
    r[12:15], r[15:18], r[18], r[19] = size, rgb, typ + 256 * idx, ghost
    return r


@functools.lru_cache(None)
def zoo():
    """(prims [6, REC], cam [CAM]) in float64: one sphere, capsule, ellipsoid and box side by side, each rotated off its axes, in front of a plane
    that is tilted towards the camera (the backdrop: the only primitive anything is in front of, and bounded in distance — no horizon in view);
    one ghost ellipsoid over part of the box and of the plane."""
    prims = np.array([
        _rec(rr.SPHERE, 0, (-0.36, 0.00, 0.64), (0.3, 0.2, 0.1), (0.09, 0, 0), (0.9, 0.2, 0.1)),
        _rec(rr.CAPSULE, 1, (-0.12, 0.05, 0.62), (0.7, 0.4, 0.2), (0.05, 0.10, 0), (0.0, 0.6, 0.7)),
        _rec(rr.ELLIPSOID, 2, (0.15, -0.05, 0.66), (0.4, -0.5, 0.9), (0.11, 0.05, 0.07), (0.2, 0.8, 0.3)),
        _rec(rr.BOX, 3, (0.40, 0.00, 0.60), (0.5, 0.3, 0.6), (0.07, 0.05, 0.09), (0.7, 0.7, 0.1)),
        _rec(rr.PLANE, 4, (0.0, 0.0, 0.0), (0.45, 0.08, 0.0), (1, 1, 1), (0.5, 0.5, 0.5)),
        _rec(rr.ELLIPSOID, 5, (0.36, -0.25, 0.50), (0.2, 0.9, -0.4), (0.12, 0.06, 0.08), (0.5, 0.5, 0.5), ghost=1),
    ])
    return prims, _look((0.05, -1.0, 0.5), (0.04, 1.0, -0.03), 45.0)


@functools.lru_cache(None)
def zoo_reference(w=W, h=H):
    """dict: the float64 render, `interior`, and `depth_bound` = 4 x max |float32 - float64| depth of the reference on interior hit pixels."""
    prims, cam = zoo()
    return _reference(prims, cam, w, h)


def _reference(prims, cam, w, h, prims32=None, cam32=None):
    """`prims32`, `cam32`: the reference's own float32 tables (default: the float64 ones rounded, which is what the kernels are handed)."""
    ref = rr.render(prims, cam, w, h)
    ref["interior"] = rr.interior(prims, cam, w, h, ref)
    r32 = rr.render(prims.astype(np.float32) if prims32 is None else prims32, cam.astype(np.float32) if cam32 is None else cam32, w, h, dtype=np.float32)
    m = ref["interior"] & np.isfinite(ref["depth"]) & (r32["geom_id"] == ref["geom_id"])
    ref["depth_err32"] = float(np.abs(r32["depth"][m].astype(np.float64) - ref["depth"][m]).max()) if m.any() else 0.0
    ref["depth_bound"] = 4 * ref["depth_err32"]
    return ref


@functools.lru_cache(None)
def walker_setup(config="torque090"):
    w, cfg = make_walker(config)
    m = rr.model_of(w.model)
    clip = _clips.make_synthetic_clips(w.model, 2, seed=0)
    qpos = np.concatenate([clip.position, clip.quaternion, clip.joints], -1).astype(np.float32)      # [2, 250, nq]: clip 0 the walker, clip 1 the ghost
    return w, m, qpos


def close_camera(w) -> dict:
    """The walker test's camera: trackcom on the torso, 0.25 m from the subtree's centre of mass along close_profile's direction, fovy 45."""
    c = w.cameras()["close_profile"]
    return dict(body=c["body"], mode=rr.MODE_TRACKCOM, offset=0.25 * c["pos"] / np.linalg.norm(c["pos"]), quat=c["wquat0"], fovy=45.0)


def walker_frames(config="torque090"):
    """(qpos [3, nq], qpos_ghost [3, nq]) float32: frames of synthetic clip 0, the ghost at the same frames of clip 1 moved beside it."""
    w, m, qpos = walker_setup(config)
    q, g = qpos[0, list(WALKER_FRAMES)].copy(), qpos[1, list(WALKER_FRAMES)].copy()
    g[:, 0:3] = q[:, 0:3] + np.array([0.02, 0.03, 0.0], np.float32)
    return q, g


@functools.lru_cache(None)
def walker_reference(config="torque090"):
    """Per test frame: the float64 tables from the float32 qpos the kernels are given, and the _reference dict of each."""
    w, m, _ = walker_setup(config)
    q, g = walker_frames(config)
    cam = close_camera(w)
    out = []
    for f in range(len(q)):
        prims = rr.pose_prims(m, q[f].astype(np.float64), g[f].astype(np.float64))
        crec = rr.camera_record(m, cam, q[f].astype(np.float64))
        ref = _reference(prims, crec, W, H, rr.pose_prims(m, q[f], g[f], dtype=np.float32), rr.camera_record(m, cam, q[f], dtype=np.float32))
        ref["prims"], ref["cam"] = prims, crec
        out.append(ref)
    return out


def pose_frames(config):
    w, m, qpos = walker_setup(config)
    return np.concatenate([qpos[0, list(POSE_FRAMES)], np.asarray(w.model["qpos0"], np.float32)[None]], 0)


@functools.lru_cache(None)
def pose_reference(config):
    """float64 tables [6, ngeom, REC] (5 clip frames + qpos0, no ghost) and (centre bound, rotation bound) = 4 x the float32 run's worst error."""
    w, m, _ = walker_setup(config)
    q = pose_frames(config)
    p64 = np.array([rr.pose_prims(m, f.astype(np.float64)) for f in q])
    p32 = np.array([rr.pose_prims(m, f, dtype=np.float32) for f in q])
    e_c = float(np.abs(p32[..., 0:3].astype(np.float64) - p64[..., 0:3]).max())
    e_r = float(np.abs(p32[..., 3:12].astype(np.float64) - p64[..., 3:12]).max())
    return p64, (e_c, e_r)


# ------------------------------------------------------------------------------------------------------------------ checks
def check_pixels(ref, rgba, depth, gid, what=""):
    """The interior-pixel checks of one frame; prints each figure before asserting it."""
    I = ref["interior"]
    ids_bad = int((gid[I] != ref["geom_id"][I]).sum())
    hit = I & np.isfinite(ref["depth"])
    derr = float(np.abs(depth[hit].astype(np.float64) - ref["depth"][hit]).max()) if hit.any() else 0.0
    miss_ok = bool(np.all(np.isinf(depth[I & ~hit]))) if (I & ~hit).any() else True
    cerr = np.abs(rgba[..., :3].astype(int) - ref["rgb"].astype(int)).max(-1)
    plain, blend = I & ~ref["blended"], I & ref["blended"]
    c_plain = int(cerr[plain].max()) if plain.any() else 0
    c_blend = int(cerr[blend].max()) if blend.any() else 0
    print(f"{what}: interior {int(I.sum())}/{I.size}, id mismatches {ids_bad}, depth err {derr:.3e} (bound {ref['depth_bound']:.3e} = 4 x {ref['depth_err32']:.3e}), "
          f"colour err plain {c_plain} blended {c_blend} ({int(blend.sum())} blended)")
    assert ids_bad == 0
    assert miss_ok
    assert derr <= ref["depth_bound"]
    assert c_plain <= 1 and c_blend <= 2
    assert np.all(rgba[..., 3] == 255)


def zoo_interior_counts(ref):
    """Interior pixels whose nearest opaque surface is each of the five types (ghost pixels count for what lies behind them too)."""
    prims, _ = zoo()
    ids = np.rint(prims[:, 18]).astype(int) // 256
    ko = ref["k_o"]
    return {t: int((ref["interior"] & (ko >= 0) & (ids[np.maximum(ko, 0)] == i)).sum()) for i, t in ZOO_TYPES.items()}


def walker_interior_share(ref):
    """Interior share of the pixels whose centre hits the walker or the ghost (not the floor, not the sky)."""
    plane_k = [k for k, r in enumerate(ref["prims"]) if int(round(r[18])) % 256 == rr.PLANE]
    on = ((ref["k_o"] >= 0) & ~np.isin(ref["k_o"], plane_k)) | (ref["k_g"] >= 0)
    return float((ref["interior"] & on).sum()) / max(int(on.sum()), 1), int(on.sum())
