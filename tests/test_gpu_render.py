"""The roll-out renderer's kernels (csrc/tmjx_render.hip) against the float64 reference (tests/render_ref.py) under the bounds of
tests/render_scenes.py, the bit-for-bit identities between the entry points, and the refusals.  Measured on an MI355X (the reference-side number
each bound is 4 x of in brackets; DESIGN.md "Rendering" keeps the table): see profiles/render_bench.txt and DESIGN.md."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import render_ref as rr
from tests import render_scenes as S
from tests.common import default_walker
from track_mjx_amd import blob as _blob
from track_mjx_amd import hip
from track_mjx_amd import walker as _walker
from track_mjx_amd.analysis.render import Renderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = tuple(S.WALKERS)


@functools.lru_cache(None)
def renderer(config="torque090", camera="close_profile", size=(S.W, S.H)):
    w, _ = S.make_walker(config)
    cam = S.close_camera(w) if camera == "close" else camera
    if isinstance(cam, dict):
        cam = dict(cam, mode="trackcom")
    return Renderer(w, DEV, height=size[1], width=size[0], camera=cam), w


def host(t):
    return tuple(x.cpu().numpy() for x in t)


def same_bits(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


@pytest.mark.parametrize("config", CONFIGS)
def test_pose(config):
    r, w = renderer(config)
    p64, (e_c, e_r) = S.pose_reference(config)
    cams, prims = host(r.pose(S.pose_frames(config)))
    err_c = np.abs(prims[..., 0:3] - p64[..., 0:3]).max()
    err_r = np.abs(prims[..., 3:12] - p64[..., 3:12]).max()
    print(f"{config}: centre err {err_c:.3e} (reference float32 {e_c:.3e}), rotation err {err_r:.3e} (reference float32 {e_r:.3e})")
    assert err_c <= 4 * e_c and err_r <= 4 * e_r
    np.testing.assert_array_equal(prims[..., 12:18], p64[..., 12:18].astype(np.float32))
    np.testing.assert_array_equal(prims[..., 18:20].view(np.int32), rr.pack_prims(p64)[..., 18:20].view(np.int32))
    m = S.walker_setup(config)[1]
    for f, q in enumerate(S.pose_frames(config)):
        want = rr.camera_record(m, rr.named_camera(w, "close_profile"), q.astype(np.float64))
        np.testing.assert_allclose(cams[f, :13], want[:13], atol=4 * e_c + 1e-7)


@pytest.mark.parametrize("size", S.SIZES)
def test_zoo(size):
    r, _ = renderer()
    prims, cam = S.zoo()
    ref = S.zoo_reference(*size)
    rgba, depth, gid = host(r.render_prims(rr.pack_prims(prims)[None], cam.astype(np.float32)[None], height=size[1], width=size[0]))
    S.check_pixels(ref, rgba[0], depth[0], gid[0], f"zoo {size}")


def test_walker():
    r, w = renderer(camera="close")
    q, g = S.walker_frames()
    rgba, depth, gid = host(r.render_device(q, g))
    for f, ref in enumerate(S.walker_reference()):
        share, n = S.walker_interior_share(ref)
        assert share >= 0.60, (f, share)
        S.check_pixels(ref, rgba[f], depth[f], gid[f], f"walker frame {f}")


def test_identities():
    r, w = renderer(size=(75, 50))
    q, g = S.walker_frames()
    full = host(r.render_device(q, g))
    same_bits([x[1] for x in full], [x[0] for x in host(r.render_device(q[1:2], g[1:2]))])      # frame k of a batch = that frame alone
    cams, prims = r.pose(q, g)
    same_bits(full, host(r.render_prims(prims, cams)))                                           # tmjx_render = pose, then prims
    off = host(r.render_device(q, None))
    nvis = r.info(1, True).ngeom
    no_ghost = full[2] < nvis
    assert no_ghost.any() and (~no_ghost).any()
    same_bits([x[no_ghost] for x in full], [x[no_ghost] for x in off])                           # ghost on = ghost off where no ghost is reported
    byhand = Renderer(w, DEV, height=50, width=75, camera=dict(rr.named_camera(w, "close_profile"), mode="trackcom"))
    same_bits(full, host(byhand.render_device(q, g)))                                            # a named camera = the same camera by hand
    frames, depth, ids = r.render(q, g, return_depth=True, return_ids=True)                      # the public call: the same pixels, rgb only
    same_bits([frames, depth, ids], [full[0][..., :3], full[1], full[2]])
    ego = host(renderer(camera="egocentric", size=(75, 50))[0].render_device(q, g))
    assert (ego[2] >= 0).any()


def test_refusals():
    r, w = renderer()
    q, g = S.walker_frames()
    bare = _walker.build_blob(w, n_frames=1, iterations=1, ls_iterations=1, timestep=0.002, mocap_hz=50, clip_length=250, traj_length=5, window=50,
                              episode_length=1, reward_f=np.zeros(25))
    bare = _blob.pack({k: v for k, v in _blob.unpack(bare).items() if not k.startswith(("rgeom_", "rcam_"))})
    with pytest.raises(hip.TmjxError, match="no render tables"):
        Renderer(w, DEV, blob=bare)
    with pytest.raises(hip.TmjxError, match="unknown camera 'nose'"):
        Renderer(w, DEV, camera="nose")
    with pytest.raises(hip.TmjxError, match="ghost frames: 2 frames against 3"):
        r.render_device(q, g[:2])
    with pytest.raises(hip.TmjxError, match="F must be >= 1"):
        r.render_device(q[:0], None)
    with pytest.raises(hip.TmjxError, match="W and H must be >= 1"):
        Renderer(w, DEV, height=0, width=8).render_device(q, g)
    torch.cuda.synchronize()


def test_cli_frame_0_is_renderer_render(tmp_path):
    """python -m track_mjx_amd.analysis.render on a synthetic clip_0.h5: frame 0 of clip_0.frames.h5 is Renderer.render on the same qpos."""
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import render as R
    w, m, qpos = S.walker_setup()
    (tmp_path / "in").mkdir()
    h5lite.write_tree(tmp_path / "in" / "clip_0.h5", {"qposes_rollout": qpos[0, :5], "qposes_ref": qpos[1, :5]})
    assert R.main([f"rollouts={tmp_path / 'in'}", f"out={tmp_path / 'out'}", "size=40x30", "camera=side"]) == 0
    with h5lite.File(tmp_path / "out" / "clip_0.frames.h5") as h:
        frames, fps = h["frames"][()], float(h["fps"][()])
    assert frames.shape == (5, 30, 40, 3) and frames.dtype == np.uint8 and fps == pytest.approx(50.0)
    want = Renderer(w, DEV, height=30, width=40, camera="side").render(qpos[0, :1], qpos[1, :1])
    np.testing.assert_array_equal(frames[0], want[0])
    assert len(np.unique(frames[0].reshape(-1, 3), axis=0)) > 10      # a picture, not a constant
