"""Rendering roll-outs: the walker and a translucent ghost driven by the clip, ray-cast on the GPU (csrc/tmjx_render.hip; DESIGN.md "Rendering").

Reference: track_mjx/analysis/render.py:render_rollout (MuJoCo's GL renderer on a model with a ghost copy attached).  Here the model's
analytic primitives are ray-cast directly: no meshes, textures, shadows, sites or contact markers; what is drawn and how it is shaded is fixed
in DESIGN.md so that a float64 restatement can check it.

    python -m track_mjx_amd.analysis.render rollouts=<dir of clip_<i>.h5> out=<dir> [camera=close_profile] [size=640x480] [ghost=true] [every=1]
        [checkpoint=<run dir | step dir>] [pca=<pca.h5>] [pca_window=530] [key=value config overrides ...]

writes clip_<i>.frames.h5 (frames uint8 [F, H, W, 3], fps, camera) per roll-out file, and clip_<i>.gif where PIL imports.  With pca=<the file
python -m track_mjx_amd.analysis.pca wrote> every frame carries the PCA-progression panel on its right (reference: render_with_pca_progression;
DESIGN.md "PCA") and the file also holds pca_feature, pca_explained_variance_ratio and pca_colors: the legend as data, no text is drawn.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import sys

import numpy as np

from .. import hip as _hip
from .. import walker as _walker
from . import cli
from .backend import resolve

CLI_OPTIONS = ("rollouts", "out", "camera", "size", "ghost", "every", "checkpoint", "step", "pca", "pca_window")
MAX_FRAMES_PER_CALL = 64      # frames rendered per launch pair: bounds the output buffers (64 frames of 640 x 480: 79 MB rgba)


def _camera_struct(cam) -> _hip.Camera:
    if isinstance(cam, _hip.Camera):
        return cam
    modes = {"fixed": _hip.CAMERA_FIXED, "track": _hip.CAMERA_TRACK, "trackcom": _hip.CAMERA_TRACKCOM}
    c = _hip.Camera()
    c.body, c.mode, c.fovy = int(cam["body"]), int(modes.get(cam["mode"], cam["mode"])), float(cam["fovy"])
    c.offset[:] = [float(x) for x in cam["offset"]]
    c.quat[:] = [float(x) for x in cam["quat"]]
    return c


class Renderer:
    """Renders qpos frames of `walker` from one camera: `camera` a name of walker.cameras(), a dict {body, mode, offset, quat, fovy} or a
    hip.Camera (include/tmjx.h: tmjx_camera_t)."""

    def __init__(self, walker: _walker.Rodent, device="cuda", height: int = 480, width: int = 640, camera="close_profile", render_ghost: bool = True,
                 blob: bytes | None = None, lib=None):
        """`blob`: a packed model blob for the handle (default: the walker's with a placeholder task configuration); `lib`: a hip.load()ed
        alternative build of the library (A/B runs: tools/render_bench.py)."""
        import torch
        self.walker, self.device = walker, torch.device(device)
        self.height, self.width, self.render_ghost = int(height), int(width), bool(render_ghost)
        self._L = _hip.lib() if lib is None else lib
        self._handle = C.c_void_p()
        if blob is None:      # the task's configuration is not the renderer's business: any valid one makes a handle
            blob = _walker.build_blob(walker, n_frames=1, iterations=1, ls_iterations=1, timestep=0.002, mocap_hz=50, clip_length=250, traj_length=5,
                                      window=50, episode_length=1, reward_f=np.zeros(25))
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_model_create(blob, len(blob), C.byref(self._handle)), "tmjx_model_create")
        self.camera_name = camera if isinstance(camera, str) else None
        if isinstance(camera, str):
            self.camera = _hip.Camera()
            _hip.check(self._L.tmjx_render_camera(self._handle, camera.encode(), C.byref(self.camera)), "tmjx_render_camera")
        else:
            self.camera = _camera_struct(camera)
        self.info(1, False)      # a handle without render tables is refused here, by name

    def __del__(self):
        try:
            if self._handle:
                self._L.tmjx_model_destroy(self._handle)
                self._handle = C.c_void_p()
        except Exception:
            pass

    def info(self, F: int, ghost: bool) -> _hip.RenderInfo:
        out = _hip.RenderInfo()
        _hip.check(self._L.tmjx_render_info(self._handle, int(F), int(ghost), C.byref(out)), "tmjx_render_info")
        return out

    def _frames(self, qposes, qposes_ref):
        import torch
        q = torch.as_tensor(np.asarray(qposes, np.float32) if not isinstance(qposes, torch.Tensor) else qposes, dtype=torch.float32, device=self.device)
        if q.dim() != 2 or q.shape[1] != self.walker.nq:
            raise ValueError(f"qposes must be [F, {self.walker.nq}], got {tuple(q.shape)}")
        g = None
        if qposes_ref is not None and self.render_ghost:
            g = torch.as_tensor(np.asarray(qposes_ref, np.float32) if not isinstance(qposes_ref, torch.Tensor) else qposes_ref, dtype=torch.float32,
                                device=self.device)
            if g.dim() != 2 or g.shape[1] != self.walker.nq:
                raise ValueError(f"qposes_ref must be [F, {self.walker.nq}], got {tuple(g.shape)}")
            g = g.contiguous()
        return q.contiguous(), g

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def pose(self, qposes, qposes_ref=None):
        """Stage A alone: (cams [F, 16], prims [F, P, 20]) float32 device tensors, views of one workspace."""
        import torch
        q, g = self._frames(qposes, qposes_ref)
        F, Fg = q.shape[0], 0 if g is None else g.shape[0]
        info = self.info(max(F, 1), g is not None)
        ws = torch.empty(int(info.workspace_floats), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_render_pose(self._handle, q.data_ptr(), None if g is None else g.data_ptr(), F, Fg, C.byref(self.camera),
                                                ws.data_ptr(), self._stream()), "tmjx_render_pose")
        o = int(info.prims_offset)
        return ws[:o].view(F, info.cam_floats), ws[o:o + F * info.nprim * info.rec_floats].view(F, info.nprim, info.rec_floats)

    def render_prims(self, prims, cams, height: int | None = None, width: int | None = None):
        """Stage B alone on caller-supplied tables: (rgba uint8 [F, H, W, 4], depth [F, H, W], geom_id [F, H, W]) device tensors."""
        import torch
        H, W = self.height if height is None else int(height), self.width if width is None else int(width)
        p = torch.as_tensor(prims, dtype=torch.float32, device=self.device).contiguous()
        c = torch.as_tensor(cams, dtype=torch.float32, device=self.device).contiguous()
        if p.dim() != 3 or c.dim() != 2 or c.shape[0] != p.shape[0]:
            raise ValueError("prims must be [F, P, 20] and cams [F, 16]")
        F, P = p.shape[0], p.shape[1]
        rgba, depth, gid = self._outputs(F, H, W)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_render_prims(p.data_ptr(), c.data_ptr(), F, P, W, H, rgba.data_ptr(), depth.data_ptr(), gid.data_ptr(), self._stream()),
                       "tmjx_render_prims")
        return rgba, depth, gid

    def _outputs(self, F, H, W, depth=True, ids=True):
        import torch
        shape = (F, max(H, 0), max(W, 0))
        return (torch.empty(shape + (4,), dtype=torch.uint8, device=self.device),
                torch.empty(shape, dtype=torch.float32, device=self.device) if depth else None,
                torch.empty(shape, dtype=torch.int32, device=self.device) if ids else None)

    def render_device(self, qposes, qposes_ref=None, depth: bool = True, ids: bool = True):
        """One tmjx_render call: (rgba uint8 [F, H, W, 4], depth, geom_id) device tensors (None for an output not asked for), nothing synchronised."""
        import torch
        q, g = self._frames(qposes, qposes_ref)
        F, Fg = q.shape[0], 0 if g is None else g.shape[0]
        info = self.info(max(F, 1), g is not None)
        ws = torch.empty(int(info.workspace_floats), dtype=torch.float32, device=self.device)
        rgba, dep, gid = self._outputs(F, self.height, self.width, depth, ids)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_render(self._handle, q.data_ptr(), None if g is None else g.data_ptr(), F, Fg, C.byref(self.camera), self.width,
                                           self.height, ws.data_ptr(), rgba.data_ptr(), None if dep is None else dep.data_ptr(), None if gid is None else gid.data_ptr(),
                                           self._stream()), "tmjx_render")
        return rgba, dep, gid

    def render(self, qposes, qposes_ref=None, return_depth: bool = False, return_ids: bool = False):
        """uint8 [F, H, W, 3] on the host (with return_depth / return_ids: a tuple with float32 [F, H, W] / int32 [F, H, W] behind it)."""
        q, g = self._frames(qposes, qposes_ref)
        outs = [[], [], []]
        for i in range(0, q.shape[0], MAX_FRAMES_PER_CALL):
            part = self.render_device(q[i:i + MAX_FRAMES_PER_CALL], None if g is None else g[i:i + MAX_FRAMES_PER_CALL], return_depth, return_ids)
            outs[0].append(part[0][..., :3].cpu().numpy())
            if return_depth:
                outs[1].append(part[1].cpu().numpy())
            if return_ids:
                outs[2].append(part[2].cpu().numpy())
        if not outs[0]:
            self.render_device(q, g)      # F = 0: refused by name
        res = [np.concatenate(outs[0], 0)] + ([np.concatenate(outs[1], 0)] if return_depth else []) + ([np.concatenate(outs[2], 0)] if return_ids else [])
        return res[0] if len(res) == 1 else tuple(res)


def _get(node, key, default=None):
    return node.get(key, default) if hasattr(node, "get") else getattr(node, key, default)


def render_fps(cfg) -> float:
    """The reference's rule (analysis/render.py:217-223): real time, 1 / timestep / physics_steps_per_control_step, unless env_config.render_fps is set."""
    env = _get(cfg, "env_config")
    fps = _get(env, "render_fps", None)
    if fps is not None:
        return float(fps)
    ea = _get(env, "env_args")
    return 1.0 / float(_get(ea, "mj_model_timestep")) / float(_get(ea, "physics_steps_per_control_step"))


def render_rollout(cfg, rollout, height: int = 480, width: int = 640, render_ghost: bool = True, device="cuda", every: int = 1, camera: str | None = None,
                   renderer_cls=None):
    """(frames uint8 [F, H, W, 3], fps) of a roll-out's qposes_rollout, with the ghost at qposes_ref (reference: analysis/render.py:render_rollout).
    The camera is env_config.render_camera_name (default close_profile).  `renderer_cls`: a stand-in for Renderer with its constructor and
    `.render` (the CPU tests pass the host emulation's)."""
    wc = dict(_get(cfg, "walker_config"))
    w = _walker.Rodent(**wc)
    name = camera or _get(_get(cfg, "env_config"), "render_camera_name", "close_profile") or "close_profile"
    r = (renderer_cls or Renderer)(w, device, height=height, width=width, camera=name, render_ghost=render_ghost)
    q = np.asarray(rollout["qposes_rollout"], np.float32)[::every]
    g = np.asarray(rollout["qposes_ref"], np.float32)[::every] if render_ghost else None
    return r.render(q, g), render_fps(cfg)


def plot_pca_progression(projections, frame_idx, n_components: int = 4, window_size: int = 530, size=(640, 480), terminated=None, device="cuda",
                         backend=None, style=None) -> np.ndarray:
    """The progression panel of every frame (reference: plot_pca_intention, one matplotlib figure per frame): uint8 [F, H, Wp, 3].  Frame f shows the
    first `n_components` columns of `projections` [T, K] over the timesteps [0, frame_idx[f]); `terminated` [F] bool marks the frames that draw the
    terminated line.  The y limits are min - 0.2 / max + 0.2 over those columns of the whole clip, as the reference takes them.  Drawn in batches of
    MAX_FRAMES_PER_CALL frames; `backend`: a stand-in for pca.HipBackend."""
    from . import pca as _pca
    b = resolve(backend, device)
    width, height = int(size[0]), int(size[1])
    host = projections if isinstance(projections, np.ndarray) else None
    p = b.asarray(projections)
    k = int(n_components)
    if not 1 <= k <= min(int(p.shape[1]), _hip.PCA_MAX_K):
        raise ValueError(f"n_components = {k}: a panel draws 1 .. {min(int(p.shape[1]), _hip.PCA_MAX_K)} of the {int(p.shape[1])} projected components")
    idx = np.asarray(frame_idx, np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() > p.shape[0]):
        raise ValueError(f"frame_idx must lie in [0, {int(p.shape[0])}] (got {int(idx.min())} .. {int(idx.max())})")
    flags = np.zeros(idx.size, np.uint8) if terminated is None else np.asarray(terminated).reshape(-1).astype(bool).astype(np.uint8)
    if flags.size != idx.size:
        raise ValueError(f"terminated has {flags.size} entries for {idx.size} frames")
    cols = (host if host is not None else b.to_numpy(p))[:, :k]
    finite = cols[np.isfinite(cols)]
    lo, hi = (float(finite.min()), float(finite.max())) if finite.size else (0.0, 0.0)
    st = _pca.strip_style(width, height) if style is None else style
    out = [b.strips(p, k, idx[i:i + MAX_FRAMES_PER_CALL], flags[i:i + MAX_FRAMES_PER_CALL], lo - 0.2, hi + 0.2, int(window_size), st, width, height)[..., :3]
           for i in range(0, idx.size, MAX_FRAMES_PER_CALL)]
    return np.concatenate(out, 0) if out else np.zeros((0, height, width, 3), np.uint8)


def render_with_pca_progression(cfg, rollout, pca_projections, n_components: int = 4, feature_name: str = "ctrl", hold: int = 50, window_size: int = 530,
                                panel_width: int = 640, backend=None, **render_kwargs):
    """(frames uint8 [F + hold, H, W + Wp, 3], fps): render_rollout's frames with the progression panel on the right (reference:
    render_with_pca_progression).  Frame f shows the curves up to timestep f * every; the last frame is repeated `hold` times with the terminated
    line, the reference's stoppage.  `feature_name` is not drawn (no text in the panel): the command-line tool stores it beside the frames.
    `render_kwargs` go to render_rollout (height, width, every, camera, render_ghost, device, renderer_cls)."""
    frames, fps = render_rollout(cfg, rollout, **render_kwargs)
    every = int(render_kwargs.get("every", 1))
    T = int(np.shape(pca_projections)[0])
    idx = np.minimum(np.arange(frames.shape[0]) * every, T)
    idx = np.concatenate([idx, idx[-1:]])                      # the last frame once more, terminated
    term = np.zeros(idx.size, bool)
    term[-1] = True
    panel = plot_pca_progression(pca_projections, idx, n_components, window_size, (int(panel_width), frames.shape[1]), term,
                                 device=render_kwargs.get("device", "cuda"), backend=backend)
    wide = np.concatenate([frames, panel[:-1]], 2)
    stop = np.concatenate([frames[-1], panel[-1]], 1)[None]
    return np.concatenate([wide, np.repeat(stop, int(hold), 0)], 0), fps


def _write_gif(path, frames, fps) -> bool:
    try:
        from PIL import Image
    except Exception:
        return False
    imgs = [Image.fromarray(f) for f in frames]
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=max(int(round(1000.0 / fps)), 10), loop=0)
    return True


def main(argv=None, renderer_cls=None, pca_backend=None) -> int:
    from .. import config as _config
    from .. import h5lite
    opts, rest = cli.split(list(sys.argv[1:] if argv is None else argv), CLI_OPTIONS)      # (the rest: config overrides)
    if "rollouts" not in opts or "out" not in opts:
        print("usage: python -m track_mjx_amd.analysis.render rollouts=<dir of clip_<i>.h5> out=<dir> [camera=close_profile] [size=640x480] "
              "[ghost=true] [every=1] [checkpoint=<run dir | step dir>] [pca=<pca.h5>] [pca_window=530] [key=value config overrides ...]", file=sys.stderr)
        return 2
    cfg = _config.default_config()
    if "checkpoint" in opts:
        from ..agent import checkpoint as ckpt
        cfg = _config._deep_update(cfg, ckpt.load_config_from_checkpoint(opts["checkpoint"], int(opts["step"]) if "step" in opts else None) or {})
    for ov in rest:                                   # the same key=value parsing as train
        import yaml
        key, _, val = ov.partition("=")
        node = cfg
        for part in key.split(".")[:-1]:
            node = node.setdefault(part, {})
        node[key.split(".")[-1]] = yaml.safe_load(val)
    m = re.fullmatch(r"(\d+)x(\d+)", opts.get("size", "640x480"))
    if not m:
        print("[render] size=<width>x<height>", file=sys.stderr)
        return 2
    width, height = int(m.group(1)), int(m.group(2))
    ghost = str(opts.get("ghost", "true")).lower() in ("1", "true", "yes")
    every = max(int(opts.get("every", 1)), 1)
    files = sorted((f for f in os.listdir(opts["rollouts"]) if re.fullmatch(r"clip_\d+\.h5", f)), key=lambda f: int(f[5:-3]))
    if not files:
        print(f"[render] no clip_<i>.h5 in {opts['rollouts']}", file=sys.stderr)
        return 2
    os.makedirs(opts["out"], exist_ok=True)
    camera = opts.get("camera") or cfg["env_config"].get("render_camera_name", "close_profile") or "close_profile"
    gifs = 0
    pca = None
    if "pca" in opts:
        with h5lite.File(opts["pca"]) as h:
            pca = {"feature": bytes(h["feature"][()]).decode(), "ratio": np.asarray(h["explained_variance_ratio"][()], np.float32),
                   "projections": {k: np.asarray(h["projections"][k][()], np.float32) for k in h["projections"].keys()}}
    for f in files:
        with h5lite.File(os.path.join(opts["rollouts"], f)) as h:
            rollout = {k: np.asarray(h[k][()]) for k in ("qposes_rollout", "qposes_ref") if k in h}
        if ghost and "qposes_ref" not in rollout:
            print(f"[render] {f}: no qposes_ref (ghost=false renders without)", file=sys.stderr)
            return 2
        stem = f[:-3]
        tree = {}
        if pca is None:
            frames, fps = render_rollout(cfg, rollout, height=height, width=width, render_ghost=ghost, every=every, camera=camera, renderer_cls=renderer_cls)
        else:
            if stem not in pca["projections"]:
                print(f"[render] {opts['pca']} has no projections/{stem}", file=sys.stderr)
                return 2
            k = min(4, pca["ratio"].size, _hip.PCA_MAX_K)
            from . import pca as _pca
            frames, fps = render_with_pca_progression(cfg, rollout, pca["projections"][stem], n_components=k, feature_name=pca["feature"],
                                                      window_size=int(opts.get("pca_window", 530)), backend=pca_backend, height=height, width=width,
                                                      render_ghost=ghost, every=every, camera=camera, renderer_cls=renderer_cls)
            tree = {"pca_feature": pca["feature"], "pca_explained_variance_ratio": pca["ratio"][:k], "pca_colors": np.asarray(_pca.STRIP_COLOURS[:k], np.uint8)}
        fps = fps / every
        h5lite.write_tree(os.path.join(opts["out"], stem + ".frames.h5"), {"frames": frames, "fps": np.float64(fps), "camera": camera, **tree})
        gifs += _write_gif(os.path.join(opts["out"], stem + ".gif"), frames, fps)
    print(f"[render] wrote {len(files)} frame files to {opts['out']} ({width}x{height}, camera {camera}, ghost {ghost}, {gifs} gifs)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
