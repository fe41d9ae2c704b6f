"""ctypes wrapper of the TEST-ONLY host emulation of the renderer's C-ABI (tests/hostemu/render_emu.cpp): numpy arrays in, numpy arrays out,
the entry points and refusals of include/tmjx.h's tmjx_render_* one for one."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests.hostemu import loader
from track_mjx_amd.hip import Camera, RenderInfo

_HERE = Path(__file__).resolve().parent
_FP = C.POINTER(C.c_float)


def _lib():
    L = loader.load("render_emu.cpp")
    vp = C.c_void_p
    L.remu_create.restype = vp
    L.remu_create.argtypes = [C.c_char_p, C.c_size_t]
    L.remu_last_error.restype = C.c_char_p
    L.remu_destroy.argtypes = [vp]
    L.remu_info.argtypes = [vp, C.c_int, C.c_int, C.POINTER(RenderInfo)]
    L.remu_camera.argtypes = [vp, C.c_char_p, C.POINTER(Camera)]
    L.remu_pose.argtypes = [vp, _FP, _FP, C.c_int, C.c_int, C.POINTER(Camera), _FP]
    L.remu_prims.argtypes = [_FP, _FP] + [C.c_int] * 4 + [vp, _FP, vp]
    L.remu_render.argtypes = [vp, _FP, _FP, C.c_int, C.c_int, C.POINTER(Camera), C.c_int, C.c_int, _FP, vp, _FP, vp]
    return L


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main: render_emu.cpp, -DRENDER_EMU_MAIN), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DRENDER_EMU_MAIN", *flags, "-o", str(out), str(_HERE / "render_emu.cpp")], check=True, capture_output=True)
    return out


def make_camera(body, mode, offset, quat, fovy) -> Camera:
    c = Camera()
    c.body, c.mode, c.fovy = int(body), int(mode), float(fovy)
    c.offset[:] = [float(x) for x in offset]
    c.quat[:] = [float(x) for x in quat]
    return c


def _f(a):
    return None if a is None else a.ctypes.data_as(_FP)


def _aligned(n, dtype=np.float32):
    raw = np.zeros(n * np.dtype(dtype).itemsize + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * np.dtype(dtype).itemsize].view(dtype)


class RenderEmu:
    def __init__(self, blob: bytes):
        self.L = _lib()
        self.h = C.c_void_p(self.L.remu_create(blob, len(blob)))
        if not self.h:
            raise ValueError(self.L.remu_last_error().decode())

    def __del__(self):
        try:
            self.L.remu_destroy(self.h)
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ValueError(self.L.remu_last_error().decode())

    def info(self, F: int, ghost: bool) -> RenderInfo:
        out = RenderInfo()
        self._check(self.L.remu_info(self.h, F, int(ghost), C.byref(out)))
        return out

    def camera(self, name: str) -> Camera:
        out = Camera()
        self._check(self.L.remu_camera(self.h, name.encode(), C.byref(out)))
        return out

    def _frames(self, qpos, qghost):
        q = np.ascontiguousarray(qpos, np.float32)
        g = None if qghost is None else np.ascontiguousarray(qghost, np.float32)
        return q, g, q.shape[0], 0 if g is None else g.shape[0]

    def pose(self, qpos, qghost, cam: Camera):
        """-> (cams [F, 16], prims [F, P, 20]) float32, views of one workspace."""
        q, g, F, Fg = self._frames(qpos, qghost)
        info = self.info(max(F, 1), g is not None)
        ws = _aligned(int(info.workspace_floats))
        self._check(self.L.remu_pose(self.h, _f(q), _f(g), F, Fg, C.byref(cam), _f(ws)))
        o = int(info.prims_offset)
        return ws[:o].reshape(F, info.cam_floats), ws[o:o + F * info.nprim * info.rec_floats].reshape(F, info.nprim, info.rec_floats)

    @staticmethod
    def _outs(F, H, W):
        return np.zeros((F, H, W, 4), np.uint8), np.zeros((F, H, W), np.float32), np.zeros((F, H, W), np.int32)

    def prims(self, prims, cams, W: int, H: int):
        """-> (rgba uint8 [F, H, W, 4], depth [F, H, W], geom_id [F, H, W])."""
        p = np.ascontiguousarray(prims, np.float32)
        pa = _aligned(p.size)
        pa[:] = p.ravel()
        c = np.ascontiguousarray(cams, np.float32)
        F, P = p.shape[0], p.shape[1]
        rgba, depth, gid = self._outs(F, max(H, 0), max(W, 0))
        self._check(self.L.remu_prims(_f(pa), _f(c), F, P, W, H, rgba.ctypes.data, _f(depth), gid.ctypes.data))
        return rgba, depth, gid

    def render(self, qpos, qghost, cam: Camera, W: int, H: int):
        q, g, F, Fg = self._frames(qpos, qghost)
        info = self.info(max(F, 1), g is not None)
        ws = _aligned(int(info.workspace_floats))
        rgba, depth, gid = self._outs(F, max(H, 0), max(W, 0))
        self._check(self.L.remu_render(self.h, _f(q), _f(g), F, Fg, C.byref(cam), W, H, _f(ws), rgba.ctypes.data, _f(depth), gid.ctypes.data))
        return rgba, depth, gid
