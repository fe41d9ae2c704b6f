"""ctypes wrapper of the TEST-ONLY host emulation of the PCA and panel C-ABI (tests/hostemu/pca_emu.cpp): the entry points and refusals of
include/tmjx.h's tmjx_pca_* and tmjx_plot_strips one for one on numpy arrays, and `EmuBackend`, the stand-in for analysis.pca.HipBackend."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from track_mjx_amd.hip import PcaInfo, StripStyle

_HERE = Path(__file__).resolve().parent
_CSRC = _HERE.parents[1] / "track_mjx_amd" / "csrc"
_FP = C.POINTER(C.c_float)
_lib_cache = None


def _lib():
    global _lib_cache
    if _lib_cache is not None:
        return _lib_cache
    src = [_HERE / "pca_emu.cpp", _CSRC / "pca_core.h", _CSRC / "pca_host.h", _HERE.parents[1] / "include" / "tmjx.h"]
    so = _HERE / "libpca_emu.so"
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in src):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(_HERE / "pca_emu.cpp")], check=True, capture_output=True)
    L = C.CDLL(str(so))
    vp = C.c_void_p
    L.pemu_last_error.restype = C.c_char_p
    L.pemu_workspace.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.pemu_fit.argtypes = [vp, C.c_int, C.c_int, C.c_int64, vp, vp, vp, vp, C.POINTER(PcaInfo)]
    L.pemu_transform.argtypes = [vp, C.c_int, C.c_int, C.c_int64, vp, vp, C.c_int, vp, C.c_int64]
    L.pemu_strips.argtypes = [vp, C.c_int, C.c_int, C.c_int64, vp, vp, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(StripStyle), C.c_int, C.c_int, vp]
    _lib_cache = L
    return L


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main: pca_emu.cpp, -DPCA_EMU_MAIN), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DPCA_EMU_MAIN", *flags, "-o", str(out), str(_HERE / "pca_emu.cpp")], check=True, capture_output=True)
    return out


def _check(rc):
    if rc != 0:
        raise ValueError(_lib().pemu_last_error().decode())


def _aligned(n, dtype=np.float32):
    raw = np.zeros(n * np.dtype(dtype).itemsize + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * np.dtype(dtype).itemsize].view(dtype)


def _ld(a) -> int:
    return a.strides[0] // 4


def workspace(n: int, d: int) -> int:
    out = C.c_int64(0)
    _check(_lib().pemu_workspace(n, d, C.byref(out)))
    return int(out.value)


def fit(x, n=None, d=None, ldx=None):
    """x float32 [n, d] whose columns are contiguous (a row stride is fine); n / d / ldx override what is passed down (the refusal tests)."""
    n, d, ldx = x.shape[0] if n is None else n, x.shape[1] if d is None else d, _ld(x) if ldx is None else ldx
    ws = _aligned(workspace(n, d))
    mean, comp, var, info = np.zeros(d, np.float32), np.zeros((d, d), np.float32), np.zeros(d, np.float32), PcaInfo()
    _check(_lib().pemu_fit(x.ctypes.data, n, d, ldx, mean.ctypes.data, comp.ctypes.data, var.ctypes.data, ws.ctypes.data, C.byref(info)))
    return mean, comp, var, info


def transform(x, mean, components, k=None, ldx=None, ldo=None):
    n, d = x.shape
    k = components.shape[0] if k is None else k
    out = np.zeros((n, max(k, 1)), np.float32)
    m, c = np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(components, np.float32)
    _check(_lib().pemu_transform(x.ctypes.data, n, d, _ld(x) if ldx is None else ldx, m.ctypes.data, c.ctypes.data, k, out.ctypes.data, k if ldo is None else ldo))
    return out


def strips(proj, k, frame_idx, flags, ymin, ymax, window, style, width, height, T=None, ldp=None):
    fi = np.ascontiguousarray(frame_idx, np.int32)
    fl = None if flags is None else np.ascontiguousarray(flags, np.uint8)
    out = np.zeros((fi.shape[0], max(height, 0), max(width, 0), 4), np.uint8)
    _check(_lib().pemu_strips(proj.ctypes.data, proj.shape[0] if T is None else T, k, _ld(proj) if ldp is None else ldp, fi.ctypes.data,
                              None if fl is None else fl.ctypes.data, fi.shape[0], ymin, ymax, window, C.byref(style), width, height, out.ctypes.data))
    return out


class EmuBackend:
    """analysis.pca.HipBackend's methods on the host emulation."""

    @staticmethod
    def asarray(x):
        a = np.asarray(x)
        if a.ndim != 2:
            raise ValueError(f"expected a 2-D array [n, d], got shape {a.shape}")
        ok = a.dtype == np.float32 and a.strides[1] == 4 and a.strides[0] >= 4 * a.shape[1] and a.strides[0] % 4 == 0
        return a if ok else np.ascontiguousarray(a, np.float32)

    @staticmethod
    def to_numpy(t):
        return t

    fit = staticmethod(fit)
    transform = staticmethod(transform)
    strips = staticmethod(strips)
