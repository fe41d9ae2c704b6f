"""ctypes wrapper of the TEST-ONLY host emulation of the wide PCA C-ABI (tests/hostemu/pca_wide_emu.cpp): tmjx_pca_wide_workspace,
tmjx_pca_fit_wide and tmjx_pca_transform_wide one for one on numpy arrays, and `EmuWideBackend`, the stand-in for analysis.pca.HipBackend with
`fit_wide` / `transform_wide` beside the narrow methods."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests.hostemu import pca_emu as _narrow
from track_mjx_amd.hip import PcaInfo, StripStyle

_HERE = Path(__file__).resolve().parent
_CSRC = _HERE.parents[1] / "track_mjx_amd" / "csrc"
_lib_cache = None


def _lib():
    global _lib_cache
    if _lib_cache is not None:
        return _lib_cache
    src = [_HERE / "pca_wide_emu.cpp", _HERE / "pca_emu.cpp", _CSRC / "pca_core.h", _CSRC / "pca_host.h", _CSRC / "pca_wide_core.h", _CSRC / "pca_wide_host.h",
           _HERE.parents[1] / "include" / "tmjx.h"]
    so = _HERE / "libpca_wide_emu.so"
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in src):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(_HERE / "pca_wide_emu.cpp")], check=True, capture_output=True)
    L = C.CDLL(str(so))
    vp = C.c_void_p
    L.pemu_last_error.restype = C.c_char_p
    L.pwemu_workspace.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.pwemu_fit.argtypes = [vp, C.c_int, C.c_int, C.c_int64, vp, vp, vp, vp, C.POINTER(PcaInfo)]
    L.pwemu_transform.argtypes = [vp, C.c_int, C.c_int, C.c_int64, vp, vp, C.c_int, vp, C.c_int64]
    L.pemu_strips.argtypes = [vp, C.c_int, C.c_int, C.c_int64, vp, vp, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(StripStyle), C.c_int, C.c_int, vp]
    _lib_cache = L
    return L


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main: -DPCA_WIDE_EMU_MAIN), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DPCA_WIDE_EMU_MAIN", *flags, "-o", str(out), str(_HERE / "pca_wide_emu.cpp")], check=True,
                   capture_output=True)
    return out


def _check(rc):
    if rc != 0:
        raise ValueError(_lib().pemu_last_error().decode())


_aligned, _ld = _narrow._aligned, _narrow._ld


def workspace(n: int, d: int) -> int:
    out = C.c_int64(0)
    _check(_lib().pwemu_workspace(n, d, C.byref(out)))
    return int(out.value)


def fit_wide(x, n=None, d=None, ldx=None):
    """x float32 [n, d] whose columns are contiguous (a row stride is fine); n / d / ldx override what is passed down (the refusal tests)."""
    n, d, ldx = x.shape[0] if n is None else n, x.shape[1] if d is None else d, _ld(x) if ldx is None else ldx
    ws = _aligned(workspace(n, d))
    mean, comp, var, info = np.zeros(d, np.float32), np.zeros((d, d), np.float32), np.zeros(d, np.float32), PcaInfo()
    _check(_lib().pwemu_fit(x.ctypes.data, n, d, ldx, mean.ctypes.data, comp.ctypes.data, var.ctypes.data, ws.ctypes.data, C.byref(info)))
    return mean, comp, var, info


def transform_wide(x, mean, components, k=None, ldx=None, ldo=None):
    n, d = x.shape
    k = components.shape[0] if k is None else k
    ldo = k if ldo is None else ldo
    out = np.zeros((n, max(k, ldo, 1)), np.float32)
    m, c = np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(components, np.float32)
    _check(_lib().pwemu_transform(x.ctypes.data, n, d, _ld(x) if ldx is None else ldx, m.ctypes.data, c.ctypes.data, k, out.ctypes.data, ldo))
    return out[:, :max(k, 1)]


class EmuWideBackend(_narrow.EmuBackend):
    """analysis.pca.HipBackend's methods on the host emulation, the wide ones included."""

    fit_wide = staticmethod(fit_wide)
    transform_wide = staticmethod(transform_wide)
