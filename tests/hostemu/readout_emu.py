"""ctypes wrapper of the TEST-ONLY host emulation of the readout C-ABI (tests/hostemu/readout_emu.cpp): tmjx_readout_workspace, _fit, _weights,
_predict and _score one for one on numpy arrays, and `EmuReadoutBackend`, the stand-in for analysis.pca.HipBackend with the `readout_*` methods
beside the PCA's."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests.hostemu import pca_emu as _narrow
from tests.hostemu import pca_wide_emu as _wide
from track_mjx_amd.hip import PcaInfo

_HERE = Path(__file__).resolve().parent
_CSRC = _HERE.parents[1] / "track_mjx_amd" / "csrc"
_lib_cache = None


def _lib():
    global _lib_cache
    if _lib_cache is not None:
        return _lib_cache
    src = [_HERE / "readout_emu.cpp", _HERE / "pca_wide_emu.cpp", _HERE / "pca_emu.cpp", _HERE.parents[1] / "include" / "tmjx.h",
           *[_CSRC / f for f in ("pca_core.h", "pca_host.h", "pca_wide_core.h", "pca_wide_host.h", "readout_core.h", "readout_host.h")]]
    so = _HERE / "libreadout_emu.so"
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in src):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(_HERE / "readout_emu.cpp")], check=True, capture_output=True)
    L = C.CDLL(str(so))
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.pemu_last_error.restype = C.c_char_p
    L.remu_workspace.argtypes = [i, i, i, i, C.POINTER(i64)]
    L.remu_extents.argtypes = [i, i, i, i, C.POINTER(i64), C.POINTER(i64)]
    L.remu_fit.argtypes = [vp, i, i, i64, vp, i, i64, vp, vp, vp, vp, vp, vp, C.POINTER(PcaInfo)]
    L.remu_weights.argtypes = [vp, vp, vp, i, i, vp, i, vp]
    L.remu_predict.argtypes = [vp, i, i, i64, vp, vp, vp, i, vp, i64]
    L.remu_score.argtypes = [vp, i, i, i64, vp, i, i64, vp, vp, vp, i, vp, vp, vp]
    _lib_cache = L
    return L


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main: -DREADOUT_EMU_MAIN), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DREADOUT_EMU_MAIN", *flags, "-o", str(out), str(_HERE / "readout_emu.cpp")], check=True,
                   capture_output=True)
    return out


def _check(rc):
    if rc != 0:
        raise ValueError(_lib().pemu_last_error().decode())


_aligned, _ld = _narrow._aligned, _narrow._ld
_f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731


def workspace(n: int, d: int, m: int, n_lambda: int) -> int:
    out = C.c_int64(0)
    _check(_lib().remu_workspace(n, d, m, n_lambda, C.byref(out)))
    return int(out.value)


def extents(n: int, d: int, m: int, n_lambda: int):
    """(fit, score): the floats a fit and a score of exactly n rows touch from the start of the workspace."""
    fit, score = C.c_int64(0), C.c_int64(0)
    _check(_lib().remu_extents(n, d, m, n_lambda, C.byref(fit), C.byref(score)))
    return int(fit.value), int(score.value)


GUARD = 1 << 16      # floats behind a workspace sized for `ws_rows`
_CANARY = np.float32(-7.25)


def _guarded(floats: int):
    ws = _aligned(floats + GUARD)
    ws[floats:] = _CANARY
    return ws


def _guard_intact(ws, floats: int):
    if not (ws[floats:] == _CANARY).all():
        raise AssertionError(f"the call wrote behind its workspace of {floats} floats (first at +{int(np.argmax(ws[floats:] != _CANARY))})")


def readout_fit(x, y, n=None, d=None, m=None, ldx=None, ldy=None, misalign=False, ws_rows=None, n_lambda=1):
    """x [n, d], y [n, m] float32 whose columns are contiguous (a row stride is fine) -> (mean_x, components, variance, mean_y, z, info);
    n / d / m / ldx / ldy override what is passed down and `misalign` shifts the workspace by 4 bytes (the refusal tests).  With `ws_rows` the
    workspace is exactly tmjx_readout_workspace's of that many rows and `n_lambda` penalties, with a guard behind it that must come back untouched."""
    n, d, m = x.shape[0] if n is None else n, x.shape[1] if d is None else d, y.shape[1] if m is None else m
    ldx, ldy = _ld(x) if ldx is None else ldx, _ld(y) if ldy is None else ldy
    ok = 2 <= n and 1 <= d <= 1024 and 1 <= m <= 512
    floats = workspace(ws_rows, d, m, n_lambda) if ws_rows is not None else None
    ws = _guarded(floats) if floats is not None else _aligned(workspace(n, d, m, 1) + 4 if ok else 64)
    dd, mm = max(d, 1), max(m, 1)
    mean_x, comp, var, info = np.zeros(dd, np.float32), np.zeros((dd, dd), np.float32), np.zeros(dd, np.float32), PcaInfo()
    mean_y, z = np.zeros(mm, np.float32), np.zeros((dd, mm), np.float32)
    _check(_lib().remu_fit(x.ctypes.data, n, d, ldx, y.ctypes.data, m, ldy, mean_x.ctypes.data, comp.ctypes.data, var.ctypes.data, mean_y.ctypes.data,
                           z.ctypes.data, ws.ctypes.data + (4 if misalign else 0), C.byref(info)))
    if floats is not None:
        _guard_intact(ws, floats)
    return mean_x, comp, var, mean_y, z, info


def readout_weights(components, variance, z, lambdas, d=None, m=None, n_lambda=None):
    comp, var, zz = _f32(components), _f32(variance), _f32(z)
    lam = np.ascontiguousarray(lambdas, np.float64)
    d, m, L = zz.shape[0] if d is None else d, zz.shape[1] if m is None else m, lam.shape[0] if n_lambda is None else n_lambda
    w = np.zeros((max(L, 1), zz.shape[0], zz.shape[1]), np.float32)
    _check(_lib().remu_weights(comp.ctypes.data, var.ctypes.data, zz.ctypes.data, d, m, lam.ctypes.data, L, w.ctypes.data))
    return w


def readout_predict(x, mean_x, w, mean_y, out=None, n=None, ldx=None, ldo=None, d=None, m=None):
    """w [d, m] -> float32 [n, m]; `out` (a view with a row stride) is written in place."""
    ww, mx, my = _f32(w), _f32(mean_x), _f32(mean_y)
    d, m = ww.shape[0] if d is None else d, ww.shape[1] if m is None else m
    n = x.shape[0] if n is None else n
    out = np.zeros((max(n, 1), ww.shape[1]), np.float32) if out is None else out
    _check(_lib().remu_predict(x.ctypes.data, n, d, _ld(x) if ldx is None else ldx, mx.ctypes.data, ww.ctypes.data, my.ctypes.data, m, out.ctypes.data,
                               _ld(out) if ldo is None else ldo))
    return out


def readout_score(x, y, mean_x, w, mean_y, n=None, ldx=None, ldy=None, n_lambda=None, misalign=False, d=None, m=None, ws_rows=None):
    """w [L, d, m] -> (sse [L, m], sst [m]) float64.  `ws_rows`: as in readout_fit."""
    ww, mx, my = _f32(w), _f32(mean_x), _f32(mean_y)
    L, wd, wm = ww.shape
    d, m = wd if d is None else d, wm if m is None else m
    n, L = x.shape[0] if n is None else n, L if n_lambda is None else n_lambda
    floats = workspace(ws_rows, d, m, L) if ws_rows is not None else None
    ws = _guarded(floats) if floats is not None else _aligned(workspace(max(n, 2), wd, wm, min(max(L, 1), 16)) + 4)
    sse, sst = np.zeros((max(L, 1), wm), np.float64), np.zeros(wm, np.float64)
    _check(_lib().remu_score(x.ctypes.data, n, d, _ld(x) if ldx is None else ldx, y.ctypes.data, m, _ld(y) if ldy is None else ldy, mx.ctypes.data,
                             ww.ctypes.data, my.ctypes.data, L, sse.ctypes.data, sst.ctypes.data, ws.ctypes.data + (4 if misalign else 0)))
    if floats is not None:
        _guard_intact(ws, floats)
    return sse, sst


def pca_fit_wide(x):
    """tmjx_pca_fit_wide's emulation (tests/hostemu/pca_wide_emu.py), for the bit-level comparison of the readout's PCA outputs."""
    return _wide.fit_wide(x)


class EmuReadoutBackend(_wide.EmuWideBackend):
    """analysis.pca.HipBackend's methods on the host emulation, the readout's included."""

    readout_fit = staticmethod(lambda x, y: readout_fit(x, y))
    readout_weights = staticmethod(lambda components, variance, z, lambdas: readout_weights(components, variance, z, lambdas))
    readout_predict = staticmethod(lambda x, mean_x, w, mean_y: readout_predict(x, mean_x, w, mean_y))
    readout_score = staticmethod(lambda x, y, mean_x, w, mean_y: readout_score(x, y, mean_x, w, mean_y))
