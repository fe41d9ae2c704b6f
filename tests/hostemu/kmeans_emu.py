"""ctypes wrapper of the TEST-ONLY host emulation of the k-means C-ABI (tests/hostemu/kmeans_emu.cpp): tmjx_kmeans_workspace, _assign, _update,
_seed and _fit one for one on numpy arrays, and `EmuKMeansBackend`, the stand-in for analysis.pca.HipBackend with the `kmeans_*` methods."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests.hostemu import pca_emu as _narrow
from tests.hostemu import pca_wide_emu as _wide
from track_mjx_amd.hip import KMeansInfo

_HERE = Path(__file__).resolve().parent
_CSRC = _HERE.parents[1] / "track_mjx_amd" / "csrc"
_lib_cache = None


def _lib():
    global _lib_cache
    if _lib_cache is not None:
        return _lib_cache
    src = [_HERE / "kmeans_emu.cpp", _HERE / "pca_wide_emu.cpp", _HERE / "pca_emu.cpp", _HERE.parents[1] / "include" / "tmjx.h",
           *[_CSRC / f for f in ("pca_core.h", "pca_host.h", "pca_wide_core.h", "pca_wide_host.h", "kmeans_core.h", "kmeans_host.h")]]
    so = _HERE / "libkmeans_emu.so"
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in src):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(_HERE / "kmeans_emu.cpp")], check=True, capture_output=True)
    L = C.CDLL(str(so))
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.pemu_last_error.restype = C.c_char_p
    L.kemu_workspace.argtypes = [i, i, i, C.POINTER(i64)]
    L.kemu_assign.argtypes = [vp, i, i, i64, vp, i, vp, vp, vp, vp, vp, vp]
    L.kemu_update.argtypes = [vp, i, i, i64, vp, i, vp, vp, vp]
    L.kemu_seed.argtypes = [vp, i, i, i64, i, vp, vp, vp, vp]
    L.kemu_fit.argtypes = [vp, i, i, i64, i, vp, vp, vp, i, C.c_double, C.POINTER(KMeansInfo), vp]
    _lib_cache = L
    return L


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main: -DKMEANS_EMU_MAIN), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-std=c++17", "-DKMEANS_EMU_MAIN", *flags, "-o", str(out), str(_HERE / "kmeans_emu.cpp")], check=True,
                   capture_output=True)
    return out


def _check(rc):
    if rc != 0:
        raise ValueError(_lib().pemu_last_error().decode())


_aligned, _ld = _narrow._aligned, _narrow._ld
_f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731
GUARD = 4096      # floats behind the workspace, which must come back untouched
_CANARY = np.float32(-7.25)


def workspace(n: int, d: int, k: int) -> int:
    out = C.c_int64(0)
    _check(_lib().kemu_workspace(n, d, k, C.byref(out)))
    return int(out.value)


class _Ws:
    """A workspace of exactly tmjx_kmeans_workspace's size (64 floats where the shape is refused anyway) with a guard behind it."""

    def __init__(self, n, d, k, misalign=False):
        ok = n >= 1 and 1 <= d <= 1024 and 1 <= k <= 256 and k <= n
        self.floats = workspace(n, d, k) if ok else 64
        self.buf = _aligned(self.floats + GUARD + 4)
        self.buf[self.floats:] = _CANARY
        self.ptr = self.buf.ctypes.data + (4 if misalign else 0)

    def check(self):
        if not (self.buf[self.floats:] == _CANARY).all():
            raise AssertionError(f"the call wrote behind its workspace of {self.floats} floats")


def kmeans_assign(x, centroids, labels_prev=None, n=None, d=None, k=None, ldx=None, misalign=False, null=()):
    """-> (labels int32 [n], dist2 float32 [n], inertia, changed).  n / d / k / ldx override what is passed down, `misalign` shifts the workspace
    and `null` names outputs passed as null pointers (the refusal tests)."""
    cen = _f32(centroids)
    n, d, k = x.shape[0] if n is None else n, x.shape[1] if d is None else d, cen.shape[0] if k is None else k
    prev = None if labels_prev is None else np.ascontiguousarray(labels_prev, np.int32)
    labels, dist2 = np.full(max(x.shape[0], 1), -1, np.int32), np.full(max(x.shape[0], 1), -1, np.float32)
    inertia, changed, ws = np.zeros(1, np.float64), np.full(1, -1, np.int32), _Ws(n, d, k, misalign)
    ptr = lambda name, a: None if name in null else a.ctypes.data      # noqa: E731
    _check(_lib().kemu_assign(x.ctypes.data, n, d, _ld(x) if ldx is None else ldx, cen.ctypes.data, k, None if prev is None else prev.ctypes.data,
                              ptr("labels", labels), ptr("dist2", dist2), ptr("inertia", inertia), ptr("changed", changed), ws.ptr))
    ws.check()
    return labels, dist2, float(inertia[0]), int(changed[0])


def kmeans_update(x, labels, centroids, null=()):
    """-> (centroids float32 [k, d], counts int32 [k])."""
    cen, lab = _f32(centroids).copy(), np.ascontiguousarray(labels, np.int32)
    (n, d), k = x.shape, cen.shape[0]
    counts, ws = np.full(k, -1, np.int32), _Ws(n, d, k)
    _check(_lib().kemu_update(x.ctypes.data, n, d, _ld(x), lab.ctypes.data, k, cen.ctypes.data, None if "counts" in null else counts.ctypes.data, ws.ptr))
    ws.check()
    return cen, counts


def kmeans_seed(x, k, u, n=None):
    """-> (centroids float32 [k, d], index int32 [k])."""
    uu = np.ascontiguousarray(u, np.float64)
    n, d = x.shape[0] if n is None else n, x.shape[1]
    cen, index, ws = np.zeros((max(k, 1), d), np.float32), np.full(max(k, 1), -1, np.int32), _Ws(n, d, k)
    _check(_lib().kemu_seed(x.ctypes.data, n, d, _ld(x), k, uu.ctypes.data, cen.ctypes.data, index.ctypes.data, ws.ptr))
    ws.check()
    return cen, index


def kmeans_fit(x, centroids, max_iter=100, tol=1e-4):
    """-> (centroids, labels int32 [n], dist2 float32 [n], KMeansInfo)."""
    cen = _f32(centroids).copy()
    (n, d), k = x.shape, cen.shape[0]
    labels, dist2, info, ws = np.full(n, -1, np.int32), np.full(n, -1, np.float32), KMeansInfo(), _Ws(n, d, k)
    _check(_lib().kemu_fit(x.ctypes.data, n, d, _ld(x), k, cen.ctypes.data, labels.ctypes.data, dist2.ctypes.data, int(max_iter), float(tol), C.byref(info),
                           ws.ptr))
    ws.check()
    return cen, labels, dist2, info


class EmuKMeansBackend(_wide.EmuWideBackend):
    """analysis.pca.HipBackend's methods on the host emulation, the k-means' included."""

    kmeans_seed = staticmethod(lambda x, k, u: kmeans_seed(x, k, u))
    kmeans_assign = staticmethod(lambda x, centroids, labels_prev=None: kmeans_assign(x, centroids, labels_prev))
    kmeans_update = staticmethod(lambda x, labels, centroids: kmeans_update(x, labels, centroids))
    kmeans_fit = staticmethod(lambda x, centroids, max_iter=100, tol=1e-4: kmeans_fit(x, centroids, max_iter, tol))
