"""The analysis calls on the CPU: track_mjx_amd.analysis.backend.Backend, the marshalling the product runs on the device, on numpy arrays against
the TEST-ONLY host emulation of the kernels (tests/hostemu/analysis_emu.cpp, which exports the C-ABI's own names).

`B` is that backend; a test calls its methods (B.fit, B.kmeans_assign, ...) as analysis code does.  What the provider below adds to every call:
16-byte aligned buffers, every output pre-filled with a sentinel (`sentinel(dtype)`), a workspace of exactly the size the *_workspace entry reports,
and a guard of canaries behind the workspace and behind every output the call allocates, checked after every call.  A refusal is a ValueError with
the library's message.

`over(entry, **substitutes)` replaces arguments of the NEXT call of one entry point, by the parameter names of include/tmjx.h, and returns `B`:
    over("tmjx_kmeans_assign", n=100, k=101).kmeans_assign(x, c)        # the refusal tests
    over("tmjx_kmeans_assign", dist2=None).kmeans_assign(x, c)          # a null pointer; an array stands for its address
    over("tmjx_readout_fit", misalign=True).readout_fit(x, y)           # the workspace pointer plus 4 bytes
    over("tmjx_readout_score", ws_rows=4352).readout_score(...)         # the workspace sized for that many rows instead of the call's"""
from __future__ import annotations

import contextlib
import ctypes as C
from pathlib import Path

import numpy as np

from tests.abi_header import parameter_names
from tests.hostemu import loader
from track_mjx_amd.analysis.backend import Backend

SOURCE = "analysis_emu.cpp"
GUARD, WORKSPACE_GUARD = 4096, 1 << 16      # elements behind an output / floats behind a workspace, which must come back untouched


def sentinel(dtype):
    """What an output of `dtype` holds before the call."""
    kind = np.dtype(dtype).kind
    return np.dtype(dtype).type(-7.25 if kind == "f" else -7 if kind == "i" else 0xA5)


class _Calls:
    """The library as the backend sees it: every entry point with the pending substitutes applied and the guards checked behind it."""

    def __init__(self, arrays):
        self._a = arrays

    def __getattr__(self, name):
        fn, a = getattr(self._a.library, name), self._a

        def call(*args):
            args = list(args)
            if a.ws_rows is not None and name.endswith("_workspace"):
                args[0], a.ws_rows = a.ws_rows, None
            for key, value in a.pending.pop(name, {}).items():
                i = parameter_names(name).index("workspace" if key == "misalign" else key)
                args[i] = args[i] + 4 if key == "misalign" else value.ctypes.data if isinstance(value, np.ndarray) else value
            rc = fn(*args)
            a.check_guards()
            return rc
        return call


class NumpyArrays:
    """The provider of numpy arrays (track_mjx_amd/analysis/backend.py says what a provider is)."""

    def __init__(self, library):
        self.library, self.lib = library, _Calls(self)
        self.pending, self.ws_rows, self._guards = {}, None, []

    def check(self, rc, what):
        if rc != 0:
            raise ValueError(self.library.tmjx_last_error().decode())

    @staticmethod
    def rows(x):
        a = np.asarray(x)
        ok = a.dtype == np.float32 and a.strides[1] == 4 and a.strides[0] >= 4 * a.shape[1] and a.strides[0] % 4 == 0
        return a if ok else np.ascontiguousarray(a, np.float32)

    @staticmethod
    def upload(a, dtype, copy=False):
        return np.array(a, dtype=dtype, order="C") if copy else np.ascontiguousarray(a, dtype)

    def _alloc(self, shape, dtype, guard, what):
        dtype, n = np.dtype(dtype), int(np.prod(shape, dtype=np.int64))
        raw = np.empty((n + guard) * dtype.itemsize + 16, np.uint8)
        start = (-raw.ctypes.data) % 16
        flat = raw[start:start + (n + guard) * dtype.itemsize].view(dtype)
        flat[:] = sentinel(dtype)
        self._guards.append((flat, n, what))
        return flat[:n].reshape(shape)

    def empty(self, shape, dtype, zero=False):      # (`zero`: what the device clears keeps the sentinel here, so that a test sees whether it was written)
        return self._alloc(shape, dtype, GUARD, "an output")

    host_empty = empty

    def workspace(self, floats):
        return self._alloc((floats,), np.float32, WORKSPACE_GUARD, "its workspace")

    def check_guards(self):
        guards, self._guards = self._guards, []
        for flat, n, what in guards:
            if not (flat[n:] == sentinel(flat.dtype)).all():
                raise AssertionError(f"the call wrote behind {what} of {n} {'floats' if what == 'its workspace' else 'elements'} "
                                     f"(first at +{int(np.argmax(flat[n:] != sentinel(flat.dtype)))})")

    @staticmethod
    def ptr(a):
        return a.ctypes.data

    @staticmethod
    def ld(a):
        return a.strides[0] // a.itemsize

    @staticmethod
    def dense_columns(a):
        return a.dtype == np.float32 and a.strides[1] == 4

    @staticmethod
    def stream():
        return None

    guard = staticmethod(contextlib.nullcontext)

    @staticmethod
    def to_numpy(a):
        return a

    @staticmethod
    def sync():
        pass


def lib() -> C.CDLL:
    """The emulation library itself, its entry points declared by hip.declare (and the emulation's own, remu_extents)."""
    L = loader.load(SOURCE)
    L.remu_extents.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int64)] * 2
    return L


ARRAYS = NumpyArrays(lib())
B = Backend(ARRAYS)


def product() -> Backend:
    """The same backend and provider on the PRODUCT library, for refusals only: it checks its arguments before it launches anything, so a refused
    call touches no device (and one that is not refused must never be made with these host arrays)."""
    from track_mjx_amd import hip
    return Backend(NumpyArrays(hip.lib()))


def over(entry: str, ws_rows=None, on=None, **substitutes) -> Backend:
    """See the module's text; `on`: another backend on a NumpyArrays provider (`product()`) instead of `B`."""
    backend = B if on is None else on
    arrays = backend._p
    assert not arrays.pending and arrays.ws_rows is None, "an earlier over() was never used"
    unknown = set(substitutes) - set(parameter_names(entry)) - {"misalign"}
    assert not unknown, f"{entry} has no parameter {sorted(unknown)}"
    arrays.pending[entry], arrays.ws_rows = substitutes, ws_rows
    return backend


def workspace(entry: str, *dims) -> int:
    """The floats `entry` (tmjx_pca_workspace, tmjx_readout_workspace, ...) reports for `dims`."""
    floats = C.c_int64(0)
    ARRAYS.check(getattr(lib(), entry)(*dims, C.byref(floats)), entry)
    return int(floats.value)


def readout_extents(n: int, d: int, m: int, n_lambda: int):
    """(fit, score): the floats a readout fit and a score of exactly n rows touch from the start of the workspace."""
    fit, score = C.c_int64(0), C.c_int64(0)
    ARRAYS.check(lib().remu_extents(n, d, m, n_lambda, C.byref(fit), C.byref(score)), "remu_extents")
    return int(fit.value), int(score.value)


def build_main(which: str, out: Path, flags=()) -> Path:
    """The emulation of one analysis (`which` of pca, pca_wide, readout, kmeans, hmm, spectrogram) as a stand-alone program: <which>_emu.cpp with its
    main(), which compiles that file and the ones it includes only."""
    return loader.build_main(f"{which}_emu.cpp", f"{which.upper()}_EMU_MAIN", out, flags)
