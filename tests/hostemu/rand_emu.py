"""ctypes wrapper of the TEST-ONLY host emulation of the domain-randomisation physics kernel (tests/hostemu/rand_emu.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests.hostemu import loader

_FP = C.POINTER(C.c_float)


def _lib():
    L = loader.load("rand_emu.cpp")
    L.rand_model_create.restype = C.c_void_p
    L.rand_model_create.argtypes = [C.c_char_p, C.c_size_t]
    L.rand_last_error.restype = C.c_char_p
    L.rand_physics_wave.argtypes = [C.c_void_p, _FP, _FP, C.c_int, C.c_int, _FP, C.c_int, _FP, C.c_int, C.c_int, C.c_int]
    L.rand_model_destroy.argtypes = [C.c_void_p]
    return L


def _f(a):
    return None if a is None else a.ctypes.data_as(_FP)


class RandEmu:
    """Runs the RAND build of the wave kernel body on an `emu.Emu`'s state arrays (same blob), each env with its own scales."""

    def __init__(self, blob: bytes):
        self.L = _lib()
        self.m = C.c_void_p(self.L.rand_model_create(blob, len(blob)))
        if not self.m:
            raise RuntimeError(self.L.rand_last_error().decode())

    def __del__(self):
        try:
            self.L.rand_model_destroy(self.m)
        except Exception:
            pass

    def physics(self, E, action, nsub, scales, *, e0=0, dump=True, chains=True):
        """`nsub` substeps on E.st (E: emu.Emu of the same blob); `scales` [3, >= e0 + E.n] float32: friction | actuator | damping."""
        a = None if action is None else np.ascontiguousarray(action, np.float32)
        s = np.ascontiguousarray(scales, np.float32)
        if s.ndim != 2 or s.shape[0] != 3 or s.shape[1] < e0 + E.n:
            raise ValueError(f"scales must be [3, >= {e0 + E.n}], got {s.shape}")
        self.L.rand_physics_wave(self.m, _f(E.st), _f(a), nsub, 1, _f(E.ws) if dump else None, E.n, _f(s), s.shape[1], int(e0), int(chains))
