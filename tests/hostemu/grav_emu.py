"""ctypes wrapper of the TEST-ONLY host emulation of the domain-randomisation physics kernel with both tables (tests/hostemu/grav_emu.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests.hostemu import loader

_FP = C.POINTER(C.c_float)


def _lib():
    L = loader.load("grav_emu.cpp")
    L.grav_model_create.restype = C.c_void_p
    L.grav_model_create.argtypes = [C.c_char_p, C.c_size_t]
    L.grav_last_error.restype = C.c_char_p
    L.grav_physics_wave.argtypes = [C.c_void_p, _FP, _FP, C.c_int, C.c_int, _FP, C.c_int, _FP, C.c_int, _FP, C.c_int, C.c_int, C.c_int]
    L.grav_model_destroy.argtypes = [C.c_void_p]
    return L


def _f(a):
    return None if a is None else a.ctypes.data_as(_FP)


def _tab(name, t, need):
    if t is None:
        return None
    t = np.ascontiguousarray(t, np.float32)
    if t.ndim != 2 or t.shape[0] != 3 or t.shape[1] < need:
        raise ValueError(f"{name} must be [3, >= {need}], got {t.shape}")      # (the emulation reads columns e0 .. e0 + n: checked here)
    return t


class GravEmu:
    """Runs the RAND build of the wave kernel body on an `emu.Emu`'s state arrays (same blob), each env with its own scales and gravity."""

    def __init__(self, blob: bytes):
        self.L = _lib()
        self.m = C.c_void_p(self.L.grav_model_create(blob, len(blob)))
        if not self.m:
            raise RuntimeError(self.L.grav_last_error().decode())

    def __del__(self):
        try:
            self.L.grav_model_destroy(self.m)
        except Exception:
            pass

    def physics(self, E, action, nsub, scales=None, gravity=None, *, e0=0, dump=True, chains=True):
        """`nsub` substeps on E.st (E: emu.Emu of the same blob); `scales` [3, >= e0 + E.n] float32 (friction | actuator | damping) or None = unit
        scales; `gravity` [3, >= e0 + E.n] float32 (gx | gy | gz) or None = the model's gravity."""
        a = None if action is None else np.ascontiguousarray(action, np.float32)
        s, g = _tab("scales", scales, e0 + E.n), _tab("gravity", gravity, e0 + E.n)
        self.L.grav_physics_wave(self.m, _f(E.st), _f(a), nsub, 1, _f(E.ws) if dump else None, E.n, _f(s), 0 if s is None else s.shape[1],
                                 _f(g), 0 if g is None else g.shape[1], int(e0), int(chains))
