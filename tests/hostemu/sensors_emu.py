"""ctypes wrapper of the TEST-ONLY host emulation of the recording physics kernel (tests/hostemu/sensors_emu.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests.hostemu import loader

_FP = C.POINTER(C.c_float)


def _lib():
    L = loader.load("sensors_emu.cpp")
    L.sens_model_create.restype = C.c_void_p
    L.sens_model_create.argtypes = [C.c_char_p, C.c_size_t]
    L.sens_last_error.restype = C.c_char_p
    L.sens_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.sens_lds_floats.argtypes = [C.c_void_p, C.c_int]
    L.sens_physics_wave.argtypes = [C.c_void_p, _FP, _FP, C.c_int, C.c_int, _FP, C.c_int, C.c_int, _FP, _FP, C.c_int]
    L.sens_model_destroy.argtypes = [C.c_void_p]
    return L


def _f(a):
    return None if a is None else a.ctypes.data_as(_FP)


class SensorEmu:
    """Runs the wave kernel body with or without the sensor stage on an `emu.Emu`'s state arrays (same blob)."""

    def __init__(self, blob: bytes):
        self.L = _lib()
        self.m = C.c_void_p(self.L.sens_model_create(blob, len(blob)))
        if not self.m:
            raise RuntimeError(self.L.sens_last_error().decode())
        info = (C.c_int * 3)()
        self.L.sens_info(self.m, info)
        self.nsensordata, self.nbody, self.nsensor = list(info)

    def __del__(self):
        try:
            self.L.sens_model_destroy(self.m)
        except Exception:
            pass

    def lds_bytes(self, chains=True):
        return 4 * self.L.sens_lds_floats(self.m, int(chains))

    def physics(self, E, action, nsub, *, sensors=True, dump=True, chains=True):
        """`nsub` substeps on E.st (E: emu.Emu of the same blob); returns (sensordata [nsd, n], cfrc_ext [nbody*6, n]) or None."""
        n = E.n
        a = None if action is None else np.ascontiguousarray(action, np.float32)
        sd = np.full((max(self.nsensordata, 1), n), np.nan, np.float32)
        cf = np.full((self.nbody * 6, n), np.nan, np.float32)
        self.L.sens_physics_wave(self.m, _f(E.st), _f(a), nsub, 1, _f(E.ws) if dump else None, n, int(sensors),
                                 _f(sd) if self.nsensordata else None, _f(cf), int(chains))
        return (sd[:self.nsensordata], cf) if sensors else None
