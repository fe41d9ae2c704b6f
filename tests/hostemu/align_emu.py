"""ctypes wrapper of the TEST-ONLY host emulation of tmjx_step under a done-policy (tests/hostemu/align_emu.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests.hostemu import loader

_FP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_int)
DONE_NONE, DONE_RESET, DONE_ALIGN = 0, 1, 2
CLIP_KEYS = ("position", "quaternion", "joints", "body_positions", "angular_velocity")
VEL_KEYS = ("velocity", "joints_velocity")


def _lib():
    L = loader.load("align_emu.cpp")
    L.align_model_create.restype = C.c_void_p
    L.align_model_create.argtypes = [C.c_char_p, C.c_size_t]
    L.align_last_error.restype = C.c_char_p
    L.align_model_destroy.argtypes = [C.c_void_p]
    L.align_clips.argtypes = [C.c_void_p] + [_FP] * 7 + [C.c_int, C.c_int]
    L.align_set_policy.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.align_step.argtypes = [C.c_void_p, _FP, _IP, _FP, _FP, _FP, _FP, _FP, _FP, C.c_int, C.c_int]
    return L


def _f(a):
    return None if a is None else a.ctypes.data_as(_FP)


class AlignEmu:
    """Steps an `emu.Emu`'s buffers (same blob; reset through E.reset) with the wave physics + K3 + the done-policy's epilogue."""

    def __init__(self, blob: bytes, clips: dict, velocities: bool = True):
        self.L = _lib()
        self.m = C.c_void_p(self.L.align_model_create(blob, len(blob)))
        if not self.m:
            raise RuntimeError(self.L.align_last_error().decode())
        self._arrs = [np.ascontiguousarray(clips[k], dtype=np.float32) for k in CLIP_KEYS]
        self._arrs += [np.ascontiguousarray(clips[k], dtype=np.float32) if velocities else None for k in VEL_KEYS]
        nc, nf = self._arrs[0].shape[:2]
        self.L.align_clips(self.m, *[_f(a) for a in self._arrs], nc, nf)

    def __del__(self):
        try:
            self.L.align_model_destroy(self.m)
        except Exception:
            pass

    def set_policy(self, episode_length: int, policy: int):
        if self.L.align_set_policy(self.m, int(episode_length), int(policy)) != 0:
            raise ValueError(self.L.align_last_error().decode())

    def step(self, E, action, action_repeat: int = 1) -> int:
        """One tmjx_step on E's buffers; returns how many envs were aligned."""
        a = np.ascontiguousarray(action, np.float32)
        return self.L.align_step(self.m, _f(E.st), E.ist.ctypes.data_as(_IP), _f(a), _f(E.obs), _f(E.reward), _f(E.done), _f(E.trunc),
                                 _f(E.metrics), E.n, int(action_repeat))
