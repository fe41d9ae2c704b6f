"""ctypes wrapper of the TEST-ONLY host emulation of the intervention C-ABI (tests/hostemu/intervene_emu.cpp): tmjx_intervene_ok and tmjx_intervene
on numpy arrays."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests.hostemu import loader
from track_mjx_amd.hip import INTERVENE_SUBSPACE, INTERVENE_UNITS, Intervene

_HERE = Path(__file__).resolve().parent
_lib_cache = None


def _lib():
    global _lib_cache
    if _lib_cache is not None:
        return _lib_cache
    L = loader.load("intervene_emu.cpp")
    L.ivemu_last_error.restype = C.c_char_p
    L.ivemu_intervene_ok.argtypes = [C.POINTER(Intervene)]
    L.ivemu_intervene.argtypes = [C.POINTER(Intervene), C.c_int]
    _lib_cache = L
    return L


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main: -DINTERVENE_EMU_MAIN), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DINTERVENE_EMU_MAIN", *flags, "-o", str(out), str(_HERE / "intervene_emu.cpp")], check=True,
                   capture_output=True)
    return out


def _ptr(a):
    if a is None or isinstance(a, int):
        return a
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def descriptor(h, ld, w, n, mode, gain, offset, dose, t_on, t_off, dirs=None, K=0, ldv=0, center=None, proj=None, ldp=0) -> Intervene:
    """tmjx_intervene_t from numpy arrays, torch tensors or raw addresses (the caller keeps them alive)."""
    return Intervene(_ptr(h), ld, w, n, mode, _ptr(dirs), K, ldv, _ptr(center), _ptr(gain), _ptr(offset), _ptr(dose), _ptr(t_on), _ptr(t_off),
                     _ptr(proj), ldp, 0)


def last_error() -> str:
    return _lib().ivemu_last_error().decode()


def intervene_ok(d: Intervene) -> bool:
    return bool(_lib().ivemu_intervene_ok(C.byref(d)))


def intervene(d: Intervene, t: int) -> None:
    if _lib().ivemu_intervene(C.byref(d), int(t)) != 0:
        raise ValueError(last_error())


def run(buf, c0, w, mode, gain, offset, dose, t_on, t_off, t, dirs=None, center=None, want_proj=False, call=None):
    """Edit columns [c0, c0 + w) of the float32 rows buf [n, ld] in place at step t; returns proj [n, K] (subspace mode with want_proj) or None.
    `call(descriptor, t)`: what runs it (the emulation by default)."""
    assert buf.dtype == np.float32 and buf.flags.c_contiguous
    n, ld = buf.shape
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)      # noqa: E731
    gain, offset, dose, center, dirs = f32(gain), f32(offset), f32(dose), f32(center), f32(dirs)
    t_on, t_off = np.ascontiguousarray(t_on, np.int32), np.ascontiguousarray(t_off, np.int32)
    K = 0 if dirs is None else dirs.shape[0]
    proj = np.full((n, K + 1), -7.25, np.float32) if want_proj else None
    d = descriptor(buf.ctypes.data + 4 * c0, ld, w, n, mode, gain, offset, dose, t_on, t_off, dirs, K, 0 if dirs is None else dirs.shape[1], center, proj,
                   K + 1 if want_proj else 0)
    (intervene if call is None else call)(d, t)
    if want_proj:
        assert (proj[:, K] == -7.25).all(), "the call wrote behind a proj row"
        return proj[:, :K].copy()
    return None


__all__ = ["INTERVENE_SUBSPACE", "INTERVENE_UNITS", "Intervene", "build_main", "descriptor", "intervene", "intervene_ok", "last_error", "run"]
