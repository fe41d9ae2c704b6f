"""ctypes wrapper of the TEST-ONLY host emulation of the spectrogram C-ABI (tests/hostemu/spectrogram_emu.cpp): tmjx_wavelet_bank_size /
tmjx_wavelet_bank, tmjx_spectrogram_workspace and tmjx_spectrogram on numpy arrays, and `EmuSpectrogramBackend`, the stand-in for
analysis.pca.HipBackend with the `wavelet_bank` and `spectrogram` methods."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests.hostemu import hmm_emu as _hm

_HERE = Path(__file__).resolve().parent
_CSRC = _HERE.parents[1] / "track_mjx_amd" / "csrc"
_lib_cache = None


def _lib():
    global _lib_cache
    if _lib_cache is not None:
        return _lib_cache
    src = [*[_HERE / f for f in ("spectrogram_emu.cpp", "hmm_emu.cpp", "kmeans_emu.cpp", "pca_wide_emu.cpp", "pca_emu.cpp")], _HERE.parents[1] / "include" / "tmjx.h",
           *[_CSRC / f for f in ("pca_core.h", "pca_host.h", "pca_wide_core.h", "pca_wide_host.h", "kmeans_core.h", "kmeans_host.h", "hmm_core.h", "hmm_host.h",
                                 "spectrogram_core.h", "spectrogram_host.h")]]
    so = _HERE / "libspectrogram_emu.so"
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in src):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(_HERE / "spectrogram_emu.cpp")], check=True, capture_output=True)
    L = C.CDLL(str(so))
    vp, i, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    L.pemu_last_error.restype = C.c_char_p
    L.semu_bank_size.argtypes = [dbl, vp, i, dbl, dbl, C.POINTER(i64)]
    L.semu_bank.argtypes = [dbl, vp, i, dbl, dbl, vp, vp, vp]
    L.semu_workspace.argtypes = [i, i, i, i, C.POINTER(i64)]
    L.semu_spectrogram.argtypes = [vp, i, i, i64, vp, i, vp, vp, vp, i, i, i, C.c_float, vp, i64, vp, vp]
    _lib_cache = L
    return L


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main: -DSPECTROGRAM_EMU_MAIN), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-std=c++17", "-DSPECTROGRAM_EMU_MAIN", *flags, "-o", str(out), str(_HERE / "spectrogram_emu.cpp")], check=True,
                   capture_output=True)
    return out


def _check(rc):
    if rc != 0:
        raise ValueError(_lib().pemu_last_error().decode())


_aligned, _ld, _f32 = _hm._aligned, _hm._ld, _hm._f32
GUARD = 4096      # floats behind the workspace, out and coverage, which must come back untouched
_CANARY = np.float32(-7.25)


def wavelet_bank(rate, freqs, omega0=5.0, support=4.0, F=None, null=False):
    """-> (bank float32, offset int32 [F + 1], radius int32 [F]); F overrides the count passed down (the refusal tests)."""
    fr = np.ascontiguousarray(freqs, np.float64).reshape(-1)
    F = fr.shape[0] if F is None else F
    floats = C.c_int64(0)
    _check(_lib().semu_bank_size(float(rate), None if null else fr.ctypes.data, F, float(omega0), float(support), C.byref(floats)))
    bank = np.full(int(floats.value) + GUARD, _CANARY, np.float32)
    offset, radius = np.zeros(F + 1, np.int32), np.zeros(F, np.int32)
    _check(_lib().semu_bank(float(rate), fr.ctypes.data, F, float(omega0), float(support), bank.ctypes.data, offset.ctypes.data, radius.ctypes.data))
    if not (bank[int(floats.value):] == _CANARY).all():
        raise AssertionError(f"the bank builder wrote behind its {floats.value} floats")
    return np.ascontiguousarray(bank[:int(floats.value)]), offset, radius


def workspace(n: int, Cn: int, F: int, S: int = 1) -> int:
    out = C.c_int64(0)
    _check(_lib().semu_workspace(n, Cn, F, S, C.byref(out)))
    return int(out.value)


def spectrogram(x, seq_start, bank, offset, radius, detrend=True, log=False, floor=1e-3, out=None, n=None, Cn=None, F=None, S=None, ldx=None, ldo=None,
                kind=None, misalign=False, null=()):
    """-> (out [n, F C], coverage [n, F]) float32.  `out`: a preallocated [n, F C] view (a row stride is fine) to write into.  The outputs and the
    workspace have exactly the sizes the call is entitled to, with a guard of canaries behind each; n / Cn / F / S / ldx / ldo / kind override what is
    passed down, `misalign` shifts the workspace and `null` names pointers passed as null (the refusal tests)."""
    seq, off, rad, bk = np.ascontiguousarray(seq_start, np.int32), np.ascontiguousarray(offset, np.int32), np.ascontiguousarray(radius, np.int32), _f32(bank)
    n, Cn, F = x.shape[0] if n is None else n, x.shape[1] if Cn is None else Cn, rad.shape[0] if F is None else F
    S = seq.shape[0] - 1 if S is None else S
    rows, width = max(x.shape[0], 1), max(rad.shape[0] * x.shape[1], 1)
    own = out is None
    if own:
        flat = np.full(rows * width + GUARD, _CANARY, np.float32)
        out = flat[:rows * width].reshape(rows, width)
    cflat = np.full(rows * rad.shape[0] + GUARD, _CANARY, np.float32)
    cov = cflat[:rows * rad.shape[0]].reshape(rows, rad.shape[0])
    ok = n >= 1 and 1 <= Cn <= 1024 and 1 <= F <= 64 and 1 <= S <= n
    floats = workspace(n, Cn, F, S) if ok else 64
    ws = _aligned(floats + GUARD + 4)
    ws[floats:] = _CANARY
    ptr = lambda name, a: None if name in null else a.ctypes.data      # noqa: E731
    _check(_lib().semu_spectrogram(ptr("x", x), n, Cn, _ld(x) if ldx is None else ldx, ptr("seq_start", seq), S, ptr("bank", bk), ptr("offset", off),
                                   ptr("radius", rad), F, int(bool(detrend)), (1 if log else 0) if kind is None else kind, float(floor), ptr("out", out),
                                   _ld(out) if ldo is None else ldo, ptr("coverage", cov), None if "workspace" in null else ws.ctypes.data + (4 if misalign else 0)))
    if not (ws[floats:] == _CANARY).all():
        raise AssertionError(f"the call wrote behind its workspace of {floats} floats")
    if not (cflat[rows * rad.shape[0]:] == _CANARY).all() or (own and not (flat[rows * width:] == _CANARY).all()):
        raise AssertionError("the call wrote behind out or coverage")
    return out, cov


class EmuSpectrogramBackend(_hm.EmuHmmBackend):
    """analysis.pca.HipBackend's methods on the host emulation, the spectrogram's included."""

    wavelet_bank = staticmethod(lambda rate, freqs, omega0=5.0, support=4.0: wavelet_bank(rate, freqs, omega0, support))
    spectrogram = staticmethod(lambda x, seq_start, bank, offset, radius, detrend=True, log=False, floor=1e-3, out=None:
                               spectrogram(x, seq_start, bank, offset, radius, detrend, log, floor, out))
