"""ctypes wrapper of the TEST-ONLY host emulation of the hidden-Markov-model C-ABI (tests/hostemu/hmm_emu.cpp): tmjx_hmm_workspace, _emission,
_forward_backward, _mstep, _transitions, _viterbi and _fit one for one on numpy arrays, and `EmuHmmBackend`, the stand-in for
analysis.pca.HipBackend with the `hmm_*` methods."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from tests.hostemu import kmeans_emu as _km
from track_mjx_amd.hip import HmmInfo

_HERE = Path(__file__).resolve().parent
_CSRC = _HERE.parents[1] / "track_mjx_amd" / "csrc"
_lib_cache = None


def _lib():
    global _lib_cache
    if _lib_cache is not None:
        return _lib_cache
    src = [*[_HERE / f for f in ("hmm_emu.cpp", "kmeans_emu.cpp", "pca_wide_emu.cpp", "pca_emu.cpp")], _HERE.parents[1] / "include" / "tmjx.h",
           *[_CSRC / f for f in ("pca_core.h", "pca_host.h", "pca_wide_core.h", "pca_wide_host.h", "kmeans_core.h", "kmeans_host.h", "hmm_core.h", "hmm_host.h")]]
    so = _HERE / "libhmm_emu.so"
    if not so.exists() or so.stat().st_mtime < max(p.stat().st_mtime for p in src):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", str(so), str(_HERE / "hmm_emu.cpp")], check=True, capture_output=True)
    L = C.CDLL(str(so))
    vp, i, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    L.pemu_last_error.restype = C.c_char_p
    L.hemu_workspace.argtypes = [i, i, i, i, C.POINTER(i64)]
    L.hemu_emission.argtypes = [vp, i, i, i64, vp, vp, i, vp, vp]
    L.hemu_forward_backward.argtypes = [vp, i, i, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.hemu_mstep.argtypes = [vp, i, i, i64, vp, i, dbl, dbl, vp, vp, vp, vp]
    L.hemu_transitions.argtypes = [vp, vp, i, dbl, dbl, vp, vp]
    L.hemu_viterbi.argtypes = [vp, i, i, vp, i, vp, vp, i, vp, vp, vp]
    L.hemu_fit.argtypes = [vp, i, i, i64, vp, i, i, vp, vp, vp, vp, vp, vp, i, dbl, dbl, dbl, dbl, dbl, C.POINTER(HmmInfo), vp]
    _lib_cache = L
    return L


def build_main(out: Path, flags=()) -> Path:
    """The emulation as a stand-alone program (its own main: -DHMM_EMU_MAIN), e.g. flags=("-fsanitize=address,undefined",)."""
    subprocess.run(["g++", "-O1", "-std=c++17", "-DHMM_EMU_MAIN", *flags, "-o", str(out), str(_HERE / "hmm_emu.cpp")], check=True, capture_output=True)
    return out


def _check(rc):
    if rc != 0:
        raise ValueError(_lib().pemu_last_error().decode())


_aligned, _ld, _f32 = _km._aligned, _km._ld, _km._f32
GUARD = 4096      # floats behind the workspace, which must come back untouched
_CANARY = np.float32(-7.25)
_f64 = lambda a: np.ascontiguousarray(a, np.float64)      # noqa: E731
_seq = lambda s: np.ascontiguousarray(s, np.int32)      # noqa: E731


def workspace(n: int, d: int, k: int, S: int = 1) -> int:
    out = C.c_int64(0)
    _check(_lib().hemu_workspace(n, d, k, S, C.byref(out)))
    return int(out.value)


class _Ws:
    """A workspace of exactly tmjx_hmm_workspace's size (64 floats where the shape is refused anyway) with a guard behind it."""

    def __init__(self, n, d, k, S=1, misalign=False):
        ok = n >= 1 and 1 <= d <= 1024 and 1 <= k <= 128 and 1 <= S <= n
        self.floats = workspace(n, d, k, S) if ok else 64
        self.buf = _aligned(self.floats + GUARD + 4)
        self.buf[self.floats:] = _CANARY
        self.ptr = self.buf.ctypes.data + (4 if misalign else 0)

    def check(self):
        if not (self.buf[self.floats:] == _CANARY).all():
            raise AssertionError(f"the call wrote behind its workspace of {self.floats} floats")


def hmm_emission(x, means, vars, n=None, d=None, k=None, ldx=None, misalign=False):
    mu, var = _f32(means), _f32(vars)
    n, d, k = x.shape[0] if n is None else n, x.shape[1] if d is None else d, mu.shape[0] if k is None else k
    logb, ws = np.full((max(x.shape[0], 1), max(mu.shape[0], 1)), -7.25, np.float32), _Ws(n, d, k, 1, misalign)
    _check(_lib().hemu_emission(x.ctypes.data, n, d, _ld(x) if ldx is None else ldx, mu.ctypes.data, var.ctypes.data, k, logb.ctypes.data, ws.ptr))
    ws.check()
    return logb


def hmm_forward_backward(logb, seq_start, transmat, startprob, S=None):
    lb, A, pi, seq = _f32(logb), _f32(transmat), _f32(startprob), _seq(seq_start)
    n, k = lb.shape
    S = seq.shape[0] - 1 if S is None else S
    gamma, xi, start, loglik, total = np.full((n, k), -7.25, np.float32), np.full((k, k), -7.25), np.full(k, -7.25), np.full(max(S, 1), -7.25), np.full(1, -7.25)
    ws = _Ws(n, 1, k, S)
    _check(_lib().hemu_forward_backward(lb.ctypes.data, n, k, seq.ctypes.data, S, A.ctypes.data, pi.ctypes.data, gamma.ctypes.data, xi.ctypes.data,
                                        start.ctypes.data, loglik.ctypes.data, total.ctypes.data, ws.ptr))
    ws.check()
    return gamma, xi, start, loglik, float(total[0])


def hmm_mstep(x, gamma, means, vars, min_var=0.0, min_weight=0.0):
    g, mu, var = _f32(gamma), _f32(means).copy(), _f32(vars).copy()
    (n, d), k = x.shape, mu.shape[0]
    weight, ws = np.full(k, -7.25), _Ws(n, d, k)
    _check(_lib().hemu_mstep(x.ctypes.data, n, d, _ld(x), g.ctypes.data, k, float(min_var), float(min_weight), mu.ctypes.data, var.ctypes.data,
                             weight.ctypes.data, ws.ptr))
    ws.check()
    return mu, var, weight


def hmm_transitions(xi, start, prior, kappa, transmat, startprob):
    xx, st, A, pi = _f64(xi), _f64(start), _f32(transmat).copy(), _f32(startprob).copy()
    _check(_lib().hemu_transitions(xx.ctypes.data, st.ctypes.data, len(st), float(prior), float(kappa), A.ctypes.data, pi.ctypes.data))
    return A, pi


def hmm_viterbi(logb, seq_start, transmat, startprob, logspace=False):
    lb, A, pi, seq = _f32(logb), _f32(transmat), _f32(startprob), _seq(seq_start)
    (n, k), S = lb.shape, seq.shape[0] - 1
    labels, path, ws = np.full(n, -1, np.int32), np.full(S, -7.25), _Ws(n, 1, k, S)
    _check(_lib().hemu_viterbi(lb.ctypes.data, n, k, seq.ctypes.data, S, A.ctypes.data, pi.ctypes.data, int(bool(logspace)), labels.ctypes.data,
                               path.ctypes.data, ws.ptr))
    ws.check()
    return labels, path


def hmm_fit(x, seq_start, means, vars, transmat, startprob, max_iter=50, tol=1e-4, prior=0.0, kappa=0.0, min_var=0.0, min_weight=0.0, null=()):
    mu, var, A, pi, seq = _f32(means).copy(), _f32(vars).copy(), _f32(transmat).copy(), _f32(startprob).copy(), _seq(seq_start)
    (n, d), k, S = x.shape, mu.shape[0], seq.shape[0] - 1
    gamma, labels, info, ws = np.full((n, k), -7.25, np.float32), np.full(n, -1, np.int32), HmmInfo(), _Ws(n, d, k, S)
    _check(_lib().hemu_fit(x.ctypes.data, n, d, _ld(x), seq.ctypes.data, S, k, mu.ctypes.data, var.ctypes.data, A.ctypes.data, pi.ctypes.data,
                           None if "gamma" in null else gamma.ctypes.data, labels.ctypes.data, int(max_iter), float(tol), float(prior), float(kappa),
                           float(min_var), float(min_weight), C.byref(info), ws.ptr))
    ws.check()
    return mu, var, A, pi, gamma, labels, info


class EmuHmmBackend(_km.EmuKMeansBackend):
    """analysis.pca.HipBackend's methods on the host emulation, the hidden Markov model's included."""

    hmm_emission = staticmethod(lambda x, means, vars: hmm_emission(x, means, vars))
    hmm_forward_backward = staticmethod(lambda logb, seq_start, transmat, startprob: hmm_forward_backward(logb, seq_start, transmat, startprob))
    hmm_mstep = staticmethod(lambda x, gamma, means, vars, min_var=0.0, min_weight=0.0: hmm_mstep(x, gamma, means, vars, min_var, min_weight))
    hmm_transitions = staticmethod(hmm_transitions)
    hmm_viterbi = staticmethod(lambda logb, seq_start, transmat, startprob, logspace=False: hmm_viterbi(logb, seq_start, transmat, startprob, logspace))
    hmm_fit = staticmethod(lambda x, seq_start, means, vars, transmat, startprob, max_iter=50, tol=1e-4, prior=0.0, kappa=0.0, min_var=0.0, min_weight=0.0:
                           hmm_fit(x, seq_start, means, vars, transmat, startprob, max_iter, tol, prior, kappa, min_var, min_weight))
