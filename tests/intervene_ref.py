"""Float64 numpy statement of the activation intervention, written from DESIGN.md "Interventions" (not from the kernel), with the edge cases, the
data generator, the derived error bound and the checks the CPU and GPU tests share.  `call(descriptor, t)` is what runs a descriptor: the host
emulation (tests/hostemu/intervene_emu.py) or the library on device memory."""
from __future__ import annotations

import functools
import itertools

import numpy as np

EPS = 2.0 ** -24
SUBSPACE, UNITS = 0, 1
WIDTHS = (1, 4, 60, 63, 64, 65, 256, 1023, 1024)
KS = (1, 2, 16)
ROWS = (1, 3, 130)
PAD, C0 = 5, 3                                   # ld = w + PAD; the target starts at column C0 of a canary-filled buffer
S = 1.5
GAIN_OFFSET = ((0.0, 0.0), (0.0, S), (1.0, S), (0.5, 0.0))      # project out, clamp, stimulate, scale
DOSES = (0.0, 0.25, 1.0)
CANARY = np.float32(-7.25)


# ------------------------------------------------------------------------------------------------------------------ the maths
def subspace(h, dirs, center, gain, offset, dose):
    """h [n, w], dirs [K, w], center [w] | None, gain / offset [K], dose [n] -> (h' [n, w], p [n, K]) in float64."""
    h, v = np.asarray(h, np.float64), np.asarray(dirs, np.float64)
    c = np.zeros(h.shape[1]) if center is None else np.asarray(center, np.float64)
    g, o, d = np.asarray(gain, np.float64), np.asarray(offset, np.float64), np.asarray(dose, np.float64)
    p = (h - c) @ v.T
    e = ((g - 1.0) * p + o) @ v
    return h + d[:, None] * e, p


def units(h, center, gain, offset, dose):
    h = np.asarray(h, np.float64)
    c = np.zeros(h.shape[1]) if center is None else np.asarray(center, np.float64)
    g, o, d = np.asarray(gain, np.float64), np.asarray(offset, np.float64), np.asarray(dose, np.float64)
    return h + d[:, None] * ((g - 1.0) * (h - c) + o)


def gate(t, t_on, t_off, dose):
    return (np.asarray(t_on) <= t) & (t < np.asarray(t_off)) & (np.asarray(dose) != 0)


# ------------------------------------------------------------------------------------------------------------------ the derived bound
# float32 accumulation of a w-term dot product (one rounding for h - c, at most w fused steps and tree additions on any path to the sum), the
# coefficient (two roundings), a K-term fused sum and the final fused step: with u = 2^-24 every input of the final result carries at most
# (w + 2K + 6) relative roundings, so  |h' - h'_64|_j <= (w + 2K + 6) u (|h_j| + |dose| sum_k (|g_k - 1| sum_i |h_i - c_i||v_ki| + |o_k|) |v_kj|)
# to first order; the projection alone: |p_k - p_64k| <= (w + 2K + 6) u sum_i |h_i - c_i||v_ki|.  Units mode has no dot product: 6 u.
def bounds_subspace(h, dirs, center, gain, offset, dose):
    """-> (bound on h' [n, w], bound on p [n, K])."""
    h, v = np.asarray(h, np.float64), np.asarray(dirs, np.float64)
    c = np.zeros(h.shape[1]) if center is None else np.asarray(center, np.float64)
    g, o, d = np.asarray(gain, np.float64), np.asarray(offset, np.float64), np.asarray(dose, np.float64)
    K, w = v.shape
    pa = np.abs(h - c) @ np.abs(v).T                                              # [n, K]
    ea = (np.abs(g - 1.0) * pa + np.abs(o)) @ np.abs(v)                           # [n, w]
    f = (w + 2 * K + 6) * EPS
    return f * (np.abs(h) + np.abs(d)[:, None] * ea), f * pa


def bound_units(h, center, gain, offset, dose):
    h = np.asarray(h, np.float64)
    c = np.zeros(h.shape[1]) if center is None else np.asarray(center, np.float64)
    g, o, d = np.asarray(gain, np.float64), np.asarray(offset, np.float64), np.asarray(dose, np.float64)
    return 6 * EPS * (np.abs(h) + np.abs(d)[:, None] * (np.abs(g - 1.0) * np.abs(h - c) + np.abs(o)))


# ------------------------------------------------------------------------------------------------------------------ data
@functools.lru_cache(None)
def rows_of(n, w, seed=0):
    """Standard normal rows at the magnitude of LayerNorm outputs (weight 1, bias 0: unit variance per row)."""
    a = np.random.default_rng(seed + 7 * w + n).standard_normal((n, w)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def directions(K, w, seed=0):
    """K orthonormal rows: Q of a seeded normal [w, K] matrix."""
    q, _ = np.linalg.qr(np.random.default_rng(seed + 100 + 31 * w + K).standard_normal((w, K)))
    v = np.ascontiguousarray(q.T.astype(np.float32))
    v.setflags(write=False)
    return v


@functools.lru_cache(None)
def center_of(w, seed=0):
    c = (0.5 * np.random.default_rng(seed + 200 + w).standard_normal(w)).astype(np.float32)
    c.setflags(write=False)
    return c


def doses_of(n):
    """Every dose of DOSES among the rows (one row: 0.25)."""
    return np.array([DOSES[(r + 1) % 3] for r in range(n)], np.float32)


def framed(rows):
    """rows [n, w] inside a canary-filled [n, w + PAD] buffer at column C0 (the last PAD - C0 columns sit behind the target, inside ld)."""
    n, w = rows.shape
    buf = np.full((n, w + PAD), CANARY, np.float32)
    buf[:, C0:C0 + w] = rows
    return buf


def cases_of(w):
    """(K, n, (gain, offset), centred) for width w, both modes' cases (units mode ignores K: it runs at the first K only)."""
    return [c for c in itertools.product([k for k in KS if k <= min(16, w)], ROWS, GAIN_OFFSET, (False, True))]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ the shared checks
def check_width(w, run, what, other=None):
    """Every case of width w through `run` (tests.hostemu.intervene_emu.run with the backend's `call` bound), in both modes, against float64 under the
    derived bound; the canaries; with `other` (a second `run`) the two agree to the bit.  Returns the largest error / bound ratio seen."""
    worst = 0.0
    for K, n, (g, o), centred in cases_of(w):
        h, v, c, dose = rows_of(n, w), directions(K, w), (center_of(w) if centred else None), doses_of(n)
        t_on, t_off = np.zeros(n, np.int32), np.full(n, 10, np.int32)
        gk, ok = np.full(K, g, np.float32), np.full(K, o, np.float32)
        buf = framed(h)
        proj = run(buf, C0, w, SUBSPACE, gk, ok, dose, t_on, t_off, 4, dirs=v, center=c, want_proj=True)
        want, p64 = subspace(h, v, c, gk, ok, dose)
        bh, bp = bounds_subspace(h, v, c, gk, ok, dose)
        tag = f"{what}: w={w} K={K} n={n} gain={g} offset={o} centred={centred}"
        err, perr = np.abs(buf[:, C0:C0 + w] - want), np.abs(proj - p64)
        assert (err <= bh).all(), f"{tag}: subspace error {err.max():.3e}, up to {np.max(err / np.maximum(bh, 1e-300)):.2f} of the bound"
        assert (perr <= bp).all(), f"{tag}: projection error {perr.max():.3e}, up to {np.max(perr / np.maximum(bp, 1e-300)):.2f} of the bound"
        worst = max(worst, float(np.max(err / np.maximum(bh, 1e-300))), float(np.max(perr / np.maximum(bp, 1e-300))))
        frame = framed(h)
        frame[:, C0:C0 + w] = buf[:, C0:C0 + w]
        assert (bits(frame) == bits(buf)).all(), f"{tag}: a canary column was written"
        off_rows = dose == 0
        assert (bits(buf[off_rows, C0:C0 + w]) == bits(h[off_rows])).all(), f"{tag}: a row of dose 0 changed"
        if other is not None:
            buf2 = framed(h)
            proj2 = other(buf2, C0, w, SUBSPACE, gk, ok, dose, t_on, t_off, 4, dirs=v, center=c, want_proj=True)
            assert (bits(buf2) == bits(buf)).all() and (bits(proj2) == bits(proj)).all(), f"{tag}: subspace bits differ from the emulation's"
        if K != cases_of(w)[0][0]:
            continue
        # units mode: every third unit edited with (g, o), the others left alone (gain 1, offset 0)
        gw, ow = np.ones(w, np.float32), np.zeros(w, np.float32)
        gw[::3], ow[::3] = g, o
        buf = framed(h)
        run(buf, C0, w, UNITS, gw, ow, dose, t_on, t_off, 4, center=c)
        want, bu = units(h, c, gw, ow, dose), bound_units(h, c, gw, ow, dose)
        err = np.abs(buf[:, C0:C0 + w] - want)
        assert (err <= bu).all(), f"{tag}: units error {err.max():.3e}, up to {np.max(err / np.maximum(bu, 1e-300)):.2f} of the bound"
        worst = max(worst, float(np.max(err / np.maximum(bu, 1e-300))))
        frame = framed(h)
        frame[:, C0:C0 + w] = buf[:, C0:C0 + w]
        assert (bits(frame) == bits(buf)).all(), f"{tag}: a canary column was written (units)"
        if other is not None:
            buf2 = framed(h)
            other(buf2, C0, w, UNITS, gw, ow, dose, t_on, t_off, 4, center=c)
            assert (bits(buf2) == bits(buf)).all(), f"{tag}: units bits differ from the emulation's"
    return worst


def gate_problem(w=65, K=2, n=7, t=5):
    """Rows whose gates differ at step t = 5: ON, before t_on, at t_off, dose 0, ON, a never-opening window (t_on = t_off), ON; NaN and -0 planted
    in every row.  -> (rows, dirs, gain, offset, dose, t_on, t_off, on [n])."""
    h = rows_of(n, w, seed=3).copy()
    h[:, 0], h[:, w // 2] = np.float32(-0.0), np.float32(np.nan)
    dose = np.array([1, 1, 1, 0, 0.25, 1, 0.5], np.float32)
    t_on = np.array([0, 6, 0, 0, 5, 5, 4], np.int32)
    t_off = np.array([9, 9, 5, 9, 6, 5, 6], np.int32)
    on = gate(t, t_on, t_off, dose)
    assert on.tolist() == [True, False, False, False, True, False, True]
    return h, directions(K, w), np.zeros(K, np.float32), np.full(K, S, np.float32), dose, t_on, t_off, on
