"""The float64 reference of the autoregressive-HMM kernels (csrc/arhmm_core.h), the case generators and the checkers that tests/test_arhmm_cpu.py (the
host emulation) and tests/test_gpu_arhmm.py (the C-ABI) share.  A `backend` is analysis.pca.HipBackend or the same backend on numpy arrays,
tests/hostemu/arhmm_emu.B.  What does not look at x (forward-backward, transitions, Viterbi) is referenced by tests/hmm_ref.py.

The model is DEFINED on xc = float32(x - center): the reference starts from those float32 values and is float64 from there.

Cases (n, d, L, k): a single row; one row past a 256-row chunk; MoSeq's shape; odd tiles (p = 35, q = 52); every limit.  Each is cut into sequences
that include the lengths 1, L, L + 1 and one longer than a staging block of 128 rows (lengths_of).

The bounds, u = 2^-24, e = 2^-53, p = L d + 1, first order in u unless said:
  residual  pred is the intercept plus L d fmaf: every term carries at most L d roundings, so |pred^ - pred| <= L d u s, s = |b| + sum |W| |phi|;
            r^ = fl(xc - pred^): D = |r^ - r| <= (p + 1) u s + u |r|.
  q         a term is r^ fl(r^ fl(1 / var)): two roundings, then at most d in the fmaf chain of non-negative terms: relative (d + 2) u on r^2 / var,
            and r^2 - r'^2 = 2 r D + D^2 (the square kept: where r is near 0 it is the whole error):
            |q^ - q| <= sum_c (2 |r_c| D_c + D_c^2) / var_c + (d + 5) u q     (3 u of slack on the chain).
  logb      fmaf(-1/2, q^, c^): half of that, c_j rounded once from float64 (2 u |c_j| leaves room for the reference's own log), one rounding:
            u |logb|.
  moments   every term gamma psi_a psi_b is float64 from the first product: two roundings, then at most one per row of its part and one per part:
            (rows + parts + 2) e sum |gamma psi_a psi_b|, parts <= ceil(n / 256).
  solve     Cholesky and the two substitutions solve (G + dG) w = c with |dG| <= gamma_(3p+1) |L| |L^T| and || |L| |L^T| ||_2 <= p ||G||_2 (Higham,
            Accuracy and Stability, 10.2 and 10.4): ||dw|| / ||w|| <= p (3 p + 1) e cond_2(G) to first order.  numpy's LU solve of the reference has a
            bound of the same form, and both are compared normwise per row of W: 4 p (3 p + 1) e cond(G) ||W_c|| (the factor 4: the two
            solves and the first-order slack), plus the float32 rounding u ||W_c||.  The variance (M_xx - W . C) / w inherits ||dW_c|| ||C_c|| / w
            and (p + 3) e (|M_xx| + |W| . |C|) / w of its own sum, then u of rounding; the mean 4 e of two operations, then u.
            The bounds need cond(G) <= 1e6, which the tests assert on the reference.
Every checker prints the worst observed ratio to its bound."""
from __future__ import annotations

import functools

import numpy as np

from tests import hmm_ref as H

CASES = ((1, 1, 0, 1), (257, 3, 1, 2), (1000, 10, 3, 7), (4099, 17, 2, 33), (2050, 32, 4, 128))
WARMUP = {CASES[0]: 0, CASES[1]: 1, CASES[2]: 3, CASES[3]: 4, CASES[4]: 4, (300, 32, 4, 128): 4}
CPU_LIMIT = (300, 32, 4, 128)      # every limit with the rows the host emulation affords
U24, E53 = 2.0 ** -24, 2.0 ** -53
f64, f32, seq_of = H.f64, H.f32, H.seq_of


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def lengths_of(n, L):
    """Sequence lengths summing to n: one longer than a staging block first, then 1, L and L + 1 (so a short sequence follows a long one), then the
    rest in pieces of at most 700 rows; a single sequence where n is too small for that."""
    short = [1] + ([L] if L >= 1 else []) + [L + 1]
    if n <= sum(short) + 1:
        return (n,)
    rest = n - sum(short)
    out = [min(rest, 300)] + short
    rest -= out[0]
    while rest > 0:
        out.append(min(rest, 700))
        rest -= out[-1]
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- data
@functools.lru_cache(None)
def case_data(case):
    """-> (x float32 [n, d]: a stable AR(1) walk per sequence about an offset, seq_start, center float32 [d]: the column mean, weights float32
    [k, d, p], vars float32 [k, d] in [0.25, 4], gamma float32 [n, k]: soft posteriors); read-only."""
    n, d, L, k = case
    r = np.random.default_rng(9000 + n + k)
    lengths = lengths_of(n, L)
    x = np.zeros((n, d))
    t = 0
    for T in lengths:
        v = r.standard_normal(d)
        for _ in range(T):
            v = 0.8 * v + 0.6 * r.standard_normal(d)
            x[t] = v + 1.5
            t += 1
    x = f32(x)
    center = f32(f64(x).mean(0))
    p = L * d + 1
    W = 0.5 * r.standard_normal((k, d, p)) / np.sqrt(max(L * d, 1))
    W[:, :, -1] = 0.5 * r.standard_normal((k, d))
    var = r.uniform(0.25, 4.0, (k, d))
    g = r.gamma(0.3, size=(n, k)) + 1e-3
    out = (x, seq_of(lengths), center, f32(W), f32(var), f32(g / g.sum(1, keepdims=True)))
    for a in out:
        a.setflags(write=False)
    return out


def design(x, seq, L, R, center):
    """-> (xc [n, d], phi [n, p]: zeros in the unscored rows, scored [n] bool) in float64 from xc = float32(x - center)."""
    x = f32(x)
    xc = f64(x if center is None else x - f32(center)[None, :])
    n, d = xc.shape
    phi, scored = np.zeros((n, L * d + 1)), np.zeros(n, bool)
    for t0, t1 in zip(seq[:-1], seq[1:]):
        a = t0 + R
        if a >= t1:
            continue
        scored[a:t1] = True
        phi[a:t1, -1] = 1.0
        for l in range(L):
            phi[a:t1, l * d:(l + 1) * d] = xc[a - 1 - l:t1 - 1 - l]
    return xc, phi, scored


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def logb64(x, seq, L, R, center, W, var):
    """-> (logb [n, k], its bound [n, k]) in float64 (the module's text derives the bound); the unscored rows 0 with bound 0."""
    xc, phi, scored = design(x, seq, L, R, center)
    W64, var64 = f64(W), f64(var)
    (n, d), k, p = xc.shape, var64.shape[0], phi.shape[1]
    logb, bound = np.zeros((n, k)), np.zeros((n, k))
    c = -0.5 * np.log(2.0 * np.pi * var64).sum(1)
    for j in range(k):
        pred, s = phi @ W64[j].T, np.abs(phi) @ np.abs(W64[j]).T
        r = xc - pred
        D = (p + 1) * U24 * s + U24 * np.abs(r)
        q = (r * r / var64[j]).sum(1)
        bq = ((2 * np.abs(r) * D + D * D) / var64[j]).sum(1) + (d + 5) * U24 * q
        logb[:, j] = c[j] - 0.5 * q
        bound[:, j] = 0.5 * bq + 2 * U24 * abs(c[j]) + U24 * np.abs(logb[:, j])
    logb[~scored], bound[~scored] = 0.0, 0.0
    return logb, bound


def moments64(x, seq, L, R, center, gamma):
    """-> (moments [k, q, q], weight [k], sum |gamma psi_a psi_b| [k, q, q]) in float64; gamma is the float32 array the kernel is given."""
    xc, phi, scored = design(x, seq, L, R, center)
    psi = np.concatenate([phi, np.where(scored[:, None], xc, 0.0)], 1)
    g = f64(gamma) * scored[:, None]
    k, q = g.shape[1], psi.shape[1]
    M, A = np.zeros((k, q, q)), np.zeros((k, q, q))
    for j in range(k):
        M[j] = (psi * g[:, j, None]).T @ psi
        A[j] = (np.abs(psi) * np.abs(g[:, j, None])).T @ np.abs(psi)
    return M, g.sum(0), A


def solve64(M, w, d, L, center, ridge, min_var, min_weight, W_in, var_in, means_in):
    """numpy.linalg on the moments given -> (weights, vars, means float64, status int32, cond(G) [k]: 0 where the state is not solved)."""
    k, p = len(w), L * d + 1
    W, var, mu = f64(W_in).copy(), f64(var_in).copy(), f64(means_in).copy()
    status, cond = np.zeros(k, np.int32), np.zeros(k)
    cen = np.zeros(d) if center is None else f64(center)
    pen = np.append(np.full(p - 1, float(ridge)), 0.0)
    for j in range(k):
        if not (w[j] >= min_weight and w[j] > 0):
            status[j] = 1
            continue
        G, C = M[j, :p, :p] + np.diag(pen), M[j, p:, :p]
        try:
            np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            status[j] = 2
            continue
        cond[j] = np.linalg.cond(G)
        W[j] = np.linalg.solve(G, C.T).T
        var[j] = np.maximum((np.diag(M[j, p:, p:]) - (W[j] * C).sum(1)) / w[j], min_var)
        mu[j] = cen + C[:, p - 1] / w[j]
    return W, var, mu, status, cond


# ---------------------------------------------------------------------------------------------------------------- checkers
def check_emission(case, backend, what="", rows=None):
    x, seq, center, W, var, _ = case_data(case)
    n, d, L, k = case
    R = WARMUP[case]
    logb = backend.arhmm_emission(backend.asarray(x) if rows is None else rows, seq, L, R, center, W, var)
    ref, bound = logb64(x, seq, L, R, center, W, var)
    err = np.abs(f64(logb) - ref)
    _, _, scored = design(x, seq, L, R, center)
    worst = float((err[scored] / bound[scored]).max()) if scored.any() else 0.0
    print(f"[arhmm {what}] emission {n} x {d}, {L} lags, {k} states, sequences {list(np.diff(seq))[:6]}: worst error {worst:.3g} of its bound, "
          f"{int(scored.sum())} rows scored")
    assert logb.dtype == np.float32 and logb.shape == ref.shape
    assert (logb[~scored] == 0).all() and (err <= bound).all()
    return logb


def check_emission_exact(backend):
    """Data and centre multiples of 1/4 in [-2, 2], weights multiples of 1/4 in [-1, 1], 1 / var in {1, 2, 4}: every product and sum of the
    chain is a multiple of 1/256 below 2^16, exact in float32, so logb = fma(-1/2, q, c_j) is one rounding of the exact value."""
    r = np.random.default_rng(61)
    n, d, L, k = 300, 5, 2, 9
    x, center = f32(r.integers(-8, 9, (n, d)) / 4.0), f32(r.integers(-4, 5, d) / 4.0)
    W = f32(r.integers(-4, 5, (k, d, L * d + 1)) / 4.0)
    var = f32(r.choice([0.25, 0.5, 1.0], (k, d)))
    seq = seq_of((1, 2, 3, 150, 144))
    xc, phi, scored = design(x, seq, L, 3, center)
    q = np.stack([(((xc - phi @ f64(W[j]).T) ** 2) / f64(var[j])).sum(1) for j in range(k)], 1)
    assert q.max() < 2 ** 16 and (q * 256 == np.rint(q * 256)).all()
    c = f32(-0.5 * np.log(2.0 * np.pi * f64(var)).sum(1))
    want = f32(f64(c)[None, :] - 0.5 * q)
    want[~scored] = 0
    logb = backend.arhmm_emission(backend.asarray(x), seq, L, 3, center, W, var)
    np.testing.assert_array_equal(bits(logb), bits(want))


def check_moments(case, backend, what="", gamma=None):
    x, seq, center, _, _, g = case_data(case)
    n, d, L, k = case
    R = WARMUP[case]
    g = g if gamma is None else gamma
    M, w = backend.arhmm_moments(backend.asarray(x), seq, L, R, center, g)
    rM, rw, A = moments64(x, seq, L, R, center, g)
    bound = (n + (n + 255) // 256 + 2) * E53 * A
    err = np.abs(M - rM)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    p = L * d + 1
    print(f"[arhmm {what}] moments {n} x {d}, {L} lags into {k} x {p + d} x {p + d}: worst error {worst:.3g} of its bound")
    assert M.dtype == np.float64 and w.dtype == np.float64 and M.shape == rM.shape
    assert (err <= bound).all()
    np.testing.assert_array_equal(bits(M), bits(np.swapaxes(M, 1, 2)))      # symmetric to the bit
    np.testing.assert_array_equal(bits(w), bits(M[:, p - 1, p - 1]))         # the weight is the intercept's own sum
    assert (np.abs(w - rw) <= (n + (n + 255) // 256 + 2) * E53 * rw).all()
    return M, w


def check_moments_exact(backend):
    """Integer data, no centre and a one-hot gamma: every product and sum is an integer below 2^53, so the moments are exact."""
    r = np.random.default_rng(62)
    n, d, L, k = 700, 6, 2, 5
    x = f32(r.integers(-8, 9, (n, d)))
    seq = seq_of((1, 2, 3, 400, 294))
    g = np.zeros((n, k), np.float32)
    g[np.arange(n), r.integers(0, k, n)] = 1
    M, w = backend.arhmm_moments(backend.asarray(x), seq, L, 2, None, g)
    rM, rw, _ = moments64(x, seq, L, 2, None, g)
    assert (rM == np.rint(rM)).all()
    np.testing.assert_array_equal(M, rM)
    np.testing.assert_array_equal(w, rw)


def check_moments_ignore_unscored_rows(backend):
    """gamma in the unscored rows, whatever it holds, changes no bit; a sequence alone and between two neighbours that hold 1e30 (gamma 0 there)
    gives the same moments within the bound (the row parts differ), and nothing of the neighbours leaks in."""
    x, seq, center, _, _, g = case_data(CASES[2])
    n, d, L, k = CASES[2]
    R = 5
    xa = backend.asarray(x)
    M, w = backend.arhmm_moments(xa, seq, L, R, center, g)
    g2 = np.array(g)
    for t0, t1 in zip(seq[:-1], seq[1:]):
        g2[t0:min(t0 + R, t1)] = 1e6
    M2, w2 = backend.arhmm_moments(xa, seq, L, R, center, g2)
    np.testing.assert_array_equal(bits(M), bits(M2))
    np.testing.assert_array_equal(bits(w), bits(w2))
    mid = np.array(x[:300])
    batch = np.concatenate([np.full((5, d), 1e30, np.float32), mid, np.full((7, d), 1e30, np.float32)])
    gb = np.concatenate([np.zeros((5, k), np.float32), g[:300], np.zeros((7, k), np.float32)])
    Ma, _ = backend.arhmm_moments(backend.asarray(mid), seq_of((300,)), L, R, center, g[:300])
    Mb, _ = backend.arhmm_moments(backend.asarray(batch), seq_of((5, 300, 7)), L, R, center, gb)
    _, _, A = moments64(mid, seq_of((300,)), L, R, center, g[:300])
    assert np.isfinite(Mb).all() and (np.abs(Ma - Mb) <= 2 * 304 * E53 * A).all()


@functools.lru_cache(None)
def solve_ridge(case):
    """The C-level penalty of a case: one pseudo-row of the mean column variance."""
    return float(f64(case_data(case)[0]).var(0).mean())


def check_solve(case, backend, M, w, what=""):
    """The kernel's solve against numpy.linalg on the kernel's own moments (M, w from check_moments)."""
    x, seq, center, W0, var0, _ = case_data(case)
    n, d, L, k = case
    p, ridge = L * d + 1, solve_ridge(case) if L else 0.0
    mu0 = np.full((k, d), 3.5, np.float32)
    W, var, mu, status = backend.arhmm_solve(M, w, d, L, center, W0, var0, ridge, 1e-6, 1e-3, means=mu0)
    rW, rvar, rmu, rstatus, cond = solve64(M, w, d, L, center, ridge, 1e-6, 1e-3, W0, var0, mu0)
    assert cond.max() <= 1e6, f"cond(G) = {cond.max():.3g}: the case no longer meets the condition of the bound"
    np.testing.assert_array_equal(status, rstatus)
    worst = [0.0, 0.0, 0.0]
    for j in range(k):
        if rstatus[j]:
            for got, given in ((W[j], W0[j]), (var[j], var0[j]), (mu[j], mu0[j])):
                np.testing.assert_array_equal(bits(got), bits(f32(given)))
            continue
        C = M[j, p:, :p]
        bW = (U24 + 4 * p * (3 * p + 1) * E53 * cond[j]) * np.linalg.norm(rW[j], axis=1) + 1e-300
        eW = np.linalg.norm(f64(W[j]) - rW[j], axis=1)
        bV = U24 * rvar[j] + (bW * np.linalg.norm(C, axis=1) + (p + 3) * E53 * (np.abs(np.diag(M[j, p:, p:])) + (np.abs(rW[j]) * np.abs(C)).sum(1))) / w[j]
        bM = U24 * np.abs(rmu[j]) + 4 * E53 * (np.abs(f64(center)) + np.abs(C[:, p - 1]) / w[j]) + 1e-300
        worst = [max(a, float(b)) for a, b in zip(worst, ((eW / bW).max(), (np.abs(f64(var[j]) - rvar[j]) / bV).max(), (np.abs(f64(mu[j]) - rmu[j]) / bM).max()))]
        assert (var[j] >= f32(1e-6)).all()
    print(f"[arhmm {what}] solve {k} states, p = {p}: cond(G) up to {cond.max():.3g}; worst error {worst[0]:.3g} (weights), {worst[1]:.3g} (variances), "
          f"{worst[2]:.3g} (means) of the bounds; status {np.bincount(status, minlength=3).tolist()}")
    assert W.dtype == np.float32 and var.dtype == np.float32 and status.dtype == np.int32
    assert max(worst) <= 1.0, worst


def check_light_and_singular(backend, what=""):
    """Four states over integer rows without a centre, ridge = 0: state 1 is given no row (light), state 2 only rows whose channel 0 was 0 one step
    before (its first regressor column is exactly 0: the first pivot is 0).  They keep their bits; states 0 and 3 are solved."""
    r = np.random.default_rng(63)
    n, d, L, k = 600, 3, 1, 4
    x = f32(r.integers(-6, 7, (n, d)))
    x[200:330, 0] = 0
    lab = r.choice([0, 3], n)
    lab[201:330] = 2
    g = np.zeros((n, k), np.float32)
    g[np.arange(n), lab] = 1
    seq = seq_of((n,))
    M, w = backend.arhmm_moments(backend.asarray(x), seq, L, 1, None, g)
    W0, var0, mu0 = f32(r.standard_normal((k, d, L * d + 1))), f32(r.uniform(1, 2, (k, d))), f32(r.standard_normal((k, d)))
    W, var, mu, status = backend.arhmm_solve(M, w, d, L, None, W0, var0, 0.0, 1e-9, 1e-3, means=mu0)
    rW, rvar, rmu, rstatus, cond = solve64(M, w, d, L, None, 0.0, 1e-9, 1e-3, W0, var0, mu0)
    print(f"[arhmm {what}] light and singular: status {status.tolist()}, weights {w.tolist()}")
    assert status.tolist() == [0, 1, 2, 0] and rstatus.tolist() == [0, 1, 2, 0] and w[1] == 0 and w[2] == 129
    for j in (1, 2):
        for got, given in ((W[j], W0[j]), (var[j], var0[j]), (mu[j], mu0[j])):
            np.testing.assert_array_equal(bits(got), bits(given))
    for j in (0, 3):
        assert np.abs(f64(W[j]) - rW[j]).max() <= 1e-5 and np.abs(f64(var[j]) - rvar[j]).max() <= 1e-5 * rvar[j].max()
        assert np.abs(f64(mu[j]) - rmu[j]).max() <= 1e-6


def check_gaussian_chain(backend):
    """lags = 0, warmup = 0, no centre and the intercepts as means: the bits of tmjx_hmm_emission."""
    x, seq, _, _, var, _ = case_data(CASES[3])
    n, d, _, k = CASES[3]
    mu = f32(np.random.default_rng(64).standard_normal((k, d)) + 1.5)
    xa = backend.asarray(x)
    a, b = backend.arhmm_emission(xa, seq, 0, 0, None, mu[:, :, None], var), backend.hmm_emission(xa, mu, var)
    np.testing.assert_array_equal(bits(a), bits(b))


def check_boundaries(backend):
    """A sequence's logb has the same bits alone as inside a batch between two other sequences, also when the neighbours hold 1e30."""
    x, _, center, W, var, _ = case_data(CASES[2])
    n, d, L, k = CASES[2]
    mid = np.array(x[300:560])
    alone = backend.arhmm_emission(backend.asarray(mid), seq_of((260,)), L, L, center, W, var)
    assert np.isfinite(alone).all() and (alone[:L] == 0).all() and (alone[L:] != 0).all()
    for fill in (None, 1e30):
        before, after = (np.array(x[:131]), np.array(x[600:607])) if fill is None else (np.full((131, d), fill, np.float32), np.full((7, d), fill, np.float32))
        batch = np.concatenate([before, mid, after])
        got = backend.arhmm_emission(backend.asarray(batch), seq_of((131, 260, 7)), L, L, center, W, var)
        np.testing.assert_array_equal(bits(got[131:391]), bits(alone))
        assert (got[:L] == 0).all() and (got[131:131 + L] == 0).all() and (got[391:391 + L] == 0).all()


def check_short_sequences_are_unscored(backend):
    """Sequences of `warmup` rows or fewer are entirely unscored: zeros, no moments, a defined result."""
    x, _, center, W, var, g = case_data(CASES[2])
    n, d, L, k = CASES[2]
    seq = seq_of((5, 1, 3, 5))
    xa = backend.asarray(np.array(x[:14]))
    assert (backend.arhmm_emission(xa, seq, L, 5, center, W, var) == 0).all()
    M, w = backend.arhmm_moments(xa, seq, L, 5, center, g[:14])
    assert (M == 0).all() and (w == 0).all()


@functools.lru_cache(None)
def rotations(T=600, S=5, seed=2025, lengths=None):
    """Three sticky states (self-transition 0.98) over two features: state j rotates by 0.15 / 0.45 / 0.9 rad per step and contracts by 0.95, noise
    0.3.  All share one mean and one stationary cloud: only the dynamics tell them apart -> (x float32, lengths, true states)."""
    r = np.random.default_rng(seed)
    k, lengths = 3, (T,) * S if lengths is None else lengths
    A = np.full((k, k), 0.01)
    np.fill_diagonal(A, 0.98)
    rot = [0.95 * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) for a in (0.15, 0.45, 0.9)]
    z = H.draw_chain(r, lengths, A, np.full(k, 1 / k))
    x = np.zeros((len(z), 2))
    seq = seq_of(lengths)
    for t0, t1 in zip(seq[:-1], seq[1:]):
        x[t0] = r.standard_normal(2)
        for t in range(t0 + 1, t1):
            x[t] = rot[z[t]] @ x[t - 1] + 0.3 * r.standard_normal(2)
    x = f32(x)
    x.setflags(write=False)
    return x, tuple(lengths), z


def check_fit_steps(backend, what=""):
    """tmjx_arhmm_fit against the same steps called one by one: the same bits; with prior = kappa = ridge = 0 and floors that never bind the loglik
    never falls by more than relative 1e-6."""
    x, lengths, z = rotations(lengths=(37, 300, 5, 2, 1))
    seq, L, R, k = seq_of(lengths), 1, 2, 3
    xa = backend.asarray(x)
    center = f32(f64(x).mean(0))
    r = np.random.default_rng(65)
    W0 = f32(np.concatenate([np.stack([0.9 * np.eye(2) + 0.1 * r.standard_normal((2, 2)) for _ in range(k)]), np.zeros((k, 2, 1))], 2))
    v0, A0, p0 = np.full((k, 2), 0.2, np.float32), np.full((k, k), 1.0 / k, np.float32), np.full(k, 1.0 / k, np.float32)
    fit = backend.arhmm_fit(xa, seq, L, R, center, W0, v0, A0, p0, 12, 0.0, 0.0, 0.0, 0.0, 1e-9, 1e-3)
    info = fit[7]
    W_, v_, A_, p_, trace = W0, v0, A0, p0, []
    status = None
    for it in range(12):
        logb = backend.arhmm_emission(xa, seq, L, R, center, W_, v_)
        gamma, xi, start, loglik, total = backend.hmm_forward_backward(logb, seq, A_, p_)
        trace.append(total)
        if it > 0 and total - trace[-2] <= 0.0:
            break
        M, w = backend.arhmm_moments(xa, seq, L, R, center, gamma)
        W_, v_, _, status = backend.arhmm_solve(M, w, 2, L, center, W_, v_, 0.0, 1e-9, 1e-3)
        A_, p_ = backend.hmm_transitions(xi, start, 0.0, 0.0, A_, p_)
    else:
        logb = backend.arhmm_emission(xa, seq, L, R, center, W_, v_)
        gamma, xi, start, loglik, total = backend.hmm_forward_backward(logb, seq, A_, p_)
    labels, _ = backend.hmm_viterbi(logb, seq, A_, p_)
    print(f"[arhmm {what}] fit: {info.n_iter} iterations, loglik {trace[0]:.6f} -> {info.loglik:.6f}, status {status.tolist()}")
    for a, b in zip(trace, trace[1:]):
        assert b >= a - 1e-6 * abs(a), trace
    assert info.n_iter == len(trace) and info.loglik == total and info.n_singular == int((status == 2).sum()) and len(trace) >= 3
    for got, want in zip(fit[:7], (W_, v_, A_, p_, gamma, labels, status)):
        np.testing.assert_array_equal(bits(got), bits(want))


def check_repeat_and_strides(backend, strided, what=""):
    """Two calls, and strided rows (`strided(x)`: the same rows as a column slice of a wider buffer, which asarray must not copy), give the same
    bits: emission, moments and the fit."""
    case = CASES[3]
    x, seq, center, W, var, g = case_data(case)
    n, d, L, k = case
    R = WARMUP[case]
    xr, lengths, _ = rotations(lengths=(37, 300, 5))
    cr = f32(f64(xr).mean(0))
    r = np.random.default_rng(66)
    fit_args = (seq_of(lengths), 2, 2, cr, f32(0.2 * r.standard_normal((3, 2, 5))), np.full((3, 2), 0.3, np.float32), np.full((3, 3), 1 / 3, np.float32),
                np.full(3, 1 / 3, np.float32), 4, 0.0, 0.1, 0.5, 0.05, 1e-3, 1e-3)

    def run(rows, rows_fit):
        return (backend.arhmm_emission(rows, seq, L, R, center, W, var), *backend.arhmm_moments(rows, seq, L, R, center, g),
                *backend.arhmm_fit(rows_fit, *fit_args)[:7])
    want = run(backend.asarray(x), backend.asarray(xr))
    for rows, rows_fit in ((backend.asarray(x), backend.asarray(xr)), (strided(x), strided(xr))):
        for a, b in zip(run(rows, rows_fit), want):
            np.testing.assert_array_equal(bits(np.asarray(a)), bits(np.asarray(b)))


# ---------------------------------------------------------------------------------------------------------------- model level
def mstep64(xc, phi, scored, g, d, L, ridge, min_var, min_weight, W, var):
    """The float64 M-step: the moments and numpy's solve, a light state as given."""
    psi = np.concatenate([phi, np.where(scored[:, None], xc, 0.0)], 1)
    gs = g * scored[:, None]
    M = np.stack([(psi * gs[:, j, None]).T @ psi for j in range(g.shape[1])])
    return solve64(M, gs.sum(0), d, L, None, ridge, min_var, min_weight, W, var, np.zeros_like(var))[:2]


def em64(x, seq, lab0, k, L, R, center, ridge, prior, kappa, min_var, max_iter, tol):
    """Float64 EM with the initialisation and the loop of analysis.arhmm.ARHMM.fit -> (labels, loglik, weights)."""
    xc, phi, scored = design(x, seq, L, R, center)
    n, d = xc.shape
    g0 = np.zeros((n, k))
    g0[np.arange(n), lab0] = 1
    colvar = float(f64(x).var(0).mean())
    W, var = mstep64(xc, phi, scored, g0, d, L, ridge, min_var, 0.5, np.zeros((k, d, L * d + 1)), np.full((k, d), max(colvar, min_var, 1e-30)))
    trans = np.zeros((k, k))
    for t0, t1 in zip(seq[:-1], seq[1:]):
        np.add.at(trans, (lab0[t0:t1 - 1], lab0[t0 + 1:t1]), 1)
    A, pi = H.transitions64(trans, np.bincount(lab0[seq[:-1]], minlength=k), prior, kappa, np.full((k, k), 1 / k), np.full(k, 1 / k))

    def emit():
        lb = np.zeros((n, k))
        for j in range(k):
            r = xc - phi @ W[j].T
            lb[:, j] = -0.5 * (np.log(2 * np.pi * var[j]).sum() + (r * r / var[j]).sum(1))
        lb[~scored] = 0
        return lb
    prev = 0.0
    for it in range(max_iter):
        logb = emit()
        gamma, xi, start, ll = H.fb64(logb, seq, A, pi)
        total = float(ll.sum())
        if it > 0 and total - prev <= tol * abs(prev):
            break
        prev = total
        W, var = mstep64(xc, phi, scored, gamma, d, L, ridge, min_var, 1e-3, W, var)
        A, pi = H.transitions64(xi, start, prior, kappa, A, pi)
    else:
        logb = emit()
        total = float(H.fb64(logb, seq, A, pi)[3].sum())
    with np.errstate(divide="ignore"):
        return H.viterbi64(logb, seq, np.log(A), np.log(pi))[0], total, W


def angles_of(weights):
    """The rotation angle of every state's lag-1 matrix: the argument of its complex eigenvalue pair, sorted."""
    return np.sort([np.abs(np.angle(np.linalg.eigvals(f64(w)[:, :2]))).max() for w in weights])


def check_model(backend, what=""):
    """The planted rotations: the references keep telling the two models apart; ARHMM recovers the motifs and their angles as the float64 EM does;
    the Gaussian HMM on the same rows stays at chance."""
    from track_mjx_amd.analysis import arhmm as AR
    from track_mjx_amd.analysis import hmm as HM
    x, lengths, truth = rotations()
    seq = seq_of(lengths)
    m = AR.ARHMM(3, lags=1, max_iter=30, tol=1e-5, prior=0.1, n_init=2, seed=0, backend=backend).fit(x, lengths)
    lab0 = m.init_labels_
    acc_km = H.accuracy(lab0, truth, 3)
    gauss64, _ = H.em64(x, seq, lab0, 3, 0.1, 0.0, m.min_var_, 30, 1e-5)
    ar64, ll64, W64 = em64(x, seq, lab0, 3, 1, 1, m.center_, m.ridge_, 0.1, 0.0, m.min_var_, 30, 1e-5)
    acc_g64, acc_ar64, acc = H.accuracy(gauss64, truth, 3), H.accuracy(ar64, truth, 3), H.accuracy(m.labels_, truth, 3)
    g = HM.GaussianHMM(3, max_iter=30, tol=1e-5, prior=0.1, n_init=2, seed=0, backend=backend).fit(x, lengths)
    acc_g = H.accuracy(g.labels_, truth, 3)
    ang, ang64 = angles_of(m.weights_), angles_of(W64)
    print(f"[arhmm {what}] planted rotations: accuracy k-means {acc_km:.4f}, float64 Gaussian EM {acc_g64:.4f}, float64 AR EM {acc_ar64:.4f}, GaussianHMM "
          f"{acc_g:.4f}, ARHMM {acc:.4f}; angles {np.round(ang, 4).tolist()} against {np.round(ang64, 4).tolist()} in float64 (planted 0.15, 0.45, 0.9); "
          f"loglik {m.loglik_:.4f} against {ll64:.4f}")
    assert acc_g64 <= 0.5 and acc_ar64 >= 0.9, "the planted data no longer separate the two models"
    assert acc >= acc_ar64 - 0.01
    assert np.abs(ang - ang64).max() <= 0.02
    assert acc_g <= 0.5
    assert m.weights_.shape == (3, 2, 3) and m.status_.tolist() == [0, 0, 0] and m.n_scored_ == len(truth) - len(lengths)
    assert (np.diff(m.counts_) <= 0).all() and (np.bincount(m.labels_, minlength=3) == m.counts_).all()
    np.testing.assert_array_equal(m.predict(x, lengths), m.labels_)
    bound = float((2 * np.diff(seq) * (3 + 8) * U24).sum())      # hmm_ref's loglik bound of the forward pass
    # (the states were renumbered after the fit: the sums run in another order, so not the same bits)
    assert abs(m.score(x, lengths) - m.loglik_) <= 2 * bound and abs(m.score_sequences(x, lengths).sum() - m.loglik_) <= 2 * bound
    assert np.abs(m.predict_proba(x, lengths) - m.gamma_).max() <= 2 * (2 * max(lengths) * (3 + 8) * U24 + H.TINY)      # each within hmm_ref's gamma bound
    assert np.abs(m.means_).max() < 1.0      # one mean: every state's weighted mean of x lies inside one deviation (0.96) of the shared cloud


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, alloc, ptr, untouched, what=""):
    """Every refusal through the C-ABI: -22 with a message that names the value, nothing launched, sentinel-filled outputs untouched.
    `alloc(shape, dtype, fill)` -> an array of the library's memory, `ptr(a)` its address, `untouched(a, fill)` whether it still holds `fill`."""
    import ctypes as C
    n, d, L, k, S = 300, 4, 2, 3, 3
    p, q = L * d + 1, L * d + 1 + d
    x, cen = alloc((n, d), np.float32, 0.0), alloc((d,), np.float32, 0.0)
    outs = {"W": alloc((k, d, p), np.float32, -5.0), "var": alloc((k, d), np.float32, -5.0), "A": alloc((k, k), np.float32, -5.0), "pi": alloc((k,), np.float32, -5.0),
            "logb": alloc((n, k), np.float32, -5.0), "gamma": alloc((n, k), np.float32, -5.0), "labels": alloc((n,), np.int32, -5), "status": alloc((k,), np.int32, -5),
            "M": alloc((k, q, q), np.float64, -5.0), "w": alloc((k,), np.float64, -5.0), "mu": alloc((k, d), np.float32, -5.0)}
    o = {key: ptr(v) for key, v in outs.items()}
    floats = C.c_int64(0)
    assert lib.tmjx_arhmm_workspace(n, d, L, k, S, C.byref(floats)) == 0 and floats.value > 4 * n * k
    ws = alloc((int(floats.value) + 4,), np.float32, 0.0)
    X, CEN, WS = ptr(x), ptr(cen), ptr(ws)
    seq = (C.c_int32 * 4)(0, 100, 200, 300)
    err = lib.tmjx_last_error
    nan = float("nan")

    def emission(n=n, d=d, ldx=None, seq=seq, S=S, lags=L, warmup=L, k=k, x=X, weights=o["W"], vars=o["var"], out=o["logb"], ws=WS):
        return lib.tmjx_arhmm_emission(x, n, d, d if ldx is None else ldx, seq, S, lags, warmup, CEN, weights, vars, k, out, ws, None)

    def moments(d=d, seq=seq, lags=L, warmup=L, k=k, gamma=o["gamma"], M=o["M"], w=o["w"], ws=WS):
        return lib.tmjx_arhmm_moments(X, n, d, d, seq, S, lags, warmup, CEN, gamma, k, M, w, ws, None)

    def solve(d=d, lags=L, k=k, ridge=0.0, min_var=0.0, min_weight=0.0, M=o["M"], status=o["status"], ws=WS, warmup=None):      # (it has no warm-up)
        return lib.tmjx_arhmm_solve(M, o["w"], k, d, lags, CEN, ridge, min_var, min_weight, o["W"], o["var"], o["mu"], status, ws, None)
    from track_mjx_amd import hip
    info = C.byref(hip.ArhmmInfo())

    def fit(d=d, seq=seq, lags=L, warmup=L, k=k, max_iter=5, tol=1e-4, prior=0.1, kappa=0.0, ridge=0.0, min_var=1e-3, min_weight=1e-3, info=info, labels=o["labels"],
            ws=WS):
        return lib.tmjx_arhmm_fit(X, n, d, d, seq, S, lags, warmup, CEN, k, o["W"], o["var"], o["A"], o["pi"], o["gamma"], labels, o["status"], max_iter, tol, prior,
                                  kappa, ridge, min_var, min_weight, info, ws, None)
    shape = ((dict(d=33), b"limit of 32"), (dict(lags=5, warmup=5), b"outside 0 .. 4"), (dict(lags=-1), b"outside 0 .. 4"), (dict(k=129), b"limit of 128"),
             (dict(k=0), b"k must be >= 1"))
    rows = shape + ((dict(warmup=1), b"warmup = 1 is smaller than lags = 2"), (dict(seq=(C.c_int32 * 4)(1, 100, 200, 300)), b"seq_start[0] = 1"),
                    (dict(seq=(C.c_int32 * 4)(0, 200, 200, 300)), b"strictly increasing"), (dict(seq=(C.c_int32 * 4)(0, 100, 200, 299)), b"seq_start[S] = 299"),
                    (dict(seq=None), b"null"), (dict(ws=None), b"null"), (dict(ws=WS + 4), b"16-byte"))
    count = 0
    for kw, word in rows + ((dict(n=0), b"n must be >= 1"), (dict(ldx=3), b"ldx = 3"), (dict(S=0), b"S must be >= 1"), (dict(x=None), b"null"),
                            (dict(weights=None), b"null"), (dict(vars=None), b"null"), (dict(out=None), b"null")):
        assert emission(**kw) == -22 and word in err(), (kw, err())
        count += 1
    assert emission(d=32, ldx=32, lags=4, warmup=4, n=0) == -22      # (32 x 4 = 128 is inside the limit: it is n that is refused)
    assert lib.tmjx_arhmm_workspace(n, 43, 3, k, S, C.byref(floats)) == -22 and b"limit of 32" in err()
    assert lib.tmjx_arhmm_workspace(n, 32, 4, k, S, C.byref(floats)) == 0
    assert lib.tmjx_arhmm_workspace(n, 32, 5, k, S, C.byref(floats)) == -22 and lib.tmjx_arhmm_workspace(n, d, L, k, S, None) == -22
    # lags x d = 129 cannot be reached inside d <= 32 and lags <= 4 (the largest product is 128): the check stands behind those two
    for kw, word in rows + ((dict(gamma=None), b"null"), (dict(M=None), b"null"), (dict(w=None), b"null")):
        assert moments(**kw) == -22 and word in err(), (kw, err())
        count += 1
    for kw, word in shape + ((dict(ridge=-1.0), b"ridge"), (dict(ridge=nan), b"ridge"), (dict(min_var=-1.0), b"min_var"), (dict(min_var=nan), b"min_var"),
                             (dict(min_weight=-1.0), b"min_weight"), (dict(min_weight=nan), b"min_weight"), (dict(M=None), b"null"), (dict(status=None), b"null"),
                             (dict(ws=None), b"null"), (dict(ws=WS + 4), b"16-byte")):
        assert solve(**kw) == -22 and word in err(), (kw, err())
        count += 1
    for kw, word in rows + ((dict(max_iter=0), b"max_iter"), (dict(tol=-1.0), b"tol"), (dict(tol=nan), b"tol"), (dict(prior=-1.0), b"prior"), (dict(kappa=nan), b"kappa"),
                            (dict(ridge=-0.5), b"ridge"), (dict(ridge=nan), b"ridge"), (dict(min_var=nan), b"min_var"), (dict(min_weight=-1.0), b"min_weight"),
                            (dict(info=None), b"null"), (dict(labels=None), b"null")):
        assert fit(**kw) == -22 and word in err(), (kw, err())
        count += 1
    for key, v in outs.items():
        assert untouched(v, -5), key
    assert untouched(ws, 0.0)
    print(f"[arhmm {what}] {count} refusals, nothing written")


# ---------------------------------------------------------------------------------------------------------------- command line
def clip_files(tmp_path, widths=(150, 110, 130, 90)):
    """Four small synthetic clip_<i>.h5 whose activations/intention [T, 2] are planted rotations, with activations/wide [T, 40] (too wide), and a
    pca.h5 whose projections/clip_<i> [T, 6] start with the same two columns -> (directory, pca.h5, the features by clip)."""
    from track_mjx_amd import h5lite
    x, lengths, _ = rotations(lengths=tuple(widths), seed=11)
    r = np.random.default_rng(13)
    seq, feats, proj = seq_of(lengths), {}, {}
    for clip, t0, t1 in zip((0, 2, 5, 7), seq[:-1], seq[1:]):
        feats[clip] = np.array(x[t0:t1])
        proj[f"clip_{clip}"] = np.concatenate([feats[clip], f32(0.1 * r.standard_normal((t1 - t0, 4)))], 1)
        h5lite.write_tree(str(tmp_path / f"clip_{clip}.h5"), {"activations": {"intention": feats[clip], "wide": np.zeros((t1 - t0, 40), np.float32)},
                                                              "ctrl": np.zeros((t1 - t0, 2), np.float32)})
    pca = str(tmp_path.parent / "pca.h5")
    h5lite.write_tree(pca, {"projections": proj, "feature": "intention"})
    return str(tmp_path), pca, feats


def check_cli(tmp_path, backend, capsys):
    """The command-line round trip with feature= and with projections=: the file's fields and shapes, centroids, eig_freq_hz with rate=, holdout,
    the file as intervention centroids, the width refusal and the usage errors."""
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import arhmm as AR
    from track_mjx_amd.analysis.intervene import Intervention
    (tmp_path / "clips").mkdir()
    rollouts, pca, feats = clip_files(tmp_path / "clips")
    out = str(tmp_path / "out" / "arhmm.h5")
    n = sum(f.shape[0] for f in feats.values())
    assert AR.main([f"rollouts={rollouts}", "k=3", "lags=1", f"out={out}", "seed=1", "n_init=2", "posteriors=true", "rate=50", "max_iter=10"], backend=backend) == 0
    assert f"[arhmm] intention: {n} samples x 2 features from 4 clips into 3 states of 1 lags" in capsys.readouterr().out
    keys = ("means", "variances", "transmat", "startprob", "centroids", "weights", "center", "lags", "warmup", "status", "n_singular", "loglik",
            "loglik_per_step_train", "n_iter", "converged", "clips", "seed", "counts", "transitions", "dwell_mean", "init_dwell_mean", "eig_modulus", "eig_freq_hz")
    with h5lite.File(out) as h:
        got = {key: np.asarray(h[key][()]) for key in keys}
        assert "loglik_per_step_heldout" not in h and bytes(h["feature"][()]).decode() == "intention"
        labels = {c: np.asarray(h["labels"][f"clip_{c}"][()]) for c in feats}
        conf = {c: np.asarray(h["confidence"][f"clip_{c}"][()]) for c in feats}
        gam = {c: np.asarray(h["gamma"][f"clip_{c}"][()]) for c in feats}
    for key in ("means", "variances", "centroids"):
        assert got[key].shape == (3, 2) and got[key].dtype == np.float32
    np.testing.assert_array_equal(got["centroids"], got["means"])
    assert got["weights"].shape == (3, 2, 3) and got["weights"].dtype == np.float32 and got["center"].shape == (2,) and got["status"].shape == (3,)
    assert int(got["lags"]) == 1 and int(got["warmup"]) == 1 and got["status"].dtype == np.int32 and int(got["n_singular"]) == 0
    assert got["transmat"].shape == (3, 3) and np.allclose(got["transmat"].sum(1), 1, atol=1e-6) and np.isclose(got["startprob"].sum(), 1, atol=1e-6)
    assert got["counts"].dtype == np.int64 and got["counts"].sum() == n and (np.diff(got["counts"]) <= 0).all() and got["transitions"].sum() == n - 4
    assert list(got["clips"]) == [0, 2, 5, 7] and int(got["seed"]) == 1 and (got["variances"] > 0).all()
    assert np.isclose(float(got["loglik_per_step_train"]), float(got["loglik"]) / (n - 4))      # per scored row: one warm-up row per clip
    assert got["eig_modulus"].shape == (3, 2) and got["eig_freq_hz"].shape == (3, 2) and (got["eig_modulus"] < 1.2).all()
    want_hz = np.sort([np.abs(np.angle(np.linalg.eigvals(f64(w)[:, :2]))).max() * 50 / (2 * np.pi) for w in got["weights"]])
    np.testing.assert_allclose(np.sort(got["eig_freq_hz"].max(1)), want_hz, rtol=1e-12)
    assert 0.0 < got["eig_freq_hz"].max() <= 25.0
    for c, f in feats.items():
        T = f.shape[0]
        assert labels[c].dtype == np.int32 and labels[c].shape == (T,) and conf[c].dtype == np.float32 and conf[c].shape == (T,)
        assert gam[c].shape == (T, 3) and np.allclose(gam[c].sum(1), 1, atol=1e-5)
        np.testing.assert_array_equal(conf[c], gam[c][np.arange(T), labels[c]])
    np.testing.assert_array_equal(np.bincount(np.concatenate([labels[c] for c in feats]), minlength=3), got["counts"])
    assert Intervention.from_centroids(out, columns="0:2").target == "intention"
    out2 = str(tmp_path / "out" / "arhmm_proj.h5")
    assert AR.main([f"rollouts={rollouts}", f"projections={pca}", "n_components=3", "k=2", "lags=2", "warmup=4", f"out={out2}", "holdout=2", "n_init=2", "max_iter=5"],
                   backend=backend) == 0
    assert "2 held-out clips" in capsys.readouterr().out
    with h5lite.File(out2) as h:
        held, train = float(np.asarray(h["loglik_per_step_heldout"][()])), float(np.asarray(h["loglik_per_step_train"][()]))
        assert "gamma" not in h and "eig_freq_hz" not in h and np.asarray(h["weights"][()]).shape == (2, 3, 7) and int(np.asarray(h["warmup"][()])) == 4
        assert np.asarray(h["labels"]["clip_7"][()]).shape == (90,) and np.asarray(h["centroids"][()]).shape == (2, 3)
    assert np.isfinite(held) and np.isfinite(train) and abs(held - train) < 2.0
    assert AR.main([f"rollouts={rollouts}", "k=3", f"out={out}", "feature=wide"], backend=backend) == 2                # wider than 32 without projections=
    e = capsys.readouterr().err
    assert "analysis.pca" in e and "40 features" in e
    assert AR.main([f"rollouts={rollouts}", "k=3"], backend=backend) == 2                                               # no out=
    assert AR.main([f"rollouts={rollouts}", "k=3", f"out={out}", "colour=red"], backend=backend) == 2                   # an unknown option
    assert "usage:" in capsys.readouterr().err
    for bad in ("lags=5", "warmup=0", "ridge=-1", "holdout=1", "rate=0", f"projections={pca} n_components=7"):
        assert AR.main([f"rollouts={rollouts}", "k=3", f"out={out}", *bad.split()], backend=backend) == 2, bad
