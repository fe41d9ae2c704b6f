"""The float64 reference of the representation-comparison kernels (csrc/compare_core.h), the case generators and the checkers that
tests/test_compare_cpu.py (the host emulation) and tests/test_gpu_compare.py (the C-ABI) share.  A `backend` is analysis.pca.HipBackend or
tests/hostemu/compare_emu.B.

How every bound is derived.  Each checked quantity is computed twice here on the test's own input: in float64, and by a float32 restatement in
numpy of the algorithm the kernels perform (the float32 column mean, the float32 centring, one fused multiply-add per term in the kernels' order,
float64 wherever the kernels sum in float64; an FMA is restated as the float64 sum of the accumulator and the exact float64 product, rounded to
float32).  The kernel and the emulation are held to TWICE the distance between the two, the margin that allows for another summation order;
where the two agree to the bit the bound is equality.  The quantities that are exact by construction (pair counts, label mismatches, duplicate
rows, a representation against itself) are compared with ==.  What float64 itself adds is stated where it is used:
  a ratio r = c / sqrt(v v) of three equal float64 numbers is 1 within 4 x 2^-53 (the product, the root and the quotient round once each);
  the decomposition stops when every pair of columns has |cos| <= 2^-40, so by Gershgorin's circles an eigenvalue of G^T G lies within
  (r - 1) 2^-40 sigma_max^2 of its diagonal: a singular value, the vectors' orthogonality and the rebuilt matrix are good to r 2^-40 sigma_max
  (plus 1e-13 sigma_max for forming the test matrix in float64).
The CCA's float32 restatement takes the components of each side from a float32 Jacobi iteration written here (jacobi32: the PCA's algorithm, not
its rotation for rotation), and everything behind them as the kernels have it: its distance to float64 is of the kernels' size but not of their
sign, so one bound serves all the canonical correlations of a case: twice the largest gap among the first four.

Measured (check_cca): with every component kept (2000 x 20 x 30) the error is 1.00 of the gap.  At 1500 x 200 x 129 with var_keep = 0.99, 128 of
200 and 98 of 129 components kept, the first three correlations are off by 0.8e-7, 0.7e-7 and 1.6e-7 against a largest gap of 1.35e-7: 1.2 times
the gap.  Without the kernels' Ritz step around the cut (ritz_window restates it) the second was off by 3.7e-7, 2.7 times the gap: the span the
float32 PCA keeps lies 2.5e-3 rad from the float64 one, the eigenvalues at the cut being 3 % apart; DESIGN.md "Representation comparison"."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

f64 = np.float64
U53 = 2.0 ** -53
SQ, EU, CO, LA = 0, 1, 2, 3
CKA_CASES = ((3, 1, 1), (257, 5, 130), (1000, 129, 64), (513, 1024, 1))
# (n, d1, metric_x, d2, metric_y): n over tile edges and the diagonal tile, d over a stage and the limit, every ordered metric pair once
RDM_CASES = ((3, 1, SQ, 1, SQ), (64, 2, SQ, 60, EU), (65, 60, SQ, 2, CO), (129, 1024, SQ, 1, LA),
             (1000, 60, EU, 2, SQ), (3, 2, EU, 2, EU), (64, 1024, EU, 60, CO), (65, 1, EU, 1, LA),
             (129, 60, CO, 1024, SQ), (1000, 2, CO, 60, EU), (3, 60, CO, 60, CO), (64, 60, CO, 1, LA),
             (65, 1, LA, 1024, SQ), (129, 1, LA, 2, EU), (1000, 1, LA, 60, CO), (3, 1, LA, 1, LA))
RDM_OFFSET_CASES = (RDM_CASES[2], RDM_CASES[4])
COUNT_N = (3, 64, 65, 129, 1000)
CCA_CASES = ((2000, 20, 30, 1.0), (1500, 200, 129, 0.99))      # (n, d1, d2, var_keep): the second is capped at 128 components from 200
SVD_SHAPES = ((1, 1), (1, 128), (128, 128), (37, 5))


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def within(got, r64, r32, what, floor=0.0):
    """|got - r64| <= 2 |r32 - r64| (+ floor, where the text above derives one), elementwise; prints the worst ratio."""
    got, r64, r32 = (np.asarray(v, f64) for v in (got, r64, r32))
    gap = np.abs(r32 - r64)
    err = np.abs(got - r64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > floor, err / gap, 0.0)
    print(f"[compare {what}] error / float32-float64 gap: worst {float(np.max(ratio)):.3g} (the bound is 2); gap {float(np.max(gap)):.3g}")
    assert (err <= 2.0 * gap + floor).all(), (what, got, r64, r32)


# ---------------------------------------------------------------------------------------------------------------- CKA
def mean32(x):
    return (np.asarray(x, f64).sum(0) / x.shape[0]).astype(np.float32)


def moment_chain(a, b):
    """(a^T b) / (n - 1) as the kernels form it from centred float32 rows: one FMA chain per element inside a chunk of 256 rows, float64 across."""
    n = a.shape[0]
    a64, b64 = a.astype(f64), b.astype(f64)
    total = np.zeros((a.shape[1], b.shape[1]), f64)
    for c0 in range(0, n, 256):
        acc = np.zeros_like(total)
        for r in range(c0, min(c0 + 256, n)):
            acc += np.multiply.outer(a64[r], b64[r])
            acc = acc.astype(np.float32).astype(f64)
        total += acc
    return total / (n - 1)


def cka_parts(x, y, single):
    """-> [||Cxy||^2, ||Cxx||^2, ||Cyy||^2, cka] in float64 (single=False) or by the float32 restatement."""
    if single:
        xc, yc = x - mean32(x), y - mean32(y)
        same = x is y
        cxx = moment_chain(xc, xc)
        cxy, cyy = (cxx, cxx) if same else (moment_chain(xc, yc), moment_chain(yc, yc))
    else:
        x64, y64 = np.asarray(x, f64), np.asarray(y, f64)
        xc, yc = x64 - x64.mean(0), y64 - y64.mean(0)
        cxy, cxx, cyy = xc.T @ yc / (x.shape[0] - 1), xc.T @ xc / (x.shape[0] - 1), yc.T @ yc / (x.shape[0] - 1)
    o = [float((c * c).sum()) for c in (cxy, cxx, cyy)]
    return np.array(o + [o[0] / np.sqrt(o[1] * o[2])])


@functools.lru_cache(None)
def cka_data(case, offset):
    n, d1, d2 = case
    r = np.random.default_rng(977 + n + d1)
    z = r.standard_normal((n, 3))
    x = f32(z @ r.standard_normal((3, d1)) + r.standard_normal((n, d1)) + offset)
    y = f32(z @ r.standard_normal((3, d2)) + 0.7 * r.standard_normal((n, d2)) + offset)
    for a in (x, y):
        a.setflags(write=False)
    return x, y


@functools.lru_cache(None)
def cka_reference(case, offset):
    x, y = cka_data(case, offset)
    return cka_parts(x, y, False), cka_parts(x, y, True)


def cka_got(backend, x, y):
    o = backend.cka_linear(backend.asarray(x), backend.asarray(y))
    assert o.dtype == np.float64 and o.shape == (3,)
    return np.array([*o, o[0] / np.sqrt(o[1] * o[2])])


def check_cka(case, offset, backend, what=""):
    x, y = cka_data(case, offset)
    r64, r32 = cka_reference(case, offset)
    got = cka_got(backend, x, y)
    within(got / r64, r64 / r64, r32 / r64, f"{what} cka {case} offset {offset:g}")
    return got


def check_cka_properties(backend, what=""):
    r = np.random.default_rng(5)
    n, d = 300, 20
    x = f32(r.standard_normal((n, 4)) @ r.standard_normal((4, d)) + r.standard_normal((n, d)))
    q, _ = np.linalg.qr(r.standard_normal((d, d)))
    same = cka_got(backend, x, x)      # a representation against itself: the three norms are one number
    assert bits(same[0]) == bits(same[1]) == bits(same[2]) and abs(same[3] - 1.0) <= 4 * U53
    for name, y in (("x Q", f32(x @ q)), ("3 x", f32(3.0 * x))):      # rotations and isotropic scalings leave it at 1
        r64, r32 = cka_parts(x, y, False), cka_parts(x, y, True)
        got = cka_got(backend, x, y)
        within(got / r64, r64 / r64, r32 / r64, f"{what} cka(x, {name})")
        assert abs(got[3] - 1.0) <= 2 * abs(r32[3] - r64[3]) + abs(r64[3] - 1.0)
    y = f32(r.standard_normal((n, 12)))      # independent Gaussians: the reference's own value (about d / n), not 0
    r64, r32 = cka_parts(x, y, False), cka_parts(x, y, True)
    got, back = cka_got(backend, x, y), cka_got(backend, y, x)
    assert 0.0 < r64[3] < 0.5
    within(got / r64, r64 / r64, r32 / r64, f"{what} cka of independent Gaussians")
    assert bits(got[1]) == bits(back[2]) and bits(got[2]) == bits(back[1])      # symmetry: the sides' own norms swap to the bit
    assert abs(got[0] - back[0]) <= 4 * abs(r32[0] - r64[0]) and abs(got[3] - back[3]) <= 4 * abs(r32[3] - r64[3])


# ---------------------------------------------------------------------------------------------------------------- RDM correlation
def staged(x, metric, single):
    """-> (the rows as a pair's chain sees them, ok [n]) in float64, or by the float32 restatement."""
    if metric == LA:
        return (f32(x) if single else np.asarray(x, f64)), np.ones(x.shape[0], bool)
    if single:
        xc = x - mean32(x)
        if metric != CO:
            return xc, np.ones(x.shape[0], bool)
        sh = (xc.astype(f64).sum(1) / x.shape[1]).astype(np.float32)
        v = xc - sh[:, None]
        q = (v.astype(f64) ** 2).sum(1)
        ok = q > 0
        sc = np.where(ok, 1.0 / np.sqrt(np.where(ok, q, 1.0)), 0.0).astype(np.float32)
        return v * sc[:, None], ok
    x64 = np.asarray(x, f64)
    xc = x64 - x64.mean(0)
    if metric != CO:
        return xc, np.ones(x.shape[0], bool)
    v = xc - xc.mean(1, keepdims=True)
    q = (v * v).sum(1)
    ok = q > 0
    return v / np.sqrt(np.where(ok, q, 1.0))[:, None] * ok[:, None], ok


def dissimilarity(x, metric, single):
    """-> D [n, n] float64: every pair's dissimilarity, from float64 rows or from the kernels' float32 chain over the features in order."""
    a, ok = staged(x, metric, single)
    n, d = a.shape
    s = np.zeros((n, n), np.float32 if single else f64)
    for f in range(d):
        col = a[:, f]
        df = col[:, None] - col[None, :]
        s = (s.astype(f64) + df.astype(f64) ** 2).astype(np.float32) if single else s + df * df
    s = s.astype(f64)
    if metric == SQ:
        return s
    if metric == EU:
        return np.sqrt(s)
    if metric == CO:
        return np.where(ok[:, None] & ok[None, :], 0.5 * s, 1.0)
    return (s != 0).astype(f64)


def rdm_parts(x, mx, y, my, single):
    """-> [sum Dx, sum Dy, sum Dx^2, sum Dy^2, sum Dx Dy] over the pairs i < j."""
    iu = np.triu_indices(x.shape[0], 1)
    dx, dy = dissimilarity(x, mx, single)[iu], dissimilarity(y, my, single)[iu]
    return np.array([dx.sum(), dy.sum(), (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum()])


def pearson(sums, n):
    sx, sy, sxx, syy, sxy = (float(v) for v in sums)
    pairs = n * (n - 1) / 2.0
    vx, vy = sxx - sx * sx / pairs, syy - sy * sy / pairs
    return (sxy - sx * sy / pairs) / np.sqrt(vx * vy) if vx > 0 and vy > 0 else np.nan


def quantised(r, shape, scale=1.0):
    """Gaussian values on the grid of 2^-10, below 8 in magnitude: sums of them, and the same values moved by 1e3, are exact in float32."""
    return f32(np.clip(np.round(scale * r.standard_normal(shape) * 1024) / 1024, -7.5, 7.5))


@functools.lru_cache(None)
def rdm_data(case, offset=0.0):
    n, d1, mx, d2, my = case
    r = np.random.default_rng(31 + n + d1 + 7 * mx + d2)
    z = r.standard_normal((n, 4))
    lab = f32(np.argmax(z, 1))[:, None]
    x = lab if mx == LA else f32(quantised(r, (n, d1), 0.6) + f32(np.round(z @ r.standard_normal((4, d1)) * 256) / 256) + np.float32(offset))
    y = lab if my == LA else f32(quantised(r, (n, d2), 0.6) + f32(np.round(z @ r.standard_normal((4, d2)) * 256) / 256) + np.float32(offset))
    for a in (x, y):
        a.setflags(write=False)
    return x, y


@functools.lru_cache(None)
def rdm_reference(case, offset=0.0):
    x, y = rdm_data(case, offset)
    _, _, mx, _, my = case
    return rdm_parts(x, mx, y, my, False), rdm_parts(x, mx, y, my, True)


def rdm_got(backend, x, mx, y, my):
    s = backend.rdm_corr(backend.asarray(x), mx, backend.asarray(y), my)
    assert s.dtype == np.float64 and s.shape == (5,)
    return s


def check_rdm(case, backend, what="", offset=0.0):
    n, _, mx, _, my = case
    x, y = rdm_data(case, offset)
    r64, r32 = rdm_reference(case, offset)
    got = rdm_got(backend, x, mx, y, my)
    scale = np.where(r64 != 0, r64, 1.0)
    within(got / scale, r64 / scale, r32 / scale, f"{what} rdm sums {case} offset {offset:g}")
    if np.isfinite(pearson(r64, n)):
        within(pearson(got, n), pearson(r64, n), pearson(r32, n), f"{what} rdm correlation {case} offset {offset:g}")
    return got


def check_rdm_offset(case, backend, what=""):
    """The same geometry 1e3 away from the origin: the values are on a grid where the move is exact, so the float64 answers agree and the kernel's
    two answers differ by no more than their two bounds."""
    n = case[0]
    plain, moved = check_rdm(case, backend, what), check_rdm(case, backend, what, 1e3)
    (p64, p32), (m64, m32) = rdm_reference(case), rdm_reference(case, 1e3)
    slack = 2 * np.abs(p32 - p64) + 2 * np.abs(m32 - m64) + np.abs(p64 - m64)
    assert (np.abs(plain - moved) <= slack).all(), (plain, moved, slack)
    rs = 2 * abs(pearson(p32, n) - pearson(p64, n)) + 2 * abs(pearson(m32, n) - pearson(m64, n)) + abs(pearson(p64, n) - pearson(m64, n))
    assert abs(pearson(plain, n) - pearson(moved, n)) <= rs


def check_rdm_special(backend, what=""):
    r = np.random.default_rng(8)
    # rows without variance across the features under the correlation distance: the values are on a grid and every row has its negation, so the
    # column means are exactly 0 and rows 0, 20 and 40 (constant, its negation, zeros) have a centred norm of exactly 0: distance 1 to every row
    a = quantised(r, (20, 8))
    a[0] = 0.5
    x = f32(np.concatenate([a, -a, np.zeros((1, 8), np.float32)]))
    y = quantised(r, (41, 5))
    d64 = dissimilarity(x, CO, False)
    assert (d64[[0, 20, 40]][:, 1:20] == 1.0).all() and d64[0, 20] == 1.0 and d64[0, 40] == 1.0
    r64, r32 = rdm_parts(x, CO, y, SQ, False), rdm_parts(x, CO, y, SQ, True)
    within(rdm_got(backend, x, CO, y, SQ) / r64, r64 / r64, r32 / r64, f"{what} rdm with rows of no variance")
    # duplicate rows are at distance exactly 0: with the labels i mod 10 on the other side, sum Dx Dy leaves out exactly the duplicate pairs, so it
    # equals sum Dx to the bit if and only if every duplicate pair has Dx = 0
    half = quantised(r, (10, 12)) + np.float32(3)
    dup = f32(np.concatenate([half, half]))
    lab = f32(np.arange(20) % 10)[:, None]
    for m in (SQ, EU, CO):
        s = rdm_got(backend, dup, m, lab, LA)
        assert bits(s[4]) == bits(s[0]) and s[1] == 20 * 19 / 2 - 10 and s[0] > 0, (m, s)
    # labels, counted by hand: 0 0 1 2 2 2 has 15 pairs of which (0, 1), (3, 4), (3, 5), (4, 5) agree: 11 mismatches
    six = f32([0, 0, 1, 2, 2, 2])[:, None]
    np.testing.assert_array_equal(rdm_got(backend, six, LA, six, LA), np.full(5, 11.0))
    # a representation against itself: the two matrices are one, and the correlation is 1 within the rounding of its own formula
    for m in (SQ, EU, CO):
        s = rdm_got(backend, y, m, y, m)
        assert bits(s[0]) == bits(s[1]) and bits(s[2]) == bits(s[3]) == bits(s[4]) and abs(pearson(s, 41) - 1.0) <= 4 * U53, (m, s)


def check_rdm_count(n, backend):
    """All labels distinct: every dissimilarity is 1 and every sum the number of pairs, exactly."""
    lab = f32(np.arange(n))[:, None]
    np.testing.assert_array_equal(rdm_got(backend, lab, LA, lab, LA), np.full(5, n * (n - 1) / 2.0))


# ---------------------------------------------------------------------------------------------------------------- CCA
def keep(var, var_keep, max_rank):
    var = np.asarray(var, f64)
    k, cum = 0, 0.0
    while k < len(var) and k < max_rank:
        if k > 0 and var[k] <= 2.0 ** -20 * var[0]:
            break
        cum += var[k]
        k += 1
        if cum >= var_keep * var.sum():
            break
    return k


def jacobi32(c):
    """The eigen-decomposition of a symmetric float32 matrix by parallel-ordered cyclic Jacobi in float32, to off(A) <= 2^-24 ||A||_F: what the PCA's
    kernels do, restated (the pairs of a round of the round-robin tournament are disjoint and are turned together).
    -> (eigenvalues descending, eigenvectors as columns) float32."""
    a = np.array(c, np.float32)
    d = a.shape[0]
    m = (d + 1) & ~1
    v = np.eye(d, dtype=np.float32)
    one = np.float32(1)
    for _ in range(30):
        off = np.sqrt(max(float((a.astype(f64) ** 2).sum() - (np.diag(a).astype(f64) ** 2).sum()), 0.0))
        if off <= 2.0 ** -24 * np.sqrt(float((a.astype(f64) ** 2).sum())):
            break
        for r in range(m - 1):
            k = np.arange(1, m // 2)
            p = np.concatenate([[m - 1], (r + k) % (m - 1)])
            q = np.concatenate([[r], (r - k) % (m - 1)])
            p, q = np.minimum(p, q), np.maximum(p, q)
            live = q < d
            p, q = p[live], q[live]
            apq = a[p, q]
            live = apq != 0
            p, q, apq = p[live], q[live], apq[live]
            if not len(p):
                continue
            with np.errstate(over="ignore"):      # (an entry far below the diagonal: theta overflows to inf and the turn is 0)
                theta = (a[q, q] - a[p, p]) / (np.float32(2) * apq)
                t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
            cs = one / np.sqrt(t * t + one)
            sn = t * cs
            rp, rq = a[p, :].copy(), a[q, :].copy()
            a[p, :], a[q, :] = cs[:, None] * rp - sn[:, None] * rq, sn[:, None] * rp + cs[:, None] * rq
            for mat in (a, v):
                cp, cq = mat[:, p].copy(), mat[:, q].copy()
                mat[:, p], mat[:, q] = cs * cp - sn * cq, sn * cp + cs * cq
    lam = np.diag(a).copy()
    order = np.argsort(-lam, kind="stable")
    return lam[order], v[:, order]


def ritz_window(e, c, k):
    """The kernels' sharpening of the cut: within the window of at most 128 components around it (64 to each side where there is room), the
    Ritz vectors of c in descending order replace the components, and the first k rows are kept.  e: every component as a row."""
    d = e.shape[0]
    if k >= d:
        return e[:k]
    lo = max(0, k - 64)
    hi = min(d, lo + 128)
    lo = max(0, hi - 128)
    sig, q = np.linalg.eigh(e[lo:hi] @ c @ e[lo:hi].T)
    return np.concatenate([e[:lo], (q[:, ::-1].T @ e[lo:hi])[:k - lo]])


def cca_parts(x, y, var_keep, max_rank, single):
    """-> (rho, kx, ky): PCA both sides, keep, whiten the kept span against the covariance, the singular values of the whitened cross matrix;
    float64, or the float32 restatement: float32 centring, the three moments as the kernels chain them, the eigen-decomposition that picks the
    components in float32, and everything behind it in float64 as the kernels have it."""
    n = x.shape[0]
    if single:
        xc, yc = x - mean32(x), y - mean32(y)
        cxx, cyy, cxy = moment_chain(xc, xc), moment_chain(yc, yc), moment_chain(xc, yc)
    else:
        x64, y64 = np.asarray(x, f64), np.asarray(y, f64)
        xc, yc = x64 - x64.mean(0), y64 - y64.mean(0)
        cxx, cyy, cxy = xc.T @ xc / (n - 1), yc.T @ yc / (n - 1), xc.T @ yc / (n - 1)
    white = []
    for c in (cxx, cyy):
        if single:
            lam, vec = jacobi32(c.astype(np.float32))
        else:
            lam, vec = np.linalg.eigh(c)
            lam, vec = lam[::-1], vec[:, ::-1]
        lam, vec = np.maximum(lam, 0).astype(f64), vec.astype(f64)
        k = keep(lam, var_keep, max_rank)
        e = ritz_window(vec.T, c, k) if single else vec[:, :k].T
        sig, q = np.linalg.eigh(e @ c @ e.T)
        white.append((q / np.sqrt(sig)).T @ e)
    rho = np.linalg.svd(white[0] @ cxy @ white[1].T, compute_uv=False)
    return (rho.astype(np.float32).astype(f64) if single else rho), white[0].shape[0], white[1].shape[0]


@functools.lru_cache(None)
def cca_data(case):
    """x = [s, e1] A, y = [s, e2] B with s of 3 shared dimensions."""
    n, d1, d2, _ = case
    r = np.random.default_rng(64 + d1)
    s = r.standard_normal((n, 3))
    x = f32(np.concatenate([s, r.standard_normal((n, d1 - 3))], 1) @ r.standard_normal((d1, d1)) / np.sqrt(d1))
    y = f32(np.concatenate([s, r.standard_normal((n, d2 - 3))], 1) @ r.standard_normal((d2, d2)) / np.sqrt(d2))
    for a in (x, y):
        a.setflags(write=False)
    return x, y


@functools.lru_cache(None)
def cca_reference(case):
    x, y = cca_data(case)
    return cca_parts(x, y, case[3], 128, False), cca_parts(x, y, case[3], 128, True)


def cca_got(backend, x, y, var_keep=1.0, max_rank=128):
    rho, a, b, info = backend.cca(backend.asarray(x), backend.asarray(y), var_keep, max_rank)
    r = min(info.kx, info.ky)
    assert rho.dtype == np.float32 and rho.shape == (r,) and a.shape == (r, x.shape[1]) and b.shape == (r, y.shape[1]) and info.converged == 1
    assert (np.diff(rho.astype(f64)) <= 0).all(), "rho is not descending"
    return rho.astype(f64), a, b, info


def check_cca(case, backend, what=""):
    n, d1, d2, var_keep = case
    x, y = cca_data(case)
    (r64, kx64, ky64), (r32, kx32, ky32) = cca_reference(case)
    rho, a, b, info = cca_got(backend, x, y, var_keep)
    assert (info.kx, info.ky) == (kx64, ky64) == (kx32, ky32) and (d1 != 200 or info.kx == 128)
    bound = 2 * np.abs(r32[:4] - r64[:4]).max()
    err = np.abs(rho[:3] - r64[:3])
    print(f"[compare {what}] cca {case}: kept {info.kx} x {info.ky}, rho {rho[:4]}, error / gap {err.max() / (bound / 2):.3g} (the bound is 2), "
          f"{info.sweeps} sweeps")
    assert (err <= bound).all() and rho[3] <= r64[3] + bound
    # the directions: unit variance of the projections, and the correlations they give are rho (float64 on the float32 directions)
    xc, yc = np.asarray(x, f64) - np.asarray(x, f64).mean(0), np.asarray(y, f64) - np.asarray(y, f64).mean(0)
    pa, pb = xc @ a.astype(f64).T, yc @ b.astype(f64).T
    tol = 64 * 2.0 ** -24 * max(d1, d2) ** 0.5 + bound      # (the float32 PCA behind the whitening; the directions round once)
    assert np.abs(pa.var(0, ddof=1)[:3] - 1).max() <= tol and np.abs(pb.var(0, ddof=1)[:3] - 1).max() <= tol
    corr = np.array([np.corrcoef(pa[:, i], pb[:, i])[0, 1] for i in range(3)])
    assert np.abs(corr - rho[:3]).max() <= tol
    return rho


def check_cca_properties(backend, what=""):
    case = CCA_CASES[0]
    x, y = cca_data(case)
    (r64, *_), (r32, *_) = cca_reference(case)
    rho = cca_got(backend, x, y)[0]
    # an invertible linear map of a side changes no correlation
    t = np.random.default_rng(3).standard_normal((20, 20)) / np.sqrt(20) + 2 * np.eye(20)
    xt = f32(np.asarray(x, f64) @ t)
    t64, t32 = cca_parts(xt, y, 1.0, 128, False)[0], cca_parts(xt, y, 1.0, 128, True)[0]
    mapped = cca_got(backend, xt, y)[0]
    slack = 2 * np.abs(r32 - r64).max() + 2 * np.abs(t32 - t64).max() + np.abs(t64 - r64).max()
    print(f"[compare {what}] cca under a linear map: rho moves by {np.abs(mapped - rho).max():.3g} (allowed {slack:.3g})")
    assert np.abs(mapped - rho).max() <= slack
    # a representation against itself: all ones
    s64, s32 = cca_parts(x, x, 1.0, 128, False)[0], cca_parts(x, x, 1.0, 128, True)[0]
    ones = cca_got(backend, x, x)[0]
    assert ones.shape == (20,) and np.abs(ones - 1).max() <= 2 * np.abs(s32 - s64).max() + np.abs(s64 - 1).max() + 2.0 ** -24      # (rho rounds once)
    # var_keep cuts at one component: a side with one dominant direction
    r = np.random.default_rng(4)
    big = f32(r.standard_normal((500, 6)) * np.array([10, 1, 1, 1, 1, 1.0]))
    info = cca_got(backend, big, f32(big[:, :2] + r.standard_normal((500, 2))), 0.5)[3]
    assert info.kx == 1
    # max_rank caps a side
    assert cca_got(backend, x, y, 1.0, 5)[3].kx == 5
    # a rank-deficient side (every column twice): the null directions are dropped, nothing blows up
    xx = f32(np.concatenate([x[:, :10], x[:, :10]], 1))
    d64, d32 = cca_parts(xx, y, 1.0, 128, False), cca_parts(xx, y, 1.0, 128, True)
    rho_d, _, _, info = cca_got(backend, xx, y)
    assert info.kx == d64[1] == d32[1] == 10 and np.isfinite(rho_d).all()
    assert np.abs(rho_d[:3] - d64[0][:3]).max() <= 2 * np.abs(d32[0][:4] - d64[0][:4]).max() and rho_d.max() <= 1 + 2.0 ** -20


@functools.lru_cache(None)
def svd_case(shape):
    rows, cols = shape
    r, rng = min(rows, cols), np.random.default_rng(rows * 131 + cols)
    s = np.sort(rng.uniform(0.1, 3.0, r))[::-1].copy()
    if r >= 5:
        s[2] = s[1]      # a repeated value
        s[-1] = 0.0      # and a zero one
    u, _ = np.linalg.qr(rng.standard_normal((rows, rows)))
    v, _ = np.linalg.qr(rng.standard_normal((cols, cols)))
    return (u[:, :r] * s) @ v[:, :r].T, s


def check_svd(shape, backend, what=""):
    m, s = svd_case(shape)
    sigma, u, v, sweeps = backend.compare_svd(m)
    r = len(s)
    bound = (r * 2.0 ** -40 + 1e-13) * s[0]
    print(f"[compare {what}] svd {shape}: {sweeps} sweeps, sigma error {np.abs(sigma - s).max():.3g}, rebuilt within {np.abs((u.T * sigma) @ v - m).max():.3g} "
          f"(bound {bound:.3g})")
    assert sigma.shape == (r,) and u.shape == (r, shape[0]) and v.shape == (r, shape[1]) and 1 <= sweeps < 60
    assert (np.diff(sigma) <= 0).all() and np.abs(sigma - s).max() <= bound
    assert np.abs((u.T * sigma) @ v - m).max() <= bound
    live = sigma > bound
    for w in (u, v):
        g = w[live] @ w[live].T
        assert np.abs(g - np.eye(int(live.sum()))).max() <= r * 2.0 ** -40 + 1e-13


# ---------------------------------------------------------------------------------------------------------------- bits
def check_repeat_and_strides(backend, strided, what=""):
    """Two calls give the same bits, and rows with a stride (column slices of wider buffers) the bits of contiguous ones."""
    x, y = cka_data(CKA_CASES[1], 0.0)
    xs, ys = strided(x), strided(y)
    for call in (lambda p, q: backend.cka_linear(backend.asarray(p), backend.asarray(q)),
                 lambda p, q: backend.rdm_corr(backend.asarray(p), CO, backend.asarray(q), EU),
                 lambda p, q: np.concatenate([v.ravel() for v in backend.cca(backend.asarray(p), backend.asarray(q), 0.99, 128)[:3]])):
        first = call(x, y)
        np.testing.assert_array_equal(bits(first), bits(call(x, y)))
        np.testing.assert_array_equal(bits(first), bits(call(xs, ys)))


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, alloc, ptr, untouched, what=""):
    """Every refusal through the C-ABI: -22 with a message that names the value, nothing launched, sentinel-filled outputs untouched.
    `alloc(shape, dtype, fill)` -> an array of the library's memory, `ptr(a)` its address, `untouched(a, fill)` whether it still holds `fill`."""
    from track_mjx_amd import hip
    n, d1, d2 = 40, 7, 5
    x, y = alloc((n, d1), np.float32, 0.0), alloc((n, d2), np.float32, 0.0)
    outs = {"out": alloc((3,), np.float64, -5.0), "sums": alloc((5,), np.float64, -5.0), "rho": alloc((128,), np.float32, -5.0),
            "a": alloc((128, d1), np.float32, -5.0), "b": alloc((128, d2), np.float32, -5.0), "sigma": alloc((8,), np.float64, -5.0),
            "u": alloc((8, 8), np.float64, -5.0), "v": alloc((8, 8), np.float64, -5.0)}
    o = {key: ptr(v) for key, v in outs.items()}
    floats = C.c_int64(0)
    assert lib.tmjx_compare_workspace(n, d1, d2, C.byref(floats)) == 0 and floats.value > 0
    big = C.c_int64(0)
    assert lib.tmjx_compare_workspace(210000, 1024, 1024, C.byref(big)) == 0 and big.value < 32768 * 32768 // 4      # neither n x n matrix has room
    ws = alloc((int(floats.value) + 4,), np.float32, 0.0)
    m8 = alloc((8, 8), np.float64, 0.0)
    X, Y, WS, M8 = ptr(x), ptr(y), ptr(ws), ptr(m8)
    err, nan = lib.tmjx_last_error, float("nan")
    info, sweeps = C.byref(hip.CcaInfo()), C.byref(C.c_int32(0))

    def cka(n=n, d1=d1, ldx=None, d2=d2, ldy=None, x=X, y=Y, out=o["out"], ws=WS):
        return lib.tmjx_cka_linear(x, n, d1, d1 if ldx is None else ldx, y, d2, d2 if ldy is None else ldy, out, ws, None)

    def rdm(n=n, d1=d1, ldx=None, mx=0, d2=d2, ldy=None, my=0, x=X, y=Y, sums=o["sums"], ws=WS):
        return lib.tmjx_rdm_corr(x, n, d1, d1 if ldx is None else ldx, mx, y, d2, d2 if ldy is None else ldy, my, sums, ws, None)

    def cca(n=n, d1=d1, ldx=None, d2=d2, ldy=None, var_keep=0.99, max_rank=128, x=X, y=Y, rho=o["rho"], a=o["a"], b=o["b"], info=info, ws=WS):
        return lib.tmjx_cca(x, n, d1, d1 if ldx is None else ldx, y, d2, d2 if ldy is None else ldy, var_keep, max_rank, rho, a, b, info, ws, None)

    def svd(rows=8, cols=8, lda=8, m=M8, sigma=o["sigma"], u=o["u"], v=o["v"], sweeps=sweeps, ws=WS):
        return lib.tmjx_compare_svd(m, rows, cols, lda, sigma, u, v, sweeps, ws, None)
    cases = [
        (lambda: lib.tmjx_compare_workspace(2, d1, d2, C.byref(floats)), b"n >= 3"), (lambda: lib.tmjx_compare_workspace(n, 0, d2, C.byref(floats)), b"d1 must be >= 1"),
        (lambda: lib.tmjx_compare_workspace(n, d1, 1025, C.byref(floats)), b"1025"), (lambda: lib.tmjx_compare_workspace(n, d1, d2, None), b"null"),
        (lambda: cka(n=2), b"n >= 3"), (lambda: cka(d1=0), b"d1 must be >= 1"), (lambda: cka(d1=1025, ldx=1025), b"1025"), (lambda: cka(d2=0), b"d2 must be >= 1"),
        (lambda: cka(d2=1025, ldy=1025), b"1025"), (lambda: cka(ldx=d1 - 1), b"ldx"), (lambda: cka(ldy=d2 - 1), b"ldy"), (lambda: cka(x=None), b"null"),
        (lambda: cka(y=None), b"null"), (lambda: cka(out=None), b"null"), (lambda: cka(ws=None), b"null"), (lambda: cka(ws=WS + 4), b"16-byte"),
        (lambda: cka(out=o["out"] + 4), b"8-byte"), (lambda: cka(x=X + 2), b"4-byte"),
        (lambda: rdm(n=2), b"n >= 3"), (lambda: rdm(n=32769), b"32769"), (lambda: rdm(d1=0), b"d1 must be >= 1"), (lambda: rdm(d2=1025, ldy=1025), b"1025"),
        (lambda: rdm(ldx=d1 - 1), b"ldx"), (lambda: rdm(ldy=d2 - 1), b"ldy"), (lambda: rdm(mx=-1), b"metric_x = -1"), (lambda: rdm(my=4), b"metric_y = 4"),
        (lambda: rdm(mx=3), b"takes one column"), (lambda: rdm(my=3), b"takes one column"), (lambda: rdm(d1=1, mx=2), b"needs d1 >= 2"),
        (lambda: rdm(d2=1, my=2), b"needs d2 >= 2"), (lambda: rdm(x=None), b"null"), (lambda: rdm(sums=None), b"null"), (lambda: rdm(ws=None), b"null"),
        (lambda: rdm(ws=WS + 4), b"16-byte"), (lambda: rdm(sums=o["sums"] + 4), b"8-byte"),
        (lambda: cca(n=2), b"n >= 3"), (lambda: cca(d1=1025, ldx=1025), b"1025"), (lambda: cca(d2=0), b"d2 must be >= 1"), (lambda: cca(ldx=d1 - 1), b"ldx"),
        (lambda: cca(var_keep=0.0), b"var_keep"), (lambda: cca(var_keep=1.01), b"var_keep"), (lambda: cca(var_keep=nan), b"var_keep"),
        (lambda: cca(max_rank=0), b"max_rank = 0"), (lambda: cca(max_rank=129), b"max_rank = 129"), (lambda: cca(y=None), b"null"), (lambda: cca(rho=None), b"null"),
        (lambda: cca(a=None), b"null"), (lambda: cca(b=None), b"null"), (lambda: cca(info=None), b"null"), (lambda: cca(ws=None), b"null"),
        (lambda: cca(ws=WS + 4), b"16-byte"), (lambda: cca(rho=o["rho"] + 2), b"4-byte"),
        (lambda: svd(rows=0), b"rows, cols >= 1"), (lambda: svd(cols=129, lda=129), b"129"), (lambda: svd(lda=7), b"lda"), (lambda: svd(m=None), b"null"),
        (lambda: svd(sigma=None), b"null"), (lambda: svd(sweeps=None), b"null"), (lambda: svd(ws=WS + 4), b"16-byte"), (lambda: svd(u=o["u"] + 4), b"8-byte"),
    ]
    for call, word in cases:
        assert call() == -22 and word in err(), (word, err())
    for key, v in outs.items():
        assert untouched(v, -5), key
    print(f"[compare {what}] {len(cases)} refusals, nothing written")


# ---------------------------------------------------------------------------------------------------------------- the class and the command line
def clip_files(root):
    """Two directories of synthetic clip_<i>.h5: side a has clips 0, 2, 5, 7; side b lacks clip 5 and its clip 2 is 10 steps shorter.  The
    intention of b is a rotation of a's plus noise; qposes_rollout has one row more than the activations.
    -> (dir a, dir b, {clip: T} of a, {clip: T} of b, a clusters file with labels)."""
    from track_mjx_amd import h5lite
    r = np.random.default_rng(21)
    q, _ = np.linalg.qr(r.standard_normal((6, 6)))
    ta, tb = {0: 90, 2: 70, 5: 80, 7: 60}, {0: 90, 2: 60, 7: 60}
    (root / "a").mkdir(parents=True)
    (root / "b").mkdir(parents=True)
    labels = {}
    for clip, T in ta.items():
        z = r.standard_normal((T, 6))
        layer = np.tanh(z @ r.standard_normal((6, 9)))
        qpos = np.concatenate([np.zeros((T + 1, 7)), np.concatenate([z[:, :3], z[-1:, :3]])], 1)
        labels[f"clip_{clip}"] = (np.arange(T) // 10 % 3).astype(np.int32)
        h5lite.write_tree(str(root / "a" / f"clip_{clip}.h5"), {"activations": {"intention": f32(z), "decoder": {"layer_0": f32(layer)}},
                                                                "ctrl": f32(z[:, :2]), "qposes_rollout": f32(qpos)})
        if clip in tb:
            zb = (z @ q + 0.1 * r.standard_normal((T, 6)))[:tb[clip]]
            h5lite.write_tree(str(root / "b" / f"clip_{clip}.h5"), {"activations": {"intention": f32(zb)}, "ctrl": f32(zb[:, :2])})
    h5lite.write_tree(str(root / "clusters.h5"), {"labels": labels, "feature": "intention"})
    return str(root / "a"), str(root / "b"), ta, tb, str(root / "clusters.h5")


def check_cli(tmp_path, backend, capsys):
    """The command-line round trip: the pairing of clips and rows, the file's fields and shapes, side a against itself, the labels, the file as an
    intervention, the usage errors; and the class on a side without variance."""
    import warnings

    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import compare as CM
    from track_mjx_amd.analysis.intervene import Intervention
    a, b, ta, tb, clusters = clip_files(tmp_path / "clips")
    out = str(tmp_path / "out" / "compare.h5")
    assert CM.main([f"a={a}", f"b={b}", "features_a=intention,decoder/layer_0", "features_b=intention,ctrl", "max_rows=100", "seed=3",
                    "cca=intention:intention", "var_keep=1", f"out={out}"], backend=backend) == 0
    said = capsys.readouterr().out
    assert "[compare] 2 x 2 features over 210 paired rows of 3 clips, 100 rows" in said and "svcca" in said

    def load(path, keys):
        with h5lite.File(path) as h:
            return {k: np.asarray(h[k][()]) for k in keys}, {k: bytes(h[k][()]).decode() for k in ("features_a", "features_b", "rdm_metric")}
    got, text = load(out, ("clips", "rows", "row_index", "cka", "rdm_corr", "rho", "svcca", "directions_a", "directions_b", "kx", "ky", "mean", "components"))
    assert text == {"features_a": "intention,decoder/layer_0", "features_b": "intention,ctrl", "rdm_metric": "correlation"}
    assert list(got["clips"]) == [0, 2, 7] and list(got["rows"]) == [90, 60, 60]      # clip 5 is not in b; clip 2 is shorter there
    assert got["row_index"].shape == (100,) and (np.diff(got["row_index"]) > 0).all() and got["row_index"].max() < 210
    assert got["cka"].shape == (2, 2) and got["rdm_corr"].shape == (2, 2) and np.isfinite(got["cka"]).all() and np.isfinite(got["rdm_corr"]).all()
    assert got["cka"][0, 0] > 0.95 and got["rdm_corr"][0, 0] > 0.0      # b's intention is a rotation of a's: CKA does not see it, correlation distances do
    assert got["cka"].max() <= 1 + 1e-6
    assert (int(got["kx"]), int(got["ky"])) == (6, 6) and got["rho"].shape == (6,) and got["rho"].min() > 0.9 and abs(float(got["svcca"]) - got["rho"].mean()) < 1e-6
    assert got["directions_a"].shape == (6, 6) and got["directions_b"].shape == (6, 6) and got["mean"].shape == (6,) and got["components"].dtype == np.float32
    np.testing.assert_allclose(got["components"].astype(f64) @ got["components"].astype(f64).T, np.eye(6), atol=1e-6)
    first = got["directions_a"][0].astype(f64)
    np.testing.assert_allclose(got["components"][0], first / np.linalg.norm(first), atol=1e-6)
    iv = Intervention.from_pca(out, components="0:3")
    assert iv.target == "intention"
    # side a against itself, with the motif labels as one more feature of side a
    out2 = str(tmp_path / "out" / "self.h5")
    assert CM.main([f"a={a}", "features_a=intention,decoder/layer_0", f"labels={clusters}", "metric=euclidean", f"out={out2}"], backend=backend) == 0
    capsys.readouterr()
    got2, text2 = load(out2, ("clips", "rows", "cka", "rdm_corr", "row_index"))
    assert text2["features_a"] == "intention,decoder/layer_0,labels" and text2["features_b"] == "intention,decoder/layer_0" and text2["rdm_metric"] == "euclidean"
    assert list(got2["clips"]) == [0, 2, 5, 7] and list(got2["rows"]) == [90, 70, 80, 60] and got2["row_index"].shape == (300,)
    assert got2["cka"].shape == (3, 2) and abs(got2["cka"][0, 0] - 1) < 1e-12 and abs(got2["cka"][0, 1] - got2["cka"][1, 0]) < 1e-6
    assert np.isnan(got2["cka"][2]).all()      # CKA of labels is not computed
    assert abs(got2["rdm_corr"][1, 1] - 1) < 1e-12 and np.isfinite(got2["rdm_corr"]).all()
    # a readout target with columns picked: the per-frame series drops its extra row; the last three joints are the first three intentions
    out3 = str(tmp_path / "out" / "kin.h5")
    assert CM.main([f"a={a}", "features_a=qposes_rollout", "cols_a=7:", "features_b=intention", "cols_b=0:3", "metric=sqeuclidean", f"out={out3}"], backend=backend) == 0
    capsys.readouterr()
    got3, _ = load(out3, ("rows", "cka", "rdm_corr"))
    assert list(got3["rows"]) == [90, 70, 80, 60] and got3["cka"].shape == (1, 1) and abs(got3["cka"][0, 0] - 1) < 1e-6 and abs(got3["rdm_corr"][0, 0] - 1) < 1e-6
    # the usage errors
    assert CM.main([f"a={a}"]) == 2 and CM.main([f"a={a}", "features_a=intention", f"out={out}", "bogus=1"]) == 2
    assert CM.main([f"a={a}", "features_a=nothing", f"out={out}"], backend=backend) == 2
    assert CM.main([f"a={a}", "features_a=intention", "max_rows=32769", f"out={out}"], backend=backend) == 2
    assert CM.main([f"a={a}", "features_a=intention", "cca=ctrl:intention", f"out={out}"], backend=backend) == 2
    assert "usage" in capsys.readouterr().err
    # a side without variance: NaN with a warning, not an exception
    cmp_ = CM.Comparison(backend=backend)
    flat, x = np.full((50, 3), 2.0, np.float32), f32(np.random.default_rng(1).standard_normal((50, 4)))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert np.isnan(cmp_.cka(flat, x))
    assert any("without variance" in str(w.message) for w in seen)
    assert abs(cmp_.cka(x, x) - 1) < 1e-12 and abs(cmp_.rdm_corr(x, x) - 1) < 1e-12
