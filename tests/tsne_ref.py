"""The float64 reference of the behaviour-map kernels (csrc/tsne_core.h), the case generators and the checkers that tests/test_embed_cpu.py (the host
emulation) and tests/test_gpu_embed.py (the C-ABI) share.  A `backend` is analysis.pca.HipBackend or tests/hostemu/tsne_emu.B.

Every bound is derived here from the operations the kernels perform (u = 2^-24, the unit round-off of float32):
  kNN        the k-means bound on comparing two d-term float32 FMA chains on data centred at the column mean mu of x:
             tau_i = 2 (d + 4) u (||q_i - mu|| + max_j ||x_j - mu||)^2; a returned distance is within tau_i / 2 of the float64 one.
  affinities a weight w_j = expf(-beta e_j), e_j = d_j - dmin: e_j and the product each round once (a_j u each, a_j = beta e_j), expf is good to 4 u:
             eps_j = (2 a_j + 4) u relative; p_j = w_j / S then carries eps_j + sum_i p_i eps_i + 2 u, plus 2 x 2^-126 absolute where the device
             flushes a subnormal weight.  The entropy H = log S + beta SE / S moves by sum_j p_j |1 + a_j - abar| eps_j (+ 2 u abar for e_j in SE).
  gradient   per pair: dx, dy round once (1 u each), q = fma(dy, dy, fma(dx, dx, 1)) carries 2 u from its inputs and 2 u of its own (4 u), w = 1 / q
             5 u, w w 11 u, (w w) dx 13 u; Z, a sum of positive w, 5 u; the quotient by Z 18 u; the final rounding 1 u: 19 u on a repulsion term,
             (P w) dx 8 u + 1 u on an attraction term.  GRAD_C = 20 covers both; the float64 sums add 1e-12 relative.
  kl         log(P Z / w): Z and w carry 5 u each, the logarithm moves by 10 u absolute: KL_C = 12 u times sum P, plus 1e-12 of the summed |terms|.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

U24 = 2.0 ** -24
GRAD_C, Z_C, KL_C = 20, 5, 12
# (n, m, d, k, self): the smallest legal shape; one row over a tile; a cross search; one feature over a stage and rows over a tile; every limit; k at
# its ceiling; every other row returned
KNN_CASES = ((2, 2, 1, 1, True), (257, 257, 3, 5, True), (1000, 300, 60, 90, False), (4099, 129, 129, 33, False), (2050, 100, 1024, 128, False),
             (130, 130, 7, 128, True), (70, 70, 4, 69, True))
AFFINITY_K = (2, 5, 90, 128)
GRADIENT_N = (2, 3, 257, 1000, 4099)
GRADIENT_SCALES = (1e-4, 1.0, 50.0)
# The model-level data and schedule, chosen on the float64 reference (tsne_numpy) alone.  At the default exaggeration of 12 the exaggerated phase of
# the reference itself oscillates on 400 points at eta = 50: its kl rises by 2 % to 6 % in the iterations behind the switch, by an amount that
# depends on the iteration the switch falls on (6.2 % at 88, 2.1 % at 90, 3.6 % at 100), so "kl does not rise" is no property of the arithmetic
# there.  At exaggeration 4 the reference descends monotonically behind the switch (largest step -0.02 %) and reaches purity 1.0.
# The margin of checks (b) and (c): twice the relative gap between the float64 reference and its float32 numpy restatement from the same P, start
# and schedule.  Measured on this data: float64 kl 0.663112, float32 kl 0.669310, a gap of 0.93 % (the issue's prototype, at 600 rows and 500
# iterations, saw 1.0 %: 0.7787 against 0.7864).  The margin is 2 x MODEL_GAP = 1.86 %.
MODEL_GAP = 0.0093
MODEL = dict(blobs=8, per=50, d=30, sep=6.0, perplexity=15.0, n_iter=350, exaggeration=4.0, exaggeration_iters=90, momentum_early=0.5, momentum_late=0.8,
             min_gain=0.01, held_out=10)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


# ---------------------------------------------------------------------------------------------------------------- kNN
@functools.lru_cache(None)
def knn_data(case):
    """-> (x float32 [n, d], q float32 [m, d] or None for a search of x against itself); read-only."""
    n, m, d, k, self_ = case
    r = np.random.default_rng(4321 + n + d)
    blobs = max(1, min(8, n // 8))
    ctr = 2.0 * r.standard_normal((blobs, d))
    x = f32(ctr[r.integers(0, blobs, n)] + r.standard_normal((n, d))) + np.float32(3)
    q = None if self_ else f32(ctr[r.integers(0, blobs, m)] + r.standard_normal((m, d))) + np.float32(3)
    for a in (x, q):
        if a is not None:
            a.setflags(write=False)
    return x, q


def dist64(x, q):
    """Float64 squared distances [m, n] on data centred at the column mean of x."""
    x64, q64 = np.asarray(x, np.float64), np.asarray(q, np.float64)
    mu = x64.mean(0)
    xc, qc = x64 - mu, q64 - mu
    return (qc * qc).sum(1)[:, None] + (xc * xc).sum(1)[None, :] - 2.0 * (qc @ xc.T)


def knn_tau(x, q):
    x64, q64 = np.asarray(x, np.float64), np.asarray(q, np.float64)
    mu = x64.mean(0)
    xn, qn = np.sqrt(((x64 - mu) ** 2).sum(1)), np.sqrt(((q64 - mu) ** 2).sum(1))
    return 2 * (x.shape[1] + 4) * U24 * (qn + xn.max()) ** 2


def check_sorted(idx, dist2):
    assert (np.diff(dist2.astype(np.float64), axis=1) >= 0).all(), "a list is not ascending in dist2"
    tie = dist2[:, 1:] == dist2[:, :-1]
    assert (idx[:, 1:][tie] > idx[:, :-1][tie]).all(), "a tie is not in index order"


def check_knn_lists(x, q, self_, k, idx, dist2, what=""):
    """The four properties of the issue against the float64 distances."""
    n, d = x.shape
    qq = x if q is None else q
    m = qq.shape[0]
    D = dist64(x, qq)
    if self_:
        D[np.arange(n), np.arange(n)] = np.inf
    tau = knn_tau(x, qq)
    assert idx.dtype == np.int32 and idx.shape == (m, k) and dist2.dtype == np.float32 and dist2.shape == (m, k)
    assert idx.min() >= 0 and idx.max() < n
    assert (np.sort(idx, 1)[:, 1:] != np.sort(idx, 1)[:, :-1]).all(), "a row is returned twice"
    if self_:
        assert (idx != np.arange(n)[:, None]).all(), "a query returned itself"
    dk = np.partition(D, k - 1, axis=1)[:, k - 1]
    mine = np.take_along_axis(D, idx.astype(np.int64), 1)
    excess = float(((mine - dk[:, None]) / np.maximum(tau, 1e-300)[:, None]).max())
    assert (mine <= dk[:, None] + tau[:, None]).all(), "a returned row is farther than the k-th nearest by more than tau"
    sure = D < (dk - tau)[:, None]
    got = np.zeros_like(sure)
    np.put_along_axis(got, idx.astype(np.int64), True, 1)
    missing = int((sure & ~got).sum())
    err = np.abs(dist2.astype(np.float64) - mine)
    worst = float((err / np.maximum(tau / 2, 1e-300)[:, None]).max())
    print(f"[tsne {what}] knn {m} x {n} x {d}, k = {k}{' (self)' if self_ else ''}: worst excess over the k-th {excess:.3g} tau, {missing} sure rows missing, "
          f"dist2 error {worst:.3g} of tau / 2")
    assert missing == 0
    assert (dist2 >= 0).all() and (err <= tau[:, None] / 2).all()
    check_sorted(idx, dist2)


def check_knn(case, backend, what=""):
    n, m, d, k, self_ = case
    x, q = knn_data(case)
    xa = backend.asarray(x)
    idx, dist2 = backend.knn(xa, None if self_ else backend.asarray(q), k, exclude_self=self_)
    check_knn_lists(x, q, self_, k, idx, dist2, what)
    return idx, dist2


def grid_points():
    """A symmetric integer grid: every point with its negation, so the column mean is exactly 0 and every product below 2^24."""
    g = np.array(np.meshgrid(*[np.arange(-3, 4)] * 3), np.float64).reshape(3, -1).T      # 343 points of {-3 .. 3}^3
    r = np.random.default_rng(5)
    return f32(g[r.permutation(len(g))] * 5.0)


def check_knn_exact(backend):
    """On the integer grid the indices and the distances equal float64's exactly, ties in index order."""
    x = grid_points()
    n, k = x.shape[0], 40
    D = dist64(x, x)
    assert np.abs(np.asarray(x, np.float64).mean(0)).max() == 0.0 and (D == np.round(D)).all()
    for self_ in (True, False):
        idx, dist2 = backend.knn(backend.asarray(x), None, k, exclude_self=self_)
        E = D.copy()
        if self_:
            E[np.arange(n), np.arange(n)] = np.inf
        ref = np.stack([np.lexsort((np.arange(n), E[i]))[:k] for i in range(n)])
        np.testing.assert_array_equal(idx, ref)
        np.testing.assert_array_equal(dist2.astype(np.float64), np.take_along_axis(E, ref, 1))


def check_knn_duplicates(backend):
    """Every reference row stands twice: a tie goes to the lowest index, so row j + n0 never comes before (or without) row j."""
    base, _ = knn_data(KNN_CASES[1])
    base = base[:150]
    x = f32(np.concatenate([base, base], 0))
    q, _ = knn_data(KNN_CASES[2])
    q = f32(q[:40, :3])
    n0, k = base.shape[0], 31
    idx, dist2 = backend.knn(backend.asarray(x), backend.asarray(q), k)
    check_knn_lists(x, q, False, k, idx, dist2, "duplicates")
    for row, dd in zip(idx, dist2):
        pos = {int(j): p for p, j in enumerate(row)}
        for j, p in pos.items():
            if j >= n0:
                assert j - n0 in pos and pos[j - n0] == p - 1 and dd[p] == dd[p - 1], "a duplicate came before its lower twin"


def check_knn_self(backend):
    """Self is left out only in a search of x against itself with exclude_self; a copy of x as the queries keeps it, at distance exactly 0."""
    x, _ = knn_data(KNN_CASES[1])
    xa = backend.asarray(x)
    n, k = x.shape[0], 4
    own = np.arange(n)
    i0, d0 = backend.knn(xa, None, k, exclude_self=True)
    assert (i0 != own[:, None]).all()
    i1, d1 = backend.knn(xa, None, k, exclude_self=False)
    assert (i1[:, 0] == own).all() and (d1[:, 0] == 0).all()
    np.testing.assert_array_equal(i1[:, 1:], i0[:, :k - 1])
    np.testing.assert_array_equal(bits(d1[:, 1:]), bits(d0[:, :k - 1]))
    i2, d2 = backend.knn(xa, backend.asarray(np.array(x)), k, exclude_self=True)
    np.testing.assert_array_equal(i2, i1)
    np.testing.assert_array_equal(bits(d2), bits(d1))


def check_knn_repeat_and_strides(backend, strided, what=""):
    """Two calls, and rows with a stride, give the same bits."""
    case = KNN_CASES[2]
    n, m, d, k, _ = case
    x, q = knn_data(case)
    a = backend.knn(backend.asarray(x), backend.asarray(q), k)
    b = backend.knn(backend.asarray(x), backend.asarray(q), k)
    c = backend.knn(backend.asarray(strided(x)), backend.asarray(strided(q)), k)
    for u, v in ((a, b), (a, c)):
        np.testing.assert_array_equal(u[0], v[0])
        np.testing.assert_array_equal(bits(u[1]), bits(v[1]))


# ---------------------------------------------------------------------------------------------------------------- affinities
def perplexity_of(k):
    return 1.5 if k == 2 else k / 3.0


@functools.lru_cache(None)
def affinity_rows(k):
    """-> (dist2 float32 [m, k], kinds): sorted random rows, then the special ones: all equal; several zeros (more than the perplexity: no root);
    two zeros; distances of 1e12; distances of 1e-12."""
    r = np.random.default_rng(77 + k)
    rows = [np.sort(r.gamma(2.0, 1.5, k)) + r.random() for _ in range(24)]
    kinds = ["random"] * len(rows)
    rows.append(np.full(k, 2.5)); kinds.append("equal")
    z = np.sort(r.gamma(2.0, 1.5, k)); z[:min(k - 1, int(perplexity_of(k)) + 2)] = 0.0
    rows.append(z); kinds.append("zeros")
    z = np.sort(r.gamma(2.0, 1.5, k)) + 0.5; z[:min(2, k - 1)] = 0.0
    rows.append(z); kinds.append("two zeros" if k > 3 else "zeros")
    rows.append(np.sort(r.gamma(2.0, 1.5, k)) * 1e12); kinds.append("1e12")
    rows.append(np.sort(r.gamma(2.0, 1.5, k)) * 1e-12); kinds.append("1e-12")
    d = f32(np.stack(rows))
    d.setflags(write=False)
    return d, tuple(kinds)


def entropy64(e, beta):
    """-> (H, p, S, SE) in float64 for the offsets e >= 0."""
    w = np.exp(-beta * e)
    S, SE = w.sum(), (w * e).sum()
    return np.log(S) + beta * SE / S, w / S, S, SE


def root64(e, logu):
    """The float64 beta with H(beta) = logu by bisection, or None when the entropy cannot fall that far (too many zeros)."""
    if np.log((e == 0).sum()) >= logu:
        return None
    lo, hi = 0.0, 1.0
    while entropy64(e, hi)[0] > logu:
        lo, hi = hi, hi * 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if entropy64(e, mid)[0] > logu else (lo, mid)
    return 0.5 * (lo + hi)


def check_affinities(k, backend, what=""):
    d, kinds = affinity_rows(k)
    perp = perplexity_of(k)
    p, beta = backend.tsne_affinities(d, perp)
    m = d.shape[0]
    assert p.dtype == np.float32 and p.shape == (m, k) and beta.dtype == np.float32 and beta.shape == (m,)
    assert np.isfinite(p).all() and np.isfinite(beta).all() and (p >= 0).all() and (beta > 0).all()
    assert (np.abs(p.astype(np.float64).sum(1) - 1.0) <= k * 2.0 ** -23).all()
    worst_p = worst_b = 0.0
    for i, kind in enumerate(kinds):
        e = d[i].astype(np.float64) - float(d[i].min())
        if kind == "equal":
            np.testing.assert_array_equal(p[i], np.full(k, np.float32(1) / np.float32(k)))
            continue
        b = float(beta[i])
        with np.errstate(over="ignore", invalid="ignore"):
            a = np.where(e > 0, b * e, 0.0)
        _, p64, S, SE = entropy64(np.where(e > 0, e, 0.0), b) if np.isfinite(a).all() else (None, (e == 0) / (e == 0).sum(), None, None)
        eps = (2 * np.minimum(a, 200.0) + 4) * U24      # (beyond a = 200 the weight is 0 in both)
        bound = p64 * (eps + (p64 * eps).sum() + 2 * U24) + 2 * 2.0 ** -126
        err = np.abs(p[i].astype(np.float64) - p64)
        worst_p = max(worst_p, float((err / bound).max()))
        assert (err <= bound).all(), (k, kind)
        star = root64(e, np.log(perp))
        if star is None:
            assert b == 2.0 ** 100, (k, kind, b)
            zeros = e == 0
            np.testing.assert_allclose(p[i][zeros], 1.0 / zeros.sum(), rtol=2 * U24)
            assert (p[i][~zeros] == 0).all()
            continue
        H, ps, S, SE = entropy64(e, star)
        a_s = star * e
        abar = star * SE / S
        eps_s = (2 * np.minimum(a_s, 200.0) + 4) * U24
        dH = (ps * np.abs(1 + a_s - abar) * eps_s).sum() + 2 * U24 * abar
        slope = star * ((ps * e * e).sum() - (ps * e).sum() ** 2)      # |dH / dbeta| = beta Var_p(e)
        # the kernel stops where its computed entropy crosses the target, one float32 step wide: twice the first-order shift for the curvature
        bound_b = 2 * dH / slope + 2.0 ** -22 * star
        worst_b = max(worst_b, abs(b - star) / bound_b)
        assert abs(b - star) <= bound_b, (k, kind, b, star, bound_b)
    print(f"[tsne {what}] affinities k = {k}, perplexity {perp:g}: worst p error {worst_p:.3g} of its bound, worst beta error {worst_b:.3g} of its bound")


# ---------------------------------------------------------------------------------------------------------------- gradient
def random_csr(n, r, empty=None):
    """A symmetric P as (row_ptr, col, val) with ascending columns, about 8 entries a row, summing to 1; row and column `empty` hold nothing."""
    deg = min(8, n - 1)
    A = np.zeros((n, n))
    for i in range(n):
        js = r.choice(n - 1, deg, replace=False)
        js = js + (js >= i)
        A[i, js] = r.random(deg) + 0.05
    A = A + A.T
    if empty is not None:
        A[empty, :] = 0.0
        A[:, empty] = 0.0
    A = f32(A / A.sum())
    rows, cols = np.nonzero(A)
    row_ptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=row_ptr[1:])
    return row_ptr, cols.astype(np.int32), f32(A[rows, cols])


@functools.lru_cache(None)
def gradient_case(n, scale):
    """-> (y float32 [n, 2], csr); read-only.  From 257 points on: two coincident points, one point 1e6 away, one CSR row with no entries."""
    r = np.random.default_rng(900 + n + int(np.log10(scale) * 7))
    y = f32(scale * r.standard_normal((n, 2)))
    empty = None
    if n >= 3:
        y[1] = y[0]
    if n >= 257:
        y[n - 1] = (1e6, -1e6)
        y[5] = y[4]
        empty = 2
    csr = random_csr(n, r, empty)
    y.setflags(write=False)
    return y, csr


def dense_of(csr, n):
    P = np.zeros((n, n))
    row_ptr, col, val = csr
    P[np.repeat(np.arange(n), np.diff(row_ptr)), col] = np.asarray(val, np.float64)
    return P


def gradient_parts64(y, P):
    """-> (attr [n, 2], sum |attraction terms| [n, 2], rep [n, 2], sum |repulsion terms| [n, 2], Z, kl, sum |kl terms|) in float64, by blocks of rows."""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    attr, amag, rep, rmag = (np.zeros((n, 2)) for _ in range(4))
    zrow, kl, klmag = np.zeros(n), 0.0, 0.0
    W = []
    for r0 in range(0, n, 512):
        r1 = min(n, r0 + 512)
        diff = y[r0:r1, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (diff ** 2).sum(-1))
        w[np.arange(r1 - r0), np.arange(r0, r1)] = 0.0
        zrow[r0:r1] = w.sum(1)
        t = (w * w)[:, :, None] * diff
        rep[r0:r1], rmag[r0:r1] = t.sum(1), np.abs(t).sum(1)
        t = (P[r0:r1] * w)[:, :, None] * diff
        attr[r0:r1], amag[r0:r1] = t.sum(1), np.abs(t).sum(1)
        W.append(w[P[r0:r1] > 0])
    Z = zrow.sum()
    terms = P[P > 0] * np.log(P[P > 0] * Z / np.concatenate(W))
    return attr, amag, rep, rmag, Z, terms.sum(), np.abs(terms).sum()


@functools.lru_cache(None)
def gradient_reference(n, scale):
    y, csr = gradient_case(n, scale)
    return gradient_parts64(y, dense_of(csr, n))


def gradient64(n, scale, exaggeration=1.0):
    """-> (grad [n, 2], Z, kl, sum of |terms| [n, 2], attr [n, 2], sum of |kl terms|) in float64."""
    attr, amag, rep, rmag, Z, kl, klmag = gradient_reference(n, scale)
    return 4 * (exaggeration * attr - rep / Z), Z, kl, 4 * (exaggeration * amag + rmag / Z), attr, klmag


def check_gradient(n, scale, backend, what=""):
    y, csr = gradient_case(n, scale)
    P = dense_of(csr, n)
    out = {}
    for ex in (1.0, 12.0):
        grad, Z, kl = backend.tsne_gradient(y, csr, ex)
        g64, Z64, kl64, mag, attr, klmag = gradient64(n, scale, ex)
        bound = GRAD_C * U24 * mag + 1e-12 * mag + 1e-45
        err = np.abs(grad.astype(np.float64) - g64)
        assert grad.dtype == np.float32 and grad.shape == (n, 2) and np.isfinite(grad).all()
        worst = float((err / bound).max())
        zerr, klerr = abs(Z - Z64) / Z64, abs(kl - kl64)
        klbound = KL_C * U24 * P.sum() + 1e-12 * klmag
        print(f"[tsne {what}] gradient n = {n}, scale {scale:g}, exaggeration {ex:g}: worst error {worst:.3g} of its bound, Z rel {zerr:.3g} "
              f"(bound {Z_C * U24 + 1e-12:.3g}), kl error {klerr:.3g} (bound {klbound:.3g})")
        assert (err <= bound).all()
        assert zerr <= Z_C * U24 + 1e-12
        assert klerr <= klbound
        out[ex] = (grad, Z, kl, bound, attr)
    # exaggeration scales the attraction only: Z and kl keep their bits, the gradients differ by 4 x 11 attr
    assert out[1.0][1] == out[12.0][1] and out[1.0][2] == out[12.0][2]
    delta = out[12.0][0].astype(np.float64) - out[1.0][0].astype(np.float64)
    assert (np.abs(delta - 44.0 * out[1.0][4]) <= out[1.0][3] + out[12.0][3]).all()
    if n >= 257:      # the row with no entries: repulsion alone, whatever the exaggeration
        np.testing.assert_array_equal(bits(out[1.0][0][2]), bits(out[12.0][0][2]))


# ---------------------------------------------------------------------------------------------------------------- update
def sequential_sum(a):
    """The float64 sum of a 1-D array in index order."""
    return float(np.cumsum(np.asarray(a, np.float64))[-1]) if len(a) else 0.0


def update32(y, grad, velocity, gains, momentum, eta, min_gain):
    """The float32 restatement of one step: single operations in the kernel's order, then the float64 recentring (block sums of 256 points in
    point order, the blocks in block order)."""
    y, g, v, ga = (np.array(a, np.float32) for a in (y, grad, velocity, gains))
    mom, eta, floor = np.float32(momentum), np.float32(eta), np.float32(min_gain)
    differ = np.sign(g) != np.sign(v)
    ga = np.where(differ, ga + np.float32(0.2), ga * np.float32(0.8)).astype(np.float32)
    ga = np.where(ga < floor, floor, ga).astype(np.float32)
    v = (mom * v - (eta * ga) * g).astype(np.float32)
    y = (y + v).astype(np.float32)
    n = y.shape[0]
    mean = np.zeros(2)
    for c in range(2):
        blocks = [sequential_sum(y[b:b + 256, c]) for b in range(0, n, 256)]
        mean[c] = sequential_sum(blocks) / float(n)
    return (y.astype(np.float64) - mean).astype(np.float32), v, ga


def check_update(n, backend, what=""):
    r = np.random.default_rng(31 + n)
    y, grad = f32(30 * r.standard_normal((n, 2)) + 7), f32(1e-3 * r.standard_normal((n, 2)))
    vel, gains = f32(r.standard_normal((n, 2))), f32(0.01 + r.random((n, 2)) * 3)
    vel[::3] = 0.0
    grad[1::5] = 0.0
    gains[::4] = 0.0105                                  # falls below the floor when the signs agree
    y2, v2, g2 = backend.tsne_update(y, grad, vel, gains, 0.8, 200.0, 0.01)
    ry, rv, rg = update32(y, grad, vel, gains, 0.8, 200.0, 0.01)
    np.testing.assert_array_equal(bits(g2), bits(rg))
    np.testing.assert_array_equal(bits(v2), bits(rv))
    np.testing.assert_array_equal(bits(y2), bits(ry))
    mean = np.abs(y2.astype(np.float64).mean(0)).max()
    print(f"[tsne {what}] update n = {n}: exact; |mean| after recentring {mean:.3g} (bound {2.0 ** -23 * np.abs(y2).max():.3g}), least gain {g2.min():.4g}")
    assert mean <= 2.0 ** -23 * np.abs(y2).max()
    assert (g2 >= np.float32(0.01)).all() and (n < 257 or (g2 == np.float32(0.01)).any())


# ---------------------------------------------------------------------------------------------------------------- fit
def check_fit_steps(backend, what=""):
    """tmjx_tsne_fit equals gradient -> update step by step, bit for bit, across the exaggeration boundary; two calls give the same bits."""
    n, n_iter, early = 300, 12, 5
    y, csr = gradient_case(1000, 1.0)
    y = f32(1e-4 * y[:n])
    csr = random_csr(n, np.random.default_rng(3))
    fy, fv, fg, info = backend.tsne_fit(y, csr, n_iter, 12.0, early, 0.5, 0.8, 50.0, 0.01)
    fy2, fv2, fg2, info2 = backend.tsne_fit(y, csr, n_iter, 12.0, early, 0.5, 0.8, 50.0, 0.01)
    sy, sv, sg = y, np.zeros((n, 2), np.float32), np.ones((n, 2), np.float32)
    for it in range(n_iter):
        grad, _, _ = backend.tsne_gradient(sy, csr, 12.0 if it < early else 1.0)
        sy, sv, sg = backend.tsne_update(sy, grad, sv, sg, 0.5 if it < early else 0.8, 50.0, 0.01)
    _, Z, kl = backend.tsne_gradient(sy, csr, 1.0)
    for a, b in ((fy, sy), (fv, sv), (fg, sg), (fy, fy2), (fv, fv2), (fg, fg2)):
        np.testing.assert_array_equal(bits(a), bits(b))
    assert info.n_iter == n_iter and info.kl == kl and info.z == Z and info2.kl == kl and info2.z == Z
    print(f"[tsne {what}] fit of {n} points, {n_iter} iterations: equals its steps, kl {info.kl:.6f}, Z {info.z:.6f}")


# ---------------------------------------------------------------------------------------------------------------- place
def place32(idx, p, y):
    out = np.zeros((idx.shape[0], 2), np.float32)
    for j in range(idx.shape[1]):
        out = (out + (p[:, j, None] * y[idx[:, j]]).astype(np.float32)).astype(np.float32)
    return out


def in_hull(pt, pts, slack):
    """Whether pt lies in the convex hull of pts (2-D), to within `slack`: on the inner side of every edge of the monotone-chain hull."""
    P = sorted(set(map(tuple, np.asarray(pts, np.float64))))
    if len(P) < 3:
        lo, hi = np.min(P, 0), np.max(P, 0)
        return bool((pt >= lo - slack).all() and (pt <= hi + slack).all())
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])      # noqa: E731
    hull = []
    for seq in (P, P[::-1]):
        part = []
        for q in seq:
            while len(part) >= 2 and cross(part[-2], part[-1], q) <= 0:
                part.pop()
            part.append(q)
        hull += part[:-1]
    for a, b in zip(hull, hull[1:] + hull[:1]):
        if cross(a, b, pt) < -slack * np.hypot(b[0] - a[0], b[1] - a[1]):
            return False
    return True


def check_place(backend, what=""):
    r = np.random.default_rng(8)
    n, m, k = 500, 300, 17
    y = f32(20 * r.standard_normal((n, 2)))
    idx = np.stack([r.choice(n, k, replace=False) for _ in range(m)]).astype(np.int32)
    p = r.random((m, k)) ** 3
    p = f32(p / p.sum(1, keepdims=True))
    out = backend.tsne_place(idx, p, y)
    np.testing.assert_array_equal(bits(out), bits(place32(idx, p, y)))
    # a query equal to a training row, through knn and the affinities: inside its neighbours' hull
    x, _ = knn_data(KNN_CASES[2])
    x = x[:n]
    xa = backend.asarray(x)
    qi, qd = backend.knn(xa, backend.asarray(np.array(x[:60])), k)
    qp, _ = backend.tsne_affinities(qd, 5.0)
    placed = backend.tsne_place(qi, qp, y)
    assert (qi[:, 0] == np.arange(60)).all()
    for i in range(60):
        assert in_hull(placed[i].astype(np.float64), y[qi[i]], 1e-5 * np.abs(y[qi[i]]).max()), i
    print(f"[tsne {what}] place {m} x {k}: exact; 60 training rows placed inside their neighbours' hulls")


# ---------------------------------------------------------------------------------------------------------------- the model level
@functools.lru_cache(None)
def blobs():
    """-> (x float32 [400, 30], labels, held-out x [80, 30], its labels): unit-variance blobs on orthogonal axes, separation 6; read-only."""
    M = MODEL
    r = np.random.default_rng(2024)
    lab = np.repeat(np.arange(M["blobs"]), M["per"])
    perm = r.permutation(len(lab))
    lab = lab[perm]
    x = r.standard_normal((len(lab), M["d"]))
    x[np.arange(len(lab)), lab] += M["sep"]
    # the held-out rows have a generator of their own: the draw that followed the training rows held one row whose nearest training rows in the
    # 30-D space are another blob's, which the float64 reference places there too (79 of 80); on this draw the reference places all 80
    r = np.random.default_rng(3001)
    hl = np.repeat(np.arange(M["blobs"]), M["held_out"])
    hx = r.standard_normal((len(hl), M["d"]))
    hx[np.arange(len(hl)), hl] += M["sep"]
    x, hx = f32(x), f32(hx)
    for a in (x, lab, hx, hl):
        a.setflags(write=False)
    return x, lab, hx, hl


def purity(y, lab, k=10):
    """The share of each row's k nearest neighbours that carry its label."""
    y = np.asarray(y, np.float64)
    D = ((y[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, 1, kind="stable")[:, :k]
    return float((lab[nn] == lab[:, None]).mean())


def tsne_numpy(y0, P, n_iter, exaggeration, exaggeration_iters, momentum_early, momentum_late, eta, min_gain, dtype=np.float64):
    """The schedule in numpy at `dtype`, vectorised over all pairs -> (y, kl of the final y, [kl at the start of every iteration])."""
    y = np.array(y0, dtype)
    P = np.asarray(P, dtype)
    v, ga = np.zeros_like(y), np.ones_like(y)
    nz = P > 0
    four, one = dtype(4), dtype(1)

    def parts(y):
        diff = y[:, None, :] - y[None, :, :]
        w = one / (one + (diff ** 2).sum(-1))
        np.fill_diagonal(w, 0)
        return diff, w, w.sum()
    kls = []
    for it in range(n_iter + 1):
        diff, w, Z = parts(y)
        kls.append(float((P[nz].astype(np.float64) * np.log(P[nz].astype(np.float64) * float(Z) / w[nz].astype(np.float64))).sum()))
        if it == n_iter:
            break
        ex = dtype(exaggeration if it < exaggeration_iters else 1.0)
        grad = four * (ex * ((P * w)[:, :, None] * diff).sum(1) - ((w * w)[:, :, None] * diff).sum(1) / Z)
        ga = np.where(np.sign(grad) != np.sign(v), ga + dtype(0.2), ga * dtype(0.8))
        ga = np.maximum(ga, dtype(min_gain))
        v = dtype(momentum_early if it < exaggeration_iters else momentum_late) * v - dtype(eta) * ga * grad
        y = y + v
        y = y - y.mean(0, dtype=np.float64).astype(dtype)
    return y, kls[-1], kls


@functools.lru_cache(None)
def model_inputs(backend_key, backend):
    """The device's own neighbours, affinities, CSR and start for the blobs (shared by the model-level checks of one backend)."""
    from track_mjx_amd.analysis import embed as EM
    x, lab, _, _ = blobs()
    M = MODEL
    t = EM.TSNE(M["perplexity"], n_iter=M["n_iter"], exaggeration=M["exaggeration"], exaggeration_iters=M["exaggeration_iters"], backend=backend)
    t.fit(x)
    y0 = t.initial(backend.asarray(x))
    return t, y0


@functools.lru_cache(None)
def model_reference(backend_key, backend):
    """The float64 reference and its float32 restatement from the device's P and start -> (y64, kl64, kls64, kl32)."""
    t, y0 = model_inputs(backend_key, backend)
    M = MODEL
    P = dense_of(t.csr_, y0.shape[0])
    args = (M["n_iter"], M["exaggeration"], M["exaggeration_iters"], M["momentum_early"], M["momentum_late"], t.eta_, M["min_gain"])
    y64, kl64, kls64 = tsne_numpy(y0, P, *args)
    _, kl32, _ = tsne_numpy(y0, P, *args, dtype=np.float32)
    return y64, kl64, kls64, kl32


def check_model(backend, what=""):
    """(a) purity of the device embedding >= 0.99 where the first two PCs stay below 0.6; (b) the final kl within (1 + margin) of the float64
    reference's from the same start and schedule; (c) after the exaggeration phase the kl of the steps never rises by more than that margin."""
    x, lab, _, _ = blobs()
    M = MODEL
    t, y0 = model_inputs(what, backend)
    y64, kl64, kls64, kl32 = model_reference(what, backend)
    gap = abs(kl32 - kl64) / kl64
    margin = 2 * MODEL_GAP
    p_ref, p_dev, p_pc = purity(y64, lab), purity(t.embedding_, lab), purity(y0, lab)
    print(f"[tsne {what}] model: purity float64 {p_ref:.4f}, device {p_dev:.4f}, first two PCs {p_pc:.4f}; kl float64 {kl64:.6f}, float32 numpy {kl32:.6f} "
          f"(gap {gap:.3g}, margin {margin:.3g}), device {t.kl_:.6f}")
    assert p_ref >= 0.99, "the data does not let the float64 reference reach 0.99"
    assert p_pc < 0.6
    assert p_dev >= 0.99
    assert t.kl_ <= kl64 * (1 + margin)
    # (c) the steps, from the same start
    sy, sv, sg = y0, np.zeros_like(y0), np.ones_like(y0)
    kls = []
    for it in range(M["n_iter"]):
        early = it < M["exaggeration_iters"]
        grad, _, kl = backend.tsne_gradient(sy, t.csr_, M["exaggeration"] if early else 1.0)
        kls.append(kl)
        sy, sv, sg = backend.tsne_update(sy, grad, sv, sg, M["momentum_early"] if early else M["momentum_late"], t.eta_, M["min_gain"])
    np.testing.assert_array_equal(bits(sy), bits(t.embedding_))
    late = np.array(kls[M["exaggeration_iters"]:])
    rise = float((late[1:] / late[:-1]).max() - 1)
    print(f"[tsne {what}] model: the largest rise of kl between two iterations after the exaggeration phase {rise:.3g} (margin {margin:.3g})")
    assert rise <= margin


def check_transform(backend, what=""):
    """The blob of a held-out row is the majority blob of the 10 nearest training points on the map, for >= 0.99 of them; the float64 reference
    (float64 neighbours, affinities and placement on the float64 embedding) is checked first."""
    x, lab, hx, hl = blobs()
    t, y0 = model_inputs(what, backend)
    y64 = model_reference(what, backend)[0]
    k, perp = t.n_neighbours_, MODEL["perplexity"]

    def majority(placed, emb):
        D = ((np.asarray(placed, np.float64)[:, None, :] - np.asarray(emb, np.float64)[None, :, :]) ** 2).sum(-1)
        nn = np.argsort(D, 1, kind="stable")[:, :10]
        return np.array([np.bincount(lab[row], minlength=MODEL["blobs"]).argmax() for row in nn])
    D = dist64(x, hx)
    nn = np.argsort(D, 1, kind="stable")[:, :k]
    ref = np.zeros((hx.shape[0], 2))
    for i in range(hx.shape[0]):
        e = D[i, nn[i]] - D[i, nn[i]].min()
        ref[i] = entropy64(e, root64(e, np.log(perp)))[1] @ y64[nn[i]]
    good_ref = float((majority(ref, y64) == hl).mean())
    placed = t.transform(hx)
    good = float((majority(placed, t.embedding_) == hl).mean())
    print(f"[tsne {what}] transform: {hx.shape[0]} held-out rows in their blob: float64 {good_ref:.4f}, device {good:.4f}")
    assert placed.dtype == np.float32 and placed.shape == (hx.shape[0], 2)
    assert good_ref >= 0.99
    assert good >= 0.99


def check_tsne_inputs(backend, strided, what=""):
    """Numpy inputs and strided arrays of the provider give the same bits through TSNE, also with a training stride."""
    from track_mjx_amd.analysis import embed as EM
    x, _, hx, _ = blobs()
    kw = dict(n_iter=20, exaggeration_iters=8, backend=backend)
    a = EM.TSNE(10, **kw).fit(np.array(x))
    b = EM.TSNE(10, **kw).fit(strided(x))
    for name in ("embedding_", "beta_", "train_index_"):
        np.testing.assert_array_equal(bits(getattr(a, name)), bits(getattr(b, name)))
    assert a.kl_ == b.kl_ and a.embedding_.shape == (x.shape[0], 2) and a.eta_ == 50.0 and a.n_neighbours_ == 30
    np.testing.assert_array_equal(bits(a.transform(np.array(hx))), bits(b.transform(strided(hx))))
    c = EM.TSNE(10, max_train=150, **kw).fit(np.array(x))
    d = EM.TSNE(10, max_train=150, **kw).fit(strided(x))
    assert list(c.train_index_) == list(range(0, x.shape[0], 3)) and c.embedding_.shape == (134, 2)
    np.testing.assert_array_equal(bits(c.embedding_), bits(d.embedding_))
    full = c.fit_transform(np.array(x))
    assert full.shape == (x.shape[0], 2)
    np.testing.assert_array_equal(bits(full[c.train_index_]), bits(c.embedding_))


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, alloc, ptr, untouched, what=""):
    """Every refusal through the C-ABI: -22 with a message that names the value, nothing launched, sentinel-filled outputs untouched.
    `alloc(shape, dtype, fill)` -> an array of the library's memory, `ptr(a)` its address, `untouched(a, fill)` whether it still holds `fill`."""
    from track_mjx_amd import hip
    n, m, d, k = 130, 130, 7, 20
    x = alloc((n, d), np.float32, 0.0)
    outs = {"idx": alloc((m, 128), np.int32, -5), "dist2": alloc((m, 128), np.float32, -5.0), "p": alloc((m, 128), np.float32, -5.0), "beta": alloc((m,), np.float32, -5.0),
            "y": alloc((n, 2), np.float32, -5.0), "grad": alloc((n, 2), np.float32, -5.0), "vel": alloc((n, 2), np.float32, -5.0), "gains": alloc((n, 2), np.float32, -5.0),
            "z": alloc((1,), np.float64, -5.0), "kl": alloc((1,), np.float64, -5.0), "out": alloc((m, 2), np.float32, -5.0)}
    o = {key: ptr(v) for key, v in outs.items()}
    floats = C.c_int64(0)
    assert lib.tmjx_tsne_workspace(n, m, d, 128, C.byref(floats)) == 0 and 0 < floats.value < n * m
    big = C.c_int64(0)
    assert lib.tmjx_tsne_workspace(65536, 210000, 1024, 128, C.byref(big)) == 0 and big.value < 65536 * 1024      # nothing scales with n n or m n
    ws = alloc((int(floats.value) + 4,), np.float32, 0.0)
    col, val = alloc((40,), np.int32, 0), alloc((40,), np.float32, 0.0)
    X, WS, COL, VAL = ptr(x), ptr(ws), ptr(col), ptr(val)
    row_ptr = (C.c_int32 * (n + 1))(*([0] + [40] * n))
    bad_end = (C.c_int32 * (n + 1))(*([0] + [39] * n))
    falling = (C.c_int32 * (n + 1))(*([0, 5, 3] + [40] * (n - 2)))
    err, nan = lib.tmjx_last_error, float("nan")
    info = C.byref(hip.TsneInfo())

    def knn(n=n, d=d, ldx=None, q=X, m=m, ldq=None, self_=1, k=k, x=X, idx=o["idx"], dist2=o["dist2"], ws=WS):
        return lib.tmjx_knn(x, n, d, d if ldx is None else ldx, q, m, d if ldq is None else ldq, self_, k, idx, dist2, ws, None)

    def aff(m=m, k=k, perplexity=5.0, dist2=o["dist2"], p=o["p"], beta=o["beta"]):
        return lib.tmjx_tsne_affinities(dist2, m, k, perplexity, p, beta, None)

    def gradient(n=n, row_ptr=row_ptr, col=COL, val=VAL, nnz=40, ex=1.0, y=o["y"], grad=o["grad"], z=o["z"], kl=o["kl"], ws=WS):
        return lib.tmjx_tsne_gradient(y, n, row_ptr, col, val, nnz, ex, grad, z, kl, ws, None)

    def update(n=n, momentum=0.5, eta=50.0, min_gain=0.01, y=o["y"], grad=o["grad"], ws=WS):
        return lib.tmjx_tsne_update(y, grad, o["vel"], o["gains"], n, momentum, eta, min_gain, ws, None)

    def fit(n=n, row_ptr=row_ptr, nnz=40, n_iter=3, ex=12.0, early=1, m0=0.5, m1=0.8, eta=50.0, min_gain=0.01, info=info, y=o["y"], ws=WS):
        return lib.tmjx_tsne_fit(y, n, row_ptr, COL, VAL, nnz, n_iter, ex, early, m0, m1, eta, min_gain, o["vel"], o["gains"], info, ws, None)

    def place(m=m, k=k, n=n, idx=o["idx"], p=o["p"], y=o["y"], out=o["out"]):
        return lib.tmjx_tsne_place(idx, p, m, k, y, n, out, None)
    cases = [
        (lambda: lib.tmjx_tsne_workspace(1, m, d, k, C.byref(floats)), b"n must be >= 2"), (lambda: lib.tmjx_tsne_workspace(65537, m, d, k, C.byref(floats)), b"65537"),
        (lambda: lib.tmjx_tsne_workspace(n, 0, d, k, C.byref(floats)), b"m must be >= 1"), (lambda: lib.tmjx_tsne_workspace(n, m, 1025, k, C.byref(floats)), b"1025"),
        (lambda: lib.tmjx_tsne_workspace(n, m, d, 129, C.byref(floats)), b"129"), (lambda: lib.tmjx_tsne_workspace(n, m, d, k, None), b"null"),
        (lambda: knn(n=1), b"n must be >= 2"), (lambda: knn(n=65537), b"65537"), (lambda: knn(m=0), b"m must be >= 1"), (lambda: knn(d=0), b"d must be >= 1"),
        (lambda: knn(d=1025, ldx=1025, ldq=1025), b"1025"), (lambda: knn(k=0), b"k must be >= 1"), (lambda: knn(k=129), b"129"),
        (lambda: knn(k=130, n=130), b"130"), (lambda: knn(n=100, m=100, k=100), b"99 candidate"), (lambda: knn(n=100, m=50, k=101, self_=0), b"100 candidate"),
        (lambda: knn(ldx=d - 1), b"ldx"), (lambda: knn(ldq=d - 1), b"ldq"), (lambda: knn(x=None), b"null"), (lambda: knn(q=None), b"null"),
        (lambda: knn(idx=None), b"null"), (lambda: knn(dist2=None), b"null"), (lambda: knn(ws=None), b"null"), (lambda: knn(ws=WS + 4), b"16-byte"),
        (lambda: knn(idx=o["idx"] + 2), b"4-byte"),
        (lambda: aff(perplexity=float(k)), b"below k"), (lambda: aff(perplexity=0.99), b"perplexity must be >= 1"), (lambda: aff(perplexity=nan), b"perplexity"),
        (lambda: aff(k=129), b"129"), (lambda: aff(m=0), b"m must be"), (lambda: aff(p=None), b"null"), (lambda: aff(beta=o["beta"] + 1), b"4-byte"),
        (lambda: gradient(n=1), b"n must be >= 2"), (lambda: gradient(row_ptr=bad_end), b"disagrees"), (lambda: gradient(nnz=41), b"disagrees"),
        (lambda: gradient(row_ptr=falling), b"decreases"), (lambda: gradient(row_ptr=None), b"null"), (lambda: gradient(col=None), b"null"),
        (lambda: gradient(ex=0.0), b"exaggeration"), (lambda: gradient(ex=nan), b"exaggeration"), (lambda: gradient(grad=None), b"null"),
        (lambda: gradient(z=None), b"null"), (lambda: gradient(ws=WS + 4), b"16-byte"), (lambda: gradient(y=o["y"] + 4), b"8-byte"),
        (lambda: update(n=65537), b"65537"), (lambda: update(momentum=1.0), b"momentum"), (lambda: update(eta=0.0), b"eta"), (lambda: update(min_gain=-1.0), b"min_gain"),
        (lambda: update(y=None), b"null"), (lambda: update(ws=WS + 4), b"16-byte"), (lambda: update(grad=o["grad"] + 4), b"8-byte"),
        (lambda: fit(n_iter=-1), b"n_iter"), (lambda: fit(early=-1), b"exaggeration_iters"), (lambda: fit(ex=-1.0), b"exaggeration"), (lambda: fit(m1=1.5), b"momentum"),
        (lambda: fit(eta=nan), b"eta"), (lambda: fit(info=None), b"null"), (lambda: fit(row_ptr=bad_end), b"disagrees"), (lambda: fit(ws=None), b"null"),
        (lambda: place(k=0), b"k must be"), (lambda: place(n=1), b"n must be"), (lambda: place(m=0), b"m must be"), (lambda: place(out=None), b"null"),
        (lambda: place(idx=o["idx"] + 1), b"4-byte"),
    ]
    for call, word in cases:
        assert call() == -22 and word in err(), (word, err())
    for key, v in outs.items():
        assert untouched(v, -5), key
    print(f"[tsne {what}] {len(cases)} refusals, nothing written")


# ---------------------------------------------------------------------------------------------------------------- the host map and the command line
def check_density_and_watershed():
    from track_mjx_amd.analysis import embed as EM
    r = np.random.default_rng(12)
    y = np.concatenate([r.standard_normal((700, 2)) + (6, 0), 0.8 * r.standard_normal((300, 2)) - (6, 1)])
    density, extent, counts = EM.density_map(y, grid=128, sigma=0.7)
    assert density.shape == (128, 128) and counts.sum() == 1000 and abs(density.sum() - 1000) <= 1e-9 * 1000 and (density >= 0).all()
    regions = EM.watershed(density, counts)
    labels = EM.region_labels(regions, y, extent)
    assert regions.dtype == np.int32 and labels.dtype == np.int32 and labels.min() >= 0
    live = np.bincount(labels)
    assert (np.diff(live) <= 0).all(), "regions are not numbered by descending count"
    assert (labels[:700] == 0).mean() > 0.99 and (labels[700:] == 1).mean() > 0.99
    # analytic densities: exactly two regions on two Gaussians, one on a single Gaussian
    g = np.linspace(-8, 8, 96)
    X, Y = np.meshgrid(g, g)
    one = np.exp(-0.5 * (X ** 2 + Y ** 2))
    two = np.exp(-0.5 * ((X - 3) ** 2 + Y ** 2)) + 0.6 * np.exp(-0.5 * ((X + 3) ** 2 + (Y - 1) ** 2))
    r1, r2 = EM.watershed(one), EM.watershed(two)
    assert set(np.unique(r1)) <= {-1, 0} and (r1 == 0).any()
    assert set(np.unique(r2[r2 >= 0])) == {0, 1}
    assert r2[48, int(np.argmin(np.abs(g - 3)))] == 0 and r2[int(np.argmin(np.abs(g - 1))), int(np.argmin(np.abs(g + 3)))] == 1      # the heavier first


def clip_files(tmp_path, widths=(90, 70, 80, 60)):
    """Four small synthetic clip_<i>.h5 whose activations/intention [T, 6] are planted blobs -> (directory, the features by clip)."""
    from track_mjx_amd import h5lite
    r = np.random.default_rng(21)
    feats = {}
    for clip, T in zip((0, 2, 5, 7), widths):
        lab = (np.arange(T) // 10 + clip) % 3
        f = r.standard_normal((T, 6))
        f[np.arange(T), lab] += 8.0
        feats[clip] = f32(f)
        h5lite.write_tree(str(tmp_path / f"clip_{clip}.h5"), {"activations": {"intention": feats[clip]}, "ctrl": np.zeros((T, 2), np.float32)})
    return str(tmp_path), feats


def check_cli(tmp_path, backend, capsys):
    """The command-line round trip: the file's fields and shapes, labels by descending count, the file as intervention centroids, the usage errors."""
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import embed as EM
    from track_mjx_amd.analysis.intervene import Intervention
    (tmp_path / "clips").mkdir()
    rollouts, feats = clip_files(tmp_path / "clips")
    out = str(tmp_path / "out" / "map.h5")
    n = sum(f.shape[0] for f in feats.values())
    assert EM.main([f"rollouts={rollouts}", "perplexity=8", "max_train=200", "n_iter=150", "grid=64", f"out={out}"], backend=backend) == 0
    assert f"[embed] intention: {n} samples x 6 features from 4 clips, 150 trained" in capsys.readouterr().out
    with h5lite.File(out) as h:
        got = {key: np.asarray(h[key][()]) for key in ("train_index", "kl", "density", "regions", "extent", "counts", "transitions", "dwell_mean", "centroids", "clips")}
        assert bytes(h["feature"][()]).decode() == "intention"
        emb = {c: np.asarray(h["embedding"][f"clip_{c}"][()]) for c in feats}
        labels = {c: np.asarray(h["labels"][f"clip_{c}"][()]) for c in feats}
    K = got["counts"].shape[0]
    assert list(got["train_index"]) == list(range(0, n, 2)) and got["density"].shape == (64, 64) and got["regions"].shape == (64, 64) and got["extent"].shape == (4,)
    assert got["regions"].dtype == np.int32 and int(got["regions"].max()) == K - 1 and float(got["kl"]) > 0
    assert got["counts"].sum() == n and (np.diff(got["counts"]) <= 0).all() and got["transitions"].shape == (K, K) and got["transitions"].sum() == n - 4
    assert got["centroids"].shape == (K, 6) and got["centroids"].dtype == np.float32 and got["dwell_mean"].shape == (K,) and list(got["clips"]) == [0, 2, 5, 7]
    for c, f in feats.items():
        assert emb[c].shape == (f.shape[0], 2) and emb[c].dtype == np.float32 and labels[c].shape == (f.shape[0],) and labels[c].dtype == np.int32
    lab = np.concatenate([labels[c] for c in feats])
    np.testing.assert_array_equal(np.bincount(lab, minlength=K), got["counts"])
    allf = np.concatenate([feats[c] for c in feats])
    np.testing.assert_allclose(got["centroids"][0], allf[lab == 0].astype(np.float64).mean(0), rtol=1e-6, atol=1e-6)
    assert Intervention.from_centroids(out, columns="0:2").target == "intention"
    assert EM.main([f"rollouts={rollouts}"]) == 2 and EM.main([f"rollouts={rollouts}", f"out={out}", "bogus=1"]) == 2
    assert EM.main([f"rollouts={rollouts}", f"out={out}", "feature=nothing"], backend=backend) == 2
    assert "usage" in capsys.readouterr().err
