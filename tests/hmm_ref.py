"""The float64 reference of the hidden-Markov-model kernels, a float32 numpy restatement of them, the case generators and the checkers that
tests/test_hmm_cpu.py (the host emulation) and tests/test_gpu_hmm.py (the C-ABI) share.  A `backend` is analysis.pca.HipBackend or the same backend on numpy arrays,
tests/hostemu/analysis_emu.B.

Emission and M-step cases (n, d, k): one row; one row past a 256-row block; the intention's width; odd tile edges; both limits.  Sequence cases
(lengths, k): a single row; sequences of one and two rows; short, long and odd; eight full clips and a stub; the state limit.

The bounds, u = 2^-24, are worst-case first-order errors of sums and products of NON-NEGATIVE quantities, where componentwise relative errors add:
  logb     q is a sum of d non-negative terms v (v / var), v = x - mu: v carries one rounding and enters twice, 1 / var and the product one each, the
           fma chain at most d more: (d + 4) u q / 2; c_j is rounded once from float64 (2 u |c_j| leaves room for the reference's own log), the last
           fma once more: u |logb|.
  loglik   the scaled forward pass is a product of T non-negative matrices diag(bt_t) A, each applied with relative error <= (k + 8) u (a k-term
           fma chain, then exp, the product, the sum of k terms in groups, the division, the log): 2 T (k + 8) u absolute on the log, the factor 2
           slack for library ulps.  It needs log c_t = O(1): transition entries >= 2^-10 keep every |log c_t| below 7.
  gamma    the same product, forward and backward: 2 T (k + 8) u relative, plus 2^-40 for entries that underflow in float32.
  xi       a sum of T products alpha A w, each within 2 T (k + 8) u, summed in float64: 3 T_max (k + 8) u relative, plus 2^-40 per row.
  M-step   x - m is rounded once (u |x - m|) and squared (2 u), everything else is float64: see check_mstep.
  Viterbi  delta is a sum of at most 2 T float32 additions of magnitude <= max |delta|: tau = 4 T u max |delta|.
The bounds are loose for well-mixing chains; every checker prints the worst observed ratio to its bound."""
from __future__ import annotations

import functools
import itertools

import numpy as np

EMISSION_CASES = ((1, 1, 1), (257, 3, 2), (1000, 60, 7), (4099, 129, 33), (2050, 1024, 128))
SEQ_CASES = (((1,), 1), ((1, 2, 1), 2), ((37, 300, 5), 7), ((250,) * 8 + (3,), 33), ((64,) * 4 + (301,), 128))
U24 = 2.0 ** -24
TINY = 2.0 ** -40
f64 = lambda a: np.asarray(a, np.float64)      # noqa: E731  (np.float64(a) turns a one-element array into a scalar)
f32 = lambda a: np.asarray(a, np.float32)      # noqa: E731


def seq_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- data
@functools.lru_cache(None)
def emission_data(case):
    """Blobs as kmeans_ref.case_data -> (x float32 [n, d], means float32 [k, d], vars float32 [k, d] in [0.25, 4]); read-only."""
    n, d, k = case
    r = np.random.default_rng(4321 + n)
    ctr = 2.0 * r.standard_normal((k, d))
    lab = r.integers(0, k, n)
    x = f32(ctr[lab] + r.standard_normal((n, d))) + f32(3)
    mu = f32(ctr + 3 + 0.25 * r.standard_normal((k, d)))
    var = f32(r.uniform(0.25, 4.0, (k, d)))
    for a in (x, mu, var):
        a.setflags(write=False)
    return x, mu, var


def sticky_chain(r, k, stay=0.9):
    """A transition matrix with `stay` on the diagonal and every entry >= 2^-10, and a start vector likewise; float32, rows summing to 1 in float64
    within 2^-23."""
    A = (1.0 - stay) * r.dirichlet(np.ones(k), k) + stay * np.eye(k)
    A = np.maximum(A, 2.0 ** -9)
    A /= A.sum(1, keepdims=True)
    pi = np.maximum(r.dirichlet(np.ones(k)), 2.0 ** -9)
    pi /= pi.sum()
    return f32(A), f32(pi)


def draw_chain(r, lengths, A, pi):
    A64, pi64 = f64(A) / f64(A).sum(1, keepdims=True), f64(pi) / f64(pi).sum()
    z = []
    for T in lengths:
        s = r.choice(len(pi64), p=pi64)
        for _ in range(T):
            z.append(s)
            s = r.choice(len(pi64), p=A64[s])
    return np.asarray(z)


@functools.lru_cache(None)
def seq_data(case, d=3):
    """Rows drawn from a planted sticky chain -> (x [n, d], means, vars in [0.25, 4], transmat, startprob, seq_start, logb float32 [n, k]: the
    float64 log densities rounded once, the input of the forward-backward and Viterbi checks); read-only."""
    lengths, k = case
    r = np.random.default_rng(77 + k)
    A, pi = sticky_chain(r, k)
    mu = f32(1.5 * r.standard_normal((k, d)))
    var = f32(r.uniform(0.25, 4.0, (k, d)))
    z = draw_chain(r, lengths, A, pi)
    x = f32(mu[z] + np.sqrt(var[z]) * r.standard_normal((len(z), d)))
    logb = f32(logb64(x, mu, var)[0])
    out = (x, mu, var, A, pi, seq_of(lengths), logb)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def logb64(x, mu, var):
    """-> (logb [n, k], q [n, k] the quadratic form, c [k]) in float64 from the float32 inputs."""
    x64, mu64, var64 = (np.asarray(a, np.float64) for a in (x, mu, var))
    q = np.empty((x64.shape[0], mu64.shape[0]))
    for j in range(mu64.shape[0]):
        q[:, j] = (((x64 - mu64[j]) ** 2) / var64[j]).sum(1)
    c = -0.5 * np.log(2.0 * np.pi * var64).sum(1)
    return c[None, :] - 0.5 * q, q, c


def fb64(logb, seq, A, pi, dtype=np.float64):
    """The scaled forward-backward recursion -> (gamma [n, k], xi [k, k], start [k], loglik [S]).  dtype=float32 is the numpy restatement of the
    kernel: the same recursion in float32 (numpy sums where the kernel has fma chains), the loglik and xi accumulated in float64."""
    f = dtype
    lb, A_, pi_ = np.asarray(logb, f), np.asarray(A, f), np.asarray(pi, f)
    n, k = lb.shape
    gamma, xi, start, loglik = np.zeros((n, k), f), np.zeros((k, k)), np.zeros(k), np.zeros(len(seq) - 1)
    for s, (t0, t1) in enumerate(zip(seq[:-1], seq[1:])):
        T = t1 - t0
        m = lb[t0:t1].max(1)
        with np.errstate(invalid="ignore"):
            bt = np.where(np.isneginf(m)[:, None], f(0), np.exp(lb[t0:t1] - m[:, None])).astype(f)
        ah, cs, ll = np.zeros((T, k), f), np.zeros(T, f), 0.0
        for t in range(T):
            a = (pi_ * bt[t] if t == 0 else bt[t] * (ah[t - 1] @ A_)).astype(f)
            cs[t] = a.sum(dtype=f)
            ah[t] = a / cs[t] if cs[t] > 0 else 0
            with np.errstate(divide="ignore"):
                ll += float(np.log(cs[t])) + float(m[t])
        loglik[s] = ll
        bh = np.ones(k, f)
        for t in range(T - 1, -1, -1):
            g = ah[t] * bh
            G = g.sum(dtype=f)
            gamma[t0 + t] = g / G if G > 0 else 0
            w = (bt[t] * bh / cs[t]).astype(f) if cs[t] > 0 else np.zeros(k, f)
            if t > 0:
                xi += f64(A_) * np.outer(f64(ah[t - 1]), f64(w))
                bh = (A_ @ w).astype(f)
        start += f64(gamma[t0])
    return gamma, xi, start, loglik


def mstep64(x, gamma, mu_in, var_in, min_var=0.0, min_weight=0.0):
    """-> (means, vars, weight) float64; a state below min_weight as given.  gamma is the float32 array the kernel is given."""
    x64, g = np.asarray(x, np.float64), np.asarray(gamma, np.float64)
    w = g.sum(0)
    mu, var = np.asarray(mu_in, np.float64).copy(), np.asarray(var_in, np.float64).copy()
    for j in range(g.shape[1]):
        if w[j] >= min_weight and w[j] > 0:
            mu[j] = (g[:, j, None] * x64).sum(0) / w[j]
            var[j] = np.maximum((g[:, j, None] * (x64 - mu[j]) ** 2).sum(0) / w[j], min_var)
    return mu, var, w


def mstep32(x, gamma, mu_in, var_in, min_var=0.0, min_weight=0.0):
    """The restatement: the centring in float32 about the float32 column mean, the sums in float64."""
    m = f32(np.asarray(x, np.float64).mean(0))
    xc, g = f64(f32(x) - m), np.asarray(gamma, np.float64)
    w = g.sum(0)
    mu, var = np.array(mu_in, np.float32), np.array(var_in, np.float32)
    for j in range(g.shape[1]):
        if w[j] >= min_weight and w[j] > 0:
            s1, s2 = (g[:, j, None] * xc).sum(0) / w[j], (g[:, j, None] * xc * xc).sum(0) / w[j]
            mu[j], var[j] = f32(f64(m) + s1), f32(np.maximum(s2 - s1 * s1, min_var))
    return mu, var, w


def transitions64(xi, start, prior, kappa, A_in, pi_in):
    k = len(start)
    num = np.asarray(xi, np.float64) + prior + kappa * np.eye(k)
    den = num.sum(1, keepdims=True)
    A = np.where(den > 0, num / np.where(den > 0, den, 1), np.asarray(A_in, np.float64))
    sn = np.asarray(start, np.float64) + prior
    return A, (sn / sn.sum() if sn.sum() > 0 else np.asarray(pi_in, np.float64))


def viterbi64(logb, seq, logA, logpi, dtype=np.float64):
    """-> (labels, score [S], margin [S]: the smallest gap, over the steps of the best path and its final choice, between the chosen candidate and the
    runner-up, max |delta| [S]).  The first of equal maxima wins: the lowest index.  dtype=float32: the restatement."""
    f = dtype
    lb, lA, lpi = np.asarray(logb, f), np.asarray(logA, f), np.asarray(logpi, f)
    n, k = lb.shape
    labels, score, margin, dmax = np.zeros(n, np.int32), np.zeros(len(seq) - 1), np.full(len(seq) - 1, np.inf), np.zeros(len(seq) - 1)
    for s, (t0, t1) in enumerate(zip(seq[:-1], seq[1:])):
        T = t1 - t0
        delta, bp, gap = (lpi + lb[t0]).astype(f), np.zeros((T, k), np.int64), np.full((T, k), np.inf)
        big = float(np.abs(delta[np.isfinite(delta)]).max(initial=0.0))
        for t in range(1, T):
            cand = (delta[:, None] + lA).astype(f)
            bp[t] = cand.argmax(0)
            if k > 1:
                two = np.sort(cand, 0)[-2:]
                with np.errstate(invalid="ignore"):
                    gap[t] = np.where(np.isfinite(two[1]), two[1] - two[0], 0.0)
            delta = (lb[t0 + t] + cand.max(0)).astype(f)
            big = max(big, float(np.abs(delta[np.isfinite(delta)]).max(initial=0.0)))
        j = int(delta.argmax())
        score[s], dmax[s] = delta[j], big
        if k > 1:
            two = np.sort(delta)[-2:]
            margin[s] = two[1] - two[0]
        for t in range(T - 1, -1, -1):
            labels[t0 + t] = j
            if t > 0:
                margin[s] = min(margin[s], gap[t, j])
                j = int(bp[t, j])
    return labels, score, margin, dmax


def path_score64(logb, seq, logA, logpi, labels):
    lb, lA, lpi = (np.asarray(a, np.float64) for a in (logb, logA, logpi))
    out = np.zeros(len(seq) - 1)
    for s, (t0, t1) in enumerate(zip(seq[:-1], seq[1:])):
        p = labels[t0:t1]
        out[s] = lpi[p[0]] + lb[np.arange(t0, t1), p].sum() + lA[p[:-1], p[1:]].sum()
    return out


def emission32(x, mu, var):
    """The restatement: the kernel's chain in float32 numpy, one feature at a time (a product and a sum where the kernel has an fma)."""
    x, mu, var = f32(x), f32(mu), f32(var)
    iv = f32(1) / var
    q = np.zeros((x.shape[0], mu.shape[0]), np.float32)
    for c in range(x.shape[1]):
        v = x[:, c, None] - mu[None, :, c]
        q += v * (v * iv[None, :, c])
    cj = f32(-0.5 * np.log(2.0 * np.pi * f64(var)).sum(1))
    return f32(-0.5) * q + cj[None, :]


# ---------------------------------------------------------------------------------------------------------------- checkers
def check_emission(x, mu, var, logb, what=""):
    ref, q, c = logb64(x, mu, var)
    d = x.shape[1]
    bound = (d + 4) * U24 * 0.5 * q + 2 * U24 * np.abs(c)[None, :] + U24 * np.abs(ref)
    err = np.abs(f64(logb) - ref)
    worst = float((err / bound).max())
    print(f"[hmm {what}] emission {x.shape[0]} x {d} vs {mu.shape[0]}: worst error {worst:.3g} of its bound")
    assert logb.dtype == np.float32 and logb.shape == ref.shape
    assert (err <= bound).all()
    return worst


def check_fb(logb, seq, A, pi, out, what=""):
    gamma, xi, start, loglik, total = out
    n, k = logb.shape
    rg, rxi, rstart, rll = fb64(logb, seq, A, pi)
    T = np.diff(seq).astype(np.float64)
    rowT = np.repeat(T, np.diff(seq))
    e_ll = np.abs(loglik - rll) / (2 * T * (k + 8) * U24)
    bg = 2 * rowT[:, None] * (k + 8) * U24 * rg + TINY
    e_g = np.abs(f64(gamma) - rg) / bg
    e_sum = np.abs(f64(gamma).sum(1) - 1.0) / ((k + 2) * U24)
    bxi = 3 * T.max() * (k + 8) * U24 * rxi + TINY * n
    e_xi = np.abs(xi - rxi) / bxi
    bst = np.zeros(k)
    for s, t0 in enumerate(seq[:-1]):
        bst += 2 * T[s] * (k + 8) * U24 * rg[t0] + TINY
    e_st = np.abs(start - rstart) / bst
    worst = {"loglik": float(e_ll.max()), "gamma": float(e_g.max()), "rowsum": float(e_sum.max()), "xi": float(e_xi.max()), "start": float(e_st.max())}
    print(f"[hmm {what}] forward-backward {list(np.diff(seq))[:6]}{'...' if len(seq) > 7 else ''} x {k}: worst ratios to the bounds " +
          ", ".join(f"{key} {v:.3g}" for key, v in worst.items()))
    assert gamma.dtype == np.float32 and xi.dtype == np.float64 and start.dtype == np.float64 and loglik.dtype == np.float64
    assert all(v <= 1.0 for v in worst.values()), worst
    assert total == float(np.add.accumulate(loglik)[-1])      # the fixed-order total: in sequence order
    return worst


def check_mstep(x, gamma, mu_in, var_in, out, min_var=0.0, min_weight=0.0, what=""):
    mu, var, weight = out
    rmu, rvar, rw = mstep64(x, gamma, mu_in, var_in, min_var, min_weight)
    x64, g = np.asarray(x, np.float64), np.asarray(gamma, np.float64)
    xc = x64 - x64.mean(0)
    assert np.allclose(weight, rw, rtol=1e-12, atol=0)
    worst_mu = worst_var = 0.0
    kept = 0
    for j in range(g.shape[1]):
        if not (rw[j] >= min_weight and rw[j] > 0):
            kept += 1
            np.testing.assert_array_equal(mu[j].view(np.uint32), f32(mu_in[j]).view(np.uint32))
            np.testing.assert_array_equal(var[j].view(np.uint32), f32(var_in[j]).view(np.uint32))
            continue
        e1, e2 = (g[:, j, None] * np.abs(xc)).sum(0) / rw[j], (g[:, j, None] * xc * xc).sum(0) / rw[j]
        bmu, bvar = 2.0 ** -22 * e1 + 2.0 ** -23 * np.abs(rmu[j]), 2.0 ** -20 * e2
        worst_mu = max(worst_mu, float((np.abs(f64(mu[j]) - rmu[j]) / np.maximum(bmu, 1e-300)).max()))
        worst_var = max(worst_var, float((np.abs(f64(var[j]) - rvar[j]) / np.maximum(np.maximum(bvar, 2.0 ** -23 * rvar[j]), 1e-300)).max()))
        assert (var[j] >= f32(min_var)).all()
    print(f"[hmm {what}] M-step {x.shape[0]} x {x.shape[1]} into {g.shape[1]}: worst error {worst_mu:.3g} (means) and {worst_var:.3g} (variances) of the "
          f"bounds, {kept} states kept")
    assert mu.dtype == np.float32 and var.dtype == np.float32 and weight.dtype == np.float64
    assert worst_mu <= 1.0 and worst_var <= 1.0, (worst_mu, worst_var)
    return worst_mu, worst_var


def check_viterbi(logb, seq, A, pi, labels, path, what="", logspace=False):
    with np.errstate(divide="ignore"):
        lA, lpi = (f64(A), f64(pi)) if logspace else (np.log(f64(A)), np.log(f64(pi)))
    ref, score, margin, dmax = viterbi64(logb, seq, lA, lpi)
    T = np.diff(seq).astype(np.float64)
    tau = 4 * T * U24 * dmax
    mine = path_score64(logb, seq, lA, lpi, labels)
    sure = margin > tau
    rowsure = np.repeat(sure, np.diff(seq))
    worst = float(((score - mine) / np.maximum(tau, 1e-300)).max())
    print(f"[hmm {what}] Viterbi {list(np.diff(seq))[:6]} x {logb.shape[1]}: the path's float64 score within {worst:.3g} tau of the optimum, "
          f"{int(sure.sum())} of {len(sure)} sequences sure, {int((labels != ref)[rowsure].sum())} of their labels differ")
    assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() < logb.shape[1]
    assert (mine >= score - tau).all()
    assert (np.abs(path - mine) <= tau + 1e-300).all()
    np.testing.assert_array_equal(labels[rowsure], ref[rowsure])
    return worst


# ---------------------------------------------------------------------------------------------------------------- exact grids
@functools.lru_cache(None)
def viterbi_grid(k=6, lengths=(40, 1, 75)):
    """logb, log A and log pi multiples of 1/8 of small magnitude, two states duplicated: ties at nearly every step, every float32 sum exact."""
    r = np.random.default_rng(8)
    logb = f32(r.integers(-16, 1, (sum(lengths), k)) / 8.0)
    lA, lpi = f32(r.integers(-12, 1, (k, k)) / 8.0), f32(r.integers(-12, 1, k) / 8.0)
    logb[:, 4], lA[4], lA[:, 4], lpi[4] = logb[:, 1], lA[1], lA[:, 1], lpi[1]
    lA[2, 3] = -np.inf      # a forbidden transition
    for a in (logb, lA, lpi):
        a.setflags(write=False)
    return logb, lA, lpi, seq_of(lengths)


def check_viterbi_exact(backend):
    logb, lA, lpi, seq = viterbi_grid()
    ref, score, margin, _ = viterbi64(logb, seq, lA, lpi)
    assert (margin == 0).any()      # planted ties on the best path
    labels, path = backend.hmm_viterbi(logb, seq, lA, lpi, logspace=True)
    np.testing.assert_array_equal(labels, ref)
    np.testing.assert_array_equal(path, score)
    assert not ((labels[:-1] == 2) & (labels[1:] == 3) & (np.isin(np.arange(1, len(labels)), seq[1:-1], invert=True))).any()


def check_emission_exact(backend):
    """x and mu on an integer grid with var = 1: the quadratic form is an integer below 2^24, so logb = fma(-1/2, q, c_j) is one rounding of the
    exact value."""
    r = np.random.default_rng(6)
    x, mu = f32(r.integers(-8, 9, (300, 70))), f32(r.integers(-8, 9, (9, 70)))
    var = np.ones((9, 70), np.float32)
    ref, q, c = logb64(x, mu, var)
    assert q.max() < 2 ** 24 and (q == np.rint(q)).all()
    logb = backend.hmm_emission(backend.asarray(x), mu, var)
    want = f32(f64(f32(c))[None, :] - 0.5 * q)      # c rounded once, then one rounding of the sum
    np.testing.assert_array_equal(logb.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- properties
def soft_gamma(case):
    """The reference posteriors of a uniform-transition model over the emission case's rows, tempered by 1 / d so that several states share every
    row whatever the width, rounded to float32: a soft gamma for the M-step."""
    x, mu, var = emission_data(case)
    lb = logb64(x, mu, var)[0]
    g = np.exp((lb - lb.max(1, keepdims=True)) / x.shape[1])
    return f32(g / g.sum(1, keepdims=True))


def onehot_gamma(case):
    x, mu, var = emission_data(case)
    lab = logb64(x, mu, var)[0].argmax(1)
    g = np.zeros((case[0], case[2]), np.float32)
    g[np.arange(case[0]), lab] = 1
    return g


def check_split(backend, what=""):
    """No transition crosses a boundary: the same rows as one sequence and as two, against the reference of each."""
    _, _, _, A, pi, _, logb = seq_data(SEQ_CASES[2])
    n = logb.shape[0]
    one, two = np.asarray([0, n], np.int32), np.asarray([0, 120, n], np.int32)
    o1, o2 = backend.hmm_forward_backward(logb, one, A, pi), backend.hmm_forward_backward(logb, two, A, pi)
    check_fb(logb, one, A, pi, o1, what + ", one sequence")
    check_fb(logb, two, A, pi, o2, what + ", split in two")
    r1, r2 = fb64(logb, one, A, pi), fb64(logb, two, A, pi)
    assert abs((o1[1].sum() - o2[1].sum()) - 1.0) < 1e-4 and abs((r1[1].sum() - r2[1].sum()) - 1.0) < 1e-9      # one pair fewer
    assert abs(o2[2].sum() - 2.0) < 1e-5 and abs(o1[2].sum() - 1.0) < 1e-5


def check_zero_probability(backend):
    """A sequence whose first row no state with a positive start probability can emit: -inf and zero rows; the other sequences as alone."""
    _, _, _, A, _, _, logb = seq_data(SEQ_CASES[2])
    lb = np.array(logb[:90])
    pi = np.zeros(7, np.float32)
    pi[2] = 1.0
    lb[30, 2] = -np.inf                    # row 30 starts the second sequence
    seq = np.asarray([0, 30, 60, 90], np.int32)
    gamma, xi, start, loglik, total = backend.hmm_forward_backward(lb, seq, A, pi)
    assert loglik[1] == -np.inf and total == -np.inf and (gamma[30:60] == 0).all()
    for s, (a, b) in enumerate(((0, 30), (60, 90))):
        alone = backend.hmm_forward_backward(lb[a:b], np.asarray([0, b - a], np.int32), A, pi)
        np.testing.assert_array_equal(gamma[a:b].view(np.uint32), alone[0].view(np.uint32))
        assert loglik[2 * s] == alone[3][0]
    assert np.isfinite(xi).all() and abs(start.sum() - 2.0) < 1e-5


def check_fit_steps(backend, what=""):
    """tmjx_hmm_fit against the same steps called one by one: the same bits; with prior = kappa = 0 and a floor that never binds the loglik never
    falls by more than relative 1e-6."""
    x, mu, var, A, pi, seq, _ = seq_data(SEQ_CASES[2])
    xa = backend.asarray(x)
    mu0, var0 = f32(mu + 0.3), np.ones_like(var)
    A0, pi0 = np.full_like(A, 1.0 / 7), np.full_like(pi, 1.0 / 7)
    fit = backend.hmm_fit(xa, seq, mu0, var0, A0, pi0, 12, 0.0, 0.0, 0.0, 1e-9, 1e-3)
    info = fit[6]
    m_, v_, A_, p_, trace = mu0, var0, A0, pi0, []
    for it in range(12):
        logb = backend.hmm_emission(xa, m_, v_)
        gamma, xi, start, loglik, total = backend.hmm_forward_backward(logb, seq, A_, p_)
        trace.append(total)
        if it > 0 and total - trace[-2] <= 0.0:
            break
        m_, v_, _ = backend.hmm_mstep(xa, gamma, m_, v_, 1e-9, 1e-3)
        A_, p_ = backend.hmm_transitions(xi, start, 0.0, 0.0, A_, p_)
    else:
        logb = backend.hmm_emission(xa, m_, v_)
        gamma, xi, start, loglik, total = backend.hmm_forward_backward(logb, seq, A_, p_)
    labels, _ = backend.hmm_viterbi(logb, seq, A_, p_)
    print(f"[hmm {what}] fit: {info.n_iter} iterations, loglik {trace[0]:.6f} -> {info.loglik:.6f}")
    for a, b in zip(trace, trace[1:]):
        assert b >= a - 1e-6 * abs(a), trace
    assert info.n_iter == len(trace) and info.loglik == total
    for got, want in zip(fit[:6], (m_, v_, A_, p_, gamma, labels)):
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- model level
@functools.lru_cache(None)
def planted(sep=1.6, T=600, S=5):
    """A planted 5-state sticky chain (self-transition 0.95) with overlapping unit-variance emissions in two features, S sequences of T rows
    -> (x, lengths, true states)."""
    r = np.random.default_rng(2024)
    k = 5
    A = np.full((k, k), 0.05 / (k - 1))
    np.fill_diagonal(A, 0.95)
    ang = 2 * np.pi * np.arange(k) / k
    mu = sep * np.stack([np.cos(ang), np.sin(ang)], 1)
    z = draw_chain(r, (T,) * S, A, np.full(k, 1.0 / k))
    x = f32(mu[z] + r.standard_normal((len(z), 2)))
    x.setflags(write=False)
    return x, (T,) * S, z


def accuracy(labels, truth, k=5):
    """The share of rows labelled right under the best permutation of the states."""
    conf = np.zeros((k, k), np.int64)
    np.add.at(conf, (labels, truth), 1)
    return max(sum(conf[i, p[i]] for i in range(k)) for p in itertools.permutations(range(k))) / len(truth)


def em64(x, seq, lab0, k, prior, kappa, min_var, max_iter, tol):
    """Float64 EM with the initialisation and the loop of GaussianHMM.fit -> (labels, loglik)."""
    n = len(lab0)
    g0 = np.zeros((n, k))
    g0[np.arange(n), lab0] = 1
    mu, var, _ = mstep64(x, g0, np.zeros((k, x.shape[1])), np.ones((k, x.shape[1])), min_var, 0.5)
    trans = np.zeros((k, k))
    for t0, t1 in zip(seq[:-1], seq[1:]):
        np.add.at(trans, (lab0[t0:t1 - 1], lab0[t0 + 1:t1]), 1)
    A, pi = transitions64(trans, np.bincount(lab0[seq[:-1]], minlength=k), prior, kappa, np.full((k, k), 1 / k), np.full(k, 1 / k))
    prev = 0.0
    for it in range(max_iter):
        logb = logb64(x, mu, var)[0]
        gamma, xi, start, ll = fb64(logb, seq, A, pi)
        total = float(ll.sum())
        if it > 0 and total - prev <= tol * abs(prev):
            break
        prev = total
        mu, var, _ = mstep64(x, gamma, mu, var, min_var, 1e-3)
        A, pi = transitions64(xi, start, prior, kappa, A, pi)
    else:
        logb = logb64(x, mu, var)[0]
        total = float(fb64(logb, seq, A, pi)[3].sum())
    with np.errstate(divide="ignore"):
        return viterbi64(logb, seq, np.log(A), np.log(pi))[0], total


def check_model(backend, what=""):
    from track_mjx_amd.analysis import cluster as CL
    from track_mjx_amd.analysis import hmm as H
    x, lengths, truth = planted()
    seq = seq_of(lengths)
    hmm = H.GaussianHMM(5, max_iter=30, tol=1e-5, prior=0.1, kappa=0.0, n_init=2, seed=0, backend=backend).fit(x, lengths)
    acc_km = accuracy(hmm.init_labels_, truth)
    lab64, _ = em64(x, seq, hmm.init_labels_, 5, 0.1, 0.0, hmm.min_var_, 30, 1e-5)
    acc64, acc = accuracy(lab64, truth), accuracy(hmm.labels_, truth)
    logb = backend.hmm_emission(backend.asarray(x), hmm.means_, hmm.vars_)
    ref_ll = float(fb64(logb, seq, hmm.transmat_, hmm.startprob_)[3].sum())
    bound = float((2 * np.diff(seq) * (5 + 8) * U24).sum())
    dwell = CL.segment_summary([hmm.labels_[a:b] for a, b in zip(seq[:-1], seq[1:])], 5)[2]
    dwell0 = CL.segment_summary([hmm.init_labels_[a:b] for a, b in zip(seq[:-1], seq[1:])], 5)[2]
    print(f"[hmm {what}] planted chain: accuracy k-means {acc_km:.4f}, float64 EM {acc64:.4f}, kernel path {acc:.4f}; loglik {hmm.loglik_:.6f} against "
          f"{ref_ll:.6f} in float64 on the same logb ({abs(hmm.loglik_ - ref_ll) / bound:.3g} of the bound); mean dwell {dwell.mean():.2f} against "
          f"{dwell0.mean():.2f} at the start")
    assert acc64 >= acc_km + 0.05, "the planted data no longer separate EM from k-means"
    assert acc >= acc64 - 0.01
    assert abs(hmm.loglik_ - ref_ll) <= bound
    assert dwell.mean() > dwell0.mean()
    assert (np.diff(hmm.counts_) <= 0).all() and (np.bincount(hmm.labels_, minlength=5) == hmm.counts_).all()
    np.testing.assert_array_equal(hmm.predict(x, lengths), hmm.labels_)
    # (the states were renumbered after the fit: the sums run in another order, so not the same bits)
    assert abs(hmm.score(x, lengths) - hmm.loglik_) <= 2 * bound and abs(hmm.score_sequences(x, lengths).sum() - hmm.loglik_) <= 2 * bound
    assert np.abs(hmm.predict_proba(x, lengths) - hmm.gamma_).max() <= 2 * (2 * max(lengths) * (5 + 8) * U24 + TINY)      # each within the gamma bound


# ---------------------------------------------------------------------------------------------------------------- command line
def clip_files(tmp_path, widths=(120, 90, 100, 80), d=4, k=3):
    """A directory of four small synthetic clip_<i>.h5 with activations/intention [T, d] drawn from a sticky 3-state chain with overlapping
    emissions -> (directory, features)."""
    from track_mjx_amd import h5lite
    r = np.random.default_rng(12)
    ctr = 1.3 * r.standard_normal((k, d))
    A = np.full((k, k), 0.04)
    np.fill_diagonal(A, 0.92)
    feats = {}
    for clip, T in zip((0, 2, 5, 7), widths):
        z = draw_chain(r, (T,), A, np.full(k, 1 / k))
        feats[clip] = f32(ctr[z] + r.standard_normal((T, d)))
        h5lite.write_tree(str(tmp_path / f"clip_{clip}.h5"), {"activations": {"intention": feats[clip]}, "ctrl": np.zeros((T, 2), np.float32)})
    return str(tmp_path), feats


def check_cli(tmp_path, backend, capsys):
    """The command-line round trip: keys, shapes and dtypes, states numbered by count, the smoothing visible in the file, holdout, the file as
    intervention centroids, usage errors return 2."""
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import hmm as H
    from track_mjx_amd.analysis.intervene import Intervention
    (tmp_path / "clips").mkdir()
    rollouts, feats = clip_files(tmp_path / "clips")
    out = str(tmp_path / "out" / "hmm.h5")
    n = sum(f.shape[0] for f in feats.values())
    assert H.main([f"rollouts={rollouts}", "k=3", f"out={out}", "seed=1", "n_init=2", "posteriors=true"], backend=backend) == 0
    assert f"[hmm] intention: {n} samples x 4 features from 4 clips into 3 states" in capsys.readouterr().out
    with h5lite.File(out) as h:
        keys = ("means", "variances", "transmat", "startprob", "centroids", "loglik", "loglik_per_step_train", "n_iter", "converged", "clips", "seed", "counts",
                "transitions", "dwell_mean", "init_dwell_mean")
        got = {key: np.asarray(h[key][()]) for key in keys}
        assert "loglik_per_step_heldout" not in h
        feature = bytes(h["feature"][()])
        labels = {c: np.asarray(h["labels"][f"clip_{c}"][()]) for c in feats}
        conf = {c: np.asarray(h["confidence"][f"clip_{c}"][()]) for c in feats}
        gam = {c: np.asarray(h["gamma"][f"clip_{c}"][()]) for c in feats}
    assert feature.decode() == "intention"
    for key in ("means", "variances", "centroids"):
        assert got[key].shape == (3, 4) and got[key].dtype == np.float32
    np.testing.assert_array_equal(got["centroids"], got["means"])
    assert got["transmat"].shape == (3, 3) and np.allclose(got["transmat"].sum(1), 1, atol=1e-6) and np.isclose(got["startprob"].sum(), 1, atol=1e-6)
    assert got["counts"].dtype == np.int64 and got["counts"].sum() == n and (np.diff(got["counts"]) <= 0).all()
    assert got["transitions"].sum() == n - 4 and got["dwell_mean"].shape == (3,) and got["init_dwell_mean"].shape == (3,)
    assert got["dwell_mean"].mean() > got["init_dwell_mean"].mean()
    assert list(got["clips"]) == [0, 2, 5, 7] and int(got["seed"]) == 1 and int(got["n_iter"]) >= 1 and (got["variances"] > 0).all()
    assert np.isclose(float(got["loglik_per_step_train"]), float(got["loglik"]) / n)
    for c, f in feats.items():
        T = f.shape[0]
        assert labels[c].dtype == np.int32 and labels[c].shape == (T,) and conf[c].dtype == np.float32 and conf[c].shape == (T,)
        assert gam[c].shape == (T, 3) and np.allclose(gam[c].sum(1), 1, atol=1e-5)
        np.testing.assert_array_equal(conf[c], gam[c][np.arange(T), labels[c]])
    np.testing.assert_array_equal(np.bincount(np.concatenate([labels[c] for c in feats]), minlength=3), got["counts"])
    iv = Intervention.from_centroids(out, columns="0:2")
    assert iv.target == "intention"
    out2 = str(tmp_path / "out" / "hmm_holdout.h5")
    assert H.main([f"rollouts={rollouts}", "k=3", f"out={out2}", "holdout=2", "n_init=2"], backend=backend) == 0
    assert "2 held-out clips" in capsys.readouterr().out
    with h5lite.File(out2) as h:
        held, train = float(np.asarray(h["loglik_per_step_heldout"][()])), float(np.asarray(h["loglik_per_step_train"][()]))
        assert "gamma" not in h and list(np.asarray(h["clips"][()])) == [0, 2, 5, 7] and np.asarray(h["labels"]["clip_7"][()]).shape == (80,)
    assert np.isfinite(held) and held < 0 and abs(held - train) < 1.0
    assert H.main([f"rollouts={rollouts}", "k=3"], backend=backend) == 2                                   # no out=
    assert H.main([f"rollouts={rollouts}", "k=3", f"out={out}", "colour=red"], backend=backend) == 2       # an unknown option
    assert "usage:" in capsys.readouterr().err
    assert H.main([f"rollouts={rollouts}", "k=3", f"out={out}", "feature=decoder/layer_9"], backend=backend) == 2
    assert "decoder/layer_9" in capsys.readouterr().err
    assert H.main([f"rollouts={rollouts}", "k=3", f"out={out}", "holdout=1"], backend=backend) == 2
    assert H.main([f"rollouts={rollouts}", "k=3", f"out={out}", "kappa=-1"], backend=backend) == 2
