"""The float64 reference of the LSTM-decoder-Jacobian kernels (csrc/lstm_jacobian_core.h), the case lists and the checkers that
tests/test_lstm_jacobian_cpu.py (the host emulation) and tests/test_gpu_lstm_jacobian.py (the C-ABI) share, built by the method of
tests/jacobian_ref.py.  A `backend` is analysis.pca.HipBackend or tests/hostemu/lstm_jacobian_emu.B.

The reference (`reference64`) is the analytic reverse pass in numpy float64, in the expressions of DESIGN.md "LSTM decoder Jacobian": forward per
layer pre = W_ih x_k + W_hh h_k + b_hh, c' = sig(f) c + sig(i) tanh(g), h' = sig(o) tanh(c'), loc = Wp[:A] h'_top + bp[:A]; reverse
G = diag(1 - ctrl^2) Wp[:A], Gc = Gh sig(o) (1 - tanh(c')^2), D = [Gc tanh(g) sig'(i) | Gc c sig'(f) | Gc sig(i) (1 - tanh(g)^2) | Gh tanh(c') sig'(o)],
d / d c = Gc sig(f), d / d h = D W_hh, d / d x = D W_ih.  It is itself checked against torch.autograd.functional.jacobian of a double-precision step
built on the product's own agent.lstm._torch_lstm_layer on the CPU, with respect to the input columns, every h_k and every c_k
(check_reference_against_autograd).  Measured over CASES: the largest ||J_ref - J_autograd||_F / ||J_autograd||_F over the three Jacobians is
AUTOGRAD_GAP (a wrong formula shows at O(1)); the check holds it to 8 times that.

How every bound is derived (tests/jacobian_ref.py, tests/compare_ref.py).  Each checked array is computed twice on the test's own input: in
float64, and by `restated32`, a float32 numpy restatement of what the kernels perform: every product a chain acc = fmaf(a_k, b_k, acc) from 0 in
ascending k, pre = (xg + b) + hg, c' = (sig(f) c) + (sig(i) tanh(g)), the six kept coefficients and the backward's products in the kernels' order,
carry_gain by its 256 threads' chains and their tree, float64 where the kernels sum in float64 (groups of 32 rows in row order, the groups in
order).  The kernel and the emulation are held to TWICE the distance between the two.  The arrays that carry the same roundings form a family
(ctrl; linear in J: jac, carry_jac, mean_sum, carry_sum; quadratic in J: gain, col2, row2, action_var, gram_in, gram_out, carry_gain), each
array's distance is taken relative to its scale (the same expression on |J| in float64; 1 for ctrl), and the largest relative distance of a family
serves every array of it, times that array's scale (`within`).  Where a transcendental enters, the library's result may differ from numpy's by
its documented error (the logistic function 2^-22 relative, tanhf 2^-22): the floor that allows for it is derived, not chosen: the float64
reference is evaluated a second time with every logistic value and every tanh (the gates', tanh(c'), ctrl) multiplied by 1 + delta, delta =
+- 2^-22 with seeded random signs, and the floor of an array is the largest absolute change that makes in it.  Quantities that are exact by
construction are compared with == or bit for bit."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.jacobian_ref import CHUNK, SUM_ROWS, bits, chain, f32, f64, fma, lane_sums, same_bits  # noqa: F401
from tests.jacobian_ref import outputs_of as input_outputs_of
from track_mjx_amd import hip

AUTOGRAD_GAP = 8.0e-15
# (m, d_in, (wrt_col0, wrt_cols), H, L, A, ldx: None = dense, ld_carry: None = dense)
CASES = ((1, 1, (0, 1), 32, 1, 1, None, None),
         (3, 5, (0, 2), 32, 1, 1, None, None),
         (CHUNK + 1, 7, (0, 3), 32, 2, 5, None, None),            # one row more than a pass; in_0 != H catches a transposed weight or a wrong stride
         (5, 286, (0, 60), 128, 2, 38, 291, 2 * 128 + 3),         # the shipped shape with row strides
         (3, 286, (60, 128), 256, 4, 38, None, None),             # the H, L and wrt limits, wrt off column 0
         (2, 64, (0, 64), 64, 3, 64, None, None))                 # the A limit
INPUT_ARRAYS = ("ctrl", "jac", "gain", "col2", "row2", "action_var", "mean_sum", "gram_in", "gram_out")
ARRAYS = INPUT_ARRAYS + ("carry_jac", "carry_gain", "carry_sum")
PER_ROW = ("ctrl", "jac", "gain", "col2", "row2", "action_var", "carry_jac", "carry_gain")
WANT = ("ctrl", "jac", "gain", "col2", "row2", "carry_jac", "carry_gain")


# ---------------------------------------------------------------------------------------------------------------- the problems
class Net:
    """layers [(W_ih [4H, in_k], W_hh [4H, H], b_hh [4H])], the projection (wp [2A, H], bp [2A]) and A, L, H, float32."""

    def __init__(self, d_in, H, L, A, seed):
        rng = np.random.default_rng(seed)
        self.layers, K = [], d_in
        for _ in range(L):      # LeCun-scaled kernels, biases N(0, 1/4): the conditioning of a trained net
            self.layers.append([(rng.standard_normal((4 * H, K)) / np.sqrt(K)).astype(f32), (rng.standard_normal((4 * H, H)) / np.sqrt(H)).astype(f32),
                                (0.5 * rng.standard_normal(4 * H)).astype(f32)])
            K = H
        self.wp, self.bp = (rng.standard_normal((2 * A, H)) / np.sqrt(H)).astype(f32), rng.standard_normal(2 * A).astype(f32)
        self.A, self.L, self.H, self.d_in = A, L, H, d_in

    @property
    def head(self):
        return self.wp, self.bp, self.A


def _slice_of(values, ld):
    """`values` as a column slice of a buffer `ld` wide (None: dense) filled with 1e6."""
    if ld is None:
        return np.ascontiguousarray(values, f32)
    buf = np.full((values.shape[0], ld), 1e6, f32)
    off = (ld - values.shape[1]) // 2
    buf[:, off:off + values.shape[1]] = values
    return buf[:, off:off + values.shape[1]]


@functools.lru_cache(None)
def problem(case):
    """-> (net, x [m, d_in], h [m, L H], c [m, L H] (column slices of wider buffers where the case has row strides), scale [m, wrt_cols],
    carry_scale [2 L H]), float32, read-only."""
    m, d_in, (c0, Z), H, L, A, ldx, ldc = case
    net = Net(d_in, H, L, A, 200 + CASES.index(case) if case in CASES else 199)
    rng = np.random.default_rng(11)
    x = _slice_of(rng.standard_normal((m, d_in)), ldx)
    h = _slice_of(np.clip(0.5 * rng.standard_normal((m, L * H)), -0.99, 0.99), ldc)      # (a carried h is sig(o) tanh(c'): inside (-1, 1))
    c = _slice_of(rng.standard_normal((m, L * H)), ldc)
    scale = np.exp(0.5 * (-2.0 + 0.5 * rng.standard_normal((m, Z)))).astype(f32)
    carry_scale = np.exp(0.5 * rng.standard_normal(2 * L * H)).astype(f32)
    for a in (x, h, c, scale, carry_scale, *[t for layer in net.layers for t in layer], net.wp, net.bp):
        a.setflags(write=False)
    return net, x, h, c, scale, carry_scale


# ---------------------------------------------------------------------------------------------------------------- float64
def outputs_of(ctrl, J, CJ, scale, carry_scale, L):
    out = input_outputs_of(ctrl, J, scale)
    m, A, W = CJ.shape
    t = CJ if carry_scale is None else CJ * np.asarray(carry_scale, f64)
    out.update({"carry_jac": CJ, "carry_gain": (t * t).reshape(m, A, 2 * L, W // (2 * L)).sum((1, 3)), "carry_sum": CJ.sum(0)})
    return out


def reference64(net, x, h, c, wrt, mode, scale=None, carry_scale=None, rel=None):
    """The analytic Jacobians and everything the call returns, float64.  `rel`: the relative perturbation of every logistic value and every tanh,
    with seeded random signs, for the floors."""
    return outputs_of(*jacobians64(net, x, h, c, wrt, mode, rel), scale, carry_scale, net.L)


def jacobians64(net, x, h, c, wrt, mode, rel=None):
    """-> (ctrl [m, A], J [m, A, Z], CJ [m, A, 2 L H]) float64."""
    c0, Z = wrt
    A, L, H = net.A, net.L, net.H
    rng = np.random.default_rng(5)
    jig = (lambda v: v * (1.0 + rel * rng.choice((-1.0, 1.0), v.shape))) if rel is not None else (lambda v: v)
    sig = lambda v: jig(1.0 / (1.0 + np.exp(-v)))      # noqa: E731
    tanh = lambda v: np.clip(jig(np.tanh(v)), -1.0, 1.0)      # noqa: E731
    xk, hh, cc, kept = np.asarray(x, f64), np.asarray(h, f64), np.asarray(c, f64), []
    for k, (wi, wh, b) in enumerate(net.layers):
        hk, ck = hh[:, k * H:(k + 1) * H], cc[:, k * H:(k + 1) * H]
        pre = xk @ wi.astype(f64).T + hk @ wh.astype(f64).T + b
        gi, gf, gg, go = sig(pre[:, :H]), sig(pre[:, H:2 * H]), tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
        tc = tanh(gf * ck + gi * gg)
        kept.append((gi, gf, gg, go, tc, ck))
        xk = go * tc
    wp = net.wp[:A].astype(f64)
    ctrl = tanh(xk @ wp.T + net.bp[:A])
    g = np.broadcast_to(wp[None], (x.shape[0], *wp.shape)).copy()
    if mode == 0:
        g *= (1.0 - ctrl * ctrl)[:, :, None]
    CJ = np.zeros((x.shape[0], A, 2 * L * H))
    for k in range(L - 1, -1, -1):
        wi, wh, _ = net.layers[k]
        gi, gf, gg, go, tc, ck = (v[:, None] for v in kept[k])
        gc = g * go * (1.0 - tc * tc)
        d = np.concatenate([gc * gg * gi * (1.0 - gi), gc * ck * gf * (1.0 - gf), gc * gi * (1.0 - gg * gg), g * tc * go * (1.0 - go)], 2)
        CJ[:, :, (L + k) * H:(L + k + 1) * H] = gc * gf
        CJ[:, :, k * H:(k + 1) * H] = d @ wh.astype(f64)
        g = d @ (wi[:, c0:c0 + Z] if k == 0 else wi).astype(f64)
    return ctrl, g, CJ


# ---------------------------------------------------------------------------------------------------------------- the float32 restatement
def restated32(net, x, h, c, wrt, mode, scale=None, carry_scale=None):
    return restated32_outputs(*restated32_jacobians(net, x, h, c, wrt, mode), scale, carry_scale, net.L)


def restated32_jacobians(net, x, h, c, wrt, mode):
    """-> (ctrl [m, A], J [m, A, Z], CJ [m, A, 2 L H]) float32, in the kernels' order."""
    c0, Z = wrt
    A, L, H, one = net.A, net.L, net.H, f32(1)
    sig = lambda v: one / (one + np.exp(-v))      # noqa: E731
    xk, hh, cc, kept = np.asarray(x, f32), np.asarray(h, f32), np.asarray(c, f32), []
    for k, (wi, wh, b) in enumerate(net.layers):
        hk, ck = hh[:, k * H:(k + 1) * H], cc[:, k * H:(k + 1) * H]
        pre = (chain(xk, wi.T) + b) + chain(hk, wh.T)
        gi, gf, gg, go = sig(pre[:, :H]), sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
        tc = np.tanh((gf * ck) + (gi * gg))
        kept.append((go * fma(-tc, tc, one), gg * (gi * (one - gi)), ck * (gf * (one - gf)), gi * fma(-gg, gg, one), tc * (go * (one - go)), gf))
        xk = go * tc
    wp = net.wp[:A]
    ctrl = np.tanh(chain(xk, wp.T) + net.bp[:A])
    dd = fma(-ctrl, ctrl, one) if mode == 0 else np.ones_like(ctrl)
    g = (dd[:, :, None] * wp[None]).reshape(-1, H)
    m = x.shape[0]
    CJ = np.zeros((m * A, 2 * L * H), f32)
    for k in range(L - 1, -1, -1):
        wi, wh, _ = net.layers[k]
        ka, ki, kf, kg, ko, gf = (np.repeat(v, A, 0) for v in kept[k])
        gc = g * ka
        d = np.concatenate([gc * ki, gc * kf, gc * kg, g * ko], 1)
        CJ[:, (L + k) * H:(L + k + 1) * H] = gc * gf
        CJ[:, k * H:(k + 1) * H] = chain(d, wh)
        g = chain(d, wi[:, c0:c0 + Z] if k == 0 else wi)
    return ctrl, g.reshape(m, A, Z), CJ.reshape(m, A, 2 * L * H)


def restated32_outputs(ctrl, J, CJ, scale, carry_scale, L):
    """The outputs of a row and the sums from the float32 Jacobians, in the kernels' order."""
    (m, A, Z), H = J.shape, CJ.shape[2] // (2 * L)
    out = {"ctrl": ctrl, "jac": J, "carry_jac": CJ}
    row2, col2, av = np.zeros((m, A), f32), np.zeros((m, Z), f32), np.zeros((m, A), f32)
    for j in range(Z):
        row2 = fma(J[:, :, j], J[:, :, j], row2)
        if scale is not None:
            t = J[:, :, j] * scale[:, j:j + 1]
            av = fma(t, t, av)
    for a in range(A):
        col2 = fma(J[:, a], J[:, a], col2)
    gain = np.zeros(m, f32)
    for a in range(A):
        gain = gain + row2[:, a]
    out.update({"gain": gain, "col2": col2, "row2": row2})
    if scale is not None:
        out["action_var"] = av
    cg = np.zeros((m, 2 * L), f32)
    for b in range(2 * L):      # thread t folds the elements t, t + 256, ... of the block's [A, H] in order; then the tree
        t = CJ[:, :, b * H:(b + 1) * H]
        if carry_scale is not None:
            t = t * carry_scale[b * H:(b + 1) * H]
        cg[:, b] = lane_sums([np.ascontiguousarray(t).reshape(m, A * H)], 256, lambda acc, v: fma(v, v, acc))[:, 0]
    out["carry_gain"] = cg
    gi_, go_ = np.zeros((m, Z, Z), f32), np.zeros((m, A, A), f32)
    for a in range(A):
        gi_ = fma(J[:, a, :, None], J[:, a, None, :], gi_)
    for j in range(Z):
        go_ = fma(J[:, :, None, j], J[:, None, :, j], go_)
    for name, per_row in (("mean_sum", J), ("gram_in", gi_), ("gram_out", go_), ("carry_sum", CJ)):
        total = np.zeros(per_row.shape[1:], f64)
        for i0 in range(0, m, SUM_ROWS):
            total = total + np.cumsum(per_row[i0:i0 + SUM_ROWS].astype(f64), 0)[-1]      # (cumsum adds in row order)
        out[name] = total
    return out


@functools.lru_cache(None)
def _jacobians(case, mode):
    """The three sets of Jacobians of a case (float64, the float32 restatement, float64 with the perturbed transcendentals), computed once."""
    net, x, h, c, _, _ = problem(case)
    return (jacobians64(net, x, h, c, case[2], mode), restated32_jacobians(net, x, h, c, case[2], mode),
            jacobians64(net, x, h, c, case[2], mode, rel=2.0 ** -22))


@functools.lru_cache(None)
def references(case, mode, scaled=True):
    """-> (float64, the float32 restatement, the floors) of a case, computed once; `scaled`: with scale and carry_scale."""
    net, _, _, _, scale, cs = problem(case)
    if not scaled:
        scale = cs = None
    j64, j32, jjig = _jacobians(case, mode)
    r64, r32, jig = outputs_of(*j64, scale, cs, net.L), restated32_outputs(*j32, scale, cs, net.L), outputs_of(*jjig, scale, cs, net.L)
    return r64, r32, {k: float(np.abs(jig[k] - r64[k]).max()) for k in r64}


FAMILIES = (("ctrl",), ("jac", "carry_jac", "mean_sum", "carry_sum"),
            ("gain", "col2", "row2", "action_var", "gram_in", "gram_out", "carry_gain"))      # value, linear in J, quadratic in J


def within(got, r64, r32, floors, L, carry_scale, what):
    """Every array of `got` against the references, family by family (the module's text): |got - r64| <= (2 gap + floor) scale elementwise-max, with
    gap and floor the family's largest relative distance and floor and scale the array's magnitude; prints the figures."""
    J, CJ = np.abs(r64["jac"]), np.abs(r64["carry_jac"])
    mags = outputs_of(np.ones_like(r64["ctrl"]), J, CJ, None if "action_var" not in r64 else np.ones((J.shape[0], J.shape[2])), carry_scale, L)
    scale = {k: float(v.max()) for k, v in mags.items()}
    if "action_var" in r64:
        scale["action_var"] = float(r64["action_var"].max())
    for fam in FAMILIES:
        live = [k for k in fam if k in r64 and scale[k] > 0.0]
        gap = max([float(np.abs(np.asarray(r32[k], f64) - r64[k]).max()) / scale[k] for k in live], default=0.0)
        floor = max([floors[k] / scale[k] for k in live], default=0.0)
        for k in [k for k in fam if k in got]:
            err = float(np.abs(np.asarray(got[k], f64) - r64[k]).max())
            bound = (2.0 * gap + floor) * scale[k]
            print(f"[lstm jacobian {what} {k}] error {err:.3g}; the family's float32-float64 gap {gap:.3g} and transcendental floor {floor:.3g} of the scale "
                  f"{scale[k]:.3g}: {err / bound if err else 0.0:.3g} of the bound")
            assert np.isfinite(np.asarray(got[k], f64)).all() and err <= bound, (what, k, err, bound)


# ---------------------------------------------------------------------------------------------------------------- the calls
def run(backend, net, x, h, c, wrt, mode=0, scale=None, carry_scale=None, row_index=None, want=WANT):
    return backend.lstm_decoder_jacobian(backend.asarray(x), backend.asarray(h), backend.asarray(c), net.layers, net.head, wrt, row_index,
                                         None if scale is None else backend.asarray(scale), carry_scale, mode, want)


def check_case(case, backend, what=""):
    """Every output of both modes against the references, with and without scale / carry_scale; the call without the carry outputs (and without
    jac) gives the same bits in every other output; the consistency of the sums with the stored Jacobians."""
    net, x, h, c, scale, cs = problem(case)
    m, _, wrt, H, L, A, _, _ = case
    Z = wrt[1]
    for mode in (0, 1):
        for scaled in (False, True):
            r64, r32, floors = references(case, mode, scaled)
            got = run(backend, net, x, h, c, wrt, mode, scale if scaled else None, cs if scaled else None)
            assert set(got) == set(ARRAYS) - (set() if scaled else {"action_var"})
            within(got, r64, r32, floors, L, cs if scaled else None, f"{what} case {CASES.index(case)} mode {mode}{'' if scaled else ' unscaled'}")
        lean = run(backend, net, x, h, c, wrt, mode, scale, cs, want=("ctrl", "gain", "col2", "row2"))
        assert "jac" not in lean and "carry_jac" not in lean and "carry_gain" not in lean
        assert all(same_bits(lean[k], got[k]) for k in lean), "the call without jac and the carry outputs changed another output"
        half = run(backend, net, x, h, c, wrt, mode, scale, None, want=("ctrl", "jac", "gain", "col2", "row2", "carry_jac"))
        assert all(same_bits(half[k], got[k]) for k in half), "the call without carry_gain changed another output"
        # the sums are the float64 sums of the stored Jacobians: an element itself is exact up to the float64 additions over the rows
        for k, stored in (("mean_sum", got["jac"]), ("carry_sum", got["carry_jac"])):
            bound = m * 2.0 ** -52 * np.abs(stored.astype(f64)).sum(0)
            assert (np.abs(got[k] - stored.astype(f64).sum(0)) <= bound).all(), k
        # carry_gain sums to the squared norm of the scaled carry Jacobian: A H non-negative terms a block, float32 chains and a tree
        t = got["carry_jac"].astype(f64) * cs.astype(f64)
        total = (t * t).reshape(m, A, 2 * L, H).sum((1, 3))
        assert (np.abs(got["carry_gain"].astype(f64) - total) <= 2.0 * (A * H // 256 + 10 + 2) * 2.0 ** -24 * total).all()


PROPERTY_CASE = (6, 9, (2, 4), 32, 2, 3, None, None)


def _variant(net, **change):
    """A copy of `net` with parts replaced: wp=, bp=, or w_hh=(layer, values)."""
    v = Net.__new__(Net)
    v.layers, v.wp, v.bp, v.A, v.L, v.H, v.d_in = [list(layer) for layer in net.layers], net.wp, net.bp, net.A, net.L, net.H, net.d_in
    for k, val in change.items():
        if k == "w_hh":
            v.layers[val[0]][1] = val[1]
        else:
            setattr(v, k, val)
    return v


def check_properties(backend, strided, what=""):
    """The properties that hold exactly.  `strided(a)`: the backend's array of a's values as a column slice of a wider buffer."""
    net, x, h, c, scale, cs = problem(PROPERTY_CASE)
    m, d_in, wrt, H, L, A, _, _ = PROPERTY_CASE
    go = lambda n=net, mode=0, **kw: run(backend, n, kw.pop("x", x), kw.pop("h", h), kw.pop("c", c), wrt, mode, kw.pop("scale", scale), cs, **kw)      # noqa: E731
    base = go()
    assert np.abs(base["jac"]).min() > 0 and np.abs(base["carry_jac"]).min() > 0
    # a zero row of the projection: a zero row of both Jacobians, the other rows as they were
    wp = net.wp.copy()
    wp[1] = 0
    got = go(_variant(net, wp=wp))
    assert (got["jac"][:, 1] == 0).all() and (got["carry_jac"][:, 1] == 0).all() and (got["row2"][:, 1] == 0).all()
    assert same_bits(got["jac"][:, 0], base["jac"][:, 0]) and same_bits(got["carry_jac"][:, 2], base["carry_jac"][:, 2])
    # |loc| > 20: tanh is exactly +-1 in float32, the mode-0 rows exactly 0 and finite, the mode-1 rows not
    bp = net.bp.copy()
    bp[0], bp[2] = 60.0, -60.0
    sat = _variant(net, bp=bp)
    g0, g1 = go(sat), go(sat, 1)
    assert (np.abs(g0["ctrl"][:, (0, 2)]) == 1).all() and (g0["jac"][:, (0, 2)] == 0).all() and (g0["carry_jac"][:, (0, 2)] == 0).all()
    assert np.isfinite(g0["jac"]).all() and np.isfinite(g0["carry_jac"]).all() and (g1["jac"][:, (0, 2)] != 0).all() and (g1["carry_jac"][:, (0, 2)] != 0).all()
    assert np.abs(g0["jac"][:, 1]).min() > 0 and same_bits(g0["ctrl"], g1["ctrl"])
    # W_hh[k] = 0: d out / d h_k is exactly 0, the other blocks are not
    for k in range(L):
        got = go(_variant(net, w_hh=(k, np.zeros((4 * H, H), f32))))
        blocks = got["carry_jac"].reshape(m, A, 2 * L, H)
        assert (blocks[:, :, k] == 0).all() and (got["carry_gain"][:, k] == 0).all() and (got["carry_sum"].reshape(A, 2 * L, H)[:, k] == 0).all(), k
        assert all(np.abs(blocks[:, :, b]).min() > 0 for b in range(2 * L) if b != k), k
    # a permuted list with a repeated entry permutes and repeats the per-row outputs; no list = arange
    idx = np.array([3, 0, 0, 5, 2, 4, 1, 3], np.int32)
    perm = go(row_index=idx)
    for k in PER_ROW:
        assert same_bits(perm[k], base[k][idx]), k
    ar = go(row_index=np.arange(m, dtype=np.int32))
    assert all(same_bits(ar[k], base[k]) for k in ARRAYS)
    # two calls, and dense against strided rows: the same bits in every output, the sums included
    again, wide = go(), go(x=strided(x), h=strided(h), c=strided(c), scale=strided(scale))
    assert all(same_bits(again[k], base[k]) and same_bits(wide[k], base[k]) for k in ARRAYS)
    # a row alone is the row in the middle of the call
    alone = go(row_index=np.array([4], np.int32))
    assert all(same_bits(alone[k][0], base[k][4]) for k in PER_ROW)
    # an index outside 0 .. n - 1 gives the outputs of a zero row with a zero carry (and no scale: action_var 0), the rows beside it as they were
    zero = go(x=np.zeros((1, d_in), f32), h=np.zeros((1, L * H), f32), c=np.zeros((1, L * H), f32), scale=scale[:1])
    for bad in (m, -1, 2 ** 31 - 1):
        out = go(row_index=np.array([1, bad, 2], np.int32))
        assert all(same_bits(out[k][1], zero[k][0]) for k in PER_ROW if k != "action_var") and (out["action_var"][1] == 0).all(), bad
        assert all(same_bits(out[k][(0, 2),], base[k][(1, 2),]) for k in PER_ROW), bad


def check_rows_across_passes(backend):
    """Row CHUNK (the first of the second pass), the row before it and row 0 of the case with one row more than a pass, each alone, give the bits
    they have in the whole call."""
    case = CASES[2]
    net, x, h, c, scale, cs = problem(case)
    full = run(backend, net, x, h, c, case[2], 0, scale, cs)
    for i in (0, CHUNK - 1, CHUNK):
        one = run(backend, net, x, h, c, case[2], 0, scale, cs, row_index=np.array([i], np.int32))
        assert all(same_bits(one[k][0], full[k][i]) for k in PER_ROW), i


# ---------------------------------------------------------------------------------------------------------------- autograd
def torch_step64(net, mode):
    """(x [d_in], h [L, H], c [L, H]) -> ctrl or loc [A]: one double-precision step on agent.lstm._torch_lstm_layer."""
    import torch
    from track_mjx_amd.agent.lstm import _torch_lstm_layer
    layers = [[torch.from_numpy(np.asarray(t, f64)) for t in layer] for layer in net.layers]
    wp, bp = torch.from_numpy(net.wp[:net.A].astype(f64)), torch.from_numpy(net.bp[:net.A].astype(f64))

    def step(xv, hv, cv):
        xk = xv[None]
        for k, (wi, wh, b) in enumerate(layers):
            xk = _torch_lstm_layer((xk @ wi.t())[None], wh, b, hv[k][None], cv[k][None], None)[0][0]
        loc = xk[0] @ wp.t() + bp
        return torch.tanh(loc) if mode == 0 else loc
    return step


def check_reference_against_autograd():
    import torch
    worst = 0.0
    for case in CASES:
        net, x, h, c, _, _ = problem(case)
        m, d_in, (c0, Z), H, L, A, _, _ = case
        for mode in (0, 1):
            r64 = reference64(net, x, h, c, (c0, Z), mode)
            step = torch_step64(net, mode)
            for i in range(min(m, 3)):
                args = (torch.from_numpy(np.asarray(x[i], f64)), torch.from_numpy(np.asarray(h[i], f64).reshape(L, H)), torch.from_numpy(np.asarray(c[i], f64).reshape(L, H)))
                jx, jh, jc = (t.numpy() for t in torch.autograd.functional.jacobian(step, args))
                for mine, auto in ((r64["jac"][i], jx[:, c0:c0 + Z]), (r64["carry_jac"][i][:, :L * H], jh.reshape(A, L * H)),
                                   (r64["carry_jac"][i][:, L * H:], jc.reshape(A, L * H))):
                    worst = max(worst, float(np.linalg.norm(mine - auto)) / float(np.linalg.norm(auto)))
    print(f"[lstm jacobian] the analytic float64 reference against torch autograd: largest relative difference {worst:.3g} (recorded {AUTOGRAD_GAP})")
    assert worst <= 8 * AUTOGRAD_GAP and worst < 1e-9


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, alloc, ptr, untouched, what=""):
    """Every limit exceeded by one and every condition of include/tmjx.h returns TMJX_EINVAL (-22) and writes nothing; the workspace entry and the
    call agree on the descriptor's limits.  The pointers of the descriptor are a dummy address: a refused call never reads them."""
    a = 1 << 20
    sums, ws, outs = alloc((64,), f64, -7.25), alloc((4096,), f32, -7.25), alloc((4096,), f32, -7.25)
    floats = C.c_int64(0)

    def desc(L=2, H=32, d_in=9, A=3, wrt=(2, 4), ldwi=None, ldwh=None, ldwp=None, null=None):
        d = hip.LstmJacobianDesc()
        d.L, d.H, d.d_in, d.A, d.wrt_col0, d.wrt_cols = L, H, d_in, A, wrt[0], wrt[1]
        K = d_in
        for k in range(min(max(L, 0), 4)):
            y = d.layer[k]
            y.W_ih, y.W_hh, y.b_hh = a, a, a
            y.ldwi, y.ldwh = K if ldwi is None or ldwi[0] != k else ldwi[1], H if ldwh is None or ldwh[0] != k else ldwh[1]
            K = H
        d.Wp, d.bp, d.ldwp = a, a, H if ldwp is None else ldwp
        if null is not None:
            setattr(d.layer[0] if null in ("W_ih", "W_hh", "b_hh") else d, null, None)
        return d

    def call(d, x=a, n=6, ldx=9, h_in=a, c_in=a, ld_carry=64, row_index=None, m=6, scale=None, ld_scale=4, carry_scale=None, mode=0, action_var=None, sums_=None,
             ws_=None, carry_jac=None):
        o = ptr(outs)
        return lib.tmjx_lstm_decoder_jacobian(None if d is None else C.byref(d), x, n, ldx, h_in, c_in, ld_carry, row_index, m, scale, ld_scale, carry_scale, mode, o, None,
                                              o, None, None, action_var, o if carry_jac is None else carry_jac, o, ptr(sums) if sums_ is None else sums_,
                                              ptr(ws) if ws_ is None else ws_, None)
    assert lib.tmjx_lstm_jacobian_workspace(C.byref(desc()), 6, C.byref(floats)) == 0 and floats.value > 0
    assert lib.tmjx_lstm_jacobian_workspace(C.byref(desc(L=4, H=256, A=64, wrt=(896, 128), d_in=1024)), 6, C.byref(floats)) == 0      # the limits themselves
    bad_desc = (desc(L=0), desc(L=5), desc(H=0), desc(H=48), desc(H=16), desc(H=512), desc(A=0), desc(A=65), desc(wrt=(2, 0)), desc(wrt=(0, 129), d_in=200),
                desc(wrt=(6, 4)), desc(wrt=(-1, 4)), desc(d_in=0), desc(d_in=1025), desc(ldwi=(0, 8)), desc(ldwi=(1, 31)), desc(ldwh=(0, 31)), desc(ldwh=(1, 31)),
                desc(ldwp=31), *[desc(null=k) for k in ("W_ih", "W_hh", "b_hh", "Wp", "bp")])
    for i, d in enumerate(bad_desc):
        assert lib.tmjx_lstm_jacobian_workspace(C.byref(d), 6, C.byref(floats)) == -22 and lib.tmjx_last_error(), (what, i)
        assert call(d) == -22 and lib.tmjx_last_error(), (what, i)
    assert lib.tmjx_lstm_jacobian_workspace(C.byref(desc()), 0, C.byref(floats)) == -22 and lib.tmjx_lstm_jacobian_workspace(C.byref(desc()), 6, None) == -22
    assert lib.tmjx_lstm_jacobian_workspace(None, 6, C.byref(floats)) == -22
    good = desc()
    bad_call = (dict(d=None), dict(x=None), dict(h_in=None), dict(c_in=None), dict(sums_=0), dict(ws_=0), dict(ldx=8), dict(ld_carry=63), dict(m=0), dict(n=0),
                dict(m=7), dict(mode=2), dict(mode=-1), dict(action_var=a), dict(scale=a, ld_scale=3), dict(ws_=ptr(ws) + 4), dict(sums_=ptr(sums) + 4),
                dict(x=a + 2), dict(h_in=a + 1), dict(c_in=a + 2), dict(carry_scale=a + 2), dict(carry_jac=ptr(outs) + 2))
    for kw in bad_call:
        d = kw.pop("d", good)
        assert call(d, **kw) == -22 and lib.tmjx_last_error(), (what, kw)
    assert untouched(sums, -7.25) and untouched(ws, -7.25) and untouched(outs, -7.25), f"{what}: a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------- the tool
TOOL_ROWS = (7, 9, 4)
TOOL_ALIGNED = (1, 4)      # clip 1 ends step 4 with a re-alignment: step 5 starts from a zero carry


def tool_policy(seed=0, latents=6, prop=8, H=32, L=2, A=5):
    """A seeded LSTMDecoderPolicy on the CPU without a normaliser (its input's proprioceptive columns are the normalised ones the roll-out records)."""
    import torch
    from track_mjx_amd.agent.checkpoint import LSTMDecoderPolicy
    net = Net(latents + prop, H, L, A, 300 + seed)
    t = lambda a: torch.from_numpy(np.array(a))      # noqa: E731
    return LSTMDecoderPolicy([t(y[0]) for y in net.layers], [t(y[1]) for y in net.layers], [t(y[2]) for y in net.layers], t(net.wp), t(net.bp), None, None, latents, 12)


def tool_clips(root, pol, rows=TOOL_ROWS, hidden_state=True, egocentric_obs=True, replay=False):
    """clip_<i>.h5 files as an LSTM roll-out with log_decoder_input=true writes them: the decoder's input rows, the carry AFTER every step and the ctrl
    this policy gives when it is stepped through the clip in float32 torch on the CPU, the carry zeroed behind the TOOL_ALIGNED step."""
    import torch
    from track_mjx_amd.analysis.utils import save_to_h5py
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(3)
    Z, P, A, L, H = pol.latent_size, pol.proprioceptive_obs_size, pol.action_size, pol.hidden_layer_num, pol.hidden_state_size
    for cl, T in enumerate(rows):
        z, prop = rng.standard_normal((T, Z)).astype(f32), rng.standard_normal((T, P)).astype(f32)
        aligned = np.zeros(T, bool)
        if cl == TOOL_ALIGNED[0]:
            aligned[TOOL_ALIGNED[1]] = True
        carry, ctrl, hs, cs = pol.zero_carry(1, "cpu"), [], [], []
        for t in range(T):
            if t > 0 and aligned[t - 1]:
                carry = pol.zero_carry(1, "cpu")
            lg, carry = pol.logits(torch.from_numpy(np.concatenate([z[t], prop[t]])[None]), carry)
            ctrl.append(torch.tanh(lg[0, :A]).numpy()); hs.append(carry[0][0].numpy().copy()); cs.append(carry[1][0].numpy().copy())
        acts = {"intention": z, "encoder": {"logvar": (-2.0 + 0.5 * rng.standard_normal((T, Z))).astype(f32)}}
        if egocentric_obs:
            acts["egocentric_obs"] = prop
        if hidden_state:
            acts["hidden_state"] = (np.stack(hs), np.stack(cs))
        tree = {"ctrl": np.stack(ctrl), "activations": acts, "meta": {"clip_idx": np.int64(cl), "seed": np.int64(42), "model": "lstm"}}
        if cl == TOOL_ALIGNED[0]:
            tree["aligned"] = aligned
        if replay:
            tree["meta"]["replay_latents"] = "somewhere"
        save_to_h5py(os.path.join(root, f"clip_{cl}.h5"), tree)
    return root


def tool_inputs(rollouts, rows=TOOL_ROWS):
    """-> (x [n, d_in], h_in, c_in [n, L H], scale [n, Z]) of the clips as the tool must place them: the carry entering step t is the recorded one of
    row t - 1, zeros at t = 0 and behind the aligned step (restated here, independently of the tool)."""
    from track_mjx_amd.analysis.utils import load_from_h5py
    xs, hs, cs, lv = [], [], [], []
    for cl in range(len(rows)):
        r = load_from_h5py(os.path.join(rollouts, f"clip_{cl}.h5"))
        a = r["activations"]
        xs.append(np.concatenate([a["intention"], a["egocentric_obs"]], 1))
        lv.append(a["encoder"]["logvar"])
        for dst, rec in ((hs, a["hidden_state"][0]), (cs, a["hidden_state"][1])):
            rec = np.asarray(rec, f32).reshape(rec.shape[0], -1)
            ent = np.concatenate([np.zeros_like(rec[:1]), rec[:-1]], 0)
            if cl == TOOL_ALIGNED[0]:
                ent[TOOL_ALIGNED[1] + 1] = 0.0
            dst.append(ent)
    cat = lambda v: np.ascontiguousarray(np.concatenate(v, 0), f32)      # noqa: E731
    return cat(xs), cat(hs), cat(cs), np.exp(0.5 * np.concatenate(lv, 0).astype(f64)).astype(f32)


def run_tool(tmp, backend, extra=(), pol=None, name="jacobian.h5", rollouts=None):
    from track_mjx_amd.analysis import jacobian as JT
    from track_mjx_amd.analysis.utils import load_from_h5py
    pol = tool_policy() if pol is None else pol
    rollouts = tool_clips(os.path.join(tmp, "rollouts"), pol) if rollouts is None else rollouts
    out = os.path.join(tmp, name)
    rc = JT.main([f"rollouts={rollouts}", f"out={out}", *extra], backend=backend, policy=pol)
    return rc, (load_from_h5py(out) if rc == 0 else None), pol, rollouts


def check_tool(tmp_path, backend, capsys):
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import jacobian as JT
    from track_mjx_amd.analysis import pca as PCA
    from track_mjx_amd.analysis.utils import load_from_h5py
    tmp = str(tmp_path)
    n, A, Z, L, H = sum(TOOL_ROWS), 5, 6, 2, 32
    W = 2 * L * H
    labels = os.path.join(tmp, "clusters.h5")
    lab = [np.arange(T) % 2 for T in TOOL_ROWS]
    h5lite.write_tree(labels, {"labels": {f"clip_{c}": v.astype(np.int32) for c, v in enumerate(lab)}})
    feat = os.path.join(tmp, "jac_dir")
    rc, f, pol, rollouts = run_tool(tmp, backend, ("store=true", f"labels={labels}", f"features_out={feat}"))
    assert rc == 0 and "forward mismatch" in capsys.readouterr().out
    cat = lambda k: np.concatenate([f[k][f"clip_{c}"] for c in range(3)], 0)      # noqa: E731
    for c, T in enumerate(TOOL_ROWS):      # every dataset with its shape
        assert f["gain"][f"clip_{c}"].shape == (T,) and f["latent_sensitivity"][f"clip_{c}"].shape == (T, Z) and f["actuator_sensitivity"][f"clip_{c}"].shape == (T, A)
        assert f["action_var"][f"clip_{c}"].shape == (T, A) and f["jacobian"][f"clip_{c}"].shape == (T, A, Z)
        assert f["memory_sensitivity"][f"clip_{c}"].shape == (T, 2 * L) and f["carry_jacobian"][f"clip_{c}"].shape == (T, A, W)
        assert np.isfinite(f["carry_jacobian"][f"clip_{c}"]).all() and (f["memory_sensitivity"][f"clip_{c}"][1:] > 0).all()
    assert f["mean_jacobian"].shape == (A, Z) and f["mean_carry_jacobian"].shape == (A, W) and f["carry_std"].shape == (W,) and f["components"].shape == (Z, Z)
    assert bytes(f["model"]) == b"lstm" and int(f["hidden_state_size"]) == H and int(f["hidden_layer_num"]) == L and bytes(f["feature"]) == b"intention"
    assert int(f["rows"]) == n and f["clips"].tolist() == [0, 1, 2] and bytes(f["mode"]) == b"ctrl"
    # the recomputed forward is the recorded one: float32 torch against the float32 kernels on the same rows, which holds only if the carry
    # entering every step is placed right (the shift, the zero rows at t = 0 and behind the aligned step)
    assert float(f["forward_mismatch"]) < 1e-5
    # the stored Jacobians are the call's on the inputs as this module places them, and the means are theirs
    x, h_in, c_in, scale = tool_inputs(rollouts)
    starts = np.cumsum((0,) + TOOL_ROWS[:-1])
    zero_rows = [*starts, starts[TOOL_ALIGNED[0]] + TOOL_ALIGNED[1] + 1]
    assert (h_in[zero_rows] == 0).all() and (c_in[zero_rows] == 0).all() and np.abs(h_in[np.setdiff1d(np.arange(n), zero_rows)]).min(1).max() > 0
    layers, head = JT.lstm_decoder_weights(pol)
    std = np.concatenate([h_in, c_in], 1).astype(f64).std(0).astype(f32)
    assert same_bits(f["carry_std"], std)
    direct = backend.lstm_decoder_jacobian(backend.asarray(x), backend.asarray(h_in), backend.asarray(c_in), layers, head, (0, Z), None, backend.asarray(scale), std)
    assert same_bits(cat("jacobian"), direct["jac"]) and same_bits(cat("carry_jacobian"), direct["carry_jac"]) and same_bits(cat("memory_sensitivity"), direct["carry_gain"])
    assert same_bits(cat("action_var"), direct["action_var"])
    assert np.abs(f["mean_jacobian"] - direct["jac"].astype(f64).mean(0)).max() < 1e-12 and np.abs(f["mean_carry_jacobian"] - direct["carry_jac"].astype(f64).mean(0)).max() < 1e-12
    # the rows with a zero carry (row 0 of every clip, the row behind the aligned step): the same rows of x evaluated against an all-zero carry
    alone = backend.lstm_decoder_jacobian(backend.asarray(x), backend.asarray(np.zeros_like(h_in)), backend.asarray(np.zeros_like(c_in)), layers, head, (0, Z),
                                          np.asarray(zero_rows, np.int32), None, std, want=("ctrl", "jac", "carry_jac"))
    assert same_bits(alone["jac"], direct["jac"][zero_rows]) and same_bits(alone["carry_jac"], direct["carry_jac"][zero_rows])
    # labels: the count-weighted mean of the motif means is the mean; a motif's memory sensitivity is the mean of its rows'
    flat = np.concatenate(lab)
    counts = np.array([(flat == k).sum() for k in range(2)])
    assert f["motif_mean_carry_jacobian"].shape == (2, A, W) and f["motif_memory_sensitivity"].shape == (2, 2 * L) and f["motif_rows"].tolist() == counts.tolist()
    assert np.abs((f["motif_mean_carry_jacobian"] * counts[:, None, None]).sum(0) / n - f["mean_carry_jacobian"]).max() < 1e-12
    assert np.abs((f["motif_mean_jacobian"] * counts[:, None, None]).sum(0) / n - f["mean_jacobian"]).max() < 1e-12
    ms = cat("memory_sensitivity").astype(f64)
    for k in range(2):
        assert np.abs(f["motif_memory_sensitivity"][k] - ms[flat == k].mean(0)).max() <= 1e-12 * ms.max()
    # features_out is a roll-out directory for the other tools, with the memory's sensitivity as a feature
    assert sorted(os.listdir(feat)) == ["clip_0.h5", "clip_1.h5", "clip_2.h5"]
    assert PCA.main([f"rollouts={feat}", "feature=memory_sensitivity", "n_components=2", f"out={os.path.join(tmp, 'pca.h5')}"], backend=backend) == 0
    one = load_from_h5py(os.path.join(feat, "clip_1.h5"))
    assert int(one["meta"]["clip_idx"]) == 1 and same_bits(one["activations"]["memory_sensitivity"], f["memory_sensitivity"]["clip_1"])
    assert same_bits(one["activations"]["latent_sensitivity"], f["latent_sensitivity"]["clip_1"])
    # max_rows: NaN exactly in the unsampled rows (carry_std is then over the sampled rows: the memory's sensitivity is compared through the call)
    rc, s, _, _ = run_tool(tmp, backend, ("max_rows=5", "seed=1"), pol, "sampled.h5", rollouts)
    assert rc == 0 and int(s["rows"]) == 5 and s["row_index"].shape == (5,) and (np.diff(s["row_index"]) > 0).all()
    picked = np.zeros(n, bool)
    picked[s["row_index"]] = True
    mem = np.concatenate([s["memory_sensitivity"][f"clip_{c}"] for c in range(3)])
    gain = np.concatenate([s["gain"][f"clip_{c}"] for c in range(3)])
    assert (np.isnan(mem).all(1) == ~picked).all() and (np.isnan(gain) == ~picked).all() and same_bits(gain[picked], cat("gain")[picked])
    assert same_bits(s["carry_std"], np.concatenate([h_in, c_in], 1)[picked].astype(f64).std(0).astype(f32))
    # mode=loc and a column range of the whole input: no action_var (the columns are not all intention columns)
    rc, l, _, _ = run_tool(tmp, backend, ("mode=loc", "wrt=input:4:9"), pol, "loc.h5", rollouts)
    assert rc == 0 and l["mean_jacobian"].shape == (A, 5) and bytes(l["feature"]) == b"input:4:9" and "action_var" not in l and l["mean_carry_jacobian"].shape == (A, W)
    # the eigen-decomposition block an intervention reads
    comp, ev = f["components"].astype(f64), f["explained_variance"].astype(f64)
    assert np.abs(comp @ comp.T - np.eye(Z)).max() < 1e-6 and (np.diff(ev) <= 0).all() and abs(ev.sum() - np.trace(f["gram_in"])) <= 1e-6 * ev.sum()
    capsys.readouterr()
    # refusals, each by name: no recorded carry, no recorded input, a replay directory, widths that do not match, options that do not parse
    for kw, word in ((dict(hidden_state=False), "hidden_state"), (dict(egocentric_obs=False), "log_decoder_input=true"), (dict(replay=True), "replay_latents")):
        bad = tool_clips(os.path.join(tmp, "bad_" + next(iter(kw))), pol, **kw)
        assert run_tool(tmp, backend, (), pol, "bad.h5", bad)[0] == 2
        err = capsys.readouterr().err
        assert word in err and "LSTM" in err, (kw, err)
    assert run_tool(tmp, backend, (), tool_policy(latents=7), "bad.h5", rollouts)[0] == 2 and "did not make these roll-outs" in capsys.readouterr().err
    assert run_tool(tmp, backend, (), tool_policy(H=64), "bad.h5", rollouts)[0] == 2 and "did not make these roll-outs" in capsys.readouterr().err
    assert run_tool(tmp, backend, (), tool_policy(L=1), "bad.h5", rollouts)[0] == 2 and "did not make these roll-outs" in capsys.readouterr().err
    for extra, word in ((("mode=both",), "mode"), (("wrt=input:3",), "wrt"), (("store=maybe",), "store"), (("max_rows=5", f"features_out={feat}"), "features_out")):
        assert run_tool(tmp, backend, extra, pol, "bad.h5", rollouts)[0] == 2 and word in capsys.readouterr().err, extra
    return f, pol, rollouts


def check_tool_files_agree(tmp_path, backend, emulation, capsys):
    """The tool on `backend` writes the file the emulation writes, within the bounds: the stored arrays of both lie within `within` of the same
    references."""
    from track_mjx_amd.analysis import jacobian as JT
    files = []
    for name, bk in (("device", backend), ("emulation", emulation)):
        rc, f, pol, rollouts = run_tool(os.path.join(str(tmp_path), name), bk, ("store=true",))
        assert rc == 0
        files.append(f)
    capsys.readouterr()
    layers, (wp, bp, A) = JT.lstm_decoder_weights(pol)
    net = Net.__new__(Net)
    net.layers, net.wp, net.bp, net.A, net.L, net.H, net.d_in = [list(y) for y in layers], wp, bp, A, len(layers), layers[0][1].shape[1], layers[0][0].shape[1]
    x, h_in, c_in, scale = tool_inputs(rollouts)
    n, Z = x.shape[0], scale.shape[1]
    std = np.concatenate([h_in, c_in], 1).astype(f64).std(0).astype(f32)
    j64, j32, jjig = jacobians64(net, x, h_in, c_in, (0, Z), 0), restated32_jacobians(net, x, h_in, c_in, (0, Z), 0), jacobians64(net, x, h_in, c_in, (0, Z), 0, rel=2.0 ** -22)
    r64, r32, jig = outputs_of(*j64, scale, std, net.L), restated32_outputs(*j32, scale, std, net.L), outputs_of(*jjig, scale, std, net.L)
    floors = {k: float(np.abs(jig[k] - r64[k]).max()) for k in r64}
    cat = lambda f, k: np.concatenate([f[k][f"clip_{c}"] for c in range(len(TOOL_ROWS))], 0)      # noqa: E731
    for name, f in zip(("device", "emulation"), files):
        assert same_bits(f["carry_std"], std)
        got = {"jac": cat(f, "jacobian"), "gain": cat(f, "gain"), "col2": cat(f, "latent_sensitivity"), "row2": cat(f, "actuator_sensitivity"),
               "action_var": cat(f, "action_var"), "mean_sum": f["mean_jacobian"] * n, "gram_in": f["gram_in"] * n, "gram_out": f["gram_out"] * n,
               "carry_jac": cat(f, "carry_jacobian"), "carry_gain": cat(f, "memory_sensitivity"), "carry_sum": f["mean_carry_jacobian"] * n}
        within(got, r64, r32, floors, net.L, std, f"tool file, {name}")
    dev, emu = files
    assert abs(float(dev["forward_mismatch"]) - float(emu["forward_mismatch"])) < 1e-5
