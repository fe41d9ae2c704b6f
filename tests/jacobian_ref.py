"""The float64 reference of the decoder-Jacobian kernels (csrc/jacobian_core.h), the case lists and the checkers that tests/test_jacobian_cpu.py
(the host emulation) and tests/test_gpu_jacobian.py (the C-ABI) share.  A `backend` is analysis.pca.HipBackend or tests/hostemu/jacobian_emu.B.

The reference (`reference64`) is the analytic Jacobian in numpy float64, in the expressions of DESIGN.md "Decoder Jacobian": forward
u = W h + b, s = silu(u), xhat = (s - mean) r, h = gamma xhat + beta; reverse G = diag(1 - ctrl^2) Wh[:A], q = g gamma,
ds = r (q - mean(q) - xhat mean(q xhat)), du = ds silu'(u), g = du W.  It is itself checked against torch.autograd.functional.jacobian on the
product's own DecoderNet(...).double() on the CPU, an independent derivation (check_reference_against_autograd).  Measured over CASES: the largest
||J_ref - J_autograd||_F / ||J_autograd||_F is AUTOGRAD_GAP = 5.4e-15 (a wrong formula shows at O(1)); the check holds it to 8 times that, far
below the 1e-9 the test also asserts.

How every bound is derived (the method of tests/compare_ref.py).  Each checked array is computed twice on the test's own input: in float64, and
by `restated32`, a float32 numpy restatement of what the kernels perform: every product a chain acc = fmaf(a_k, b_k, acc) from 0 in ascending k (an
FMA is restated as the float64 sum of the accumulator and the exact float64 product, rounded to float32), the LayerNorm's two sums as the threads'
partial sums in column order joined by the kernels' fixed trees, the backward's two sums by its 64 lanes and their tree, every other operation in
the kernels' order, float64 where the kernels sum in float64 (the sums over the rows: groups of 32 rows in row order, the groups in order).  The
kernel and the emulation are held to TWICE the distance between the two, the margin that allows for another rounding of the same size.  The
distance is the largest absolute difference over an array; an array of one element (one actuator: gram_out is [1, 1]) makes that a single draw,
which is zero by chance now and then, so the arrays that carry the same roundings form a family (ctrl; what is linear in J: jac, mean_sum; what
is quadratic in J: gain, col2, row2, action_var, gram_in, gram_out), each array's distance is taken relative to its scale (the same expression on
|J| in float64: the magnitude its roundings are proportional to; 1 for ctrl), and the largest relative distance of a family serves every array
of it, times that array's scale (`within`).  Where a transcendental enters the library's result may differ from numpy's by its documented
error: expf 1 ulp and the add and the correctly rounded divide behind it (the logistic function: 2 ulp = 2^-22 relative), tanhf 2 ulp (2^-22,
the result kept inside [-1, 1]), the square root and the divide of r (1 ulp = 2^-23).  The floor that allows for it is derived here, not chosen:
the float64 reference is evaluated a second time with every logistic value, every ctrl and every r multiplied by 1 + delta, delta = +- that
relative error with seeded random signs, and the floor of an array is the largest absolute change that makes in it (`references`), used relative to the scale like the distance.  Quantities that
are exact by construction (a zero row of the head, gamma = 0, a saturated tanh, permuted or repeated rows, a second call, a row stride, the
outputs of a call without jac) are compared with == or bit for bit."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from track_mjx_amd import hip

f64, f32 = np.float64, np.float32
CHUNK, SUM_ROWS = 1024, 32      # JAC_CHUNK, JAC_SUM_ROWS (csrc/jacobian_core.h)
assert CHUNK == hip.JACOBIAN_CHUNK
AUTOGRAD_GAP = 5.4e-15
EPS = 1e-6
# (m, d_in, (wrt_col0, wrt_cols), widths, A, ldx: None = dense)
CASES = ((1, 1, (0, 1), (1,), 1, None),                       # a width-1 LayerNorm has xhat = 0: J is exactly 0
         (3, 5, (0, 2), (4,), 1, None),                       # one block, one actuator
         (CHUNK + 1, 7, (0, 3), (8, 12), 5, None),            # one row more than a pass; unequal widths catch a transposed weight
         (5, 286, (0, 60), (260, 20), 38, 291),               # widths off every tile edge, the shipped A and Z, a row stride
         (3, 286, (60, 128), (1024, 1024), 38, None),         # the width limit, wrt not at column 0 and at its limit
         (2, 64, (0, 64), (16,) * 8, 64, None))               # the layer and actuator limits
ARRAYS = ("ctrl", "jac", "gain", "col2", "row2", "action_var", "mean_sum", "gram_in", "gram_out")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ---------------------------------------------------------------------------------------------------------------- the problems
class Net:
    """layers [(W [H, K], b, gamma, beta)], the head (Wh [2A, H_L], bh [2A]) and A, float32."""

    def __init__(self, d_in, widths, A, seed):
        rng = np.random.default_rng(seed)
        self.layers, K = [], d_in
        for H in widths:      # LeCun-scaled weights, gamma = 1 + 0.1 N, beta and b N(0, 1): the conditioning of a trained net
            self.layers.append([(rng.standard_normal((H, K)) / np.sqrt(K)).astype(f32), rng.standard_normal(H).astype(f32),
                                (1.0 + 0.1 * rng.standard_normal(H)).astype(f32), rng.standard_normal(H).astype(f32)])
            K = H
        self.wh, self.bh, self.A, self.d_in = (rng.standard_normal((2 * A, K)) / np.sqrt(K)).astype(f32), rng.standard_normal(2 * A).astype(f32), A, d_in

    @property
    def head(self):
        return self.wh, self.bh, self.A


@functools.lru_cache(None)
def problem(case):
    """-> (net, x [m, d_in] float32 (a column slice of a wider buffer where the case has a row stride), scale [m, wrt_cols])."""
    m, d_in, (c0, Z), widths, A, ldx = case
    net = Net(d_in, widths, A, 100 + CASES.index(case) if case in CASES else 99)
    rng = np.random.default_rng(7)
    buf = np.full((m, ldx or d_in), 1e6, f32)
    off = (ldx - d_in) // 2 if ldx else 0
    buf[:, off:off + d_in] = rng.standard_normal((m, d_in))
    scale = np.exp(0.5 * (-2.0 + 0.5 * rng.standard_normal((m, Z)))).astype(f32)
    for a in (buf, scale, *[t for layer in net.layers for t in layer], net.wh, net.bh):
        a.setflags(write=False)
    return net, buf[:, off:off + d_in], scale


# ---------------------------------------------------------------------------------------------------------------- float64
def reference64(net, x, wrt, mode, scale=None, rel=None):
    """The analytic Jacobian and everything the call returns, float64.  `rel`: (sigmoid, tanh, r) relative perturbations with seeded random signs,
    for the floors."""
    c0, Z = wrt
    A = net.A
    rng = np.random.default_rng(5)
    jig = (lambda shape, mag: 1.0 + mag * rng.choice((-1.0, 1.0), shape)) if rel is not None else (lambda shape, mag: 1.0)
    h, kept = np.asarray(x, f64), []
    for W, b, gamma, beta in net.layers:
        u = h @ W.astype(f64).T + b
        sig = 1.0 / (1.0 + np.exp(-u))
        sig = sig * jig(sig.shape, rel[0] if rel else 0)
        s = u * sig
        mean = s.mean(1, keepdims=True)
        r = 1.0 / np.sqrt(((s - mean) ** 2).mean(1, keepdims=True) + EPS)
        r = r * jig(r.shape, rel[2] if rel else 0)
        xhat = (s - mean) * r
        kept.append((xhat, r, sig * (1.0 + u * (1.0 - sig))))
        h = gamma * xhat + beta
    wh = net.wh[:A].astype(f64)
    loc = h @ wh.T + net.bh[:A]
    ctrl = np.tanh(loc)
    ctrl = np.clip(ctrl * jig(ctrl.shape, rel[1] if rel else 0), -1.0, 1.0)
    g = np.broadcast_to(wh[None], (x.shape[0], *wh.shape)).copy()
    if mode == 0:
        g *= (1.0 - ctrl * ctrl)[:, :, None]
    for l in range(len(net.layers) - 1, -1, -1):
        W, _, gamma, _ = net.layers[l]
        xhat, r, dsilu = kept[l]
        q = g * gamma
        ds = r[:, None] * (q - q.mean(2, keepdims=True) - xhat[:, None] * (q * xhat[:, None]).mean(2, keepdims=True))
        du = ds * dsilu[:, None]
        g = du @ (W[:, c0:c0 + Z] if l == 0 else W).astype(f64)
    return outputs_of(ctrl, g, scale)


def outputs_of(ctrl, J, scale):
    out = {"ctrl": ctrl, "jac": J, "gain": (J * J).sum((1, 2)), "col2": (J * J).sum(1), "row2": (J * J).sum(2), "mean_sum": J.sum(0),
           "gram_in": np.einsum("iaj,iak->jk", J, J), "gram_out": np.einsum("iaj,ibj->ab", J, J)}
    if scale is not None:
        out["action_var"] = ((J * np.asarray(scale, f64)[:, None]) ** 2).sum(2)
    return out


# ---------------------------------------------------------------------------------------------------------------- the float32 restatement
def fma(a, b, c):
    return (np.asarray(c, f64) + np.asarray(a, f64) * np.asarray(b, f64)).astype(f32)


def chain(a, b):
    """[M, K] . [K, N]: one fmaf a term from 0 in ascending k."""
    acc = np.zeros((a.shape[0], b.shape[1]), f32)
    for k in range(a.shape[1]):
        acc = fma(a[:, k:k + 1], b[k:k + 1], acc)
    return acc


def lane_sums(vals, lanes, step):
    """Lane t of `lanes` folds the columns t, t + lanes, ... in order with step(acc, column block); then the kernels' tree.  vals: arrays [R, H]."""
    R, H = vals[0].shape
    part = np.zeros((R, lanes), f32)
    for e in range(0, H, lanes):
        w = min(lanes, H - e)
        part[:, :w] = step(part[:, :w], *[v[:, e:e + w] for v in vals])
    half = lanes // 2
    while half >= 1:
        part[:, :half] = part[:, :half] + part[:, half:2 * half]
        half //= 2
    return part[:, :1]


def restated32(net, x, wrt, mode, scale=None):
    c0, Z = wrt
    A, one = net.A, f32(1)
    h, kept = np.asarray(x, f32), []
    for W, b, gamma, beta in net.layers:
        H = f32(W.shape[0])
        u = chain(h, W.T) + b
        sig = one / (one + np.exp(-u))
        s = u * sig
        d = sig * (one + u * (one - sig))
        mean = lane_sums([s], 256, lambda acc, v: acc + v) / H
        c = s - mean
        r = one / np.sqrt(lane_sums([c], 256, lambda acc, v: fma(v, v, acc)) / H + f32(EPS))
        xhat = c * r
        kept.append((xhat, r * d))
        h = fma(gamma, xhat, beta)
    wh = net.wh[:A]
    ctrl = np.tanh(chain(h, wh.T) + net.bh[:A])
    dd = fma(-ctrl, ctrl, one) if mode == 0 else np.ones_like(ctrl)
    g = (dd[:, :, None] * wh[None]).reshape(-1, wh.shape[1])
    for l in range(len(net.layers) - 1, -1, -1):
        W, _, gamma, _ = net.layers[l]
        H = f32(W.shape[0])
        xhat, rs = (np.repeat(v, A, 0) for v in kept[l])
        q = g * gamma
        mq = lane_sums([q], 64, lambda acc, v: acc + v) / H
        mqx = lane_sums([q, xhat], 64, lambda acc, v, w: fma(v, w, acc)) / H
        du = fma(-xhat, mqx, q - mq) * rs
        g = chain(du, W[:, c0:c0 + Z] if l == 0 else W)
    J = g.reshape(-1, A, Z)
    m = J.shape[0]
    out = {"ctrl": ctrl, "jac": J}
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
    gi, go = np.zeros((m, Z, Z), f32), np.zeros((m, A, A), f32)
    for a in range(A):
        gi = fma(J[:, a, :, None], J[:, a, None, :], gi)
    for j in range(Z):
        go = fma(J[:, :, None, j], J[:, None, :, j], go)
    for name, per_row in (("mean_sum", J), ("gram_in", gi), ("gram_out", go)):
        total = np.zeros(per_row.shape[1:], f64)
        for i0 in range(0, m, SUM_ROWS):
            part = np.zeros_like(total)
            for i in range(i0, min(i0 + SUM_ROWS, m)):
                part = part + per_row[i].astype(f64)
            total = total + part
        out[name] = total
    return out


@functools.lru_cache(None)
def references(case, mode):
    """-> (float64, the float32 restatement, the floors) of a case, computed once."""
    net, x, scale = problem(case)
    wrt = case[2]
    r64, r32 = reference64(net, x, wrt, mode, scale), restated32(net, x, wrt, mode, scale)
    jig = reference64(net, x, wrt, mode, scale, rel=(2.0 ** -22, 2.0 ** -22, 2.0 ** -23))
    return r64, r32, {k: float(np.abs(jig[k] - r64[k]).max()) for k in r64}


FAMILIES = (("ctrl",), ("jac", "mean_sum"), ("gain", "col2", "row2", "action_var", "gram_in", "gram_out"))      # value, linear in J, quadratic in J


def within(got, r64, r32, floors, what):
    """Every array of `got` against the references, family by family (the module's text): |got - r64| <= (2 gap + floor) scale elementwise-max, with
    gap and floor the family's largest relative distance and floor and scale the array's magnitude; prints the figures."""
    J = np.abs(r64["jac"])
    scale = {k: float(v.max()) for k, v in outputs_of(np.ones_like(r64["ctrl"]), J, None if "action_var" not in r64 else np.ones((J.shape[0], J.shape[2]))).items()}
    if "action_var" in r64:
        scale["action_var"] = float(r64["action_var"].max())
    for fam in FAMILIES:
        live = [k for k in fam if scale[k] > 0.0]
        gap = max([float(np.abs(np.asarray(r32[k], f64) - r64[k]).max()) / scale[k] for k in live], default=0.0)
        floor = max([floors[k] / scale[k] for k in live], default=0.0)
        for k in [k for k in fam if k in got]:
            err = float(np.abs(np.asarray(got[k], f64) - r64[k]).max())
            bound = (2.0 * gap + floor) * scale[k]
            print(f"[jacobian {what} {k}] error {err:.3g}; the family's float32-float64 gap {gap:.3g} and transcendental floor {floor:.3g} of the scale {scale[k]:.3g}: "
                  f"{err / bound if err else 0.0:.3g} of the bound")
            assert np.isfinite(np.asarray(got[k], f64)).all() and err <= bound, (what, k, err, bound)


# ---------------------------------------------------------------------------------------------------------------- the calls
def run(backend, net, x, wrt, mode=0, scale=None, row_index=None, want=("ctrl", "jac", "gain", "col2", "row2")):
    return backend.decoder_jacobian(backend.asarray(x), net.layers, net.head, wrt, EPS, row_index, None if scale is None else backend.asarray(scale), mode, want)


def check_case(case, backend, what=""):
    """Every output of both modes against the references; the call without jac gives the same bits in every other output; the consistency of the
    sums and of the three gains."""
    net, x, scale = problem(case)
    m, _, wrt, _, A, _ = case
    Z = wrt[1]
    for mode in (0, 1):
        r64, r32, floors = references(case, mode)
        got = run(backend, net, x, wrt, mode, scale)
        assert set(got) == set(ARRAYS)
        within(got, r64, r32, floors, f"{what} case {CASES.index(case)} mode {mode}")
        lean = run(backend, net, x, wrt, mode, scale, want=("ctrl", "gain", "col2", "row2"))
        assert "jac" not in lean and all(same_bits(lean[k], got[k]) for k in lean), "the call without jac changed another output"
        # the sums against the float64 sums of the stored Jacobians: the element itself is exact; a Gram element is per row a float32 chain of
        # A (or Z) fused terms, good to (terms) 2^-24 of the sum of the terms' magnitudes; the float64 sums across rows add m 2^-52 of that
        J = got["jac"].astype(f64)
        mine, mag = outputs_of(got["ctrl"].astype(f64), J, None), outputs_of(got["ctrl"].astype(f64), np.abs(J), None)
        for k, terms in (("mean_sum", 0), ("gram_in", A), ("gram_out", Z)):
            bound = (terms * 2.0 ** -24 + m * 2.0 ** -52) * mag[k]
            assert (np.abs(got[k] - mine[k]) <= bound).all(), (k, float(np.abs(got[k] - mine[k]).max()), float(bound.max()))
        # gain = sum col2 = sum row2: three orders of the same A Z non-negative terms, each float32 sum good to (terms in its chains) 2^-24
        g64 = got["gain"].astype(f64)
        slack = 2.0 * (A + Z + 2) * 2.0 ** -24 * g64
        assert (np.abs(got["col2"].astype(f64).sum(1) - g64) <= slack).all() and (np.abs(got["row2"].astype(f64).sum(1) - g64) <= slack).all()
    if CASES.index(case) == 0:
        assert (got["jac"] == 0).all() and (got["gain"] == 0).all() and (got["gram_in"] == 0).all()


PROPERTY_CASE = (6, 9, (2, 4), (8, 12), 3, None)


def _variant(net, **change):
    """A copy of `net` with parts replaced: wh=, bh=, or gamma=(layer, values)."""
    v = Net.__new__(Net)
    v.layers, v.wh, v.bh, v.A, v.d_in = [list(layer) for layer in net.layers], net.wh, net.bh, net.A, net.d_in
    for k, val in change.items():
        if k == "gamma":
            v.layers[val[0]][2] = val[1]
        else:
            setattr(v, k, val)
    return v


def check_properties(backend, strided, what=""):
    """The properties that hold exactly.  `strided(a)`: the backend's array of a's values as a column slice of a wider buffer."""
    net, x, scale = problem(PROPERTY_CASE)
    m, _, wrt, widths, A, _ = PROPERTY_CASE
    base = run(backend, net, x, wrt, 0, scale)
    assert np.abs(base["jac"]).min() > 0
    # a zero row of the head: a zero row of J, the other rows as they were
    wh = net.wh.copy()
    wh[1] = 0
    got = run(backend, _variant(net, wh=wh), x, wrt, 0, scale)
    assert (got["jac"][:, 1] == 0).all() and (got["row2"][:, 1] == 0).all() and same_bits(got["jac"][:, 0], base["jac"][:, 0])
    # gamma = 0 in any layer: J = 0
    for l, H in enumerate(widths):
        got = run(backend, _variant(net, gamma=(l, np.zeros(H, f32))), x, wrt, 0, scale)
        assert (got["jac"] == 0).all() and (got["gain"] == 0).all() and (got["gram_out"] == 0).all(), l
    # |loc| > 20: tanh is exactly +-1 in float32, the mode-0 rows exactly 0 and finite, the mode-1 rows not
    bh = net.bh.copy()
    bh[0], bh[2] = 60.0, -60.0
    sat = _variant(net, bh=bh)
    g0, g1 = run(backend, sat, x, wrt, 0, scale), run(backend, sat, x, wrt, 1, scale)
    assert (np.abs(g0["ctrl"][:, (0, 2)]) == 1).all() and (g0["jac"][:, (0, 2)] == 0).all() and np.isfinite(g0["jac"]).all()
    assert (g1["jac"][:, (0, 2)] != 0).all() and np.abs(g0["jac"][:, 1]).min() > 0 and same_bits(g0["ctrl"], g1["ctrl"])
    # a permuted list with a repeated entry permutes and repeats the per-row outputs; no list = arange
    idx = np.array([3, 0, 0, 5, 2, 4, 1, 3], np.int32)
    perm = run(backend, net, x, wrt, 0, scale, row_index=idx)
    for k in ("ctrl", "jac", "gain", "col2", "row2", "action_var"):
        assert same_bits(perm[k], base[k][idx]), k
    ar = run(backend, net, x, wrt, 0, scale, row_index=np.arange(m, dtype=np.int32))
    assert all(same_bits(ar[k], base[k]) for k in ARRAYS)
    # two calls, and dense against strided rows: the same bits in every output, the sums included
    again, wide = run(backend, net, x, wrt, 0, scale), run(backend, net, strided(x), wrt, 0, strided(scale))
    assert all(same_bits(again[k], base[k]) and same_bits(wide[k], base[k]) for k in ARRAYS)
    # a row alone is the row in the middle of the call (the bits of a row do not depend on m or on its place)
    alone = run(backend, net, x, wrt, 0, scale, row_index=np.array([4], np.int32))
    assert all(same_bits(alone[k][0], base[k][4]) for k in ("ctrl", "jac", "gain", "col2", "row2", "action_var"))


def check_rows_across_passes(backend):
    """Row CHUNK (the first of the second pass) and row 0 of the case with one row more than a pass, each alone, give the bits they have in the
    whole call."""
    case = CASES[2]
    net, x, scale = problem(case)
    full = run(backend, net, x, case[2], 0, scale)
    for i in (0, CHUNK - 1, CHUNK):
        one = run(backend, net, x, case[2], 0, scale, row_index=np.array([i], np.int32))
        assert all(same_bits(one[k][0], full[k][i]) for k in ("ctrl", "jac", "gain", "col2", "row2", "action_var")), i


# ---------------------------------------------------------------------------------------------------------------- autograd
def check_reference_against_autograd():
    import torch
    from track_mjx_amd.agent.networks import DecoderNet
    worst = 0.0
    for case in CASES:
        net, x, _ = problem(case)
        m, d_in, (c0, Z), widths, A, _ = case
        tn = DecoderNet(d_in, A, widths).double()
        with torch.no_grad():
            for blk, (W, b, gamma, beta) in zip(tn.decoder, net.layers):
                for dst, src in ((blk.dense.weight, W), (blk.dense.bias, b), (blk.norm.weight, gamma), (blk.norm.bias, beta)):
                    dst.copy_(torch.from_numpy(np.asarray(src, f64)))
            tn.head.weight.copy_(torch.from_numpy(net.wh.astype(f64)))
            tn.head.bias.copy_(torch.from_numpy(net.bh.astype(f64)))
        assert all(float(blk.norm.eps) == EPS for blk in tn.decoder)
        for mode in (0, 1):
            r64 = reference64(net, x, (c0, Z), mode)
            for i in range(min(m, 3)):
                fn = (lambda v: torch.tanh(tn(v)[:A])) if mode == 0 else (lambda v: tn(v)[:A])
                jt = torch.autograd.functional.jacobian(fn, torch.from_numpy(np.asarray(x[i], f64)))[:, c0:c0 + Z].numpy()
                if (r64["jac"][i] == 0).all():      # (the width-1 LayerNorm: exactly 0 here, rounding noise of the natural scale in autograd)
                    assert float(np.linalg.norm(jt)) <= 1e-9 * float(np.prod([np.linalg.norm(layer[0]) for layer in net.layers]) * np.linalg.norm(net.wh[:A]))
                else:
                    worst = max(worst, float(np.linalg.norm(r64["jac"][i] - jt)) / float(np.linalg.norm(jt)))
    print(f"[jacobian] the analytic float64 reference against torch autograd: largest relative difference {worst:.3g} (recorded {AUTOGRAD_GAP})")
    assert worst <= 8 * AUTOGRAD_GAP and worst < 1e-9


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, alloc, ptr, untouched, what=""):
    """Every limit exceeded by one and every condition of include/tmjx.h returns TMJX_EINVAL (-22) and writes nothing; the workspace entry and the
    call agree on the descriptor's limits.  The pointers of the descriptor are a dummy address: a refused call never reads them."""
    a = 1 << 20
    sums, ws = alloc((64,), f64, -7.25), alloc((4096,), f32, -7.25)
    floats = C.c_int64(0)

    def desc(L=2, d_in=9, widths=(8, 12, 8, 8, 8, 8, 8, 8, 8), A=3, wrt=(2, 4), ldw=None, ldwh=None, null=None):
        d = hip.JacobianDesc()
        d.L, d.d_in, d.eps, d.A, d.wrt_col0, d.wrt_cols = L, d_in, EPS, A, wrt[0], wrt[1]
        K = d_in
        for l in range(min(max(L, 0), 8)):
            y = d.layer[l]
            y.W, y.b, y.gamma, y.beta, y.width, y.ldw = a, a, a, a, widths[l], K if ldw is None or ldw[0] != l else ldw[1]
            K = widths[l]
        d.Wh, d.bh, d.ldwh = a, a, K if ldwh is None else ldwh
        if null is not None:
            setattr(d.layer[0] if null in ("W", "b", "gamma", "beta") else d, null, None)
        return d

    def call(d, x=a, n=6, ldx=9, row_index=None, m=6, scale=None, ld_scale=4, mode=0, action_var=None, sums_=None, ws_=None):
        return lib.tmjx_decoder_jacobian(None if d is None else C.byref(d), x, n, ldx, row_index, m, scale, ld_scale, mode, None, None, None, None, None, action_var,
                                         ptr(sums) if sums_ is None else sums_, ptr(ws) if ws_ is None else ws_, None)
    assert lib.tmjx_jacobian_workspace(C.byref(desc()), 6, C.byref(floats)) == 0 and floats.value > 0
    assert lib.tmjx_jacobian_workspace(C.byref(desc(L=8, widths=(1024,) * 8, A=64, wrt=(0, 128), d_in=128)), 6, C.byref(floats)) == 0      # the limits themselves
    bad_desc = (desc(L=0), desc(L=9), desc(widths=(0, 12)), desc(widths=(8, 1025)), desc(A=0), desc(A=65), desc(wrt=(2, 0)), desc(wrt=(0, 129), d_in=200),
                desc(wrt=(6, 4)), desc(wrt=(-1, 4)), desc(d_in=0), desc(ldw=(0, 8)), desc(ldw=(1, 7)), desc(ldwh=11),
                *[desc(null=k) for k in ("W", "b", "gamma", "beta", "Wh", "bh")])
    for i, d in enumerate(bad_desc):
        assert lib.tmjx_jacobian_workspace(C.byref(d), 6, C.byref(floats)) == -22 and lib.tmjx_last_error(), (what, i)
        assert call(d) == -22 and lib.tmjx_last_error(), (what, i)
    assert lib.tmjx_jacobian_workspace(C.byref(desc()), 0, C.byref(floats)) == -22 and lib.tmjx_jacobian_workspace(C.byref(desc()), 6, None) == -22
    assert lib.tmjx_jacobian_workspace(None, 6, C.byref(floats)) == -22
    good = desc()
    bad_call = (dict(d=None), dict(x=None), dict(sums_=0), dict(ws_=0), dict(ldx=8), dict(m=0), dict(n=0), dict(m=7), dict(mode=2), dict(mode=-1),
                dict(action_var=a), dict(scale=a, ld_scale=3), dict(ws_=ptr(ws) + 4), dict(sums_=ptr(sums) + 4), dict(x=a + 2))
    for kw in bad_call:
        d = kw.pop("d", good)
        assert call(d, **kw) == -22 and lib.tmjx_last_error(), (what, kw)
    assert untouched(sums, -7.25) and untouched(ws, -7.25), f"{what}: a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------- the tool
TOOL_ROWS = (7, 9, 4)


def tool_policy(seed=0, decoder_layers=(24, 16), latents=6):
    """A seeded IntentionPolicy on the CPU (obs 20 = 12 reference + 8 proprioceptive, 5 actuators) with LayerNorms off their defaults."""
    import torch
    from track_mjx_amd.agent.networks import IntentionPolicy
    torch.manual_seed(seed)
    pol = IntentionPolicy(20, 12, 5, latents, (16,), decoder_layers).float().eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for blk in pol.decoder:
            blk.norm.weight.add_(0.1 * torch.randn(blk.norm.weight.shape, generator=g))
            blk.norm.bias.add_(0.5 * torch.randn(blk.norm.bias.shape, generator=g))
            blk.dense.bias.add_(0.5 * torch.randn(blk.dense.bias.shape, generator=g))
    return pol


def tool_clips(root, pol, rows=TOOL_ROWS, with_logvar=True):
    """clip_<i>.h5 files with the decoder's input rows and the ctrl this policy gives for them (float32 torch on the CPU)."""
    import torch
    from track_mjx_amd import h5lite
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(3)
    Z, P, A = pol.latents, pol.decoder[0].dense.in_features - pol.latents, pol.action_size
    for c, T in enumerate(rows):
        z, prop = rng.standard_normal((T, Z)).astype(f32), rng.standard_normal((T, P)).astype(f32)
        with torch.no_grad():
            ctrl = torch.tanh(pol.head(pol.decoder(torch.from_numpy(np.concatenate([z, prop], 1))))[:, :A]).numpy()
        acts = {"intention": z, "egocentric_obs": prop}
        if with_logvar:
            acts["encoder"] = {"logvar": (-2.0 + 0.5 * rng.standard_normal((T, Z))).astype(f32)}
        h5lite.write_tree(os.path.join(root, f"clip_{c}.h5"), {"ctrl": ctrl, "activations": acts, "meta": {"clip_idx": np.int64(c), "seed": np.int64(42)}})
    return root


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
    from track_mjx_amd.analysis.recorded import feature_of
    from track_mjx_amd.analysis.utils import load_from_h5py
    tmp = str(tmp_path)
    n, A, Z = sum(TOOL_ROWS), 5, 6
    labels = os.path.join(tmp, "clusters.h5")
    lab = [np.arange(T) % 2 for T in TOOL_ROWS]
    h5lite.write_tree(labels, {"labels": {f"clip_{c}": v.astype(np.int32) for c, v in enumerate(lab)}})
    feat = os.path.join(tmp, "jac_dir")
    rc, f, pol, rollouts = run_tool(tmp, backend, ("store=true", f"labels={labels}", f"features_out={feat}"))
    assert rc == 0 and "forward mismatch" in capsys.readouterr().out
    for c, T in enumerate(TOOL_ROWS):      # every dataset with its shape
        assert f["gain"][f"clip_{c}"].shape == (T,) and f["latent_sensitivity"][f"clip_{c}"].shape == (T, Z) and f["actuator_sensitivity"][f"clip_{c}"].shape == (T, A)
        assert f["action_var"][f"clip_{c}"].shape == (T, A) and f["jacobian"][f"clip_{c}"].shape == (T, A, Z)
        assert np.isfinite(f["jacobian"][f"clip_{c}"]).all() and (f["action_var"][f"clip_{c}"] > 0).all()
    assert f["mean_jacobian"].shape == (A, Z) and f["gram_in"].shape == (Z, Z) and f["gram_out"].shape == (A, A) and f["components"].shape == (Z, Z)
    assert f["mean"].shape == (Z,) and f["explained_variance"].shape == (Z,) and f["explained_variance_ratio"].shape == (Z,)
    assert bytes(f["feature"]) == b"intention" and bytes(f["mode"]) == b"ctrl" and bytes(f["wrt"]) == b"0:6" and int(f["rows"]) == n and f["clips"].tolist() == [0, 1, 2]
    assert float(f["forward_mismatch"]) < 1e-5      # (float32 torch against the float32 kernels on the same rows)
    # the eigen-decomposition: orthonormal rows, eigenvalues descending that sum to the trace, G v = lambda v
    comp, ev = f["components"].astype(f64), f["explained_variance"].astype(f64)
    assert np.abs(comp @ comp.T - np.eye(Z)).max() < 1e-6 and (np.diff(ev) <= 0).all() and abs(ev.sum() - np.trace(f["gram_in"])) <= 1e-6 * ev.sum()
    assert np.abs(f["gram_in"] @ comp.T - comp.T * ev).max() <= 1e-6 * ev[0] and abs(float(f["explained_variance_ratio"].sum()) - 1) < 1e-6
    # the stored Jacobians are the call's, and the means are theirs
    layers, head, eps = JT.decoder_weights(pol)
    x = np.concatenate([np.concatenate([feature_of(r, k, "") for k in ("intention", "egocentric_obs")], 1)
                        for r in (load_from_h5py(os.path.join(rollouts, f"clip_{c}.h5")) for c in range(3))], 0)
    direct = backend.decoder_jacobian(backend.asarray(x), layers, head, (0, Z), eps)
    stored = np.concatenate([f["jacobian"][f"clip_{c}"] for c in range(3)], 0)
    assert same_bits(stored, direct["jac"]) and np.abs(f["mean_jacobian"] - stored.astype(f64).mean(0)).max() < 1e-12
    # labels: the count-weighted mean of the motif means is the mean
    flat = np.concatenate(lab)
    counts = np.array([(flat == k).sum() for k in range(2)])
    assert f["motif_mean_jacobian"].shape == (2, A, Z) and f["motif_gram_in"].shape == (2, Z, Z) and f["motif_gain"].shape == (2,) and f["motif_rows"].tolist() == counts.tolist()
    assert np.abs((f["motif_mean_jacobian"] * counts[:, None, None]).sum(0) / n - f["mean_jacobian"]).max() < 1e-12
    assert np.abs(f["motif_mean_jacobian"][1] - stored[flat == 1].astype(f64).mean(0)).max() < 1e-12
    # features_out is a roll-out directory for the other tools
    assert sorted(os.listdir(feat)) == ["clip_0.h5", "clip_1.h5", "clip_2.h5"]
    assert PCA.main([f"rollouts={feat}", "feature=latent_sensitivity", "n_components=2", f"out={os.path.join(tmp, 'pca.h5')}"], backend=backend) == 0
    assert PCA.main([f"rollouts={feat}", "feature=jacobian_gain", "n_components=1", f"out={os.path.join(tmp, 'pca1.h5')}"], backend=backend) == 0
    one = load_from_h5py(os.path.join(feat, "clip_1.h5"))
    assert int(one["meta"]["clip_idx"]) == 1 and same_bits(one["activations"]["latent_sensitivity"], f["latent_sensitivity"]["clip_1"])
    # max_rows: NaN exactly in the unsampled rows
    rc, s, _, _ = run_tool(tmp, backend, ("max_rows=5", "seed=1"), pol, "sampled.h5", rollouts)
    assert rc == 0 and int(s["rows"]) == 5 and s["row_index"].shape == (5,) and (np.diff(s["row_index"]) > 0).all()
    gain = np.concatenate([s["gain"][f"clip_{c}"] for c in range(3)])
    picked = np.zeros(n, bool)
    picked[s["row_index"]] = True
    assert (np.isnan(gain) == ~picked).all() and same_bits(gain[picked], np.concatenate([f["gain"][f"clip_{c}"] for c in range(3)])[picked])
    # mode=loc and a column range of the whole input; no logvar: no action_var
    rc, l, _, _ = run_tool(tmp, backend, ("mode=loc", "wrt=input:4:9"), pol, "loc.h5", rollouts)
    assert rc == 0 and l["mean_jacobian"].shape == (A, 5) and bytes(l["feature"]) == b"input:4:9" and "action_var" not in l
    capsys.readouterr()
    # refusals: a checkpoint of another width, an LSTM policy, options that do not parse
    assert run_tool(tmp, backend, (), tool_policy(decoder_layers=(24, 16), latents=7), "bad.h5", rollouts)[0] == 2 and "did not make these roll-outs" in capsys.readouterr().err
    from track_mjx_amd.agent.lstm import LSTMIntentionPolicy
    lstm = LSTMIntentionPolicy(20, 12, 5, 6, (16,), hidden_state_size=32, hidden_layer_num=1)
    assert run_tool(tmp, backend, (), lstm, "bad.h5", rollouts)[0] == 2 and "LSTM" in capsys.readouterr().err
    for extra, word in ((("mode=both",), "mode"), (("wrt=input:3",), "wrt"), (("wrt=input:0:15",), "wrt"), (("store=maybe",), "store"), (("max_rows=-1",), "max_rows"),
                        (("max_rows=5", f"features_out={feat}"), "features_out")):
        assert run_tool(tmp, backend, extra, pol, "bad.h5", rollouts)[0] == 2 and word in capsys.readouterr().err, extra
    assert JT.main(["rollouts=x"], backend=backend) == 2
    return f, pol, rollouts


def check_tool_files_agree(tmp_path, backend, emulation, capsys):
    """The tool on `backend` writes the file the emulation writes, within the bounds: the stored arrays of both lie within `within` of the same
    references, and the eigenvalues differ by no more than the Gram matrices do (Weyl) plus the decomposition's 2^-40."""
    from track_mjx_amd.analysis import jacobian as JT
    from track_mjx_amd.analysis.utils import load_from_h5py
    files = []
    for name, bk in (("device", backend), ("emulation", emulation)):
        rc, f, pol, rollouts = run_tool(os.path.join(str(tmp_path), name), bk, ("store=true",))
        assert rc == 0
        files.append(f)
    capsys.readouterr()
    layers, (wh, bh, A), _ = JT.decoder_weights(pol)
    net = Net.__new__(Net)
    net.layers, net.wh, net.bh, net.A, net.d_in = [list(layer) for layer in layers], wh, bh, A, layers[0][0].shape[1]
    clips = [load_from_h5py(os.path.join(rollouts, f"clip_{c}.h5")) for c in range(len(TOOL_ROWS))]
    x = np.concatenate([np.concatenate([c["activations"]["intention"], c["activations"]["egocentric_obs"]], 1) for c in clips], 0).astype(f32)
    scale = np.exp(0.5 * np.concatenate([c["activations"]["encoder"]["logvar"] for c in clips], 0).astype(f64)).astype(f32)
    Z, n = scale.shape[1], x.shape[0]
    r64, r32 = reference64(net, x, (0, Z), 0, scale), restated32(net, x, (0, Z), 0, scale)
    jig = reference64(net, x, (0, Z), 0, scale, rel=(2.0 ** -22, 2.0 ** -22, 2.0 ** -23))
    floors = {k: float(np.abs(jig[k] - r64[k]).max()) for k in r64}
    cat = lambda f, k: np.concatenate([f[k][f"clip_{c}"] for c in range(len(TOOL_ROWS))], 0)      # noqa: E731
    for name, f in zip(("device", "emulation"), files):
        got = {"jac": cat(f, "jacobian"), "gain": cat(f, "gain"), "col2": cat(f, "latent_sensitivity"), "row2": cat(f, "actuator_sensitivity"),
               "action_var": cat(f, "action_var"), "mean_sum": f["mean_jacobian"] * n, "gram_in": f["gram_in"] * n, "gram_out": f["gram_out"] * n}
        within(got, r64, r32, floors, f"tool file, {name}")
    dev, emu = files
    assert abs(float(dev["forward_mismatch"]) - float(emu["forward_mismatch"])) < 1e-5
    weyl = float(np.linalg.norm(dev["gram_in"] - emu["gram_in"])) + 2.0 ** -38 * float(emu["explained_variance"][0]) + 2.0 ** -22 * float(emu["explained_variance"][0])
    assert np.abs(dev["explained_variance"].astype(f64) - emu["explained_variance"]).max() <= weyl      # (the last term: both are stored as float32)
