"""The float64 reference of the LSTM-decoder-dynamics kernels (csrc/lstm_tangent_core.h), the case lists and the checkers that
tests/test_lstm_dynamics_cpu.py (the host emulation) and tests/test_gpu_lstm_dynamics.py (the C-ABI) share, built by the method of
tests/lstm_jacobian_ref.py.  A `backend` is analysis.pca.HipBackend or tests/hostemu/lstm_dynamics_emu.B.

The reference forms the dense carry-to-carry Jacobian J_t [W, W] of every row (W = 2 L H: the h blocks of every layer, then the c blocks) from the
analytic expressions of DESIGN.md "LSTM decoder dynamics" in numpy float64 (`dense_jacobians64`): with E_hk, E_ck the selectors of a layer's blocks
and A_(-1) = 0,  P_k = W_ih[k] A_(k-1) + W_hh[k] E_hk,  C_k = diag(gf) E_ck + diag(ki) P_i + diag(kf) P_f + diag(kg) P_g,  A_k = diag(ko) P_o +
diag(ka) C_k,  J = [A_0; ..; A_(L-1); C_0; ..; C_(L-1)].  It is checked once against torch.autograd.functional.jacobian of a double-precision step
built on the product's own agent.lstm._torch_lstm_layer (check_reference_against_autograd; a wrong formula shows at O(1), the check holds the
relative difference to 1e-12).  Along a sequence it pushes V = Q J_t^T, applies modified Gram-Schmidt twice in float64 and takes log R_jj
(`lyapunov64`).

How every bound is derived (tests/lstm_jacobian_ref.py).  Each checked array is computed twice on the test's own input: in float64, and by
`lyapunov32` / `step32`, a float32 numpy restatement of what the kernels perform in the order csrc/lstm_tangent_core.h states: every product a chain
acc = fmaf(a_k, b_k, acc) from 0 in ascending k, dpre = dxp + dhp, dc' = fmaf(kg, dg, fmaf(kf, df, fmaf(ki, di, gf dc))), dh' = fmaf(ka, dc', ko do),
the norms and dots as the chains of 256 threads over the elements tid, tid + 256, .. and their tree, q = v / r, v_i = fmaf(-d, q_j, v_i), two
sweeps, local = log(r1) + log(r2), the sums float64 in row order.  The kernel and the emulation are held to TWICE the distance between the two, plus a
floor: the float64 reference evaluated a second time with every logistic value and every tanh multiplied by 1 + delta, delta = +- 2^-22 with
seeded random signs, and the floor of an array is the largest absolute change that makes in it.  The bound is taken per family (the tangents:
q_out and the step's output; local; energy; sums), relative to each array's scale: the largest magnitude of the float64 array.  No tolerance is fixed
in advance; the figures are printed.

The reference asserts a condition on its own inputs (check_conditioning, on the CPU): in float64 every step of every case has
min_j R_jj / max_j R_jj >= 1e-3 and no sequence is longer than 16 rows, so that the basis never drifts inside a near-degenerate subspace, which
would hide or invent a failure.  Weight scales and seeds are picked for it: LeCun-scaled kernels, the forget gate's bias raised by FORGET_BIAS."""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

from tests.lstm_jacobian_ref import CHUNK, Net, _slice_of, chain, f32, f64, fma, same_bits  # noqa: F401
from tests.lstm_jacobian_ref import TOOL_ALIGNED, TOOL_ROWS, tool_clips, tool_policy
from track_mjx_amd import hip

FORGET_BIAS = 1.0
MIN_RATIO, MAX_ROWS = 1e-3, 16
# (H, L, d_in, K, the lengths of the sequences, ldx: None = dense, ld_carry: None = dense)
CASES = ((32, 1, 5, 1, (3, 1, 4), None, None),
         (32, 1, 5, 32, (3, 1, 4), None, None),                            # as many tangents as the limit: half the carry space
         (64, 2, 37, 5, (2, 5, 1), 41, 2 * 64 + 4),                        # an odd input width; row strides with poison in the padding
         (128, 2, 286, 16, (1, 2, 7, 13, 3, 5, 9, 4, 6), None, None),      # the shipped shape: 144 tangent rows cross a product tile, sequences end apart
         (256, 4, 1024, 32, (3, 3), None, None))                           # every limit at once
STEP_CASE = (32, 2, 7, 3, CHUNK + 1)      # (H, L, d_in, K, n): one row more than a pass
PROPERTY_CASE = (32, 2, 9, 4, (5, 1, 3), None, None)
LYAPUNOV_ARRAYS = ("local", "energy", "q_out", "status", "sums")


# ---------------------------------------------------------------------------------------------------------------- the problems
def make_net(d_in, H, L, seed):
    net = Net(d_in, H, L, 1, seed)
    for layer in net.layers:
        b = layer[2].copy()
        b[H:2 * H] += f32(FORGET_BIAS)
        layer[2] = b
    return net


def basis(W, K, seed=0):
    """[K, W] float32: orthonormal rows (the tool's first basis)."""
    from track_mjx_amd.analysis.dynamics import first_basis
    return first_basis(W, K, seed)


@functools.lru_cache(None)
def problem(case):
    """-> (net, x [n, d_in], h [n, L H], c [n, L H] (column slices of wider buffers where the case has row strides), seq_start int32 [S + 1],
    q0 [K, W]) float32, read-only."""
    H, L, d_in, K, lens, ldx, ldc = case
    n = int(sum(lens))
    net = make_net(d_in, H, L, 400 + (CASES.index(case) if case in CASES else 99))
    rng = np.random.default_rng(17)
    x = _slice_of(rng.standard_normal((n, d_in)), ldx)
    h = _slice_of(np.clip(0.5 * rng.standard_normal((n, L * H)), -0.99, 0.99), ldc)
    c = _slice_of(rng.standard_normal((n, L * H)), ldc)
    seq = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    q0 = basis(2 * L * H, K)
    for a in (x, h, c, seq, q0, *[t for layer in net.layers for t in layer]):
        a.setflags(write=False)
    return net, x, h, c, seq, q0


# ---------------------------------------------------------------------------------------------------------------- float64
def coefficients64(net, x, h, c, rel=None):
    """Per layer (ka, ki, kf, kg, ko, gf) [n, H] float64.  `rel`: the relative perturbation of every logistic value and every tanh."""
    H = net.H
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
        kept.append((go * (1.0 - tc * tc), gg * gi * (1.0 - gi), ck * gf * (1.0 - gf), gi * (1.0 - gg * gg), tc * go * (1.0 - go), gf))
        xk = go * tc
    return kept


def dense_jacobians64(net, x, h, c, rel=None):
    """-> J [n, W, W] float64: J[r] = d (h', c') / d (h, c) at row r, rows and columns in the order of the carry space."""
    L, H = net.L, net.H
    W, n = 2 * L * H, x.shape[0]
    kept = coefficients64(net, x, h, c, rel)
    J, eye, prev = np.zeros((n, W, W)), np.eye(W), None
    for k, (wi, wh, _) in enumerate(net.layers):
        ka, ki, kf, kg, ko, gf = (v[:, :, None] for v in kept[k])
        P = np.broadcast_to((wh.astype(f64) @ eye[k * H:(k + 1) * H])[None], (n, 4 * H, W))
        if prev is not None:
            P = P + wi.astype(f64)[None] @ prev
        Ck = gf * eye[None, (L + k) * H:(L + k + 1) * H] + ki * P[:, :H] + kf * P[:, H:2 * H] + kg * P[:, 2 * H:3 * H]
        prev = ko * P[:, 3 * H:] + ka * Ck
        J[:, k * H:(k + 1) * H], J[:, (L + k) * H:(L + k + 1) * H] = prev, Ck
    return J


def mgs2_64(V):
    """V [K, W] float64 -> (Q', the norms r1, r2 [K] of the two sweeps)."""
    V, rs = V.copy(), []
    for _ in range(2):
        r = np.zeros(V.shape[0])
        for j in range(V.shape[0]):
            r[j] = np.sqrt((V[j] * V[j]).sum())
            V[j] = V[j] / r[j] if r[j] > 0 else 0.0
            for i in range(j + 1, V.shape[0]):
                V[i] = V[i] - (V[j] @ V[i]) * V[j]
        rs.append(r)
    return V, rs[0], rs[1]


def energy_of(Q, L, H):
    return (Q * Q).reshape(Q.shape[0], 2 * L, H).sum(2)


def lyapunov64(net, x, h, c, seq, q0, warmup, rel=None):
    """-> {local [n, K], energy [n, K, 2 L], q_out [S, K, W], sums [S, K], ratio: the smallest min_j R_jj / max_j R_jj of any step} float64."""
    L, H, K = net.L, net.H, q0.shape[-2]
    J = dense_jacobians64(net, x, h, c, rel)
    n, S = x.shape[0], len(seq) - 1
    out = {"local": np.zeros((n, K)), "energy": np.zeros((n, K, 2 * L)), "q_out": np.zeros((S, K, 2 * L * H)), "sums": np.zeros((S, K)), "ratio": np.inf}
    for s in range(S):
        Q = np.asarray(q0 if q0.ndim == 2 else q0[s], f64)
        for r in range(seq[s], seq[s + 1]):
            Q, r1, r2 = mgs2_64(Q @ J[r].T)
            with np.errstate(divide="ignore"):
                out["local"][r] = np.log(r1 * r2)
            out["energy"][r] = energy_of(Q, L, H)
            if (r1 * r2).max() > 0:
                out["ratio"] = min(out["ratio"], float((r1 * r2).min() / (r1 * r2).max()))
            if r - seq[s] >= warmup:
                out["sums"][s] += out["local"][r]
        out["q_out"][s] = Q
    return out


# ---------------------------------------------------------------------------------------------------------------- the float32 restatement
def coefficients32(net, x, h, c):
    """Per layer (ka, ki, kf, kg, ko, gf) [n, H] float32 in the order of lsj_cell_fwd_wg."""
    H, one = net.H, f32(1)
    sig = lambda v: one / (one + np.exp(-v))      # noqa: E731
    xk, hh, cc, kept = np.asarray(x, f32), np.asarray(h, f32), np.asarray(c, f32), []
    for k, (wi, wh, b) in enumerate(net.layers):
        hk, ck = hh[:, k * H:(k + 1) * H], cc[:, k * H:(k + 1) * H]
        pre = (chain(xk, wi.T) + b) + chain(hk, wh.T)
        gi, gf, gg, go = sig(pre[:, :H]), sig(pre[:, H:2 * H]), np.tanh(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
        tc = np.tanh((gf * ck) + (gi * gg))
        kept.append((go * fma(-tc, tc, one), gg * (gi * (one - gi)), ck * (gf * (one - gf)), gi * fma(-gg, gg, one), tc * (go * (one - go)), gf))
        xk = go * tc
    return kept


def tangent32(net, kept, v, K):
    """v [rows K, W] float32 (tangent row m belongs to row m // K of `kept`) -> J v in the order of lst_cell_wg."""
    L, H = net.L, net.H
    out = np.zeros_like(v)
    for k, (wi, wh, _) in enumerate(net.layers):
        ka, ki, kf, kg, ko, gf = (np.repeat(t, K, 0) for t in kept[k])
        d = chain(v[:, k * H:(k + 1) * H], wh.T)
        if k > 0:
            d = chain(out[:, (k - 1) * H:k * H], wi.T) + d
        t = gf * v[:, (L + k) * H:(L + k + 1) * H]
        t = fma(ki, d[:, :H], t)
        t = fma(kf, d[:, H:2 * H], t)
        t = fma(kg, d[:, 2 * H:3 * H], t)
        out[:, (L + k) * H:(L + k + 1) * H] = t
        out[:, k * H:(k + 1) * H] = fma(ka, t, ko * d[:, 3 * H:])
    return out


def tree256(part):
    """part [R, 256] float32 -> [R]: the kernels' tree."""
    part, half = part.copy(), 128
    while half >= 1:
        part[:, :half] = part[:, :half] + part[:, half:2 * half]
        half //= 2
    return part[:, 0]


def dots32(a, b):
    """a [W] or [R, W], b [R, W] float32 -> [R]: thread tid folds the elements tid, tid + 256, .. into fmaf(a_e, b_e, .) from 0; then the tree."""
    a = np.broadcast_to(a, b.shape)
    part = np.zeros((b.shape[0], 256), f32)
    for e in range(0, b.shape[1], 256):
        w = min(256, b.shape[1] - e)
        part[:, :w] = fma(a[:, e:e + w], b[:, e:e + w], part[:, :w])
    return tree256(part)


def mgs2_32(V):
    """lst_qr_wg on V [K, W] float32 -> (Q', local [K] float32)."""
    V, K = V.copy(), V.shape[0]
    rs, tiny = np.zeros((2, K), f32), np.finfo(f32).tiny
    for sweep in range(2):
        for j in range(K):
            r = np.sqrt(dots32(V[j], V[j:j + 1]))[0]
            dead = not r >= tiny
            V[j] = 0 if dead else V[j] / r
            rs[sweep, j] = 0 if dead else r
            if j + 1 < K:
                d = dots32(V[j], V[j + 1:])
                V[j + 1:] = fma(-d[:, None], V[j][None], V[j + 1:])
    alive = (rs[0] > 0) & (rs[1] > 0)
    with np.errstate(divide="ignore"):
        local = np.where(alive, np.log(rs[0]) + np.log(rs[1]), -np.inf).astype(f32)
    return V, local


def energy32(Q, L, H):
    out = np.zeros((Q.shape[0], 2 * L), f32)
    for b in range(2 * L):
        part = np.zeros((Q.shape[0], 256), f32)
        lanes = (np.arange(b * H, (b + 1) * H)) % 256      # (H <= 256: one element of a block a thread)
        part[:, lanes] = Q[:, b * H:(b + 1) * H] * Q[:, b * H:(b + 1) * H]
        out[:, b] = tree256(part)
    return out


def lyapunov32(net, x, h, c, seq, q0, warmup):
    L, H, K = net.L, net.H, q0.shape[-2]
    kept = coefficients32(net, x, h, c)
    n, S = x.shape[0], len(seq) - 1
    out = {"local": np.zeros((n, K), f32), "energy": np.zeros((n, K, 2 * L), f32), "q_out": np.zeros((S, K, 2 * L * H), f32), "sums": np.zeros((S, K))}
    for s in range(S):
        Q = np.array(q0 if q0.ndim == 2 else q0[s], f32)
        for r in range(seq[s], seq[s + 1]):
            Q, out["local"][r] = mgs2_32(tangent32(net, [tuple(t[r:r + 1] for t in layer) for layer in kept], Q, K))
            out["energy"][r] = energy32(Q, L, H)
            if r - seq[s] >= warmup:
                out["sums"][s] += out["local"][r].astype(f64)
        out["q_out"][s] = Q
    return out


WARMUP = 1


@functools.lru_cache(None)
def references(case):
    """-> (float64, the float32 restatement, the floors) of a case's Lyapunov call with warmup = WARMUP, computed once."""
    net, x, h, c, seq, q0 = problem(case)
    r64, r32 = lyapunov64(net, x, h, c, seq, q0, WARMUP), lyapunov32(net, x, h, c, seq, q0, WARMUP)
    jig = lyapunov64(net, x, h, c, seq, q0, WARMUP, rel=2.0 ** -22)
    return r64, r32, {k: float(np.abs(jig[k] - r64[k]).max()) for k in ("local", "energy", "q_out", "sums")}


def within(got, r64, r32, floors, what, names=("local", "energy", "q_out", "sums")):
    """Every array of `names` against the references, each its own family: |got - r64| <= 2 |r32 - r64|_max + floor, all relative to the array's scale
    (the largest magnitude of the float64 array); prints the figures.  -> the worst ratio error / bound."""
    worst = 0.0
    for k in names:
        scale = float(np.abs(r64[k]).max())
        gap, floor = float(np.abs(np.asarray(r32[k], f64) - r64[k]).max()) / scale, floors[k] / scale
        err = float(np.abs(np.asarray(got[k], f64) - r64[k]).max()) / scale
        bound = 2.0 * gap + floor
        print(f"[lstm dynamics {what} {k}] error {err:.3g} of the scale {scale:.3g}; float32-float64 gap {gap:.3g}, transcendental floor {floor:.3g}: "
              f"{err / bound if err else 0.0:.3g} of the bound")
        assert np.isfinite(np.asarray(got[k], f64)).all() and err <= bound, (what, k, err, bound)
        worst = max(worst, err / bound if err else 0.0)
    return worst


def check_conditioning():
    """The condition the reference puts on its own inputs (the module's text)."""
    for case in CASES + (PROPERTY_CASE,):
        r64 = references(case)[0] if case in CASES else lyapunov64(*problem(case), WARMUP)
        print(f"[lstm dynamics] case {case[:4]}: the smallest min R_jj / max R_jj of any step is {r64['ratio']:.3g}")
        assert r64["ratio"] >= MIN_RATIO and max(case[4]) <= MAX_ROWS, case


# ---------------------------------------------------------------------------------------------------------------- the calls
def run(backend, net, x, h, c, seq, q0, warmup=WARMUP, want=("local", "energy", "q_out", "status")):
    return backend.lstm_lyapunov(backend.asarray(x), backend.asarray(h), backend.asarray(c), net.layers, seq, q0, warmup, want)


def check_case(case, backend, what=""):
    net, x, h, c, seq, q0 = problem(case)
    H, L, _, K, lens, _, _ = case
    r64, r32, floors = references(case)
    got = run(backend, net, x, h, c, seq, q0)
    assert set(got) == set(LYAPUNOV_ARRAYS) and (got["status"] == 0).all()
    assert got["local"].shape == (sum(lens), K) and got["energy"].shape == (sum(lens), K, 2 * L) and got["q_out"].shape == (len(lens), K, 2 * L * H)
    worst = within(got, r64, r32, floors, f"{what} case {CASES.index(case)}")
    # the rows of Q' have unit norm: the energies of a column sum to 1 (2 L H squares, each a rounded product, a tree, and the rounded quotient)
    assert (np.abs(got["energy"].astype(f64).sum(2) - 1.0) <= (2 * L * H + 8) * 2.0 ** -24).all()
    # the sums are the float64 sums of the stored local exponents from warmup on, in row order: bit for bit
    for s in range(len(lens)):
        total = np.zeros(K)
        for r in range(seq[s] + WARMUP, seq[s + 1]):
            total = total + got["local"][r].astype(f64)
        assert same_bits(got["sums"][s], total), s
    lean = run(backend, net, x, h, c, seq, q0, want=("local",))
    assert set(lean) == {"local", "sums"} and same_bits(lean["local"], got["local"]) and same_bits(lean["sums"], got["sums"])
    return worst


@functools.lru_cache(None)
def step_problem(decoupled=False):
    H, L, d_in, K, n = STEP_CASE
    net = make_net(d_in, H, L, 450)
    if decoupled:      # W_hh = 0 and W_ih[k > 0] = 0: the layers decouple, dpre = 0
        for k, layer in enumerate(net.layers):
            layer[1] = np.zeros_like(layer[1])
            if k > 0:
                layer[0] = np.zeros_like(layer[0])
    rng = np.random.default_rng(23)
    x = rng.standard_normal((n, d_in)).astype(f32)
    h = np.clip(0.5 * rng.standard_normal((n, L * H)), -0.99, 0.99).astype(f32)
    c = rng.standard_normal((n, L * H)).astype(f32)
    v = rng.standard_normal((n, K, 2 * L * H)).astype(f32)
    return net, x, h, c, v


def step(backend, net, x, h, c, v):
    return backend.lstm_tangent_step(backend.asarray(x), backend.asarray(h), backend.asarray(c), net.layers, v)


@functools.lru_cache(None)
def step_references(decoupled=False):
    net, x, h, c, v = step_problem(decoupled)
    n, K, W = v.shape
    r64 = np.einsum("rkw,ruw->rku", v.astype(f64), dense_jacobians64(net, x, h, c))
    jig = np.einsum("rkw,ruw->rku", v.astype(f64), dense_jacobians64(net, x, h, c, 2.0 ** -22))
    r32 = tangent32(net, coefficients32(net, x, h, c), v.reshape(n * K, W), K).reshape(n, K, W)
    return r64, r32, float(np.abs(jig - r64).max())


def check_step(backend, what=""):
    """tmjx_lstm_tangent_step across the pass boundary against J v in float64; a row alone has the bits it has in either pass."""
    net, x, h, c, v = step_problem()
    r64, r32, floor = step_references()
    got = step(backend, net, x, h, c, v)
    assert got.shape == v.shape
    worst = within({"out": got}, {"out": r64}, {"out": r32}, {"out": floor}, f"{what} step", names=("out",))
    assert same_bits(step(backend, net, x, h, c, v), got), "a second call gave other bits"
    for i in (0, CHUNK - 1, CHUNK):
        assert same_bits(step(backend, net, x[i:i + 1], h[i:i + 1], c[i:i + 1], v[i:i + 1])[0], got[i]), i
    return worst


def check_decoupled(backend, what=""):
    """W_hh = 0 and W_ih[k > 0] = 0 at L = 2: the c-block tangents follow the closed form dc' = gf dc, in float64 within the bound; the products
    are exactly zero, so the kernel's value is the one rounded product gf dc."""
    net, x, h, c, v = step_problem(True)
    H, L, _, K, n = STEP_CASE
    r64, r32, floor = step_references(True)
    got = step(backend, net, x, h, c, v)
    closed = np.concatenate([kept[5] for kept in coefficients64(net, x, h, c)], 1)[:, None, :] * v[:, :, L * H:].astype(f64)
    assert np.abs(closed - r64[:, :, L * H:]).max() <= 1e-15 * np.abs(closed).max()      # (the dense reference agrees with the closed form)
    within({"out": got[:, :, L * H:]}, {"out": closed}, {"out": r32[:, :, L * H:]}, {"out": floor}, f"{what} decoupled c blocks", names=("out",))
    gf32 = np.concatenate([kept[5] for kept in coefficients32(net, x, h, c)], 1)
    mine = step(backend, net, x[:4], h[:4], c[:4], np.ascontiguousarray(np.broadcast_to(np.eye(2 * L * H, dtype=f32)[L * H:L * H + K][None], (4, K, 2 * L * H))))
    # a unit tangent of c_0 comes back as gf itself in its own column and zero in every other c column; gf is the float32 gate within its documented error
    assert (mine[:, 0, L * H + 1:] == 0).all() and np.abs(mine[:, 0, L * H].astype(f64) - gf32[:4, 0]).max() <= 2.0 ** -21


def check_properties(backend, what=""):
    """The properties that hold exactly, bit for bit."""
    net, x, h, c, seq, q0 = problem(PROPERTY_CASE)
    H, L, d_in, K, lens, _, _ = PROPERTY_CASE
    S, W = len(lens), 2 * L * H
    base = run(backend, net, x, h, c, seq, q0)
    assert np.isfinite(base["local"]).all() and (base["status"] == 0).all()
    again = run(backend, net, x, h, c, seq, q0)
    assert all(same_bits(again[k], base[k]) for k in LYAPUNOV_ARRAYS), "a second call gave other bits"
    # a sequence alone
    for s in range(S):
        a, b = seq[s], seq[s + 1]
        one = run(backend, net, x[a:b], h[a:b], c[a:b], np.array([0, b - a], np.int32), q0)
        assert same_bits(one["local"], base["local"][a:b]) and same_bits(one["energy"], base["energy"][a:b]) and same_bits(one["q_out"][0], base["q_out"][s]), s
        assert same_bits(one["sums"][0], base["sums"][s]) and one["status"][0] == base["status"][s], s
    # seq_start permuted
    order = (2, 0, 1)
    rows = np.concatenate([np.arange(seq[s], seq[s + 1]) for s in order])
    pseq = np.concatenate([[0], np.cumsum([lens[s] for s in order])]).astype(np.int32)
    perm = run(backend, net, x[rows], h[rows], c[rows], pseq, q0)
    assert same_bits(perm["local"], base["local"][rows]) and same_bits(perm["energy"], base["energy"][rows])
    assert same_bits(perm["q_out"], base["q_out"][list(order)]) and same_bits(perm["sums"], base["sums"][list(order)])
    # the first j columns of a K-run are those of a K = j run
    for j in range(1, K):
        few = run(backend, net, x, h, c, seq, q0[:j])
        assert same_bits(few["local"], base["local"][:, :j]) and same_bits(few["energy"], base["energy"][:, :j]) and same_bits(few["q_out"], base["q_out"][:, :j]), j
        assert same_bits(few["sums"], base["sums"][:, :j]), j
    # one basis for all and the same basis per sequence
    per = run(backend, net, x, h, c, seq, np.broadcast_to(q0[None], (S, K, W)))
    assert all(same_bits(per[k], base[k]) for k in LYAPUNOV_ARRAYS)
    # cutting sequence 0 at row r and continuing from its q_out gives the rows of the uncut run; the sums add up
    T = lens[0]
    for r, warmup in ((2, 3), (2, 1), (4, 0)):
        whole = run(backend, net, x[:T], h[:T], c[:T], np.array([0, T], np.int32), q0, warmup)
        head = run(backend, net, x[:r], h[:r], c[:r], np.array([0, r], np.int32), q0, warmup)
        tail = run(backend, net, x[r:T], h[r:T], c[r:T], np.array([0, T - r], np.int32), head["q_out"], max(warmup - r, 0))
        assert same_bits(np.concatenate([head["local"], tail["local"]]), whole["local"]) and same_bits(np.concatenate([head["energy"], tail["energy"]]), whole["energy"])
        assert same_bits(tail["q_out"], whole["q_out"])
        if warmup >= r:      # (nothing counted before the cut: the same additions in the same order)
            assert (head["sums"] == 0).all() and same_bits(tail["sums"], whole["sums"])
        else:      # (within float64 order: the additions are regrouped)
            assert (np.abs(head["sums"] + tail["sums"] - whole["sums"]) <= T * 2.0 ** -52 * np.abs(whole["local"].astype(f64)).sum(0)).all()
    # a zero column of q0 stays zero, its local exponent is -inf, its status 1, and the other columns are those of the run without it
    dead = 1
    qz = q0.copy()
    qz[dead] = 0
    rest = [j for j in range(K) if j != dead]
    z, without = run(backend, net, x, h, c, seq, qz), run(backend, net, x, h, c, seq, q0[rest])
    assert (z["q_out"][:, dead] == 0).all() and np.isneginf(z["local"][:, dead]).all() and np.isneginf(z["sums"][np.array(lens) > WARMUP, dead]).all() and (z["energy"][:, dead] == 0).all()
    assert (z["status"] == 1).all() and (without["status"] == 0).all()
    assert same_bits(z["local"][:, rest], without["local"]) and same_bits(z["energy"][:, rest], without["energy"]) and same_bits(z["q_out"][:, rest], without["q_out"])
    assert same_bits(z["sums"][:, rest], without["sums"])
    # dense against strided rows with poison in the padding
    wide = run(backend, net, _slice_of(x, d_in + 4), _slice_of(h, L * H + 8), _slice_of(c, L * H + 8), seq, q0)
    assert all(same_bits(wide[k], base[k]) for k in LYAPUNOV_ARRAYS)


# ---------------------------------------------------------------------------------------------------------------- autograd
def check_reference_against_autograd():
    import torch
    from track_mjx_amd.agent.lstm import _torch_lstm_layer
    worst = 0.0
    for case in CASES[:4] + (PROPERTY_CASE,):
        net, x, h, c, _, _ = problem(case)
        H, L = net.H, net.L
        layers = [[torch.from_numpy(np.asarray(t, f64)) for t in layer] for layer in net.layers]
        J = dense_jacobians64(net, x[:2], h[:2], c[:2])
        for i in range(J.shape[0]):
            xv = torch.from_numpy(np.asarray(x[i], f64))

            def step(carry):
                xk, hs, cs = xv[None], [], []
                for k, (wi, wh, b) in enumerate(layers):
                    hk, ck = _torch_lstm_layer((xk @ wi.t())[None], wh, b, carry[None, k * H:(k + 1) * H], carry[None, (L + k) * H:(L + k + 1) * H], None)
                    xk = hk[0]
                    hs.append(hk[0, 0]); cs.append(ck[0, 0])
                return torch.cat(hs + cs)
            auto = torch.autograd.functional.jacobian(step, torch.from_numpy(np.concatenate([h[i], c[i]]).astype(f64))).numpy()
            worst = max(worst, float(np.linalg.norm(J[i] - auto)) / float(np.linalg.norm(auto)))
    print(f"[lstm dynamics] the analytic float64 carry-to-carry Jacobian against torch autograd: largest relative difference {worst:.3g}")
    assert worst < 1e-12


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(lib, alloc, ptr, untouched, what=""):
    """Every limit exceeded by one and every condition of include/tmjx.h returns TMJX_EINVAL (-22) and writes nothing.  The pointers of the
    descriptor and of the inputs are a dummy address: a refused call never reads them."""
    a = 1 << 20
    sums, ws, outs, stat = alloc((64,), f64, -7.25), alloc((4096,), f32, -7.25), alloc((4096,), f32, -7.25), alloc((16,), np.int32, -7)
    floats = C.c_int64(0)

    def desc(L=2, H=32, d_in=9, ldwi=None, ldwh=None, null=None, odd=None):
        d = hip.LstmJacobianDesc()
        d.L, d.H, d.d_in = L, H, d_in
        K = d_in
        for k in range(min(max(L, 0), 4)):
            y = d.layer[k]
            y.W_ih, y.W_hh, y.b_hh = a, a, a
            y.ldwi, y.ldwh = K if ldwi is None or ldwi[0] != k else ldwi[1], H if ldwh is None or ldwh[0] != k else ldwh[1]
            K = H
        if null is not None:
            setattr(d.layer[1], null, None)
        if odd is not None:
            setattr(d.layer[0], odd, a + 2)
        return d      # (Wp, bp, A and the wrt columns stay zero: they are not read)
    seq_ok = (C.c_int32 * 4)(0, 2, 3, 6)

    def lyap(d, x=a, n=6, ldx=9, h_in=a, c_in=a, ld_carry=64, seq=seq_ok, S=3, q0=a, per=0, K=4, warmup=0, local=None, q_out=None, sums_=None, ws_=None):
        o = ptr(outs)
        return lib.tmjx_lstm_lyapunov(None if d is None else C.byref(d), x, n, ldx, h_in, c_in, ld_carry, seq, S, q0, per, K, warmup, o if local is None else local, o,
                                      o if q_out is None else q_out, ptr(stat), ptr(sums) if sums_ is None else sums_, ptr(ws) if ws_ is None else ws_, None)

    def stp(d, x=a, n=6, ldx=9, h_in=a, c_in=a, ld_carry=64, v=a, K=4, out=None, ws_=None):
        return lib.tmjx_lstm_tangent_step(None if d is None else C.byref(d), x, n, ldx, h_in, c_in, ld_carry, v, K, ptr(outs) if out is None else out,
                                          ptr(ws) if ws_ is None else ws_, None)
    assert lib.tmjx_lstm_tangent_workspace(C.byref(desc()), 3, 4, C.byref(floats)) == 0 and floats.value > 0
    assert lib.tmjx_lstm_tangent_workspace(C.byref(desc(L=4, H=256, d_in=1024)), 840, 32, C.byref(floats)) == 0      # the limits themselves
    small, large = C.c_int64(0), C.c_int64(0)      # the workspace grows with S, K, H and L only: there is no n to give
    assert lib.tmjx_lstm_tangent_workspace(C.byref(desc()), 3, 4, C.byref(small)) == 0 and lib.tmjx_lstm_tangent_workspace(C.byref(desc()), 6, 4, C.byref(large)) == 0
    assert small.value < large.value <= 2 * small.value + 16
    bad_desc = (desc(L=0), desc(L=5), desc(H=0), desc(H=48), desc(H=16), desc(H=512), desc(d_in=0), desc(d_in=1025), desc(ldwi=(0, 8)), desc(ldwi=(1, 31)),
                desc(ldwh=(0, 31)), desc(ldwh=(1, 31)), *[desc(null=k) for k in ("W_ih", "W_hh", "b_hh")], *[desc(odd=k) for k in ("W_ih", "W_hh", "b_hh")])
    for i, d in enumerate(bad_desc):
        assert lib.tmjx_lstm_tangent_workspace(C.byref(d), 3, 4, C.byref(floats)) == -22 and lib.tmjx_last_error(), (what, i)
        assert lyap(d) == -22 and lib.tmjx_last_error(), (what, i)
        assert stp(d) == -22 and lib.tmjx_last_error(), (what, i)
    good = desc()
    for S, K in ((0, 4), (3, 0), (3, 33), (65537, 1), (-1, 4)):
        assert lib.tmjx_lstm_tangent_workspace(C.byref(good), S, K, C.byref(floats)) == -22 and lib.tmjx_last_error(), (what, S, K)
    assert lib.tmjx_lstm_tangent_workspace(C.byref(good), 3, 4, None) == -22 and lib.tmjx_lstm_tangent_workspace(None, 3, 4, C.byref(floats)) == -22
    seqs = {"descending": (0, 3, 2, 6), "empty": (0, 2, 2, 6), "short": (0, 2, 3, 5), "late": (1, 2, 3, 6)}
    bad_lyap = (dict(d=None), dict(x=None), dict(h_in=None), dict(c_in=None), dict(q0=None), dict(seq=None), dict(sums_=0), dict(ws_=0), dict(ldx=8), dict(ld_carry=63),
                dict(n=0), dict(S=0), dict(S=7), dict(K=0), dict(K=33), dict(warmup=-1), dict(per=2), dict(per=-1), *[dict(seq=(C.c_int32 * 4)(*v)) for v in seqs.values()],
                dict(ws_=ptr(ws) + 4), dict(sums_=ptr(sums) + 4), dict(q0=a + 4), dict(q_out=ptr(outs) + 4), dict(x=a + 2), dict(h_in=a + 1), dict(c_in=a + 2),
                dict(local=ptr(outs) + 2))
    for kw in bad_lyap:
        d = kw.pop("d", good)
        assert lyap(d, **kw) == -22 and lib.tmjx_last_error(), (what, kw)
    bad_step = (dict(d=None), dict(x=None), dict(h_in=None), dict(c_in=None), dict(v=None), dict(out=0), dict(ws_=0), dict(ldx=8), dict(ld_carry=63), dict(n=0), dict(K=0),
                dict(K=33), dict(ws_=ptr(ws) + 4), dict(v=a + 4), dict(out=ptr(outs) + 4), dict(x=a + 2), dict(h_in=a + 1), dict(c_in=a + 2))
    for kw in bad_step:
        d = kw.pop("d", good)
        assert stp(d, **kw) == -22 and lib.tmjx_last_error(), (what, kw)
    assert untouched(sums, -7.25) and untouched(ws, -7.25) and untouched(outs, -7.25) and untouched(stat, -7), f"{what}: a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------- the tool
TOOL_K, TOOL_WARMUP = 4, 2
TOOL_SEQUENCES = ((0, 0, 7), (1, 0, 5), (1, 5, 4), (2, 0, 4))      # (clip, first row, rows): clip 1 is cut behind its aligned step


def run_tool(tmp, backend, extra=(), pol=None, name="dynamics.h5", rollouts=None):
    from track_mjx_amd.analysis import dynamics as DT
    from track_mjx_amd.analysis.utils import load_from_h5py
    pol = tool_policy() if pol is None else pol
    rollouts = tool_clips(os.path.join(tmp, "rollouts"), pol) if rollouts is None else rollouts
    out = os.path.join(tmp, name)
    opts = {"rollouts": rollouts, "out": out, "k": TOOL_K, "warmup": TOOL_WARMUP, **dict(e.split("=", 1) for e in extra)}
    rc = DT.main([f"{k}={v}" for k, v in opts.items()], backend=backend, policy=pol)
    return rc, (load_from_h5py(out) if rc == 0 else None), pol, rollouts


def check_tool(tmp_path, backend, capsys):
    from track_mjx_amd.analysis import cluster as CL
    from track_mjx_amd.analysis import dynamics as DT
    from track_mjx_amd.analysis import jacobian as JT
    from track_mjx_amd.analysis.utils import load_from_h5py
    from tests.lstm_jacobian_ref import tool_inputs
    tmp = str(tmp_path)
    L, H, K = 2, 32, TOOL_K
    W, n = 2 * L * H, sum(TOOL_ROWS)
    assert TOOL_ALIGNED == (1, 4) and TOOL_ROWS == (7, 9, 4)
    feat = os.path.join(tmp, "dyn_dir")
    rc, f, pol, rollouts = run_tool(tmp, backend, ("store=true", "rate=50", f"features_out={feat}"))
    text = capsys.readouterr()
    assert rc == 0 and "conditional Lyapunov spectrum" in text.out and "forward mismatch" in text.out and "warning" not in text.err
    # file contents and shapes
    for cl, T in enumerate(TOOL_ROWS):
        assert f["local_exponents"][f"clip_{cl}"].shape == (T, K) and np.isfinite(f["local_exponents"][f"clip_{cl}"]).all()
        assert f["exponents_per_clip"][f"clip_{cl}"].shape == (K,) and f["final_basis"][f"clip_{cl}"].shape == (K, W) and f["energy_per_clip"][f"clip_{cl}"].shape == (T, K, 2 * L)
    assert f["exponents"].shape == (K,) and f["energy"].shape == (K, 2 * L) and np.abs(f["energy"].sum(1) - 1.0).max() < 1e-5
    assert f["sequences"].tolist() == [list(s) for s in TOOL_SEQUENCES] and f["status"].tolist() == [0] * 4 and f["sequence_counted_rows"].tolist() == [5, 3, 2, 2]
    counted = sum(t - TOOL_WARMUP for _, _, t in TOOL_SEQUENCES)
    assert int(f["rows"]) == n and int(f["counted_rows"]) == counted and f["clips"].tolist() == [0, 1, 2] and int(f["k"]) == K and int(f["warmup"]) == TOOL_WARMUP
    assert int(f["seed"]) == 0 and bytes(f["model"]) == b"lstm" and int(f["hidden_state_size"]) == H and int(f["hidden_layer_num"]) == L
    assert float(f["forward_mismatch"]) < 1e-5
    # exponents_per_clip is the mean of the local exponents past warmup of the clip's sequences; exponents that of all of them
    total = np.zeros(K)
    for cl in range(3):
        loc = f["local_exponents"][f"clip_{cl}"].astype(f64)
        mine = np.concatenate([loc[a + TOOL_WARMUP:a + t] for c_, a, t in TOOL_SEQUENCES if c_ == cl])
        assert np.abs(f["exponents_per_clip"][f"clip_{cl}"] - mine.mean(0)).max() <= 1e-12 * np.abs(mine).max(), cl
        total += mine.sum(0)
    assert np.abs(f["exponents"] - total / counted).max() <= 1e-12 * np.abs(total).max()
    lead = float(f["exponents"][0])
    assert np.allclose(f["exponents_per_second"], f["exponents"] * 50.0) and int(f["n_positive"]) == int((f["exponents"] > 0).sum())
    assert float(f["memory_halflife_steps"]) == (np.log(2.0) / -lead if lead < 0 else np.inf)
    assert float(f["memory_halflife_seconds"]) == float(f["memory_halflife_steps"]) / 50.0 and float(f["kaplan_yorke_dimension"]) == DT.kaplan_yorke(f["exponents"])
    assert DT.kaplan_yorke([0.5, -0.25, -1.0]) == 2.25 and DT.kaplan_yorke([-0.1, -0.2]) == 0.0 and DT.kaplan_yorke([0.3, 0.1]) == 2.0
    # the stored series are the call's on the inputs as lstm_jacobian_ref places them; the sequence behind the aligned step starts from the first basis
    x, h_in, c_in, _ = tool_inputs(rollouts)
    layers, _ = JT.lstm_decoder_weights(pol)
    starts = np.cumsum((0,) + TOOL_ROWS[:-1])
    seq = np.array([starts[c_] + a for c_, a, _ in TOOL_SEQUENCES] + [n], np.int32)
    direct = backend.lstm_lyapunov(backend.asarray(x), backend.asarray(h_in), backend.asarray(c_in), layers, seq, DT.first_basis(W, K, 0), TOOL_WARMUP)
    cat = lambda k: np.concatenate([f[k][f"clip_{c}"] for c in range(3)], 0)      # noqa: E731
    assert same_bits(cat("local_exponents"), direct["local"]) and same_bits(cat("energy_per_clip"), direct["energy"])
    assert same_bits(f["final_basis"]["clip_1"], direct["q_out"][2]) and same_bits(f["final_basis"]["clip_2"], direct["q_out"][3])
    cut = starts[1] + 5
    alone = backend.lstm_lyapunov(backend.asarray(x[cut:cut + 1]), backend.asarray(np.zeros_like(h_in[:1])), backend.asarray(np.zeros_like(c_in[:1])), layers,
                                  np.array([0, 1], np.int32), DT.first_basis(W, K, 0), 0)
    assert same_bits(alone["local"][0], direct["local"][cut])
    # features_out= round-trips through analysis.cluster, and its labels come back as labels=
    assert sorted(os.listdir(feat)) == ["clip_0.h5", "clip_1.h5", "clip_2.h5"]
    one = load_from_h5py(os.path.join(feat, "clip_1.h5"))
    assert int(one["meta"]["clip_idx"]) == 1 and same_bits(one["activations"]["local_exponents"], f["local_exponents"]["clip_1"])
    labels = os.path.join(tmp, "clusters.h5")
    assert CL.main([f"rollouts={feat}", "feature=local_exponents", "k=2", f"out={labels}"], backend=backend) == 0
    rc, g, _, _ = run_tool(tmp, backend, (f"labels={labels}",), pol, "labelled.h5", rollouts)
    assert rc == 0 and g["motif_local_exponents"].shape == (2, K) and int(g["motif_rows"].sum()) == counted and same_bits(g["exponents"], f["exponents"])
    lab = load_from_h5py(labels)["labels"]
    flat = np.concatenate([np.asarray(lab[f"clip_{c}"]).reshape(-1)[:T] for c, T in enumerate(TOOL_ROWS)])
    past = np.zeros(n, bool)
    for c_, a, t in TOOL_SEQUENCES:
        past[starts[c_] + a + TOOL_WARMUP:starts[c_] + a + t] = True
    for m in range(2):
        rows = (flat == m) & past
        assert int(g["motif_rows"][m]) == int(rows.sum())
        if rows.any():
            assert np.abs(g["motif_local_exponents"][m] - direct["local"][rows].astype(f64).mean(0)).max() <= 1e-12 * np.abs(direct["local"]).max()
    assert np.abs(np.nansum(g["motif_local_exponents"] * g["motif_rows"][:, None], 0) / counted - g["exponents"]).max() <= 1e-12 * np.abs(direct["local"]).max()
    capsys.readouterr()
    # a sequence with no row past warmup counts nothing and is named in one warning line
    rc, w, _, _ = run_tool(tmp, backend, ("warmup=4",), pol, "long_warmup.h5", rollouts)
    err = capsys.readouterr().err
    assert rc == 0 and w["sequence_counted_rows"].tolist() == [3, 1, 0, 0] and err.count("warning") == 1 and "clip_1 rows 5:9" in err and "clip_2 rows 0:4" in err
    assert int(w["counted_rows"]) == 3 + 1 and np.isnan(w["exponents_per_clip"]["clip_2"]).all() and np.isfinite(w["exponents_per_clip"]["clip_1"]).all()
    # refusals, each by name: an MLP checkpoint, no recorded carry, no recorded input, a replay directory, widths that do not match, options
    from tests.jacobian_ref import tool_policy as mlp_policy
    assert DT.main([f"rollouts={rollouts}", f"out={os.path.join(tmp, 'bad.h5')}"], backend=backend, policy=mlp_policy()) == 2 and "MLP decoder" in capsys.readouterr().err
    for kw, word in ((dict(hidden_state=False), "hidden_state"), (dict(egocentric_obs=False), "log_decoder_input=true"), (dict(replay=True), "replay_latents")):
        bad = tool_clips(os.path.join(tmp, "bad_" + next(iter(kw))), pol, **kw)
        assert run_tool(tmp, backend, (), pol, "bad.h5", bad)[0] == 2
        err = capsys.readouterr().err
        assert word in err and "LSTM" in err, (kw, err)
    assert run_tool(tmp, backend, (), tool_policy(latents=7), "bad.h5", rollouts)[0] == 2 and "did not make these roll-outs" in capsys.readouterr().err
    assert run_tool(tmp, backend, (), tool_policy(H=64), "bad.h5", rollouts)[0] == 2 and "did not make these roll-outs" in capsys.readouterr().err
    for extra, word in ((("k=0",), "k = 0"), (("k=33",), "k = 33"), (("warmup=-1",), "warmup"), (("rate=0",), "rate"), (("store=maybe",), "store")):
        assert run_tool(tmp, backend, extra, pol, "bad.h5", rollouts)[0] == 2 and word in capsys.readouterr().err, extra
    return f, pol, rollouts


def check_tool_files_agree(tmp_path, backend, emulation, capsys):
    """The tool on `backend` writes the file the emulation writes, within the bounds: the stored arrays of both lie within `within` of the same
    references."""
    from track_mjx_amd.analysis import dynamics as DT
    from track_mjx_amd.analysis import jacobian as JT
    from tests.lstm_jacobian_ref import tool_inputs
    files = []
    for name, bk in (("device", backend), ("emulation", emulation)):
        rc, f, pol, rollouts = run_tool(os.path.join(str(tmp_path), name), bk, ("store=true",))
        assert rc == 0
        files.append(f)
    capsys.readouterr()
    layers, _ = JT.lstm_decoder_weights(pol)
    net = Net.__new__(Net)
    net.layers, net.L, net.H, net.d_in = [list(y) for y in layers], len(layers), layers[0][1].shape[1], layers[0][0].shape[1]
    x, h_in, c_in, _ = tool_inputs(rollouts)
    n, starts = x.shape[0], np.cumsum((0,) + TOOL_ROWS[:-1])
    seq = np.array([starts[c_] + a for c_, a, _ in TOOL_SEQUENCES] + [n], np.int32)
    q0 = DT.first_basis(2 * net.L * net.H, TOOL_K, 0)
    r64, r32 = lyapunov64(net, x, h_in, c_in, seq, q0, TOOL_WARMUP), lyapunov32(net, x, h_in, c_in, seq, q0, TOOL_WARMUP)
    assert r64["ratio"] >= MIN_RATIO
    jig = lyapunov64(net, x, h_in, c_in, seq, q0, TOOL_WARMUP, rel=2.0 ** -22)
    floors = {k: float(np.abs(jig[k] - r64[k]).max()) for k in ("local", "energy", "q_out", "sums")}
    last = [0, 2, 3]      # the last sequence of every clip
    for name, f in zip(("device", "emulation"), files):
        cat = lambda k: np.concatenate([f[k][f"clip_{c}"] for c in range(len(TOOL_ROWS))], 0)      # noqa: E731
        got = {"local": cat("local_exponents"), "energy": cat("energy_per_clip"), "q_out": np.stack([f["final_basis"][f"clip_{c}"] for c in range(3)])}
        within(got, {**r64, "q_out": r64["q_out"][last]}, {**r32, "q_out": r32["q_out"][last]}, floors, f"tool file, {name}", names=("local", "energy", "q_out"))
        counted = int(f["counted_rows"])
        scale = float(np.abs(r64["sums"].sum(0)).max())
        err = float(np.abs(f["exponents"] * counted - r64["sums"].sum(0)).max())
        assert err <= 2.0 * float(np.abs(r32["sums"].sum(0) - r64["sums"].sum(0)).max()) + len(TOOL_SEQUENCES) * floors["sums"] + 1e-12 * scale, (name, err)
    dev, emu = files
    assert abs(float(dev["forward_mismatch"]) - float(emu["forward_mismatch"])) < 1e-5
