"""Plain torch reference for the recurrence kernels of the LSTM decoder (csrc/lstm_kernels.h: k_lstm_fwd<H> / k_lstm_bwd<H> behind tmjx_lstm_seq_fwd /
tmjx_lstm_seq_bwd), written from the RAW arrays of the two C entries (no module of track_mjx_amd.agent) and parametrised by the dtype it computes
in: float64 is the reference, the same code in float32 (the "restatement") gives the error `e32` a correct float32 evaluation has, and the kernels
must stay within `bound(e32) = max(4 e32, 2^-20)` in `array_error` — the convention of tests/loss_head_ref.py, whose metric, bound and floor are
imported here, not copied.

The cell is flax nn.LSTMCell (gate order i | f | g | o, no forget-gate offset), the carry zeroed BEFORE step t where reset[t] != 0 (so -0.0 keeps,
2.0 and -1.0 zero).  `lstm_forward` is differentiable torch; `lstm_layer` adds the backward pass BY HAND with the kernel's own formulae from the
gates and cell states of the same dtype, so that the restatement's backward is float32 throughout, as the kernel's is.
tests/test_lstm_ref_cpu.py holds the hand-written backward to float64 autograd through `lstm_forward`.

Case lists.  The template parameter H changes the kernels' shape: 256 / H row groups per 256-thread block, 8 H / 256 rows per thread, a W_h chunk
of 8 (H = 256) or 16 columns.  A block owns 8 rows.  CASES therefore crosses every H with rows 1 (one live row group), 7 / 8 / 9 (the block edge)
and 17 (three blocks, one live row in the last) and T = 1, 2 (the first step that reads hs[cur ^ 1] and c[t - 1]) and 20 (the unroll); LARGE_CASES
adds many blocks: 257 rows at the widest H, and 1365 rows (one env group: five rows in the last block) at the narrowest H and at the product's.

Conditioning cap.  A case whose e32 exceeds CAP = 2^-10 in any compared array would let the bound hide a wrong kernel:
tests/test_lstm_ref_cpu.py asserts the cap for the exact case lists, which the GPU test imports.  That is a condition on the inputs, not a
measurement of a kernel.

Intrinsics.  The kernels evaluate sigmoid as 1 / (1 + expf(-v)) and tanh as tanhf with the device math library; the restatement uses torch's CPU
float32 functions.  The device library documents expf at 1 ulp and tanhf at 2 ulp; the add and the correctly rounded divide of the sigmoid add
half an ulp each.  A gate is therefore good to about 2 ulp of a value <= 1 = 1.2e-7 of the gates' scale (1.0 in every case: each has a saturated
or near-saturated gate), an eighth of the floor 2^-20 that `bound` never goes below; through the cell, c' = f c + i g and h = o tanh(c') are
contractions of these errors (|d tanh| <= 1, gates <= 1) relative to scales >= the gates'.  So the floor already covers the documented accuracy
of the device functions at T = 1, and for T > 1 the compounded error is what e32 itself measures with functions of the same class.  No array
needed a term for the intrinsics on top of the plain bound: none is added (DESIGN.md "LSTM recurrence" has the measured table)."""
from __future__ import annotations

import numpy as np
import torch

from tests.loss_head_ref import FLOOR, array_error, bound, f32r  # noqa: F401  (re-exported)

CAP = 2.0 ** -10
FAMILIES = ("plain", "hard")
HIDDEN_SIZES = (32, 64, 128, 256)
ARRAYS = ("h", "c", "gates", "h_prev", "dgates", "dh0", "dc0")          # what the GPU test compares, in the kernels' write order
WEIGHT_GRADS = ("dW_h", "db")                                           # formed by the reference too; compared through the autograd glue
INPUT_KEYS = ("xg", "Wh", "bh", "h0", "c0", "reset", "dh")

# (family, rows, T, H)
CASES = tuple((f, r, T, H) for f in FAMILIES for H in HIDDEN_SIZES for r in (1, 7, 8, 9, 17) for T in (1, 2, 20))
LARGE_CASES = (("plain", 257, 20, 256), ("hard", 1365, 2, 32), ("plain", 1365, 3, 128))
NEG_ZERO_ROW = 2          # hard family, rows >= 3: reset[T - 1][2] = -0.0 (row 2 carries none of the family's other flags)


def case_id(case) -> str:
    return "-".join(str(v) for v in case)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def neg_zero_index(family, rows, T):
    """(t, row) of the case's -0.0 reset flag, or None"""
    return (T - 1, NEG_ZERO_ROW) if family == "hard" and rows > NEG_ZERO_ROW else None


def lstm_inputs(family, rows, T, H):
    """float32 CPU tensors under INPUT_KEYS, seeded from the arguments: xg [T, rows, 4H] (the input projection, as the GEMM in front of the
    recurrence leaves it), W_h [4H, H] = four orthogonal blocks, bh [4H], h0 / c0 [rows, H], reset [T, rows], the cotangent dh [T, rows, H].
    plain: xg ~ N(0, 1), bh ~ 0.1 N, h0, c0 ~ 0.5 N, reset = 1 with probability 0.1.
    hard: 5 % of xg at -100 and 5 % at +100 (expf overflows: sigmoids exactly 0 / 1, tanh exactly -+1), 15 % of xg times 8, c0 times 6 (tanh(c)
    saturates), reset[0, ::3] = 2.0, row 1 reset at every step with -1.0, about half the rows reset at the last step, one -0.0 (neg_zero_index)."""
    rng = np.random.default_rng([FAMILIES.index(family), rows, T, H])
    n = lambda *s: rng.standard_normal(s)  # noqa: E731
    xg = n(T, rows, 4 * H)
    Wh = np.concatenate([np.linalg.qr(n(H, H))[0] for _ in range(4)], 0)
    bh, h0, c0, dh = 0.1 * n(4 * H), 0.5 * n(rows, H), 0.5 * n(rows, H), n(T, rows, H)
    reset = (rng.random((T, rows)) < 0.1).astype(np.float64)
    if family == "hard":
        u = rng.random((T, rows, 4 * H))
        xg = np.where(u < 0.05, -100.0, np.where(u > 0.95, 100.0, np.where(u < 0.20, 8.0 * xg, xg)))
        c0 = 6.0 * c0
        last = rng.random(rows) < 0.5
        reset[T - 1, last] = 1.0
        reset[0, ::3] = 2.0
        if rows > 1:
            reset[:, 1] = -1.0
        nz = neg_zero_index(family, rows, T)
        if nz is not None:
            reset[nz] = -0.0
    return {"xg": _t(xg), "Wh": _t(Wh), "bh": _t(bh), "h0": _t(h0), "c0": _t(c0), "reset": _t(reset), "dh": _t(dh)}


def lstm_forward(xg, Wh, bh, h0, c0, reset):
    """T steps of the cell in the dtype of xg, differentiable: (h, c [T, rows, H], gates [T, rows, 4H] post-activation, h_prev, c_prev
    [T, rows, H] = the carry each step read, zero where reset).  reset [T, rows] of any dtype, or None."""
    T, rows, G4 = xg.shape
    H = G4 // 4
    h, c = h0, c0
    zero = torch.zeros((), dtype=xg.dtype)
    hs, cs, gs, hps, cps = [], [], [], [], []
    for t in range(T):
        if reset is not None:
            keep = (reset[t] == 0)[:, None]
            h, c = torch.where(keep, h, zero), torch.where(keep, c, zero)
        pre = (xg[t] + bh) + h @ Wh.t()
        gi, gf, gg, go = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        hps.append(h); cps.append(c)
        c = gf * c + gi * gg
        h = go * torch.tanh(c)
        hs.append(h); cs.append(c); gs.append(torch.cat([gi, gf, gg, go], -1))
    return tuple(torch.stack(v) for v in (hs, cs, gs, hps, cps))


def lstm_backward(dh, Wh, gates, c, c_prev, reset):
    """The reverse recurrence by hand, in the dtype of dh, with the kernel's formulae: (dgates [T, rows, 4H], dh0, dc0 [rows, H]).  c_prev is the
    cell state each step read (zero where reset)."""
    T, rows, H = dh.shape
    dhc, dcc = torch.zeros_like(dh[0]), torch.zeros_like(dh[0])          # d loss / d (h, c) of the carry that leaves step t
    zero = torch.zeros((), dtype=dh.dtype)
    out = [None] * T
    for t in range(T - 1, -1, -1):
        gi, gf, gg, go = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:3 * H], gates[t, :, 3 * H:]
        d = dh[t] + dhc
        tc = torch.tanh(c[t])
        dc = dcc + d * go * (1.0 - tc * tc)
        out[t] = torch.cat([dc * gg * gi * (1.0 - gi), dc * c_prev[t] * gf * (1.0 - gf), dc * gi * (1.0 - gg * gg), d * tc * go * (1.0 - go)], -1)
        dcc, dhc = dc * gf, out[t] @ Wh
        if reset is not None:
            keep = (reset[t] == 0)[:, None]
            dcc, dhc = torch.where(keep, dcc, zero), torch.where(keep, dhc, zero)
    return torch.stack(out), dhc, dcc


def lstm_layer(inp: dict, dtype=torch.float64) -> dict:
    """Everything the two kernels write, and the two weight gradients the learner forms from them, computed in `dtype` on the CPU from float32
    inputs.  `inp` without "dh": the forward arrays only."""
    xg, Wh, bh, h0, c0 = (inp[k].to(dtype) for k in ("xg", "Wh", "bh", "h0", "c0"))
    reset = inp.get("reset")
    with torch.no_grad():
        h, c, gates, h_prev, c_prev = lstm_forward(xg, Wh, bh, h0, c0, reset)
        out = {"h": h, "c": c, "gates": gates, "h_prev": h_prev, "c_prev": c_prev}
        if inp.get("dh") is not None:
            dgates, dh0, dc0 = lstm_backward(inp["dh"].to(dtype), Wh, gates, c, c_prev, reset)
            G4, H = gates.shape[-1], h.shape[-1]
            out.update(dgates=dgates, dh0=dh0, dc0=dc0, dW_h=dgates.reshape(-1, G4).t() @ h_prev.reshape(-1, H), db=dgates.reshape(-1, G4).sum(0))
    return out


def pre_activation(inp: dict, r64: dict) -> torch.Tensor:
    """float64 pre-activations [T, rows, 4H] of a case from its float64 result (which gates are saturated)"""
    return (inp["xg"].double() + inp["bh"].double()) + r64["h_prev"] @ inp["Wh"].double().t()


# ---- references computed once per process ------------------------------------------------------------------------------------------------
_cache: dict = {}


def reference(family, rows, T, H):
    """(inputs, float64 result, float32 result) of a case, computed once per process and shared; callers must not write to it"""
    key = (family, rows, T, H)
    if key not in _cache:
        inp = lstm_inputs(family, rows, T, H)
        _cache[key] = (inp, lstm_layer(inp, torch.float64), lstm_layer(inp, torch.float32))
    return _cache[key]


def e32_of(case) -> dict:
    """array -> error of the float32 restatement against float64, for ARRAYS and WEIGHT_GRADS"""
    _, r64, r32 = reference(*case)
    return {k: array_error(r32[k], r64[k]) for k in ARRAYS + WEIGHT_GRADS}
