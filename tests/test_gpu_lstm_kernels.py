"""GPU: the recurrence kernels of the LSTM decoder (csrc/lstm_kernels.h: k_lstm_fwd<H> / k_lstm_bwd<H>), through agent.lstm.lstm_seq_fwd /
lstm_seq_bwd, against the float64 reference of tests/lstm_ref.py at every hidden size the library is compiled for (32, 64, 128, 256 — each a
different row-to-thread mapping), rows around the 8-row block, T = 1, 2 and 20, every form of the reset flags, saturated gates, and the strided
operands the product hands them.

Against float64: each of h, c, gates, h_prev, dgates, dh0, dc0 must be within max(4 e32, 2^-20) of the reference in `array_error`, e32 being the
error of the float32 restatement of that array of that case (tests/test_lstm_ref_cpu.py keeps every e32 of these case lists under 2^-10).  The
backward pass is fed the kernel's own gates and c, as the learner feeds it.  Every case prints `LSTM | case | array | kernel error | e32 | bound |
index of the worst element`; DESIGN.md ("LSTM recurrence") has the measured table.

Bit-level properties (torch.equal): per output element the kernels run the same k-ordered fmaf chain and the same expressions whichever row group,
block, launch or row stride the element lives in.  A failure of one of them is a finding to explain, not a tolerance to loosen."""
import pytest
import torch

from tests import lstm_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 12345.0
ALL_CASES = R.CASES + R.LARGE_CASES
FWD, BWD = ("h", "c", "gates", "h_prev"), ("dgates", "dh0", "dc0")


def _dev(inp):
    return {k: v.to(DEV).contiguous() for k, v in inp.items()}


def _run(d, train=True, carry_grad=True, reset="own"):
    """forward, then backward from the kernel's own gates and c: the seven arrays (None where not asked for)"""
    from track_mjx_amd.agent.lstm import lstm_seq_bwd, lstm_seq_fwd
    rs = d["reset"] if reset == "own" else reset
    h, c, gates, h_prev = lstm_seq_fwd(d["xg"], d["Wh"], d["bh"], d["h0"], d["c0"], rs, train=train)
    out = {"h": h, "c": c, "gates": gates, "h_prev": h_prev}
    if train:
        out["dgates"], out["dh0"], out["dc0"] = lstm_seq_bwd(d["dh"], d["Wh"], gates, c, d["c0"], rs, want_carry_grad=carry_grad)
    torch.cuda.synchronize()
    return out


def _same(a, b, names, tag):
    bad = [n for n in names if not torch.equal(a[n], b[n])]
    assert not bad, (tag, {n: float((a[n] - b[n]).abs().max()) for n in bad})


def _worst(got, ref):
    d = (got.double().cpu() - ref).abs()
    return tuple(int(v) for v in torch.unravel_index(d.argmax(), d.shape))


@pytest.mark.parametrize("case", ALL_CASES, ids=R.case_id)
def test_kernels_against_float64(case):
    inp, r64, _ = R.reference(*case)
    e32 = R.e32_of(case)
    got = _run(_dev(inp))
    bad = []
    for name in R.ARRAYS:
        err, b = R.array_error(got[name], r64[name]), R.bound(e32[name])
        print(f"LSTM | {R.case_id(case)} | {name} | {err:.2e} | {e32[name]:.2e} | {b:.2e} | {_worst(got[name], r64[name])}")
        if not (bool(torch.isfinite(got[name]).all()) and err <= b):
            bad.append((name, err, e32[name], b, _worst(got[name], r64[name])))
    assert not bad, (case, bad)


# ---- bit-level properties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", R.HIDDEN_SIZES)
def test_T_steps_equal_T_launches_on_a_carry_in_place(H):
    """one T = 20 launch == 20 acting steps (T = 1) that read and overwrite one layer's slice of a [rows, L = 2, H] carry; the other layer's slice
    (a sentinel) is untouched"""
    from track_mjx_amd.agent.lstm import lstm_seq_fwd
    rows, T = 9, 20
    d = _dev(R.reference("hard", rows, T, H)[0])
    want = _run(d, train=False)
    for k in (0, 1):
        hc, cc = torch.full((rows, 2, H), SENTINEL, device=DEV), torch.full((rows, 2, H), SENTINEL, device=DEV)
        hc[:, k], cc[:, k] = d["h0"], d["c0"]
        hk, ck = hc[:, k], cc[:, k]
        for t in range(T):
            oh, oc, _, _ = lstm_seq_fwd(d["xg"][t:t + 1], d["Wh"], d["bh"], hk, ck, d["reset"][t:t + 1], out_h=hk.unsqueeze(0), out_c=ck.unsqueeze(0))
            assert oh.data_ptr() == hk.data_ptr() and oc.data_ptr() == ck.data_ptr()
            assert torch.equal(hk, want["h"][t]) and torch.equal(ck, want["c"][t]), (k, t)
        assert bool((hc[:, 1 - k] == SENTINEL).all()) and bool((cc[:, 1 - k] == SENTINEL).all())


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("H", R.HIDDEN_SIZES)
def test_rows_are_independent(family, H):
    """row r of a 17-row launch == the same row launched alone, forward and backward: first / last row of a block, the one-row last block"""
    d = _dev(R.reference(family, 17, 20, H)[0])
    full = _run(d)
    for r in (0, 7, 8, 16):
        one = {k: (v if k in ("Wh", "bh") else v[r:r + 1] if k in ("h0", "c0") else v[:, r:r + 1].contiguous()) for k, v in d.items()}
        alone = _run(one)
        part = {k: (v[r:r + 1] if k in ("dh0", "dc0") else v[:, r:r + 1]) for k, v in full.items()}
        _same(alone, part, R.ARRAYS, (family, H, r))


@pytest.mark.parametrize("case", [(f, r, T, H) for H in R.HIDDEN_SIZES for f, r, T in (("plain", 9, 20), ("hard", 17, 2))], ids=R.case_id)
def test_strided_operands_give_the_same_bits(case):
    """xg as a column slice of a wider buffer (pad = 1e6), W_h as [:, :H] of a [4H, H + 4] buffer, h0 / c0 as layer slices of a [rows, 2, H] carry;
    in the backward pass c0 strided without the carry gradient (with it, the wrapper hands the kernel a contiguous copy)"""
    from track_mjx_amd.agent.lstm import lstm_seq_bwd
    fam, rows, T, H = case
    d = _dev(R.reference(*case)[0])
    want = _run(d)
    wide = torch.full((T, rows, 4 * H + 8), 1e6, device=DEV)
    wide[:, :, :4 * H] = d["xg"]
    wbuf = torch.full((4 * H, H + 4), 1e6, device=DEV)
    wbuf[:, :H] = d["Wh"]
    hc, cc = torch.full((rows, 2, H), 1e6, device=DEV), torch.full((rows, 2, H), 1e6, device=DEV)
    hc[:, 1], cc[:, 1] = d["h0"], d["c0"]
    s = dict(d, xg=wide[:, :, :4 * H], Wh=wbuf[:, :H], h0=hc[:, 1], c0=cc[:, 1])
    assert s["xg"].stride(1) == 4 * H + 8 and s["Wh"].stride(0) == H + 4 and s["c0"].stride(0) == 2 * H
    _same(_run(s), want, R.ARRAYS, case)
    for one in ("xg", "Wh", "h0"):          # each alone, to name the operand
        s1 = dict(d, **({"h0": s["h0"], "c0": s["c0"]} if one == "h0" else {one: s[one]}))
        _same(_run(s1), want, R.ARRAYS, (case, one))
    dg, dh0, dc0 = lstm_seq_bwd(d["dh"], s["Wh"], want["gates"], want["c"], s["c0"], d["reset"], want_carry_grad=False)
    torch.cuda.synchronize()
    assert dh0 is None and dc0 is None and torch.equal(dg, want["dgates"])
    assert bool((hc[:, 0] == 1e6).all()) and bool((cc[:, 0] == 1e6).all()) and bool((wide[:, :, 4 * H:] == 1e6).all())


@pytest.mark.parametrize("H", R.HIDDEN_SIZES)
def test_optional_outputs_and_absent_reset(H):
    d = _dev(R.reference("hard", 9, 20, H)[0])
    want = _run(d)
    _same(_run(d), want, R.ARRAYS, "a second call")
    lean = _run(d, train=False)
    assert lean["gates"] is None and lean["h_prev"] is None
    _same(lean, want, ("h", "c"), "train=False")
    nocarry = _run(d, carry_grad=False)
    assert nocarry["dh0"] is None and nocarry["dc0"] is None
    _same(nocarry, want, FWD + ("dgates",), "want_carry_grad=False")
    zeros = _run(d, reset=torch.zeros_like(d["reset"]))
    _same(_run(d, reset=None), zeros, R.ARRAYS, "reset=None")
    assert not torch.equal(zeros["h"], want["h"])
    # and against float64 with no resets: the one case where the carry of every row runs through all 20 steps
    inp = {**R.reference("hard", 9, 20, H)[0], "reset": None}
    r64, r32 = R.lstm_layer(inp), R.lstm_layer(inp, torch.float32)
    for name in R.ARRAYS:
        err, e32 = R.array_error(zeros[name], r64[name]), R.array_error(r32[name], r64[name])
        print(f"LSTM | no-reset-9-20-{H} | {name} | {err:.2e} | {e32:.2e} | {R.bound(e32):.2e}")
        assert e32 <= R.CAP and err <= R.bound(e32), (name, err, e32)


HARD_EXACT = tuple(("hard", 17, T, H) for H in R.HIDDEN_SIZES for T in (2, 20)) + (("hard", 1365, 2, 32),)


@pytest.mark.parametrize("case", HARD_EXACT, ids=R.case_id)
def test_saturated_gates_and_reset_steps_are_exact(case):
    """xg = -+100: expf overflows to infinity and the stored gate is exactly 0 / 1 (g slab: -+1), asserted where the float64 pre-activation is beyond
    -+90; h_prev is exactly 0 at reset steps (whatever non-zero value the flag has), the carry otherwise; every output is finite"""
    H = case[3]
    inp, r64, _ = R.reference(*case)
    got = {k: v.cpu() for k, v in _run(_dev(inp)).items()}
    assert all(bool(torch.isfinite(got[k]).all()) for k in R.ARRAYS)
    pre = R.pre_activation(inp, r64)
    lo, hi = pre < -90, pre > 90
    sig = torch.ones(4 * H, dtype=torch.bool)
    sig[2 * H:3 * H] = False
    assert int((lo & sig).sum()) > 50 and int((hi & sig).sum()) > 50 and int((lo & ~sig).sum()) > 10 and int((hi & ~sig).sum()) > 10
    g = got["gates"]
    assert bool((g[lo & sig] == 0).all()) and bool((g[hi & sig] == 1).all()) and bool((g[lo & ~sig] == -1).all()) and bool((g[hi & ~sig] == 1).all())
    flagged = inp["reset"] != 0
    assert int(flagged.sum()) > 0 and bool((got["h_prev"][flagged] == 0).all())
    assert torch.equal(got["h_prev"][0][~flagged[0]], inp["h0"][~flagged[0]])
    if case[2] > 1:
        assert torch.equal(got["h_prev"][1:][~flagged[1:]], got["h"][:-1][~flagged[1:]])
    at0 = flagged[0]
    assert bool((got["dh0"][at0] == 0).all()) and bool((got["dc0"][at0] == 0).all())


# ---- autograd glue at the hidden sizes no other test runs --------------------------------------------------------------------------------
GLUE_TOL = 1e-4          # tests/test_gpu_lstm.py's: these go through the GEMM kernels too


@pytest.mark.parametrize("H", (32, 256))
def test_lstm_seq_function_matches_float64(H):
    from track_mjx_amd.agent.lstm import _LstmSeqFn
    case = ("plain", 50, 6, H)
    inp, r64, _ = R.reference(*case)
    d = _dev(inp)
    xg, Wh, bh = (d[k].clone().requires_grad_(True) for k in ("xg", "Wh", "bh"))
    h = _LstmSeqFn.apply(xg, Wh, bh, d["h0"], d["c0"], d["reset"])
    dxg, dWh, dbh = torch.autograd.grad(h, (xg, Wh, bh), d["dh"])
    torch.cuda.synchronize()
    errs = {n: R.array_error(g, r64[n]) for n, g in (("h", h.detach()), ("dgates", dxg), ("dW_h", dWh), ("db", dbh))}
    print(f"LSTM | _LstmSeqFn {R.case_id(case)} | {errs}")
    assert all(e <= GLUE_TOL for e in errs.values()), errs


def _ref_policy(pol, obs, h0, c0, reset):
    """float64 restatement of the policy's sequence pass over the module's parameters (Dense -> SiLU -> LayerNorm, z = mean, stacked cells of
    tests/lstm_ref.py, projection), differentiable"""
    F = torch.nn.functional
    P = {n: p.detach().double().cpu().requires_grad_(True) for n, p in pol.named_parameters()}
    x = obs[..., :pol.reference_obs_size]
    for i in range(len(pol.encoder)):
        x = F.silu(x @ P[f"encoder.{i}.dense.weight"].t() + P[f"encoder.{i}.dense.bias"])
        x = F.layer_norm(x, (x.shape[-1],), P[f"encoder.{i}.norm.weight"], P[f"encoder.{i}.norm.bias"], 1e-6)
    fc2 = x @ P["fc2.weight"].t() + P["fc2.bias"]
    x = torch.cat([fc2[..., :pol.latents], obs[..., pol.reference_obs_size:]], -1)
    for k in range(pol.hidden_layer_num):
        x = R.lstm_forward(x @ P[f"w_ih.{k}"].t(), P[f"w_hh.{k}"], P[f"b_hh.{k}"], h0[:, k], c0[:, k], reset)[0]
    return x @ P["projection.weight"].t() + P["projection.bias"], fc2, P


@pytest.mark.parametrize("H", (32, 256))
def test_lstm_policy_module_matches_float64_autograd(H):
    from track_mjx_amd.agent.lstm import LSTMIntentionPolicy
    torch.manual_seed(0)
    W, ref, A, Z, T, B, L = 96, 60, 6, 8, 6, 50, 2
    pol = LSTMIntentionPolicy(W, ref, A, Z, (64, 64), H, L).to(DEV)
    g = torch.Generator().manual_seed(H)
    obs = torch.randn(T, B, W, generator=g, dtype=torch.float64)
    h0, c0 = torch.randn(B, L, H, generator=g, dtype=torch.float64) * 0.5, torch.randn(B, L, H, generator=g, dtype=torch.float64) * 0.5
    reset = (torch.rand(T, B, generator=g) < 0.1).double()
    R1, R2 = torch.randn(T, B, 2 * A, generator=g, dtype=torch.float64), torch.randn(T, B, 2 * Z, generator=g, dtype=torch.float64)
    lr, fr, P = _ref_policy(pol, obs, h0, c0, reset)
    ((lr * R1).sum() + (fr * R2).sum()).backward()
    f = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    logits, fc2 = pol(f(obs), f(h0), f(c0), f(reset))
    grads = torch.autograd.grad((logits * f(R1)).sum() + (fc2 * f(R2)).sum(), list(pol.parameters()))
    torch.cuda.synchronize()
    errs = {"logits": R.array_error(logits.detach(), lr.detach()), "fc2": R.array_error(fc2.detach(), fr.detach())}
    errs.update({n: R.array_error(gd, P[n].grad) for (n, _), gd in zip(pol.named_parameters(), grads)})
    for n, e in errs.items():
        print(f"LSTM | policy H={H} | {n} | {e:.2e}")
    bad = {n: e for n, e in errs.items() if not e <= GLUE_TOL}
    assert not bad, bad
