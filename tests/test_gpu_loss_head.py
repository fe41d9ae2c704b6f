"""GPU: the kernels between the network outputs and the parameter update against the float64 references of tests/loss_head_ref.py, per output row
(no network, no GEMM in between) and at the shapes where they can go wrong: T = 1, the 24-step register boundary, the single-block k_ppo_b
beyond it, B below / not a multiple of 64, A and Z below the 8-lane group, saturated inputs.

The bound of every compared array: with e32 the error of the float32 restatement (the same torch code in float32) against float64 in the same
metric — largest absolute error over the array's largest reference magnitude; for the eight scalars over max(1, |ref|) — the kernel's error must
be <= max(4 e32, 2^-20).  dlogits rows within 1e-3 of a clip edge may match either branch (tests/loss_head_ref.py says why; e32 is taken
outside that band).  Every case prints `LH | case | array | kernel error | e32 | bound`; DESIGN.md ("Loss head") has the measured table."""
import ctypes as C

import pytest
import torch

from tests import loss_head_ref as R
from track_mjx_amd import hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _run_head(inp, cfg, entry, accumulate=0, out=None):
    """tmjx_ppo_loss ("one") or tmjx_ppo_loss_phases with mask 15 ("phases") -> dlogits, dbaseline, dfc2, scratch, out (gradients prefilled with NaN:
    an element the kernel leaves out fails the comparison)"""
    L = hip.lib()
    T, B = cfg["T"], cfg["B"]
    ins = [inp[k].to(DEV).contiguous() for k in R.INPUT_KEYS]
    c = hip.PpoCfg(T, B, cfg["A"], cfg["Z"], cfg["reward_scaling"], cfg["discounting"], cfg["gae_lambda"], cfg["clip_eps"], cfg["entropy_cost"],
                   cfg["kl_weight"], cfg["normalize_advantage"], accumulate)
    nan = lambda t: torch.full_like(t, float("nan"))  # noqa: E731
    outs = [nan(ins[0]), nan(ins[4]), nan(ins[9]), torch.zeros(L.tmjx_ppo_scratch_floats(T, B), device=DEV),
            torch.zeros(8, device=DEV) if out is None else out]
    ptr = [_p(a) for a in ins + outs]
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    if entry == "one":
        hip.check(L.tmjx_ppo_loss(C.byref(c), *ptr, st), "tmjx_ppo_loss")
    else:
        hip.check(L.tmjx_ppo_loss_phases(C.byref(c), *ptr, 15, st), "tmjx_ppo_loss_phases")
    torch.cuda.synchronize()
    return outs


def _check(rows, tag):
    """rows: (array, kernel error, e32).  Prints all, then asserts all."""
    bad = []
    for name, err, e32 in rows:
        b = R.bound(e32)
        print(f"LH | {tag} | {name} | {err:.2e} | {e32:.2e} | {b:.2e}")
        if not err <= b:
            bad.append((name, err, e32, b))
    assert not bad, (tag, bad)


def _head_rows(got, r64, r32, near, N):
    dl, db, df, scratch, out = got
    rows = [("scalars", R.scalar_error(out, r64["scalars"]), R.scalar_error(r32["scalars"], r64["scalars"]))]
    rows += [(R.SCALAR_NAMES[k], R.scalar_error(out[k], r64["scalars"][k]), R.scalar_error(r32["scalars"][k], r64["scalars"][k])) for k in range(8)]
    rows.append(("dlogits", R.dlogits_error(dl, r64, near), R.dlogits_error(r32["dlogits"], r64, near, only_far=True)))
    for name, a in (("dbaseline", db), ("dfc2", df), ("vs", scratch[N:2 * N].view_as(db)), ("adv", scratch[2 * N:3 * N].view_as(db))):
        rows.append((name, R.array_error(a, r64[name]), R.array_error(r32[name], r64[name])))
    return rows


HEAD = [(fam, T, B, A, Z, norm, e) for fam, T, B, A, Z, norm, entries in R.whole_head_cases() for e in entries]


@pytest.mark.parametrize("fam,T,B,A,Z,norm,entry", HEAD, ids=[f"{c[0]}-T{c[1]}-B{c[2]}-A{c[3]}-Z{c[4]}-norm{c[5]}-{c[6]}" for c in HEAD])
def test_whole_head_against_float64(fam, T, B, A, Z, norm, entry):
    """all eight scalars, dlogits, dbaseline, dfc2 and vs / adv (scratch offsets N and 2 N); T > 24 runs k_ppo_b"""
    inp, cfg, r64, r32, near = R.reference(fam, T, B, A, Z, normalize_advantage=norm)
    got = _run_head(inp, cfg, entry)
    _check(_head_rows(got, r64, r32, near, T * B), f"{fam} {T}x{B} A{A} Z{Z} norm{norm} {entry} near {int(near.sum())}")


@pytest.mark.parametrize("entry", ["one", "phases"])
@pytest.mark.parametrize("T,B", [(7, 96), (24, 65)])
def test_entropy_gradient_alone(T, B, entry):
    """reward = baseline = bootstrap = 0, no advantage normalisation, entropy_cost 1, kl_weight 0: dlogits is the entropy term and nothing else
    (in the whole head it is 1e-2 of the surrogate term's size)"""
    inp, cfg, r64, r32, near = R.reference("hard", T, B, 38, 60, zero_value=True, normalize_advantage=0, entropy_cost=1.0, kl_weight=0.0)
    got = _run_head(inp, cfg, entry)
    assert float(got[3][2 * T * B:3 * T * B].abs().max()) == 0.0          # every advantage is zero
    _check(_head_rows(got, r64, r32, near, T * B), f"entropy-only hard {T}x{B} {entry}")


@pytest.mark.parametrize("entry", ["one", "phases"])
@pytest.mark.parametrize("T", [1, 2, 24])
def test_latent_kl_alone(T, entry):
    """kl_weight 1: scalar 4 and dfc2 at the first step (the N(0, 1) term, plus the AR(1) term of step 1 where T > 1), an interior step (both
    neighbours) and the last step (no successor), each against its own largest entry"""
    B, A, Z = 65, 38, 60
    inp, cfg, r64, r32, _ = R.reference("hard", T, B, A, Z, kl_weight=1.0)
    got = _run_head(inp, cfg, entry)
    rows = [("kl", R.scalar_error(got[4][4], r64["scalars"][4]), R.scalar_error(r32["scalars"][4], r64["scalars"][4])),
            ("dfc2", R.array_error(got[2], r64["dfc2"]), R.array_error(r32["dfc2"], r64["dfc2"]))]
    for t in sorted({0, T // 2, T - 1}):
        for half, sl in (("mean", slice(0, Z)), ("logvar", slice(Z, 2 * Z))):
            rows.append((f"dfc2[{t}].{half}", R.array_error(got[2][t, :, sl], r64["dfc2"][t, :, sl]), R.array_error(r32["dfc2"][t, :, sl], r64["dfc2"][t, :, sl])))
    _check(rows, f"kl-only hard {T}x{B} {entry}")


@pytest.mark.parametrize("entry", ["one", "phases"])
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_accumulate_adds_the_scalars(fam, entry):
    """a second call with cfg.accumulate onto the first call's `out`: twice the float64 scalars"""
    T, B, A, Z = 7, 96, 38, 60
    inp, cfg, r64, r32, _ = R.reference(fam, T, B, A, Z, normalize_advantage=1)
    first = _run_head(inp, cfg, entry)[4]
    twice = _run_head(inp, cfg, entry, accumulate=1, out=first.clone())[4]
    _check([("2 x scalars", R.scalar_error(twice, 2 * r64["scalars"]), R.scalar_error(2 * r32["scalars"], 2 * r64["scalars"]))], f"accumulate {fam} {T}x{B} {entry}")


def _gae_inputs(T, B):
    g = torch.Generator().manual_seed(1000 * T + B)
    u = torch.rand(T, B, generator=g)
    trunc, term = (u < 0.05).float(), ((u >= 0.05) & (u < 0.10)).float()          # about 5 % of the steps each, never both
    rew, val, boot = torch.randn(T, B, generator=g), torch.randn(T, B, generator=g), torch.randn(B, generator=g)
    if T * B >= 200:
        assert bool(trunc.any()) and bool(term.any())
    return trunc, term, rew, val, boot


@pytest.mark.parametrize("lam", [0.95, 1.0])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
@pytest.mark.parametrize("T", [1, 24, 30])
def test_gae_against_float64_recurrence(T, B, lam):
    L = hip.lib()
    ins = _gae_inputs(T, B)
    lam, disc = R.f32r(lam), R.f32r(0.98)
    vs64, adv64 = R.gae(*[x.double() for x in ins], lam, disc)
    vs32, adv32 = R.gae(*ins, lam, disc)
    d = [x.to(DEV) for x in ins]
    vs, adv = torch.full((T, B), float("nan"), device=DEV), torch.full((T, B), float("nan"), device=DEV)
    hip.check(L.tmjx_gae(*[_p(x) for x in d], lam, disc, _p(vs), _p(adv), T, B, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)), "tmjx_gae")
    torch.cuda.synchronize()
    _check([("vs", R.array_error(vs, vs64), R.array_error(vs32, vs64)), ("adv", R.array_error(adv, adv64), R.array_error(adv32, adv64))],
           f"gae {T}x{B} lambda {lam:.2f}")


def _adam_case(n, gnorm):
    hp = R.ADAM_HP
    ins = R.make_adam_inputs(n, gnorm)
    r64 = R.adam_clip_step(*[x.double() for x in ins], **hp)
    r32 = R.adam_clip_step(*ins, **hp)
    return ins, r64, r32


def _run_adam(ins, n, frozen=None):
    L, hp = hip.lib(), R.ADAM_HP
    p, g, m, v = (x.to(DEV).clone() for x in ins)
    scratch, norm = torch.zeros(L.tmjx_adam_norm_floats(), device=DEV), torch.full((1,), float("nan"), device=DEV)
    tail = (hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["bc1"], hp["bc2"], hp["max_norm"], C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    if frozen is None:
        rc = L.tmjx_adam_clip_norm(_p(p), _p(g), _p(m), _p(v), _p(scratch), _p(norm), n, *tail)
    else:
        rc = L.tmjx_adam_clip_norm_frozen(_p(p), _p(g), _p(m), _p(v), _p(scratch), _p(norm), n, frozen[0], frozen[1], *tail)
    assert rc == 0, L.tmjx_last_error()
    torch.cuda.synchronize()
    return norm, p, m, v


@pytest.mark.parametrize("gnorm", [0.5, 3.0], ids=["below", "above"])
@pytest.mark.parametrize("n", [3, 1021, 262_147, 1_048_579])
def test_adam_clip_norm_against_float64_step(n, gnorm):
    """float4 tails of 3, 1, 3 and 3 elements; fewer float4s than one stride of the 256 workgroups (partials that stay zero) up to many strides;
    a gradient norm below and above max_norm = 1; m and v nonzero with step 3's bias corrections"""
    ins, r64, r32 = _adam_case(n, gnorm)
    got = _run_adam(ins, n)
    assert (float(r64[0]) > R.ADAM_HP["max_norm"]) == (gnorm > 1)
    _check([(name, (R.scalar_error if name == "norm" else R.array_error)(a, b), (R.scalar_error if name == "norm" else R.array_error)(c, b))
            for name, a, b, c in zip(("norm", "p", "m", "v"), got, r64, r32)], f"adam n {n} norm {gnorm}")


def test_adam_frozen_range_against_float64_step():
    """tmjx_adam_clip_norm_frozen with [1000, 200000) of 262 147: p untouched inside, the reference's outside; m, v and the norm the reference's
    everywhere"""
    n, lo, hi = 262_147, 1000, 200_000
    ins, r64, r32 = _adam_case(n, 3.0)
    norm, p, m, v = _run_adam(ins, n, frozen=(lo, hi))
    assert torch.equal(p[lo:hi].cpu(), ins[0][lo:hi])
    out = torch.ones(n, dtype=torch.bool); out[lo:hi] = False
    _check([("norm", R.scalar_error(norm, r64[0]), R.scalar_error(r32[0], r64[0])),
            ("p outside", R.array_error(p.cpu()[out], r64[1][out]), R.array_error(r32[1][out], r64[1][out])),
            ("m", R.array_error(m, r64[2]), R.array_error(r32[2], r64[2])), ("v", R.array_error(v, r64[3]), R.array_error(r32[3], r64[3]))],
           f"adam frozen n {n} [{lo}, {hi})")
