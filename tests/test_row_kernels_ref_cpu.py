"""CPU: conditions on the references of tests/row_kernels_ref.py alone, for the exact case lists tests/test_gpu_row_kernels.py compares the kernels
on.  They must hold before a GPU comparison against these references means anything: every hand-written reference agrees with torch's own ops and
autograd in float64, and the float32 restatement of every case stays under the conditioning cap 2^-10 in every compared array (a case above it
would let max(4 e32, 2^-20) hide a wrong kernel).  Also here, because they need no device: the refusals of the entry points."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import row_kernels_ref as R
from track_mjx_amd import hip


def _close(a, b, tol=1e-12):
    return R.array_error(a, b.double()) <= tol


def _cap(rows, tag):
    bad = []
    for name, e32 in rows:
        print(f"RK-ref | {tag} | {name} | e32 {e32:.2e}")
        if not e32 <= R.CAP:
            bad.append((name, e32))
    assert not bad, (tag, bad)


def test_case_lists_are_the_ones_the_comparison_was_specified_on():
    assert len(R.BLOCK_FWD_CASES) == 2 * 5 * 3 + 6 + 1 and ("hard", 8193, 1024) in R.BLOCK_FWD_CASES
    assert {c[1] for c in R.BLOCK_FWD_CASES} == {1, 3, 35, 8192, 8193, 16389} and {c[2] for c in R.BLOCK_FWD_CASES} == set(R.BLOCK_WIDTHS)
    assert len(R.BLOCK_BWD_CASES) == 2 * 5 * 6 + 5 and {c[1] for c in R.BLOCK_BWD_CASES if c[2] == 64} >= {1, 3, 5, 31, 32, 33, 256, 257, 2048, 2049, 8193}
    assert {(r + 31) // 32 for _, r, H in R.BLOCK_BWD_CASES if r >= 256} == {8, 9, 64, 65, 257}
    assert {(c[1], c[2]) for c in R.BLOCK_BF16_CASES} == {(r, H) for r in (1, 35, 8193) for H in (128, 512)}
    assert R.SILU_CASES == ((1, 1), (1, 3), (7, 5), (341, 3), (1025, 38), (33, 256), (1, 4)) and R.SILU_RANK1_CASES == ((1, 4), (333, 8), (65, 260))
    assert R.STATS_CASES == ((1, 4), (3, 260), (511, 8), (512, 8), (513, 260), (16417, 696)) and R.STATS_PINNED[1:] == (260, (0, 4, 256, 257, 260))
    assert R.LATENT_CASES == ((1, 1, 1, 0, 2), (5, 3, 7, 7, 3), (65, 60, 696, 470, 288), (8192, 16, 24, 8, 32), (8193, 16, 24, 8, 32), (700, 60, 400, 60, 400))
    assert R.LATENT_BWD_CASES == ((1, 1, 1), (65, 60, 288), (4097, 60, 64))
    assert R.ACTION_CASES == ((1, 1), (1, 38), (31, 7), (33, 8), (65, 9), (8192, 38), (8193, 38))
    assert R.HEAD_CASES == ((1, 4), (15, 252), (17, 256), (33, 260), (1, 1024))
    assert len(R.COLSUM_WIDTHS) == len(R.COLSUM_ROWS) == 16 and set(R.COLSUM_WIDTHS) >= {1, 31, 32, 33, 76, 768}
    assert set(R.COLSUM_ROWS) >= {1, 7, 8, 9, 57, 64, 65, 640}


# ---- the references against torch's own ops ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("rows,H", [(1, 64), (35, 128), (33, 1024)])
def test_block_reference_agrees_with_layer_norm_and_autograd(family, rows, H):
    inp = R.block_inputs(family, rows, H)
    r = R.block(inp)
    z, b, g, be = (inp[k].double().requires_grad_(True) for k in ("z", "bias", "gamma", "beta"))
    a = F.silu(z + b)
    y = F.layer_norm(a, (H,), g, be, R.LN_EPS)
    dz, db, dg, dbe = torch.autograd.grad(y, (z, b, g, be), inp["dy"].double())
    var, mean = torch.var_mean(a.detach(), -1, unbiased=False)
    for name, want in (("y", y.detach()), ("mean", mean), ("rstd", (var + R.LN_EPS).rsqrt()), ("dz", dz), ("dgamma", dg), ("dbeta", dbe), ("dbias", db)):
        assert _close(r[name], want), name


def test_hard_block_family_has_its_rows():
    inp, r64, _ = R.block_reference("hard", 35, 256)
    assert bool((inp["z"] == -30).any()) and float(inp["z"].max()) > 20
    assert abs(float(r64["rstd"][0]) - 1000.0) < 1e-3 and float(r64["rstd"][2:].max()) < 20          # the dead row: variance far below eps
    assert float(inp["z"][1].std()) < 2e-4
    inp1 = R.block_inputs("hard", 1, 64)
    assert float(inp1["z"].max()) > -39          # rows < 3: no dead row


@pytest.mark.parametrize("family", R.FAMILIES)
def test_silu_reference_agrees_with_autograd(family):
    inp = R.silu_inputs(family, 33, 256)
    r = R.silu_halves(inp)
    z = inp["z"].double().requires_grad_(True)
    y = F.silu(z + inp["bias"].double())
    dz, = torch.autograd.grad(y, z, inp["dy"].double(), retain_graph=True)
    d1, = torch.autograd.grad(y, z, inp["dy1"].double()[:, None] * inp["w1"].double()[None, :])
    assert _close(r["y"], y.detach()) and _close(r["dz"], dz) and _close(r["dz_rank1"], d1)
    if family == "hard":
        v = inp["z"] + inp["bias"]
        assert bool((inp["z"] == -90).any()) and float(v[inp["z"] != -90].abs().max()) <= 30 and float(v.abs().max()) > 25


def test_stats_reference_is_the_population_variance_and_the_one_pass_form():
    """from a zero state one update is the batch's mean and n x its population variance; a second update equals one update on both batches; the
    kernels' one-pass form S2 - (S1 / count) S1 is the same number"""
    rng = np.random.default_rng(7)
    a, b = torch.from_numpy(rng.standard_normal((40, 6)) * 3 + 1), torch.from_numpy(rng.standard_normal((25, 6)) - 2)
    zero = torch.zeros(6, dtype=torch.float64)
    c1, m1, v1, s1 = R.stats_update(a, 0.0, zero, zero)
    assert c1 == 40 and _close(m1, a.mean(0)) and _close(v1, 40 * a.var(0, unbiased=False)) and _close(s1, a.std(0, unbiased=False))
    c2, m2, v2, s2 = R.stats_update(b, c1, m1, v1)
    both = torch.cat([a, b])
    assert c2 == 65 and _close(m2, both.mean(0)) and _close(v2, 65 * both.var(0, unbiased=False)) and _close(s2, both.std(0, unbiased=False))
    S1, S2 = R.stats_sums(b, m1)
    assert _close(v1 + (S2 - (S1 / c2) * S1), v2) and _close(m1 + S1 / c2, m2)
    # pinned: columns >= pin_lo keep their state, the count grows
    c3, m3, v3, s3 = R.stats_update(b, c1, m1, v1, pin_lo=4, std=s1)
    assert c3 == 65 and torch.equal(m3[4:], m1[4:]) and torch.equal(v3[4:], v1[4:]) and torch.equal(s3[4:], s1[4:])
    assert torch.equal(m3[:4], m2[:4]) and torch.equal(v3[:4], v2[:4]) and torch.equal(s3[:4], s2[:4])


def test_latent_reference_agrees_with_autograd():
    n, Z, obs_w, ref_w, stride = 65, 60, 696, 470, 288
    inp = R.latent_inputs("hard", n, Z, obs_w, stride)
    fc2 = inp["fc2"].double().requires_grad_(True)
    mean, logvar = fc2[:, :Z], fc2[:, Z:]
    lat = mean + inp["eps"].double() * torch.exp(0.5 * logvar)
    prop = (inp["obs"].double()[:, ref_w:] - inp["mean_o"].double()[ref_w:]) / inp["std_o"].double()[ref_w:]
    x = torch.cat([lat, prop, torch.zeros(n, stride - Z - (obs_w - ref_w), dtype=torch.float64)], -1)
    assert _close(R.latent_concat(inp, Z, obs_w, ref_w, stride, True), x.detach())
    assert torch.equal(R.latent_concat(inp, Z, obs_w, ref_w, stride, False)[:, Z:Z + obs_w - ref_w], inp["obs"].double()[:, ref_w:])
    g, = torch.autograd.grad(x, fc2, inp["dx"].double())
    assert _close(R.latent_concat_bwd(inp, Z, False), g) and _close(R.latent_concat_bwd(inp, Z, True), g + inp["add"].double())
    assert bool((inp["fc2"][:, Z:] == 8).any()) and bool((inp["fc2"][:, Z:] == -8).any())


def test_action_reference_agrees_with_torch_distributions():
    from torch.distributions import Normal, TanhTransform, TransformedDistribution
    inp = R.action_inputs("plain", 33, 8)
    r = R.sample_action(inp)
    lg = inp["logits"].double()
    scale = F.softplus(lg[:, 8:]) + 0.001
    raw = lg[:, :8] + scale * inp["noise"].double()
    d = TransformedDistribution(Normal(lg[:, :8], scale), [TanhTransform(cache_size=1)])
    act = torch.tanh(raw)
    # (log_prob through the transform's inverse loses digits near |action| = 1: the plain family stays away from it)
    assert _close(r["raw"], raw) and _close(r["action_t"], act.t()) and R.array_error(r["logp"], d.log_prob(act).sum(-1)) <= 1e-9
    hard = R.action_inputs("hard", 65, 9)["logits"][:, 9:]
    assert bool((hard == -30).any()) and bool((hard > 20).any())


# ---- the conditioning cap, for the exact case lists ---------------------------------------------------------------------------------------
def _block_ids(cases):
    return [f"{f}-{r}x{H}" for f, r, H in cases]


_BLOCK_ALL = tuple(dict.fromkeys(R.BLOCK_FWD_CASES + R.BLOCK_BWD_CASES + R.BLOCK_BF16_CASES))


@pytest.mark.parametrize("case", _BLOCK_ALL, ids=_block_ids(_BLOCK_ALL))
def test_block_cases_are_under_the_cap(case):
    _, r64, r32 = R.block_reference(*case)
    for r in (r64, r32):
        assert all(bool(torch.isfinite(r[k]).all()) for k in R.BLOCK_ARRAYS)
    _cap([(k, R.block_error(k, r32[k], r64)) for k in R.BLOCK_ARRAYS], "block %s %dx%d" % case)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_silu_cases_are_under_the_cap(family):
    for rows, N in R.SILU_CASES + R.SILU_RANK1_CASES:
        inp = R.silu_inputs(family, rows, N)
        r64, r32 = R.silu_halves(inp), R.silu_halves(inp, torch.float32)
        _cap([(k, R.array_error(r32[k], r64[k])) for k in ("y", "dz", "dz_rank1")], f"silu {family} {rows}x{N}")


@pytest.mark.parametrize("family", R.STATS_FAMILIES)
@pytest.mark.parametrize("rows,W", R.STATS_CASES)
def test_stats_cases_are_under_the_cap(family, rows, W):
    """every compared array of the normaliser, the sigma = 1e-9 and 1e7 columns included; both binding columns give exactly the clip values, in
    both precisions; the constant column has reference variance 0"""
    inp = R.stats_inputs(family, rows, W)
    r64, r32 = R.stats_reference(inp), R.stats_reference(inp, torch.float32)
    assert r64["count"] == r32["count"] == inp["count"] + rows
    _cap(R.stats_rows(r32, r64, inp), f"stats {family} {rows}x{W}")
    deg = R.degenerate_columns(r64)
    for r in (r64, r32):
        assert bool(torch.isfinite(r["std"]).all()) and float(r["std"].min()) >= R.STD_MIN and float(r["std"].max()) <= R.STD_MAX
    if family == "cold":
        assert bool(deg[R.COL_CONSTANT]) and (rows == 1 or int(deg.sum()) == 1)
        if rows > 1:      # (one row from a zero state: every variance is 0 and every std the lower clip value)
            for r in (r64, r32):
                assert float(r["std"][R.COL_TINY]) == R.STD_MIN and float(r["std"][R.COL_HUGE]) == R.STD_MAX
            # without the clip the two columns would be far outside it
            assert float((r64["sv"][R.COL_TINY] / rows).sqrt()) < 1e-8 and float((r64["sv"][R.COL_HUGE] / rows).sqrt()) > 1e6
        else:
            assert bool((r64["std"] == R.STD_MIN).all())
    else:
        assert not bool(deg.any()) or rows == 1


@pytest.mark.parametrize("pin_lo", R.STATS_PINNED[2])
def test_pinned_stats_cases_are_under_the_cap(pin_lo):
    rows, W, _ = R.STATS_PINNED
    inp = R.stats_inputs("warm", rows, W)
    r64, r32 = R.stats_reference(inp, pin_lo=pin_lo), R.stats_reference(inp, torch.float32, pin_lo=pin_lo)
    _cap(R.stats_rows(r32, r64, inp, pin_lo), f"stats pinned {pin_lo}")
    assert torch.equal(r64["mean"][pin_lo:], inp["mean"][pin_lo:].double()) and torch.equal(r64["std"][pin_lo:], inp["std"][pin_lo:].double())


@pytest.mark.parametrize("family", R.FAMILIES)
def test_latent_cases_are_under_the_cap(family):
    for n, Z, obs_w, ref_w, stride in R.LATENT_CASES:
        inp = R.latent_inputs(family, n, Z, obs_w, stride)
        for normalise in (True, False):
            a, b = R.latent_concat(inp, Z, obs_w, ref_w, stride, normalise), R.latent_concat(inp, Z, obs_w, ref_w, stride, normalise, torch.float32)
            _cap([("x", R.array_error(b, a))], f"latent {family} {n} Z{Z} norm{int(normalise)}")
    for n, Z, stride in R.LATENT_BWD_CASES:
        inp = R.latent_inputs(family, n, Z, 1, stride)
        for add in (False, True):
            _cap([("dfc2", R.array_error(R.latent_concat_bwd(inp, Z, add, torch.float32), R.latent_concat_bwd(inp, Z, add)))], f"latent bwd {family} {n} Z{Z} add{int(add)}")


@pytest.mark.parametrize("family", R.FAMILIES)
def test_action_and_head_cases_are_under_the_cap(family):
    for n, A in R.ACTION_CASES:
        inp = R.action_inputs(family, n, A)
        r64, r32 = R.sample_action(inp), R.sample_action(inp, torch.float32)
        _cap([(k, R.array_error(r32[k], r64[k])) for k in ("raw", "action_t", "logp")], f"action {family} {n}x{A}")
    for M, K in R.HEAD_CASES:
        inp = R.head_inputs(M, K)
        _cap([("y", R.array_error(R.head_fwd(inp, b, torch.float32), R.head_fwd(inp, b))) for b in (True, False)], f"head {M}x{K}")


# ---- refusals: validation comes before any launch, so no device is needed -----------------------------------------------------------------
def _refused(rc, word):
    err = hip.lib().tmjx_last_error()
    assert rc == -22 and word in err, (rc, word, err)


def test_block_entries_refuse_bad_arguments_without_gpu():
    L, a = hip.lib(), ctypes.c_void_p(0x10000)          # a non-null, 16-byte aligned dummy that is never dereferenced: validation fails first
    for H in (0, 32, 96, 192, 2048):
        _refused(L.tmjx_silu_ln_fwd(a, a, a, a, a, a, 4, H, 1e-6, None), b"H must be")
        _refused(L.tmjx_silu_ln_bwd(a, a, a, a, a, a, a, a, 4, H, None), b"H must be")
    _refused(L.tmjx_silu_ln_fwd(a, a, a, a, a, a, 0, 64, 1e-6, None), b"rows must be")
    _refused(L.tmjx_silu_ln_bwd(a, a, a, a, a, a, a, a, 0, 64, None), b"rows must be")
    for k in range(6):
        args = [a] * 6; args[k] = None
        _refused(L.tmjx_silu_ln_fwd(*args, 4, 64, 1e-6, None), b"null")
    for k in range(8):
        args = [a] * 8; args[k] = None
        _refused(L.tmjx_silu_ln_bwd(*args, 4, 64, None), b"null")
    odd = ctypes.c_void_p(0x10004)
    for y16, ld in ((a, 127), (a, 130), (odd, 132)):          # ld < H, ld % 4, rows not 8-byte aligned
        _refused(L.tmjx_silu_ln_fwd_bf16(a, a, a, a, y16, ld, a, 4, 128, 1e-6, None), b"tmjx_silu_ln_fwd_bf16")
        _refused(L.tmjx_silu_ln_bwd_bf16(a, a, a, a, a, y16, ld, a, a, 4, 128, None), b"tmjx_silu_ln_bwd_bf16")
    _refused(L.tmjx_silu_ln_fwd_bf16(a, a, a, a, None, 128, a, 4, 128, 1e-6, None), b"null")
    _refused(L.tmjx_silu_ln_bwd_bf16(a, a, a, a, a, None, 128, a, a, 4, 128, None), b"null")
    _refused(L.tmjx_silu_ln_fwd_bf16(a, a, a, a, a, 132, a, 4, 100, 1e-6, None), b"H must be")
    assert L.tmjx_silu_ln_partial_floats(1, 64) == 3 * 64 and L.tmjx_silu_ln_partial_floats(33, 128) == 2 * 3 * 128


def test_silu_and_head_entries_refuse_bad_arguments_without_gpu():
    L, a, odd = hip.lib(), ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)
    _refused(L.tmjx_silu_fwd(a, a, a, 0, 4, None), b"bad sizes")
    _refused(L.tmjx_silu_fwd(a, a, a, 4, 0, None), b"bad sizes")
    _refused(L.tmjx_silu_fwd(a, None, a, 4, 4, None), b"null")
    _refused(L.tmjx_silu_bwd(a, a, a, a, 0, 4, None), b"bad sizes")
    _refused(L.tmjx_silu_bwd(a, a, a, None, 4, 4, None), b"null")
    for rows, N, z in ((4, 6, a), (4, 0, a), (0, 4, a), (4, 4, odd)):
        _refused(L.tmjx_silu_bwd_rank1(a, a, z, a, a, rows, N, None), b"N % 4 == 0")
    _refused(L.tmjx_silu_bwd_rank1(None, a, a, a, a, 4, 4, None), b"null")
    _refused(L.tmjx_head_fwd(a, 8, a, None, a, 4, 6, None), b"K % 4 == 0")
    _refused(L.tmjx_head_fwd(a, 10, a, None, a, 4, 8, None), b"K % 4 == 0")          # rows of x not 16-byte aligned
    _refused(L.tmjx_head_fwd(a, 8, odd, None, a, 4, 8, None), b"K % 4 == 0")
    _refused(L.tmjx_head_fwd(a, 4, a, None, a, 4, 8, None), b"leading dimensions")
    _refused(L.tmjx_head_fwd(a, 8, a, None, a, 0, 8, None), b"bad sizes")
    _refused(L.tmjx_head_fwd(a, 8, a, None, None, 4, 8, None), b"null")
    assert L.tmjx_head_fwd_ok(a, 8, a, 8) == 1 and L.tmjx_head_fwd_ok(a, 8, a, 6) == 0 and L.tmjx_head_fwd_ok(a, 10, a, 8) == 0


def test_stats_entries_refuse_bad_arguments_without_gpu():
    L, a, odd = hip.lib(), ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)
    _refused(L.tmjx_stats_sums(a, a, a, a, 0, 8, None), b"rows must be")
    _refused(L.tmjx_stats_sums(a, a, a, a, 10, 0, None), b"multiple of 4")
    for k in (0, 1, 3):
        args = [a] * 4; args[k] = odd
        _refused(L.tmjx_stats_sums(*args, 10, 8, None), b"16-byte aligned")
    for k in range(4):
        args = [a] * 4; args[k] = None
        _refused(L.tmjx_stats_sums(*args, 10, 8, None), b"null")
    _refused(L.tmjx_stats_apply(a, 8.0, a, a, a, a, 0, 1e-6, 1e6, None), b"W must be")
    _refused(L.tmjx_stats_apply(a, -1.0, a, a, a, a, 4, 1e-6, 1e6, None), b"n_added")
    _refused(L.tmjx_stats_apply(a, 8.0, a, None, a, a, 4, 1e-6, 1e6, None), b"null")
    assert L.tmjx_stats_scratch_floats(8) == 512 * 2 * 8


def test_latent_and_action_entries_refuse_bad_arguments_without_gpu():
    L, a = hip.lib(), ctypes.c_void_p(0x10000)
    ok = dict(fc2=a, eps=a, obs=a, x=a, n=4, Z=3, obs_w=7, ref_w=2, s0=7, s1=1, mean=None, std=None, x_stride=8, seed=0, rng=None)
    for bad, word in ((dict(x_stride=7), b"bad sizes"), (dict(n=0), b"bad sizes"), (dict(Z=0), b"bad sizes"), (dict(ref_w=8), b"bad sizes"), (dict(ref_w=-1), b"bad sizes"),
                      (dict(eps=None), b"needs rng_state"), (dict(fc2=None), b"null"), (dict(obs=None), b"null"), (dict(x=None), b"null")):
        _refused(L.tmjx_latent_concat(*dict(ok, **bad).values(), None), word)
    _refused(L.tmjx_latent_concat_bwd(a, a, a, a, 4, 3, 2, None), b"bad sizes")          # dx_stride < Z
    _refused(L.tmjx_latent_concat_bwd(a, a, a, a, 0, 3, 3, None), b"bad sizes")
    _refused(L.tmjx_latent_concat_bwd(a, None, a, a, 4, 3, 3, None), b"null")
    _refused(L.tmjx_latent_concat_bwd_add(a, a, a, None, a, 4, 3, 3, None), b"null")
    _refused(L.tmjx_latent_concat_bwd_add(a, a, a, a, a, 4, 3, 2, None), b"bad sizes")
    _refused(L.tmjx_sample_action(a, None, a, a, a, 4, 3, 0, None, None), b"needs rng_state")
    _refused(L.tmjx_sample_action(a, a, a, a, a, 0, 3, 0, None, None), b"bad sizes")
    _refused(L.tmjx_sample_action(a, a, a, a, a, 4, 0, 0, None, None), b"bad sizes")
    for k in (0, 2, 3, 4):
        args = [a] * 5; args[k] = None
        _refused(L.tmjx_sample_action(*args, 4, 3, 0, None, None), b"null")


def test_grouped_column_sums_refuse_bad_groups_without_gpu():
    L = hip.lib()
    arr = (hip.ColsumProblem * 17)()
    for i in range(17):
        arr[i] = hip.ColsumProblem(0x10000, 0x10000, 4, 4)
    _refused(L.tmjx_colsum_grouped(arr, 17, None), b"1 .. 16 problems")
    _refused(L.tmjx_colsum_grouped(arr, 0, None), b"1 .. 16 problems")
    _refused(L.tmjx_colsum_grouped(None, 1, None), b"1 .. 16 problems")
    for bad in (hip.ColsumProblem(None, 0x10000, 4, 4), hip.ColsumProblem(0x10000, None, 4, 4), hip.ColsumProblem(0x10000, 0x10000, 0, 4),
                hip.ColsumProblem(0x10000, 0x10000, 4, 0)):
        arr[2] = bad
        _refused(L.tmjx_colsum_grouped(arr, 3, None), b"bad problem")
