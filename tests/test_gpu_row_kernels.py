"""GPU: the element-wise and row-wise kernels of the SGD step and the acting path against the float64 references of tests/row_kernels_ref.py, each
C entry launched directly with raw pointers at the shapes where it changes path: the five widths of the Dense -> SiLU -> LayerNorm block, its
one-wave and 256-thread launches and the grid-stride trip; rows < 4 and rows % 32 != 0 in its backward pass and the partial counts 1 .. 257 of the
k_colsum behind it; the scalar and float4 paths of the SiLU halves; normaliser batches below the slab count, one row, 65 float4 groups, constant and
clipped columns, pinned columns; the latent / action kernels with pad columns, an env-minor observation, no normaliser, both block sizes and the
grid cap; the 1-wide head forward; grouped column sums with widths that are no multiple of 32.

The bound of every compared array is that of tests/test_gpu_loss_head.py: with e32 the error of the float32 restatement against float64 in the same
metric, the kernel's error must be <= max(4 e32, 2^-20) (tests/row_kernels_ref.py has the metrics; tests/test_row_kernels_ref_cpu.py keeps every e32
of these case lists under 2^-10).  Outputs are prefilled with NaN and followed by a sentinel tail: an element a kernel skips fails the comparison,
one it writes beyond its array fails the tail check.  Every case prints `RK | case | array | kernel error | e32 | bound`; DESIGN.md ("Row kernels")
has the measured table."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import row_kernels_ref as R
from track_mjx_amd import hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 12345.0
SENTINEL16 = 0x7FC1          # (a bf16 NaN pattern no kernel output has)
TAIL = 64


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _guard(n, tail=TAIL):
    """n floats of NaN followed by `tail` sentinel floats"""
    buf = torch.full((n + tail,), float("nan"), device=DEV)
    buf[n:] = SENTINEL
    return buf


def _intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def _dev(inp, *keys):
    return [inp[k].to(DEV).contiguous() for k in keys]


def _check(rows, tag):
    """rows: (array, kernel error, e32).  Prints all, then asserts all."""
    bad = []
    for name, err, e32 in rows:
        b = R.bound(e32)
        print(f"RK | {tag} | {name} | {err:.2e} | {e32:.2e} | {b:.2e}")
        if not err <= b:
            bad.append((name, err, e32, b))
    assert not bad, (tag, bad)


# ---- Dense -> SiLU -> LayerNorm block ---------------------------------------------------------------------------------------------------
def _block_fwd(inp, rows, H):
    z, b, g, be = _dev(inp, "z", "bias", "gamma", "beta")
    y, stats = _guard(rows * H), _guard(2 * rows)
    hip.check(hip.lib().tmjx_silu_ln_fwd(_p(z), _p(b), _p(g), _p(be), _p(y), _p(stats), rows, H, R.LN_EPS, _st()), "tmjx_silu_ln_fwd")
    torch.cuda.synchronize()
    assert _intact(y, rows * H) and _intact(stats, 2 * rows)
    return y[:rows * H].view(rows, H), stats[:2 * rows].view(rows, 2)


def _block_bwd(inp, stats, rows, H):
    L = hip.lib()
    dy, z, b, g = _dev(inp, "dy", "z", "bias", "gamma")
    npart = L.tmjx_silu_ln_partial_floats(rows, H)
    assert npart == (rows + 31) // 32 * 3 * H
    dz, grads, partial = _guard(rows * H), _guard(3 * H), _guard(npart)          # partial: exactly what the entry asks for, then the sentinel tail
    hip.check(L.tmjx_silu_ln_bwd(_p(dy), _p(z), _p(b), _p(g), _p(stats), _p(dz), _p(grads), _p(partial), rows, H, _st()), "tmjx_silu_ln_bwd")
    torch.cuda.synchronize()
    assert _intact(dz, rows * H) and _intact(grads, 3 * H) and _intact(partial, npart)
    return dz[:rows * H].view(rows, H), grads[:3 * H].view(3, H)


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


@pytest.mark.parametrize("fam,rows,H", R.BLOCK_FWD_CASES, ids=_ids(R.BLOCK_FWD_CASES))
def test_block_forward_against_float64(fam, rows, H):
    """y and stats = (mean, rstd) per row; rows <= 8192 launch one-wave blocks, above 256-thread blocks of 4 rows, above 16 384 the grid-stride loop"""
    inp, r64, r32 = R.block_reference(fam, rows, H)
    y, stats = _block_fwd(inp, rows, H)
    got = {"y": y, "mean": stats[:, 0], "rstd": stats[:, 1]}
    _check([(k, R.block_error(k, got[k], r64), R.block_error(k, r32[k], r64)) for k in ("y", "mean", "rstd")], f"block fwd {fam} {rows}x{H}")


@pytest.mark.parametrize("fam,rows,H", R.BLOCK_BWD_CASES, ids=_ids(R.BLOCK_BWD_CASES))
def test_block_backward_against_float64(fam, rows, H):
    """dz and grads = d gamma | d beta | d bias, each row of grads against its own largest entry; stats from the forward kernel"""
    inp, r64, r32 = R.block_reference(fam, rows, H)
    _, stats = _block_fwd(inp, rows, H)
    dz, grads = _block_bwd(inp, stats, rows, H)
    got = {"dz": dz, "dgamma": grads[0], "dbeta": grads[1], "dbias": grads[2]}
    _check([(k, R.block_error(k, got[k], r64), R.block_error(k, r32[k], r64)) for k in ("dz", "dgamma", "dbeta", "dbias")],
           f"block bwd {fam} {rows}x{H} nblk {(rows + 31) // 32}")


@pytest.mark.parametrize("fam,rows,H", R.BLOCK_BF16_CASES, ids=_ids(R.BLOCK_BF16_CASES))
def test_block_bf16_forms_are_the_rounded_float32_forms(fam, rows, H):
    """y16 / dz16 [rows][H + 4]: to the bit torch's round-to-nearest-even of the float32 kernels' output, the pad columns and the tail untouched; stats
    and grads bit-equal to the float32 forms"""
    L = hip.lib()
    inp, _, _ = R.block_reference(fam, rows, H)
    y, stats = _block_fwd(inp, rows, H)
    dz, grads = _block_bwd(inp, stats, rows, H)
    ld = H + 4
    z, b, g, be, dy = _dev(inp, "z", "bias", "gamma", "beta", "dy")

    def out16():
        return torch.full((rows * ld + TAIL,), SENTINEL16, dtype=torch.int16, device=DEV)

    def rounded(buf, want32):
        m = buf[:rows * ld].view(rows, ld)
        return torch.equal(m[:, :H], want32.to(torch.bfloat16).view(torch.int16)) and bool((m[:, H:] == SENTINEL16).all()) and bool((buf[rows * ld:] == SENTINEL16).all())

    y16, stats16 = out16(), _guard(2 * rows)
    hip.check(L.tmjx_silu_ln_fwd_bf16(_p(z), _p(b), _p(g), _p(be), _p(y16), ld, _p(stats16), rows, H, R.LN_EPS, _st()), "tmjx_silu_ln_fwd_bf16")
    npart = L.tmjx_silu_ln_partial_floats(rows, H)
    dz16, grads16, partial = out16(), _guard(3 * H), _guard(npart)
    hip.check(L.tmjx_silu_ln_bwd_bf16(_p(dy), _p(z), _p(b), _p(g), _p(stats), _p(dz16), ld, _p(grads16), _p(partial), rows, H, _st()), "tmjx_silu_ln_bwd_bf16")
    torch.cuda.synchronize()
    assert rounded(y16, y) and _intact(stats16, 2 * rows) and torch.equal(stats16[:2 * rows].view(rows, 2), stats)
    assert rounded(dz16, dz) and _intact(grads16, 3 * H) and _intact(partial, npart) and torch.equal(grads16[:3 * H].view(3, H), grads)


# ---- SiLU halves -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("rows,N", R.SILU_CASES, ids=_ids(R.SILU_CASES))
def test_silu_halves_against_float64(rows, N, fam):
    """tmjx_silu_fwd and tmjx_silu_bwd: N % 4 != 0 takes the scalar path (the last thread of (341, 3) holds three elements, of (7, 5) a tail of three)"""
    L = hip.lib()
    inp = R.silu_inputs(fam, rows, N)
    r64, r32 = R.silu_halves(inp), R.silu_halves(inp, torch.float32)
    z, b, dy = _dev(inp, "z", "bias", "dy")
    n = rows * N
    y, dz = _guard(n, 4), _guard(n, 4)
    hip.check(L.tmjx_silu_fwd(_p(z), _p(b), _p(y), rows, N, _st()), "tmjx_silu_fwd")
    hip.check(L.tmjx_silu_bwd(_p(dy), _p(z), _p(b), _p(dz), rows, N, _st()), "tmjx_silu_bwd")
    torch.cuda.synchronize()
    assert _intact(y, n) and _intact(dz, n)
    _check([("y", R.array_error(y[:n].view(rows, N), r64["y"]), R.array_error(r32["y"], r64["y"])),
            ("dz", R.array_error(dz[:n].view(rows, N), r64["dz"]), R.array_error(r32["dz"], r64["dz"]))], f"silu {fam} {rows}x{N}")


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("rows,N", R.SILU_RANK1_CASES, ids=_ids(R.SILU_RANK1_CASES))
def test_silu_backward_rank1_against_float64(rows, N, fam):
    L = hip.lib()
    inp = R.silu_inputs(fam, rows, N)
    r64, r32 = R.silu_halves(inp)["dz_rank1"], R.silu_halves(inp, torch.float32)["dz_rank1"]
    dy1, w1, z, b = _dev(inp, "dy1", "w1", "z", "bias")
    n = rows * N
    dz = _guard(n, 4)
    hip.check(L.tmjx_silu_bwd_rank1(_p(dy1), _p(w1), _p(z), _p(b), _p(dz), rows, N, _st()), "tmjx_silu_bwd_rank1")
    torch.cuda.synchronize()
    assert _intact(dz, n)
    _check([("dz", R.array_error(dz[:n].view(rows, N), r64), R.array_error(r32, r64))], f"silu rank1 {fam} {rows}x{N}")


# ---- observation normaliser --------------------------------------------------------------------------------------------------------------
def _run_stats(inp, rows, W, pin_lo=None):
    """tmjx_stats_sums + tmjx_stats_apply (or _apply_pinned) on the state of `inp` -> the keys of R.stats_reference.  std is an output only: NaN
    before the unpinned call"""
    L = hip.lib()
    x, mean, sv = _dev(inp, "x", "mean", "sv")
    mean, sv = mean.clone(), sv.clone()
    std = torch.full((W,), float("nan"), device=DEV) if pin_lo is None else inp["std"].to(DEV).clone()
    count = torch.tensor([inp["count"]], dtype=torch.float32, device=DEV)
    nscr = L.tmjx_stats_scratch_floats(W)
    sums, scratch = _guard(2 * W), _guard(nscr)
    hip.check(L.tmjx_stats_sums(_p(x), _p(mean), _p(sums), _p(scratch), rows, W, _st()), "tmjx_stats_sums")
    if pin_lo is None:
        hip.check(L.tmjx_stats_apply(_p(sums), float(rows), _p(count), _p(mean), _p(sv), _p(std), W, R.STD_MIN, R.STD_MAX, _st()), "tmjx_stats_apply")
    else:
        hip.check(L.tmjx_stats_apply_pinned(_p(sums), float(rows), _p(count), _p(mean), _p(sv), _p(std), W, pin_lo, R.STD_MIN, R.STD_MAX, _st()), "tmjx_stats_apply_pinned")
    torch.cuda.synchronize()
    assert _intact(sums, 2 * W) and _intact(scratch, nscr)
    return {"count": float(count), "mean": mean.cpu(), "sv": sv.cpu(), "std": std.cpu(), "s1": sums[:W].cpu(), "s2": sums[W:2 * W].cpu()}


def _stats_check(got, inp, rows, pin_lo, tag):
    r64, r32 = R.stats_reference(inp, pin_lo=pin_lo), R.stats_reference(inp, torch.float32, pin_lo=pin_lo)
    assert got["count"] == r64["count"] == inp["count"] + rows
    e32 = dict(R.stats_rows(r32, r64, inp, pin_lo))
    _check([(name, err, e32[name]) for name, err in R.stats_rows(got, r64, inp, pin_lo)], tag)
    assert bool(torch.isfinite(got["std"]).all()) and float(got["std"].min()) >= R.STD_MIN and float(got["std"].max()) <= R.STD_MAX
    return r64


@pytest.mark.parametrize("fam", R.STATS_FAMILIES)
@pytest.mark.parametrize("rows,W", R.STATS_CASES, ids=_ids(R.STATS_CASES))
def test_normaliser_update_against_float64(rows, W, fam):
    """count (exact), mean, summed_variance and std (per column) and the two rows of sums; cold: the constant column against its S2, both clips binding"""
    inp = R.stats_inputs(fam, rows, W)
    got = _run_stats(inp, rows, W)
    _stats_check(got, inp, rows, None, f"stats {fam} {rows}x{W}")
    if fam == "cold" and rows > 1:
        assert float(got["std"][R.COL_TINY]) == R.STD_MIN and float(got["std"][R.COL_HUGE]) == R.STD_MAX


@pytest.mark.parametrize("pin_lo", R.STATS_PINNED[2])
def test_pinned_normaliser_update_against_float64(pin_lo):
    """columns [0, pin_lo) as the float64 pinned reference, columns from pin_lo on bit-identical to their values before the call, the count grown"""
    rows, W, _ = R.STATS_PINNED
    inp = R.stats_inputs("warm", rows, W)
    got = _run_stats(inp, rows, W, pin_lo)
    _stats_check(got, inp, rows, pin_lo, f"stats pinned {rows}x{W} pin_lo {pin_lo}")
    for k in ("mean", "sv", "std"):
        assert torch.equal(got[k][pin_lo:], inp[k][pin_lo:]), k
        assert pin_lo == 0 or not torch.equal(got[k][:pin_lo], inp[k][:pin_lo]), k


# ---- latent sample + decoder input -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("layout", ["rowmajor", "envminor"])
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("n,Z,obs_w,ref_w,stride", R.LATENT_CASES, ids=_ids(R.LATENT_CASES))
def test_latent_concat_against_float64(n, Z, obs_w, ref_w, stride, fam, layout, normalise):
    """x = [latent sample | normalised observation tail | zeros] with given eps; the observation row-major or env-minor (obs_s0 = 1, obs_s1 = n), with
    and without the normaliser (mean == NULL); pad columns exactly 0"""
    inp = R.latent_inputs(fam, n, Z, obs_w, stride)
    r64 = R.latent_concat(inp, Z, obs_w, ref_w, stride, normalise)
    r32 = R.latent_concat(inp, Z, obs_w, ref_w, stride, normalise, torch.float32)
    fc2, eps, mo, so = _dev(inp, "fc2", "eps", "mean_o", "std_o")
    obs = inp["obs"].to(DEV)
    obs, s0, s1 = (obs.contiguous(), obs_w, 1) if layout == "rowmajor" else (obs.t().contiguous(), 1, n)
    x = _guard(n * stride)
    hip.check(hip.lib().tmjx_latent_concat(_p(fc2), _p(eps), _p(obs), _p(x), n, Z, obs_w, ref_w, s0, s1, _p(mo if normalise else None), _p(so if normalise else None),
                                           stride, 0, None, _st()), "tmjx_latent_concat")
    torch.cuda.synchronize()
    assert _intact(x, n * stride)
    x = x[:n * stride].view(n, stride)
    W = Z + obs_w - ref_w
    assert bool((x[:, W:] == 0).all())
    _check([("x", R.array_error(x, r64), R.array_error(r32, r64)), ("latent", R.array_error(x[:, :Z], r64[:, :Z]), R.array_error(r32[:, :Z], r64[:, :Z]))] +
           ([("obs", R.array_error(x[:, Z:W], r64[:, Z:W]), R.array_error(r32[:, Z:W], r64[:, Z:W]))] if W > Z else []),
           f"latent {fam} {n} Z{Z} obs{obs_w} ref{ref_w} ld{stride} {layout} {'norm' if normalise else 'raw'}")


@pytest.mark.parametrize("add", [False, True], ids=["bwd", "bwd_add"])
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("n,Z,stride", R.LATENT_BWD_CASES, ids=_ids(R.LATENT_BWD_CASES))
def test_latent_concat_backward_against_float64(n, Z, stride, fam, add):
    L = hip.lib()
    inp = R.latent_inputs(fam, n, Z, 1, stride)
    r64, r32 = R.latent_concat_bwd(inp, Z, add), R.latent_concat_bwd(inp, Z, add, torch.float32)
    dx, eps, fc2, ad = _dev(inp, "dx", "eps", "fc2", "add")
    out = _guard(n * 2 * Z)
    if add:
        hip.check(L.tmjx_latent_concat_bwd_add(_p(dx), _p(eps), _p(fc2), _p(ad), _p(out), n, Z, stride, _st()), "tmjx_latent_concat_bwd_add")
    else:
        hip.check(L.tmjx_latent_concat_bwd(_p(dx), _p(eps), _p(fc2), _p(out), n, Z, stride, _st()), "tmjx_latent_concat_bwd")
    torch.cuda.synchronize()
    assert _intact(out, n * 2 * Z)
    g = out[:n * 2 * Z].view(n, 2 * Z)
    _check([("dfc2", R.array_error(g, r64), R.array_error(r32, r64)), ("dmean", R.array_error(g[:, :Z], r64[:, :Z]), R.array_error(r32[:, :Z], r64[:, :Z])),
            ("dlogvar", R.array_error(g[:, Z:], r64[:, Z:]), R.array_error(r32[:, Z:], r64[:, Z:]))], f"latent {'bwd_add' if add else 'bwd'} {fam} {n} Z{Z} ld{stride}")


# ---- action sample -----------------------------------------------------------------------------------------------------------------------
def _run_action(logits, noise, n, A, rng_state=None, seed=0):
    raw, act, logp = _guard(n * A), _guard(n * A), _guard(n)
    hip.check(hip.lib().tmjx_sample_action(_p(logits), _p(noise), _p(raw), _p(act), _p(logp), n, A, seed, _p(rng_state), _st()), "tmjx_sample_action")
    torch.cuda.synchronize()
    assert _intact(raw, n * A) and _intact(act, n * A) and _intact(logp, n)
    return raw[:n * A].view(n, A), act[:n * A].view(A, n), logp[:n]


def _tanh_of_own_raw(raw, act):
    """action_t [A][n] is tanh of the kernel's own raw [n][A], to 2 float32 ulp"""
    want = torch.tanh(raw.double().cpu()).t()
    ulp = torch.from_numpy(np.spacing(want.abs().numpy().astype(np.float32)).astype(np.float64))
    return bool(((act.double().cpu() - want).abs() <= 2.0 * ulp).all())


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("n,A", R.ACTION_CASES, ids=_ids(R.ACTION_CASES))
def test_sample_action_against_float64(n, A, fam):
    """raw, action_t ([A][n]) and logp with given noise; A below, at and above the 8-lane group; 8192 / 8193 rows: one-wave and 256-thread blocks"""
    inp = R.action_inputs(fam, n, A)
    r64, r32 = R.sample_action(inp), R.sample_action(inp, torch.float32)
    logits, noise = _dev(inp, "logits", "noise")
    raw, act, logp = _run_action(logits, noise, n, A)
    _check([(k, R.array_error(g, r64[k]), R.array_error(r32[k], r64[k])) for k, g in (("raw", raw), ("action_t", act), ("logp", logp))], f"action {fam} {n}x{A}")
    assert _tanh_of_own_raw(raw, act)


def test_sample_action_draws_its_own_noise_and_advances_the_counter():
    """noise == NULL with rng_state = {draw counter, ticket}: the counter is one more after each call and the ticket word back at 0; two calls give
    different samples, each N(0, 1) once the location and scale are taken out"""
    n, A = 65, 9
    inp = R.action_inputs("plain", n, A)
    logits, = _dev(inp, "logits")
    state = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    first = _run_action(logits, None, n, A, state, seed=1234)
    assert state.tolist() == [6, 0]
    second = _run_action(logits, None, n, A, state, seed=1234)
    assert state.tolist() == [7, 0]
    lg = inp["logits"].double()
    for raw, act, logp in (first, second):
        assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(logp).all()) and _tanh_of_own_raw(raw, act)
        z = (raw.double().cpu() - lg[:, :A]) / (R.softplus(lg[:, A:]) + R.MIN_STD)
        assert abs(float(z.mean())) < 0.2 and 0.8 < float(z.std()) < 1.2          # 585 draws: the mean's sigma is 0.04, the std's 0.03
        want = R.log_prob(lg, raw.double().cpu())
        assert R.array_error(logp, want) <= R.bound(R.array_error(R.log_prob(lg.float(), raw.cpu()), want))
    assert float((first[0] - second[0]).abs().min()) > 0


# ---- 1-wide head forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,K", R.HEAD_CASES, ids=_ids(R.HEAD_CASES))
def test_head_forward_against_float64(M, K, with_bias):
    """y = x[:, :K] w + b with ldx = K + 4 (NaN in the pad columns: a read past K poisons the row), M % 16 != 0, K below / at / above one 256-column pass"""
    inp = R.head_inputs(M, K)
    r64, r32 = R.head_fwd(inp, with_bias), R.head_fwd(inp, with_bias, torch.float32)
    ldx = K + 4
    x = torch.full((M, ldx), float("nan"), device=DEV)
    x[:, :K] = inp["x"].to(DEV)
    w, b = _dev(inp, "w", "b")
    y = _guard(M)
    hip.check(hip.lib().tmjx_head_fwd(_p(x), ldx, _p(w), _p(b if with_bias else None), _p(y), M, K, _st()), "tmjx_head_fwd")
    torch.cuda.synchronize()
    assert _intact(y, M)
    _check([("y", R.array_error(y[:M], r64), R.array_error(r32, r64))], f"head {M}x{K} {'bias' if with_bias else 'nobias'}")


# ---- grouped column sums -----------------------------------------------------------------------------------------------------------------
def _colsum_group(indices):
    L = hip.lib()
    srcs = [R.colsum_inputs(i).to(DEV) for i in indices]
    outs = [_guard(R.COLSUM_WIDTHS[i]) for i in indices]
    arr = (hip.ColsumProblem * len(indices))()
    for k, i in enumerate(indices):
        arr[k] = hip.ColsumProblem(srcs[k].data_ptr(), outs[k].data_ptr(), R.COLSUM_ROWS[i], R.COLSUM_WIDTHS[i])
    hip.check(L.tmjx_colsum_grouped(arr, len(indices), _st()), "tmjx_colsum_grouped")
    torch.cuda.synchronize()
    bad = []
    for k, i in enumerate(indices):
        rows, width = R.COLSUM_ROWS[i], R.COLSUM_WIDTHS[i]
        ref = R.colsum_inputs(i).double().sum(0)
        err, tol = float((outs[k][:width].double().cpu() - ref).abs().max()), 1e-5 * float(ref.abs().max() + rows ** 0.5)      # (test_colsum_kernel_matches_torch's bound)
        print(f"RK | colsum grouped {len(indices)} | {rows}x{width} | {err:.2e} | - | {tol:.2e}")
        if not (err <= tol and _intact(outs[k], width)):
            bad.append((rows, width, err, tol))
    assert not bad, bad


def test_grouped_column_sums_against_float64():
    """16 problems in one launch, widths that are no multiple of the 32-column block (the block-to-problem lookup), partial-row counts around the 8
    row slices and the unrolled 64-row trip; one problem alone; 17 are refused"""
    _colsum_group(list(range(16)))
    _colsum_group([4])
    arr = (hip.ColsumProblem * 17)()
    assert hip.lib().tmjx_colsum_grouped(arr, 17, None) == -22
