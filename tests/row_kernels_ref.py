"""Plain torch references for the element-wise and row-wise kernels on either side of the loss head (csrc/ppo_kernels.h, csrc/act_shared.h,
csrc/tmjx_hip.hip): the Dense -> SiLU -> LayerNorm block epilogue and its backward, the SiLU halves of the value MLP, the observation normaliser
update, the latent sample + decoder input and its backward, the action sample, the 1-wide head's forward pass and grouped column sums.  Written
from the RAW arrays of each C entry (no module of track_mjx_amd.agent), every function parametrised by the dtype it computes in: float64 is the
reference, the same code in float32 (the "restatement") gives the error `e32` a correct float32 evaluation has, and the kernels must stay within
`bound(e32) = max(4 e32, 2^-20)` in the same metric — the convention of tests/loss_head_ref.py, whose metric, bound and NormalTanh pieces are
imported here, not copied.

Metrics.  `array_error` (largest absolute error / largest reference magnitude) for every array but two: the normaliser's `summed_variance` and
`std` are compared PER COLUMN (error / |reference|, largest over the columns — the columns' scales run over sixteen decades, and one metric for the
array would see the widest column only).  A column whose batch is constant has reference variance 0: its `summed_variance` is compared against
the column's S2 = sum((x - mean_old)^2) instead (the size of the two terms whose difference it is), and its `std` — the root of rounding noise —
is only required to be finite and inside [std_min, std_max].

Conditioning cap.  A case whose e32 exceeds 2^-10 in any compared array would let the bound hide a wrong kernel: tests/test_row_kernels_ref_cpu.py
asserts the cap for the exact case lists below, which the GPU tests import.  That is a condition on the inputs, not a measurement of a kernel.

Intrinsics.  `tm_sigmoid` (csrc/silu_math.h) is v_rcp_f32(1 + v_exp_f32(-v log2 e)), each instruction good to 1 ulp; the block forward multiplies
the centred activation by rstd <= 1 / sqrt(eps) = 1000.  The rows that reach rstd = 1000 here are the dead rows (z = -40: |silu| < 2e-16, so even
a relative error of 1 in the sigmoid is 2e-13 after the multiplication), and no array needed a term for the intrinsics on top of the plain bound:
none is added."""
from __future__ import annotations

import numpy as np
import torch

from tests.loss_head_ref import FLOOR, MIN_STD, array_error, bound, f32r, log_prob, make_inputs, scalar_error, softplus  # noqa: F401  (re-exported)

CAP = 2.0 ** -10
FAMILIES = ("plain", "hard")
LN_EPS = f32r(1e-6)
BLOCK_WIDTHS = (64, 128, 256, 512, 1024)
STD_MIN, STD_MAX = f32r(1e-6), f32r(1e6)


def _rng(tag: int, *key):
    return np.random.default_rng([tag] + [int(k) for k in key])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def column_error(got, ref, denom=None) -> float:
    """per column: |got - ref| / |denom| (denom = ref unless given), the largest over the columns; a column whose denominator is 0 counts absolutely"""
    got, ref = torch.as_tensor(got).double().cpu().reshape(-1), ref.double().reshape(-1)
    d = (ref if denom is None else denom.double().reshape(-1)).abs()
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / torch.where(d > 0, d, torch.ones_like(d))).max())


# ---- Dense -> SiLU -> LayerNorm block ---------------------------------------------------------------------------------------------------
# forward: (family, rows, H).  8192 is the last one-wave launch, 8193 the first 256-thread one (a one-row last block), 16389 a second trip of the
# grid-stride loop (4096 blocks x 4 rows = 16384) with a full and a partial block
BLOCK_FWD_CASES = tuple((f, r, H) for f in FAMILIES for H in BLOCK_WIDTHS for r in (1, 3, 35)) + \
    tuple(("plain", r, H) for H in (64, 256) for r in (8192, 8193, 16389)) + (("hard", 8193, 1024),)
# backward: rows < 4 leave waves without a row (zero partials), 31 / 32 / 33 straddle one block of 32 rows; H = 64 at 256 .. 8193 rows gives the
# k_colsum behind it nblk = 8, 9, 64, 65, 257 partial rows
BLOCK_BWD_CASES = tuple((f, r, H) for f in FAMILIES for H in BLOCK_WIDTHS for r in (1, 3, 5, 31, 32, 33)) + \
    tuple(("plain", r, 64) for r in (256, 257, 2048, 2049, 8193))
BLOCK_BF16_CASES = tuple(("hard" if r == 35 else "plain", r, H) for H in (128, 512) for r in (1, 35, 8193))
BLOCK_ARRAYS = ("y", "mean", "rstd", "dz", "dgamma", "dbeta", "dbias")


def block_inputs(family, rows, H):
    """float32 z, bias, gamma, beta, dy.  hard: 5 % of z at -30, 5 % at 8 z + 10, and (rows >= 3) row 0 dead — z = -40 + 0.01 N, its variance far
    below eps, rstd = 1 / sqrt(eps) — and row 1 near-constant, z = 2 + 1e-4 N"""
    rng = _rng(1, FAMILIES.index(family), rows, H)
    z = rng.standard_normal((rows, H))
    if family == "hard":
        u = rng.random((rows, H))
        z = np.where(u < 0.05, -30.0, np.where(u > 0.95, 8.0 * z + 10.0, z))
        if rows >= 3:
            z[0] = -40.0 + 0.01 * rng.standard_normal(H)
            z[1] = 2.0 + 1e-4 * rng.standard_normal(H)
    return {"z": _t(z), "bias": _t(0.3 * rng.standard_normal(H)), "gamma": _t(1.0 + 0.2 * rng.standard_normal(H)), "beta": _t(0.1 * rng.standard_normal(H)),
            "dy": _t(rng.standard_normal((rows, H)))}


def silu_grad(v):
    s = torch.sigmoid(v)
    return s * (1.0 + v * (1.0 - s))


def block(inp, eps=LN_EPS, dtype=torch.float64):
    """y = LayerNorm(silu(z + bias)) with its row statistics, and the backward pass from dy, all by hand"""
    z, b, g, be, dy = (inp[k].to(dtype) for k in ("z", "bias", "gamma", "beta", "dy"))
    v = z + b
    a = v * torch.sigmoid(v)
    mean = a.mean(-1, keepdim=True)
    var = ((a - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ah = (a - mean) * rstd
    da = dy * g
    m1, m2 = da.mean(-1, keepdim=True), (da * ah).mean(-1, keepdim=True)
    dz = rstd * (da - m1 - ah * m2) * silu_grad(v)
    return {"y": ah * g + be, "mean": mean[:, 0], "rstd": rstd[:, 0], "dz": dz, "dgamma": (dy * ah).sum(0), "dbeta": dy.sum(0), "dbias": dz.sum(0)}


# ---- SiLU halves -------------------------------------------------------------------------------------------------------------------------
# (341, 3): 1023 elements, the last thread holds three; (7, 5): a three-element tail; N % 4 == 0 takes the float4 path
SILU_CASES = ((1, 1), (1, 3), (7, 5), (341, 3), (1025, 38), (33, 256), (1, 4))
SILU_RANK1_CASES = ((1, 4), (333, 8), (65, 260))


def silu_inputs(family, rows, N):
    """float32 z, bias, dy, dy1 [rows], w1 [N].  hard: z + bias uniform over +-30 and 1 % of z at -90 (exp(90) overflows float32: sigmoid exactly 0)"""
    rng = _rng(2, FAMILIES.index(family), rows, N)
    bias = 0.3 * rng.standard_normal(N)
    if family == "plain":
        z = rng.standard_normal((rows, N))
    else:
        bias = np.clip(bias, -1.0, 1.0)
        z = rng.uniform(-29.0, 29.0, (rows, N))
        z = np.where(rng.random((rows, N)) < 0.01, -90.0, z)
        if z.size >= 8:          # (alone, silu(-90) = 7e-38 would be the array's scale: a float32 zero is then an error of 1)
            z.reshape(-1)[-1] = -90.0
    return {"z": _t(z), "bias": _t(bias), "dy": _t(rng.standard_normal((rows, N))), "dy1": _t(rng.standard_normal(rows)), "w1": _t(rng.standard_normal(N))}


def silu_halves(inp, dtype=torch.float64):
    z, b, dy, dy1, w1 = (inp[k].to(dtype) for k in ("z", "bias", "dy", "dy1", "w1"))
    v = z + b
    return {"y": v * torch.sigmoid(v), "dz": dy * silu_grad(v), "dz_rank1": (dy1[:, None] * w1[None, :]) * silu_grad(v)}


# ---- observation normaliser --------------------------------------------------------------------------------------------------------------
# rows < 512 leave most slabs empty; W = 260 = 65 float4 groups, a second block in x with one live lane; 16 417 rows = 33 per slab, the
# unrolled loop and its remainder
STATS_CASES = ((1, 4), (3, 260), (511, 8), (512, 8), (513, 260), (16417, 696))
STATS_FAMILIES = ("warm", "cold")
STATS_PINNED = (513, 260, (0, 4, 256, 257, 260))          # rows, W, every pin_lo
COL_CONSTANT, COL_TINY, COL_HUGE = 1, 2, 3                # cold family: the constant column (7.0), sigma = 1e-9 (std_min binds), sigma = 1e7 (std_max binds)


def stats_update(x, count, mean, sv, pin_lo=None, std=None, std_min=STD_MIN, std_max=STD_MAX):
    """brax running_statistics.update on one batch, two passes, in the dtype of x: (count, mean, summed_variance, std).  pin_lo: columns >= pin_lo
    keep mean, summed_variance and `std`; the count still grows"""
    n = x.shape[0]
    count_new = count + n
    d0 = x - mean
    mean_new = mean + d0.sum(0) / count_new
    sv_new = sv + (d0 * (x - mean_new)).sum(0)
    std_new = torch.sqrt(torch.clamp(sv_new, min=0.0) / count_new).clamp(std_min, std_max)
    if pin_lo is not None:
        keep = torch.arange(x.shape[1]) >= pin_lo
        mean_new, sv_new, std_new = torch.where(keep, mean, mean_new), torch.where(keep, sv, sv_new), torch.where(keep, std, std_new)
    return count_new, mean_new, sv_new, std_new


def stats_sums(x, mean):
    """what tmjx_stats_sums returns: S1 = sum(x - mean), S2 = sum((x - mean)^2)"""
    d0 = x - mean
    return d0.sum(0), (d0 * d0).sum(0)


def stats_inputs(family, rows, W):
    """float32 x [rows][W] and the state before the tested update: count (a python float), mean, sv, std.
    warm: a first update (float64, rounded to float32) on a batch of the same N(mu_c, sigma_c), sigma_c 0.1 .. 5 across the columns, mu_c in +-3.
    cold: count 0, mean 0, sv 0; the batch mean at 3 sigma (even columns) and 30 sigma (odd columns); columns 1, 2, 3 constant at 7, with sigma 1e-9
    (mean 0: 1e-9 N is representable, 7 + 1e-9 N is not) and with sigma 1e7"""
    rng = _rng(3, STATS_FAMILIES.index(family), rows, W)
    sigma = np.exp(np.linspace(np.log(0.1), np.log(5.0), W))[rng.permutation(W)]
    if family == "warm":
        mu = rng.uniform(-3.0, 3.0, W)
        first = _t(mu + sigma * rng.standard_normal((rows, W)))
        x = _t(mu + sigma * rng.standard_normal((rows, W)))
        zero = torch.zeros(W, dtype=torch.float64)
        c, m, sv, sd = stats_update(first.double(), 0.0, zero, zero)
        return {"x": x, "count": float(c), "mean": m.float(), "sv": sv.float(), "std": sd.float()}
    k = np.where(np.arange(W) % 2 == 0, 3.0, 30.0)
    sigma[COL_TINY], sigma[COL_HUGE], k[COL_TINY], k[COL_HUGE] = 1e-9, 1e7, 3.0, 3.0
    nz = rng.standard_normal((rows, W))
    if 1 < rows < 32:
        # a handful of draws can land next to each other in one of hundreds of columns: that column's variance is then 1e-3 of sigma^2, and its
        # float32 error — set by the 30 sigma offset — 1e-1 of it (measured at 3 x 260: e32 = 0.17).  Evenly spread scores, shuffled per column
        nz = rng.permuted(np.tile(np.linspace(-1.5, 1.5, rows)[:, None], (1, W)), axis=0)
    x = sigma * (k + nz)
    x[:, COL_CONSTANT] = 7.0
    z = torch.zeros(W)
    return {"x": _t(x), "count": 0.0, "mean": z.clone(), "sv": z.clone(), "std": torch.ones(W)}


def stats_reference(inp, dtype=torch.float64, pin_lo=None):
    x, mean, sv, std = (inp[k].to(dtype) for k in ("x", "mean", "sv", "std"))
    count, mean_new, sv_new, std_new = stats_update(x, inp["count"], mean, sv, pin_lo, std)
    s1, s2 = stats_sums(x, mean)
    return {"count": float(count), "mean": mean_new, "sv": sv_new, "std": std_new, "s1": s1, "s2": s2}


def stats_rows(got, r64, inp, pin_lo=None):
    """(array, error) of a normaliser result `got` (keys of stats_reference; the float32 restatement or a kernel's output) in this module's metrics.
    Columns whose batch is constant (the cold family's column 1; every column of a one-row batch from a zero state) have reference variance 0: sv
    against S2, std left to `degenerate_columns`' range check.  `ordinary`: without the sigma = 1e-9 / 1e7 columns, which own array_error's scale"""
    W = r64["mean"].numel()
    live = torch.ones(W, dtype=torch.bool) if pin_lo is None else torch.arange(W) < pin_lo
    deg = degenerate_columns(r64)
    ordinary = live.clone()
    if float(inp["count"]) == 0.0:
        ordinary[[COL_TINY, COL_HUGE]] = False
    cpu = lambda t: torch.as_tensor(t).double().cpu()  # noqa: E731
    rows = [("mean", array_error(cpu(got["mean"])[live], r64["mean"][live]) if bool(live.any()) else 0.0),
            ("mean ordinary", array_error(cpu(got["mean"])[ordinary], r64["mean"][ordinary]) if bool(ordinary.any()) else 0.0),
            ("sv", column_error(cpu(got["sv"])[live], r64["sv"][live], torch.where(deg, r64["s2"], r64["sv"])[live])),
            ("std", column_error(cpu(got["std"])[live & ~deg], r64["std"][live & ~deg]))]
    if float(inp["count"]) == 0.0 and inp["x"].shape[0] > 1:
        # the cold family's 3 sigma columns on their own: in the rows above the 30 sigma columns, a hundred times worse conditioned, set e32
        near = live & ~deg & (torch.arange(W) % 2 == 0)
        rows += [("sv 3sigma", column_error(cpu(got["sv"])[near], r64["sv"][near])), ("std 3sigma", column_error(cpu(got["std"])[near], r64["std"][near]))]
    if "s1" in got:
        rows += [("S1", array_error(got["s1"], r64["s1"])), ("S2", array_error(got["s2"], r64["s2"])),
                 ("S1 ordinary", array_error(cpu(got["s1"])[ordinary], r64["s1"][ordinary]) if bool(ordinary.any()) else 0.0),
                 ("S2 ordinary", array_error(cpu(got["s2"])[ordinary], r64["s2"][ordinary]) if bool(ordinary.any()) else 0.0)]
    return rows


def degenerate_columns(r64):
    return r64["sv"] == 0.0


# ---- latent sample + decoder input -------------------------------------------------------------------------------------------------------
# (n, Z, obs_w, ref_w, x_stride): one element; no observation part; the rodent's shapes with 2 pad columns; the switch from one-wave to 256-thread
# blocks at 8192 rows; 280 000 elements in one-wave blocks = more than the 4096-block grid holds (the grid-stride loop)
LATENT_CASES = ((1, 1, 1, 0, 2), (5, 3, 7, 7, 3), (65, 60, 696, 470, 288), (8192, 16, 24, 8, 32), (8193, 16, 24, 8, 32), (700, 60, 400, 60, 400))
LATENT_BWD_CASES = ((1, 1, 1), (65, 60, 288), (4097, 60, 64))          # (n, Z, dx_stride)


def latent_inputs(family, n, Z, obs_w, stride):
    """float32 fc2 [n][2 Z] = mean | logvar (hard: 2 N | 3 N clamped to +-8, as loss_head_ref), eps, obs [n][obs_w], the observation's normaliser,
    dx [n][stride] and add [n][2 Z] for the backward pass"""
    rng = _rng(4, FAMILIES.index(family), n, Z, obs_w, stride)
    nz = lambda *s: rng.standard_normal(s)  # noqa: E731
    fc2 = 0.3 * nz(n, 2 * Z) if family == "plain" else np.concatenate([2.0 * nz(n, Z), np.clip(3.0 * nz(n, Z), -8.0, 8.0)], -1)
    return {"fc2": _t(fc2), "eps": _t(nz(n, Z)), "obs": _t(1.0 + 3.0 * nz(n, max(obs_w, 1))), "mean_o": _t(nz(max(obs_w, 1))),
            "std_o": _t(np.exp(rng.uniform(-1.5, 1.5, max(obs_w, 1)))), "dx": _t(nz(n, stride)), "add": _t(nz(n, 2 * Z))}


def latent_concat(inp, Z, obs_w, ref_w, x_stride, normalise, dtype=torch.float64):
    fc2, eps, obs, mo, so = (inp[k].to(dtype) for k in ("fc2", "eps", "obs", "mean_o", "std_o"))
    n, W = fc2.shape[0], Z + obs_w - ref_w
    x = torch.zeros(n, x_stride, dtype=dtype)
    x[:, :Z] = fc2[:, :Z] + eps * torch.exp(fc2[:, Z:] / 2.0)
    tail = obs[:, ref_w:obs_w]
    x[:, Z:W] = (tail - mo[ref_w:obs_w]) / so[ref_w:obs_w] if normalise else tail
    return x


def latent_concat_bwd(inp, Z, add, dtype=torch.float64):
    fc2, eps, dx = (inp[k].to(dtype) for k in ("fc2", "eps", "dx"))
    g = dx[:, :Z]
    out = torch.cat([g, g * eps * torch.exp(fc2[:, Z:] / 2.0) / 2.0], -1)
    return out + inp["add"].to(dtype) if add else out


# ---- action sample -----------------------------------------------------------------------------------------------------------------------
# A below, at and not a multiple of the 8-lane group; the switch of the block size at 8192 rows
ACTION_CASES = ((1, 1), (1, 38), (31, 7), (33, 8), (65, 9), (8192, 38), (8193, 38))


def action_inputs(family, n, A):
    """logits [n][2 A] and noise [n][A]: the plain / hard logits of loss_head_ref.make_inputs (hard: raw scales at -30 and +25, 5 % of the locations x 8)"""
    inp = make_inputs(family, 1, n, A, 1)
    return {"logits": inp["logits"][0].contiguous(), "noise": inp["noise"][0].contiguous()}


def sample_action(inp, dtype=torch.float64):
    logits, noise = inp["logits"].to(dtype), inp["noise"].to(dtype)
    A = noise.shape[-1]
    raw = logits[:, :A] + (softplus(logits[:, A:]) + MIN_STD) * noise
    return {"raw": raw, "action_t": torch.tanh(raw).t().contiguous(), "logp": log_prob(logits, raw)}


# ---- 1-wide head forward -----------------------------------------------------------------------------------------------------------------
HEAD_CASES = ((1, 4), (15, 252), (17, 256), (33, 260), (1, 1024))      # (M, K): one pass of 256 columns short, exact, and a second pass with one live lane


def head_inputs(M, K):
    rng = _rng(5, M, K)
    return {"x": _t(rng.standard_normal((M, K))), "w": _t(rng.standard_normal(K) / np.sqrt(K)), "b": _t(rng.standard_normal(1))}


def head_fwd(inp, with_bias, dtype=torch.float64):
    y = inp["x"].to(dtype) @ inp["w"].to(dtype)
    return y + inp["b"].to(dtype) if with_bias else y


# ---- grouped column sums -----------------------------------------------------------------------------------------------------------------
# 16 problems of one launch: widths around the 32-column block, rows (= partial rows) around the 8 row slices and the unrolled 64-row trip
COLSUM_WIDTHS = (1, 31, 32, 33, 76, 768, 256, 3, 64, 65, 100, 120, 1024, 17, 96, 129)
COLSUM_ROWS = (1, 7, 8, 9, 57, 64, 65, 640, 2, 63, 121, 128, 129, 5, 56, 72)


def colsum_inputs(i):
    return _t(_rng(6, i).standard_normal((COLSUM_ROWS[i], COLSUM_WIDTHS[i])))


# ---- references computed once per process ------------------------------------------------------------------------------------------------
_cache: dict = {}


def cached(key, make):
    """`make()` once per process under `key`; callers must not write to what they get"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def block_reference(family, rows, H):
    """(inputs, float64 result, float32 result)"""
    def make():
        inp = block_inputs(family, rows, H)
        return inp, block(inp, LN_EPS, torch.float64), block(inp, LN_EPS, torch.float32)
    return cached(("block", family, rows, H), make)


def block_error(name, got, ref):
    return array_error(got, ref[name])          # (the three rows of `grads` are three arrays here: each against its own largest entry)
