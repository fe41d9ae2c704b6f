"""Plain numpy reference for the N(0, 1) draws the kernels make themselves (tm_philox4x32_10 / tm_normal4 / tm_normal_at, csrc/act_shared.h) and for
the minibatch gather that carries two of the four streams (k_gather_minibatch, csrc/ppo_kernels.h; launch_minibatch, csrc/tmjx_hip.hip).  Nothing of
track_mjx_amd is imported: every expected value of tests/test_gpu_noise_gather.py comes from here.

A draw is a pure function of (seed, draw counter, stream, element index):

    words   = Philox4x32-10(counter = (q, stream, ctr & 0xffffffff, ctr >> 32), key = (seed & 0xffffffff, seed >> 32)),   q = element // 4
    uniform = ((word >> 8) as float32 + 0.5f) * 2^-24                                                              (each step one IEEE operation)
    element 4 q + 0 .. 3 = r0 cos(2 pi v0), r0 sin(2 pi v0), r1 cos(2 pi v1), r1 sin(2 pi v1),  r = sqrt(-2 log u),  (u0, v0, u1, v1) = the uniforms of words 0 .. 3

Streams: 0 = latent_eps [T B Z] and 1 = entropy_noise [T B A] of tmjx_minibatch_begin, 2 = tmjx_latent_concat with eps == NULL (element e Z + c), 3 =
tmjx_sample_action with noise == NULL (element e A + a); tmjx_policy_act draws from 2 and 3.

The uniforms lie in (0, 1], not in (0, 1): `(float)(x >> 8) + 0.5f` is exact below 2^23 only, from there on an odd value rounds to the next even
integer, and the top 24-bit value gives 2^24 * 2^-24 = 1.0 exactly — radius 0, both normals 0.  Philox is integer arithmetic and the uniform is exact
float32 arithmetic, so `uniforms` is bit-exact by construction; only logf, sqrtf and sincospif have a tolerance.

Metric and bound: `array_error` and `bound` of tests/loss_head_ref.py — kernel error <= max(4 e32, 2^-20), largest absolute error over largest
reference magnitude, e32 the error of `normals(..., float32)` against `normals(..., float64)`.  The gather is element-wise IEEE arithmetic: bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.loss_head_ref import array_error as _array_error, bound  # noqa: F401  (re-exported)

CAP = 2.0 ** -10
M32 = np.uint64(0xFFFFFFFF)
STREAM_LATENT_EPS, STREAM_ENTROPY_NOISE, STREAM_ACT_LATENT, STREAM_ACT_ACTION = 0, 1, 2, 3
STATE_WORDS = 16 + 16 * 64          # TMJX_MINIBATCH_STATE_WORDS (include/tmjx.h): {draw counter, slot, top ticket, ... | 64 sub-tickets, one 128-byte line each}
SUBTICKETS = 64
GRID_CAP, BLOCK = 8192, 256

# Random123's kat_vectors for philox4x32-10: (counter[4] + key[2], output[4])
KAT = (([0, 0, 0, 0, 0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ([0xffffffff] * 6, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]))


def array_error(got, ref) -> float:
    return _array_error(torch.from_numpy(np.ascontiguousarray(got, dtype=np.float64)), torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64)))


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def _w(x):
    return np.asarray(x, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words (they broadcast against each other): the four output words"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_w(v) for v in (c0, c1, c2, c3, k0, k1)))
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def uniforms(x):
    """tm_normal4's uniform of a 32-bit word, restated operation by operation in float32 (in (0, 1]: see the module's header)"""
    return ((_w(x) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def draw_words(seed: int, ctr: int, stream: int, q):
    """the four Philox words of block(s) q of a stream"""
    return philox4x32_10(q, stream, ctr & 0xFFFFFFFF, ctr >> 32, seed & 0xFFFFFFFF, seed >> 32)


def normals(seed: int, ctr: int, stream: int, n: int, dtype=np.float64):
    """elements 0 .. n - 1 of the stream at (seed, draw counter), Box-Muller evaluated in `dtype` on the float32 uniforms"""
    x = draw_words(seed, ctr, stream, np.arange((n + 3) // 4, dtype=np.uint64))
    out = np.empty((x[0].size, 4), dtype=dtype)
    for h in range(2):
        u1, u2 = uniforms(x[2 * h]).astype(dtype), uniforms(x[2 * h + 1]).astype(dtype)
        r = np.sqrt(dtype(-2.0) * np.log(u1))
        ang = dtype(np.pi) * (dtype(2.0) * u2)
        out[:, 2 * h], out[:, 2 * h + 1] = r * np.cos(ang), r * np.sin(ang)
    return out.reshape(-1)[:n]


_cache: dict = {}


def reference(seed, ctr, stream, n):
    """(float64 draws, float32 restatement, e32), computed once per process; callers must not write to them"""
    key = (seed, ctr, stream, n)
    if key not in _cache:
        r64, r32 = normals(seed, ctr, stream, n, np.float64), normals(seed, ctr, stream, n, np.float32)
        _cache[key] = (r64, r32, array_error(r32, r64))
    return _cache[key]


# ---- the directed extreme draws (stream 0, q < 1024; tests/test_noise_ref_cpu.py re-derives them by search) ---------------------------------
DIRECTED_SEED = 0x1234567887654321
DIRECTED_ZERO_BITS = (4294972718, 756)          # (counter, q): the top 24 bits of word 0 are zero — the smallest uniform, radius sqrt(-2 log 2^-25) = 5.887
DIRECTED_ALL_ONES = (4294974497, 351)           # the top 24 bits of word 0 are all ones — uniform exactly 1.0, elements 4 q and 4 q + 1 exactly 0
R_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -25)))


def find_directed(seed, first_ctr, stream=0, nq=1024, chunk=4096):
    """the first counters >= first_ctr at which some q < nq has the top 24 bits of word 0 all zero / all ones: ((ctr, q), (ctr, q))"""
    q = np.arange(nq, dtype=np.uint64)[None, :]
    found = [None, None]
    ctr = first_ctr
    while None in found:
        c = np.arange(ctr, ctr + chunk, dtype=np.uint64)[:, None]
        top = philox4x32_10(q, stream, c & M32, c >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)[0] >> np.uint64(8)
        for k, want in enumerate((0, 0xFFFFFF)):
            if found[k] is None:
                hit = np.argwhere(top == np.uint64(want))
                if len(hit):
                    found[k] = (ctr + int(hit[0][0]), int(hit[0][1]))
        ctr += chunk
    return tuple(found)


# ---- the noise cases of tmjx_minibatch_begin ------------------------------------------------------------------------------------------------
# (T, B, Z, A).  The first five are the cases specified for the remainders of the array lengths mod 4 — T B Z | T B A = 1 | 1, 3 | 1, 2 | 2, 0 | 2, 0 | 2 —
# which leave T B A without remainder 3 (the last two cases add remainder 0): (1, 1, 1, 3) is added for it, so that both arrays end in a Philox block
# with one, two, three and four live elements.  Then the case that reaches both directed draws (3840 latent elements: q < 960) and a realistic small step
NOISE_CASES = ((1, 1, 1, 1), (1, 3, 5, 3), (2, 3, 7, 5), (1, 5, 60, 38), (3, 7, 60, 38), (1, 1, 1, 3), (1, 64, 60, 38), (20, 64, 60, 38))
DIRECTED_CASE = (1, 64, 60, 38)
NOISE_COUNTERS = (0, 7, 2 ** 32 + 7, 2 ** 63 - 1)          # (the last one with advance = 0 only: the counter is a signed 64-bit word on the device)
NOISE_SEEDS = (0, DIRECTED_SEED, 2 ** 64 - 1)
NOISE_MODES = ("both", "eps", "noise")
NOISE_W = 4                                               # the gather under the noise cases is as small as the entry takes


# ---- the launch's work items and grid ---------------------------------------------------------------------------------------------------------
def work_items(T, B, W, A, Z, eps, noise) -> int:
    """launch_minibatch's count: float4 groups of obs_n and next_n, raw-action elements, 4 scalar planes, one item per Philox block of each array drawn"""
    n_act = T * B * A
    return T * B * (W // 4) + B * (W // 4) + n_act + 4 * T * B + ((T * B * Z + 3) // 4 if eps else 0) + ((n_act + 3) // 4 if noise else 0)


def grid(T, B, W, A, Z, eps=True, noise=True) -> int:
    return min((work_items(T, B, W, A, Z, eps, noise) + BLOCK - 1) // BLOCK, GRID_CAP)


# (T, B, W, A, Z), both arrays drawn: the grids at which the two-level ticket changes shape — one workgroup; fewer than 64 (one member per sub-ticket,
# nsub = grid); exactly 64; 65 .. 129 (sub-tickets with one and with two, then with two and with three members)
TICKET_CASES = ((1, 1, 4, 1, 1), (2, 11, 8, 3, 5), (2, 665, 8, 3, 5), (2, 676, 8, 3, 5), (2, 690, 8, 3, 5), (2, 1350, 8, 3, 5), (2, 1360, 8, 3, 5), (2, 1370, 8, 3, 5))
TICKET_GRIDS = (1, 2, 63, 64, 65, 127, 128, 129)
CAPPED_CASE = (9, 1000, 696, 38, 60)                      # more than 8192 x 256 items: the noise lies in the second trip of the grid-stride loop
CAPPED_R = 1024
TICKET_C0, TICKET_S0, TICKET_LAUNCHES = 2 ** 32 - 2, 1, 4  # (the four launches carry the counter across 2^32)


def ticket_rows(B):
    """R of a ticket case: fewer rows than the minibatch has, so the permutation repeats rows"""
    return max(1, min(B, 300) - 1)


# ---- the gather -------------------------------------------------------------------------------------------------------------------------------
GATHER_W, GATHER_A, GATHER_B, GATHER_T = (4, 8, 696, 700), (1, 3, 38), (1, 77), (1, 5)
GATHER_SLOT = 2
SCALARS = ("log_prob", "reward", "discount", "truncation")      # the [4][T][B] order of scalars_g (include/tmjx.h)


def gather_rows(B):
    """R in {1 (every index 0), B, 300}"""
    return tuple(dict.fromkeys((1, B, 300)))


def gather_cases():
    return tuple((T, R, B, W, A) for W in GATHER_W for A in GATHER_A for B in GATHER_B for R in gather_rows(B) for T in GATHER_T)


def make_perm(rng, R, B, slots, slot):
    """int64 [slots * B] with values in [0, R); the slice of `slot` holds R - 1, 0 and a duplicate (as far as B allows), the other slices other rows"""
    perm = rng.integers(0, R, size=slots * B, dtype=np.int64)
    s = perm[slot * B:(slot + 1) * B]
    s[0] = R - 1
    if B >= 3:
        s[1], s[2] = 0, s[B - 1]
    return perm


def gather_inputs(T, R, B, W, A, slots=GATHER_SLOT + 2, slot=GATHER_SLOT, family="hard", tag=0):
    """float32 roll-out leaves [T][R][..], next_last [R][W], the normaliser and a permutation of `slots` minibatches.  hard: 5 % of the columns (and
    always column 1) near-constant with std = 1e-6, 2 % of the other values up to +-1e6; every quotient is 0 or in float32's normal range"""
    rng = np.random.default_rng([7, T, R, B, W, A, tag])
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    mean, std = f(rng.standard_normal(W)), f(np.exp(rng.uniform(-1.5, 1.5, W)))

    def observations(*lead):
        v = mean + 3.0 * std * rng.standard_normal(lead + (W,))
        if family == "hard":
            u = rng.random(lead + (W,))
            v = np.where(u < 0.02, rng.uniform(-1e6, 1e6, lead + (W,)), v)
        return v
    if family == "hard":
        tiny = rng.random(W) < 0.05
        tiny[1] = True
        std[tiny], mean[tiny] = np.float32(1e-6), np.float32(0.25)
    obs, nxt = observations(T, R), observations(R)
    if family == "hard":
        obs[..., tiny], nxt[..., tiny] = 0.25 + 1e-6 * rng.standard_normal((T, R, int(tiny.sum()))), 0.25 + 1e-6 * rng.standard_normal((R, int(tiny.sum())))
    out = {"obs": f(obs), "next_last": f(nxt), "raw_action": f(rng.standard_normal((T, R, A))), "mean": mean, "std": std, "perm": make_perm(rng, R, B, slots, slot)}
    for k in SCALARS:
        out[k] = f(rng.standard_normal((T, R)))
    return out


def normalise(v, mean, std):
    """(v - mean) / std in float32: two IEEE operations per element, what tm_obs_normalised and the gather kernels evaluate"""
    assert v.dtype == mean.dtype == std.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return (v - mean) / std


def gather(inp, idx):
    """the seven outputs of the fused gather at rows `idx`: obs_n [T][B][W], next_n [B][W], raw_action_g [T][B][A], scalars_g [4][T][B]"""
    return {"obs_n": normalise(inp["obs"][:, idx], inp["mean"], inp["std"]), "next_n": normalise(inp["next_last"][idx], inp["mean"], inp["std"]),
            "raw_action_g": inp["raw_action"][:, idx], "scalars_g": np.stack([inp[k][:, idx] for k in SCALARS], 0)}


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ---- bf16 -------------------------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> the uint16 pattern of its bfloat16, round to nearest, ties to even, by integer operations on the bits; NaN -> a quiet NaN"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, (b >> np.uint64(16)) | np.uint64(0x0040), rounded).astype(np.uint16)


def bf16_is_nan(h):
    return (np.asarray(h).astype(np.uint32) & 0x7FFF) > 0x7F80


# float32 patterns planted in the observations of the bf16 cases: ties with an even and an odd upper half (round-to-even and round-half-up differ on the
# even ones), just above and below a tie, the tie that rounds to infinity, both infinities, a NaN
BF16_PLANTED = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7F8000, 0xFF7F8000, 0x7F800000, 0xFF800000, 0x7FC00001)
BF16_CASES = ((1, 1, 1, 4), (2, 40, 77, 696))          # (T, R, B, W)


def bf16_inputs(T, R, B, W):
    """gather inputs with mean 0 and std 1 (obs_n is the observation, to the bit) and BF16_PLANTED in the rows the slot's slice gathers"""
    inp = gather_inputs(T, R, B, W, 3, family="plain", tag=16)
    inp["mean"][:], inp["std"][:] = 0.0, 1.0
    rows = inp["perm"][GATHER_SLOT * B:(GATHER_SLOT + 1) * B]
    flat = inp["obs"].view(np.uint32)
    rng = np.random.default_rng([16, T, R, B, W])
    for k in range(max(len(BF16_PLANTED), (T * B * W) // 50)):
        flat[rng.integers(T), rows[rng.integers(B)], rng.integers(W)] = BF16_PLANTED[k % len(BF16_PLANTED)]
    if T * B * W < 4 * len(BF16_PLANTED):              # the one-row case: its four values are the four ties
        flat[0, rows[0], :4] = BF16_PLANTED[:4]
    return inp


# ---- acting path ------------------------------------------------------------------------------------------------------------------------------
ACT_LATENT_CASES = ((1, 1), (3, 5), (33, 60), (65, 60), (8192, 16), (8193, 16))      # (n, Z): the last two cross the one-wave / 256-thread launch
ACT_ACTION_CASES = ((1, 1), (3, 7), (65, 9), (33, 38), (8192, 38), (8193, 38))       # (n, A)
ACT_COUNTERS = (5, 2 ** 32 + 5)
ACT_SEEDS = (DIRECTED_SEED, 2 ** 32 + 1234)
ACT_OBS_W, ACT_REF_W, ACT_PAD = 3, 1, 1          # the latent cases' observation part: two columns and one pad column behind the Z latent ones
