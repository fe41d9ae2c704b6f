"""CPU: conditions on the reference of tests/noise_ref.py alone, for the exact case lists tests/test_gpu_noise_gather.py compares the kernels on.  The
generator against Random123's known answers; streams, counter words and seed words that must not alias; the moments of the reference draws; the
conditioning cap e32 <= 2^-10 of every noise case (a case above it would let max(4 e32, 2^-20) hide a wrong kernel); the two directed extreme draws,
re-derived by search; the grids of the ticket cases; every index of every case inside its array; and — no device needed — the refusals of the entries."""
import ctypes

import numpy as np
import pytest

from tests import noise_ref as N
from track_mjx_amd import hip


def _u32(words):
    return [int(w) for w in words]


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for inp, want in N.KAT:
        assert _u32(N.philox4x32_10(*inp)) == want
    c = np.array([k[0] for k in N.KAT], dtype=np.uint64).T          # vectorised: the three vectors in one call
    assert [_u32(w) for w in np.array(N.philox4x32_10(*c)).T] == [k[1] for k in N.KAT]


def test_uniforms_are_the_float32_restatement_and_reach_one():
    """below 2^23 the half is exact; from there on odd values round to even; the top value gives exactly 1.0 and nothing gives 0"""
    x = np.array([0, 0xFF, 0x100, 0x7FFFFF00, 0x80000000, 0x80000100, 0x80000200, 0xFFFFFE00, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64)
    u = N.uniforms(x)
    assert u.dtype == np.float32
    want = [0.5, 0.5, 1.5, 8388607.5, 8388608.0, 8388610.0, 8388610.0, 16777214.0, 16777216.0, 16777216.0]      # x 2^-24; ties to even
    assert [float(v) * 2.0 ** 24 for v in u] == want
    assert float(u[-1]) == 1.0 and float(u.min()) == 2.0 ** -25
    r64, r32 = (N.normals(N.DIRECTED_SEED, N.DIRECTED_ALL_ONES[0], 0, 4096, d) for d in (np.float64, np.float32))
    assert np.isfinite(r64).all() and np.isfinite(r32).all()


def test_streams_counter_words_and_seed_words_do_not_alias():
    """streams 0 .. 3 differ from each other, counter c from c + 2^32 and seed s from s + 2^32, in every element of a 4096-element array"""
    n, s, c = 4096, 0x0000000187654321, 7
    base = [N.normals(s, c, k, n) for k in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert (base[i] != base[j]).all(), (i, j)
    assert (base[0] != N.normals(s, c + 2 ** 32, 0, n)).all()
    assert (base[0] != N.normals(s + 2 ** 32, c, 0, n)).all()
    assert (N.normals(s, c, 0, n) == base[0]).all() and (N.normals(s, c, 0, n - 3) == base[0][:n - 3]).all()      # a pure function, truncated to n


def test_element_map_of_one_block():
    """elements 4 q .. 4 q + 3 = r0 cos, r0 sin, r1 cos, r1 sin of the uniforms of words (0, 1) and (2, 3) of block q"""
    seed, ctr, q = N.DIRECTED_SEED, 2 ** 32 + 7, 5
    u = [float(N.uniforms(w)) for w in N.draw_words(seed, ctr, 1, np.uint64(q))]
    got = N.normals(seed, ctr, 1, 4 * q + 4)[4 * q:]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    want = [r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r1 * np.cos(2 * np.pi * u[3]), r1 * np.sin(2 * np.pi * u[3])]
    assert np.allclose(got, want, rtol=0, atol=1e-13)


def test_first_four_moments_of_the_reference_draws():
    n = 10 ** 6
    x = N.normals(N.DIRECTED_SEED, 2 ** 33 + 7, 0, n)
    m, v = x.mean(), x.var()
    skew, kurt = ((x - m) ** 3).mean() / v ** 1.5, ((x - m) ** 4).mean() / v ** 2
    print(f"NG-ref | moments | mean {m:+.5f} var {v:.5f} skew {skew:+.5f} kurt {kurt:.5f}")
    assert abs(m) < 5 / n ** 0.5 and abs(v - 1) < 5 * (2 / n) ** 0.5 and abs(skew) < 5 * (6 / n) ** 0.5 and abs(kurt - 3) < 5 * (24 / n) ** 0.5


# ---- the conditioning cap -----------------------------------------------------------------------------------------------------------------
def test_conditioning_cap_at_1_2_million_draws():
    r64, r32, e32 = N.reference(N.DIRECTED_SEED, 2 ** 33 + 7, 0, 1_200_000)
    print(f"NG-ref | 1.2 M draws | e32 {e32:.2e} max |ref| {np.abs(r64).max():.3f}")
    assert e32 <= N.CAP and r32.dtype == np.float32 and 5.0 < np.abs(r64).max() < N.R_MAX


def _cap(rows):
    bad = [(tag, e32) for tag, e32 in rows if not e32 <= N.CAP]
    print("NG-ref | largest e32 %.2e over %d arrays" % (max(e for _, e in rows), len(rows)))
    assert not bad, bad


@pytest.mark.parametrize("case", N.NOISE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_noise_cases_are_under_the_cap(case):
    T, B, Z, A = case
    counters = N.NOISE_COUNTERS + ((N.DIRECTED_ZERO_BITS[0], N.DIRECTED_ALL_ONES[0]) if case == N.DIRECTED_CASE else ())
    _cap([((seed, ctr, stream), N.reference(seed, ctr, stream, n)[2]) for seed in N.NOISE_SEEDS for ctr in counters
          for stream, n in ((0, T * B * Z), (1, T * B * A))])


def test_ticket_and_acting_cases_are_under_the_cap():
    rows = []
    for T, B, W, A, Z in N.TICKET_CASES + (N.CAPPED_CASE,):
        for k in range(N.TICKET_LAUNCHES):
            rows += [((T, B, k, s), N.reference(N.DIRECTED_SEED, N.TICKET_C0 + k, s, n)[2]) for s, n in ((0, T * B * Z), (1, T * B * A))]
    for stream, cases in ((2, N.ACT_LATENT_CASES), (3, N.ACT_ACTION_CASES)):
        rows += [((stream, n, w, seed, ctr), N.reference(seed, ctr, stream, n * w)[2]) for n, w in cases for seed in N.ACT_SEEDS for ctr in N.ACT_COUNTERS]
    _cap(rows)


# ---- the directed extreme draws -------------------------------------------------------------------------------------------------------------
def test_directed_extreme_draws_exist_where_the_case_list_says():
    """re-derived by search from counter 2^32 on (stream 0, q < 1024), then: the zero-bits draw is the smallest uniform and a radius of 5.887 (in both
    precisions), the all-ones draw a uniform of exactly 1.0 and two normals of exactly 0; both lie inside the directed case's latent array"""
    assert N.find_directed(N.DIRECTED_SEED, 2 ** 32) == (N.DIRECTED_ZERO_BITS, N.DIRECTED_ALL_ONES)
    T, B, Z, _ = N.DIRECTED_CASE
    n = T * B * Z
    for (ctr, q), top, u_want in ((N.DIRECTED_ZERO_BITS, 0, 2.0 ** -25), (N.DIRECTED_ALL_ONES, 0xFFFFFF, 1.0)):
        assert 4 * q + 1 < n and q < 1024
        w0 = int(N.draw_words(N.DIRECTED_SEED, ctr, 0, np.uint64(q))[0])
        assert w0 >> 8 == top and float(N.uniforms(w0)) == u_want
        for dtype in (np.float64, np.float32):
            pair = N.normals(N.DIRECTED_SEED, ctr, 0, n, dtype)[4 * q:4 * q + 2].astype(np.float64)
            if top:
                assert (pair == 0.0).all()
            else:
                assert abs(np.hypot(*pair) - N.R_MAX) < 1e-5 and abs(N.R_MAX - 5.887) < 1e-3
    r64 = N.normals(N.DIRECTED_SEED, N.DIRECTED_ZERO_BITS[0], 0, n)
    assert np.abs(r64).max() == np.abs(r64[4 * N.DIRECTED_ZERO_BITS[1]:4 * N.DIRECTED_ZERO_BITS[1] + 2]).max()          # nothing in the array is larger


# ---- case lists: remainders, grids, indices ------------------------------------------------------------------------------------------------
def test_noise_case_list_is_the_one_the_comparison_was_specified_on():
    assert N.NOISE_CASES[:5] == ((1, 1, 1, 1), (1, 3, 5, 3), (2, 3, 7, 5), (1, 5, 60, 38), (3, 7, 60, 38)) and N.NOISE_CASES[-2:] == ((1, 64, 60, 38), (20, 64, 60, 38))
    assert {T * B * Z % 4 for T, B, Z, A in N.NOISE_CASES} == {0, 1, 2, 3} and {T * B * A % 4 for T, B, Z, A in N.NOISE_CASES} == {0, 1, 2, 3}
    assert N.NOISE_COUNTERS == (0, 7, 2 ** 32 + 7, 2 ** 63 - 1) and N.NOISE_SEEDS == (0, 0x1234567887654321, 2 ** 64 - 1)
    assert N.ACT_LATENT_CASES == ((1, 1), (3, 5), (33, 60), (65, 60), (8192, 16), (8193, 16))
    assert N.ACT_ACTION_CASES == ((1, 1), (3, 7), (65, 9), (33, 38), (8192, 38), (8193, 38)) and 2 ** 32 + 5 in N.ACT_COUNTERS
    assert len(N.gather_cases()) == 4 * 3 * (2 * 2 + 3 * 2) and {c[1] for c in N.gather_cases()} == {1, 77, 300}
    # q_eps = 0 moves the first item of the entropy noise: the three modes give three different layouts of the same launch
    T, B, Z, A = N.NOISE_CASES[-1]
    assert len({N.work_items(T, B, N.NOISE_W, A, Z, e, n) for e, n in ((True, True), (True, False), (False, True))}) == 3


def test_ticket_grids():
    """grid() of the ticket cases is 1, 2, 63, 64, 65, 127, 128, 129, and the capped case has more than 8192 x 256 items, its draws all in the second trip"""
    assert tuple(N.grid(*c) for c in N.TICKET_CASES) == N.TICKET_GRIDS == (1, 2, 63, 64, 65, 127, 128, 129)
    T, B, W, A, Z = N.CAPPED_CASE
    assert N.CAPPED_CASE == (9, 1000, 696, 38, 60) and N.CAPPED_R == 1024
    assert N.grid(*N.CAPPED_CASE) == N.GRID_CAP == 8192 and N.work_items(T, B, W, A, Z, True, True) > 8192 * 256
    assert N.work_items(T, B, W, A, Z, False, False) > 8192 * 256          # the first draw's item index
    assert N.work_items(2, 3, 8, 5, 7, True, True) == 2 * 3 * 2 + 3 * 2 + 30 + 24 + 11 + 8
    # sub-ticket residue r of a grid has ceil((grid - r) / 64) members, and they add up to the grid
    for g in N.TICKET_GRIDS + (N.GRID_CAP,):
        assert sum((g - r + 63) // 64 for r in range(min(g, 64))) == g
    assert N.STATE_WORDS == 16 + 16 * 64 and N.TICKET_C0 < 2 ** 32 <= N.TICKET_C0 + N.TICKET_LAUNCHES - 1 and N.TICKET_S0 > 0


def _in_range(inp, R, B, slots):
    p = inp["perm"]
    return p.dtype == np.int64 and p.size == slots * B and int(p.min()) >= 0 and int(p.max()) < R and inp["obs"].shape[1] == R and inp["next_last"].shape[0] == R


def test_no_case_indexes_outside_an_array():
    for T, R, B, W, A in N.gather_cases():
        inp = N.gather_inputs(T, R, B, W, A)
        assert _in_range(inp, R, B, N.GATHER_SLOT + 2) and W % 4 == 0
        s = inp["perm"][N.GATHER_SLOT * B:(N.GATHER_SLOT + 1) * B]
        assert s.size == B and R - 1 in s and (B < 3 or (0 in s and len(set(s.tolist())) < B))
    for T, B, W, A, Z in N.TICKET_CASES + (N.CAPPED_CASE,):
        R = N.CAPPED_R if (T, B, W, A, Z) == N.CAPPED_CASE else N.ticket_rows(B)
        slots = N.TICKET_S0 + N.TICKET_LAUNCHES
        rng = np.random.default_rng(0)
        perm = N.make_perm(rng, R, B, slots, N.TICKET_S0)
        assert perm.size >= (N.TICKET_S0 + N.TICKET_LAUNCHES) * B and 0 <= int(perm.min()) and int(perm.max()) < R
    for T, R, B, W in N.BF16_CASES:
        assert _in_range(N.bf16_inputs(T, R, B, W), R, B, N.GATHER_SLOT + 2)


def test_hard_gather_family_has_its_columns_and_stays_in_the_normal_range():
    tiny_min = float(np.finfo(np.float32).tiny)
    for T, R, B, W, A in ((5, 300, 77, 696, 38), (1, 1, 1, 4, 1), (5, 77, 77, 700, 3)):
        inp = N.gather_inputs(T, R, B, W, A)
        assert float(inp["std"][1]) == float(np.float32(1e-6)) and (W < 100 or 0.02 < float((inp["std"] == np.float32(1e-6)).mean()) < 0.1)
        assert W < 100 or 5e5 < float(np.abs(inp["obs"]).max()) <= 1e6
        for k in ("obs", "next_last"):
            d = inp[k] - inp["mean"]
            q = N.normalise(inp[k], inp["mean"], inp["std"])
            assert np.isfinite(q).all() and ((q == 0) | (np.abs(q) >= tiny_min)).all() and ((d == 0) | (np.abs(d) >= tiny_min)).all()
        ref = N.gather(inp, inp["perm"][:B])
        assert ref["obs_n"].shape == (T, B, W) and ref["next_n"].shape == (B, W) and ref["raw_action_g"].shape == (T, B, A) and ref["scalars_g"].shape == (4, T, B)
        assert N.same_bits(ref["scalars_g"][2], inp["discount"][:, inp["perm"][:B]])


def test_bf16_rounding_by_integer_operations():
    import torch
    pat = np.array(N.BF16_PLANTED, dtype=np.uint32)
    got = N.bf16_rne(pat.view(np.float32))
    #       tie even -> down, tie odd -> up, the same negative; above / below a tie; the tie to infinity (both signs); infinities; NaN stays NaN
    want = [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x7F80, 0xFF80, 0x7F80, 0xFF80, None]
    for g, w in zip(got.tolist(), want):
        assert (N.bf16_is_nan(g) and g & 0x0040) if w is None else g == w, (hex(g), w)
    x = np.random.default_rng(3).standard_normal(100000).astype(np.float32) * np.float32(1e3)
    assert (N.bf16_rne(x) == torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)).all()          # (a cross-check only: the tests use bf16_rne)
    for T, R, B, W in N.BF16_CASES:
        inp = N.bf16_inputs(T, R, B, W)
        obs_n = N.gather(inp, inp["perm"][N.GATHER_SLOT * B:(N.GATHER_SLOT + 1) * B])["obs_n"]
        assert N.same_bits(obs_n[~np.isnan(obs_n)], inp["obs"][:, inp["perm"][N.GATHER_SLOT * B:(N.GATHER_SLOT + 1) * B]][~np.isnan(obs_n)])
        bits = set(obs_n.view(np.uint32).reshape(-1).tolist())
        assert bits >= set(N.BF16_PLANTED[:4]) and (T * B * W < 48 or bits >= set(N.BF16_PLANTED) - {0x7FC00001}) and (T * B * W < 48 or np.isnan(obs_n).any())


# ---- refusals: validation comes before any launch, so no device is needed -----------------------------------------------------------------
def _refused(rc, word):
    err = hip.lib().tmjx_last_error()
    assert rc == -22 and word in err, (rc, word, err)


def _mb(**over):
    a = 0x10000          # a non-null, 16-byte aligned dummy that is never dereferenced: validation fails first
    m = hip.Minibatch()
    for k in ("obs", "next_last", "raw_action", "log_prob", "reward", "discount", "truncation", "perm", "mean", "std", "obs_n", "next_n", "raw_action_g", "scalars_g",
              "eps", "noise", "state"):
        setattr(m, k, a)
    m.seed, m.T, m.R, m.B, m.W, m.A, m.Z, m.advance = 1, 2, 8, 4, 8, 3, 5, 1
    for k, v in over.items():
        setattr(m, k, v)
    return m


def test_minibatch_entries_refuse_bad_arguments_without_gpu():
    L, a = hip.lib(), ctypes.c_void_p(0x10000)
    for entry, call in (("tmjx_minibatch_begin", lambda m: L.tmjx_minibatch_begin(ctypes.byref(m), None)),
                        ("tmjx_minibatch_begin_bf16", lambda m: L.tmjx_minibatch_begin_bf16(ctypes.byref(m), a, 12, None))):
        for over in (dict(state=None), dict(state=None, eps=None), dict(state=None, noise=None), dict(state=None, eps=None, noise=None)):      # draws or advance, no state
            _refused(call(_mb(**over)), entry.encode() + b": draws / advance need the device state")
        for W in (0, 2, 6, 7, 9):
            _refused(call(_mb(W=W)), b"multiple of 4")
        for Z in (0, -1):
            _refused(call(_mb(Z=Z)), b"Z must be")
        for k in ("obs", "perm", "std", "scalars_g"):
            _refused(call(_mb(**{k: None})), b"null")
        for k in ("T", "R", "B", "A"):
            _refused(call(_mb(**{k: 0})), b"bad T / R / B / A / W")
    _refused(L.tmjx_minibatch_begin(None, None), b"null")
    m = _mb()
    for twin, ld in ((a, 4), (a, 10), (ctypes.c_void_p(0x10002), 8), (ctypes.c_void_p(0x10004), 8)):          # ld16 < W, ld16 % 4, a twin misaligned by 2 (and by 4) bytes
        _refused(L.tmjx_minibatch_begin_bf16(ctypes.byref(m), twin, ld, None), b"tmjx_minibatch_begin_bf16: the twin's rows")
    _refused(L.tmjx_minibatch_begin_bf16(ctypes.byref(m), None, 8, None), b"null")
    _refused(L.tmjx_gather_normalize(a, a, a, a, a, 1, 1, 1, 6, None), b"multiple of 4")
    _refused(L.tmjx_gather_minibatch(*[a] * 14, 1, 1, 1, 6, 1, None), b"multiple of 4")
