"""GPU: the N(0, 1) draws the kernels make themselves and the minibatch gather, element for element against tests/noise_ref.py, through the C entries
with raw pointers.  A draw is a pure function of (seed, draw counter, stream, element index), so every element of every noise array has a stated
value: latent_eps = stream 0 and entropy_noise = stream 1 of tmjx_minibatch_begin, stream 2 under tmjx_latent_concat (eps == NULL), stream 3 under
tmjx_sample_action (noise == NULL).  Moments cannot see a wrong element-to-draw map, a dropped high word of the counter or of the seed, a stream id
used twice or a last Philox block that runs over its array: these comparisons can.

The bound of every noise array: with e32 the error of the float32 restatement against float64 (largest absolute error / largest reference magnitude),
the kernel's error must be <= max(4 e32, 2^-20); tests/test_noise_ref_cpu.py keeps every e32 of these case lists under 2^-10.  The gather is IEEE
arithmetic per element and is compared bit for bit, the bf16 twin against an integer round-to-nearest-even.  Outputs are prefilled with NaN and
followed by a sentinel tail.  Every noise comparison prints `NG | case | array | kernel error | e32 | bound`; DESIGN.md ("Device-side noise and the
minibatch gather") has the measured table."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from tests import noise_ref as N
from tests import row_kernels_ref as R
from track_mjx_amd import hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 12345.0
SENTINEL16 = 0x7FC1          # (a bf16 NaN pattern no kernel output has: the hardware convert quiets a NaN to 0x7FC0 | payload of the gathered value)
TAIL = 64
LEAVES = ("obs", "next_last", "raw_action") + N.SCALARS + ("perm", "mean", "std")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _guard(n, tail=TAIL):
    buf = torch.full((n + tail,), float("nan"), device=DEV)
    buf[n:] = SENTINEL
    return buf


def _intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _upload(inp):
    return {k: torch.from_numpy(inp[k]).to(DEV) for k in LEAVES}


def _state(ctr, slot):
    st = torch.zeros(N.STATE_WORDS, dtype=torch.int64, device=DEV)
    st[0], st[1] = ctr, slot
    return st


class Outputs:
    """the output buffers of one launch of the fused gather, NaN-prefilled, each with its sentinel tail (the twin: sentinel everywhere)"""

    def __init__(self, T, B, W, A, Z, eps, noise, ld16=None):
        self.sizes = {"obs_n": T * B * W, "next_n": B * W, "raw_action_g": T * B * A, "scalars_g": 4 * T * B}
        self.shapes = {"obs_n": (T, B, W), "next_n": (B, W), "raw_action_g": (T, B, A), "scalars_g": (4, T, B)}
        if eps:
            self.sizes["eps"], self.shapes["eps"] = T * B * Z, (T * B * Z,)
        if noise:
            self.sizes["noise"], self.shapes["noise"] = T * B * A, (T * B * A,)
        self.buf = {k: _guard(n) for k, n in self.sizes.items()}
        self.ld16, self.rows16, self.W = ld16, T * B, W
        self.twin = None if ld16 is None else torch.full((T * B * ld16 + TAIL,), SENTINEL16, dtype=torch.int16, device=DEV)

    def ptr(self, k):
        return self.buf[k].data_ptr() if k in self.buf else None

    def read(self):
        """after a synchronize: every tail intact, then the arrays as numpy"""
        for k, n in self.sizes.items():
            assert _intact(self.buf[k], n), k
        out = {k: self.buf[k][:n].cpu().numpy().reshape(self.shapes[k]) for k, n in self.sizes.items()}
        if self.twin is not None:
            t = self.twin.cpu().numpy().view(np.uint16)
            body = t[:self.rows16 * self.ld16].reshape(self.rows16, self.ld16)
            assert (t[self.rows16 * self.ld16:] == SENTINEL16).all() and (body[:, self.W:] == SENTINEL16).all(), "twin: pad columns / tail"
            out["twin"] = body[:, :self.W]
        return out


def _begin(dev, out, T, R_, B, W, A, Z, state, seed=0, advance=1):
    """tmjx_minibatch_begin (or _bf16 when `out` has a twin) on uploaded leaves `dev`; no synchronize"""
    m = hip.Minibatch(*(dev[k].data_ptr() for k in LEAVES), out.ptr("obs_n"), out.ptr("next_n"), out.ptr("raw_action_g"), out.ptr("scalars_g"), out.ptr("eps"),
                      out.ptr("noise"), None if state is None else state.data_ptr(), seed, T, R_, B, W, A, Z, advance)
    if out.twin is None:
        hip.check(hip.lib().tmjx_minibatch_begin(C.byref(m), _st()), "tmjx_minibatch_begin")
    else:
        hip.check(hip.lib().tmjx_minibatch_begin_bf16(C.byref(m), _p(out.twin), out.ld16, _st()), "tmjx_minibatch_begin_bf16")


def _gather_equal(got, ref, tag):
    """the seven gathered outputs bit for bit: obs_n, next_n, raw_action_g and the four planes of scalars_g in the header's order"""
    for k in ("obs_n", "next_n", "raw_action_g"):
        assert N.same_bits(got[k], ref[k]), (tag, k, int((got[k].view(np.uint32) != ref[k].view(np.uint32)).sum()))
    for i, k in enumerate(N.SCALARS):
        assert N.same_bits(got["scalars_g"][i], ref["scalars_g"][i]), (tag, k)


def _noise_rows(got, seed, ctr, streams):
    """(array, kernel error, e32) of drawn arrays; streams: (output key, stream id)"""
    rows = []
    for key, sid in streams:
        r64, r32, e32 = N.reference(seed, ctr, sid, got[key].size)
        assert np.isfinite(got[key]).all(), key
        rows.append((key, N.array_error(got[key], r64), e32))
    return rows


def _check(rows, tag):
    bad = []
    for name, err, e32 in rows:
        b = N.bound(e32)
        print(f"NG | {tag} | {name} | {err:.2e} | {e32:.2e} | {b:.2e}")
        if not err <= b:
            bad.append((name, err, e32, b))
    return [(tag,) + r for r in bad]


# ---- a. tmjx_minibatch_begin: the noise, draw for draw ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", N.NOISE_MODES)
@pytest.mark.parametrize("T,B,Z,A", N.NOISE_CASES, ids=_ids(N.NOISE_CASES))
def test_minibatch_noise_draw_for_draw(T, B, Z, A, mode):
    """latent_eps = stream 0 [T B Z] and entropy_noise = stream 1 [T B A] at every seed and counter of the lists (high words of both set and clear; the
    largest counter with advance = 0), both arrays drawn, eps only and noise only (three layouts of the work items).  The directed case also runs the two
    counters whose block q holds the extreme uniforms: exactly 0.0 twice where the uniform is 1.0, the largest radius there is where it is 2^-25"""
    W, slots = N.NOISE_W, 2
    inp = N.gather_inputs(T, B, B, W, A, slots=slots, slot=0, family="plain", tag=2)
    dev, ref = _upload(inp), N.gather(inp, inp["perm"][:B])
    eps, noise = mode in ("both", "eps"), mode in ("both", "noise")
    streams = ([("eps", 0)] if eps else []) + ([("noise", 1)] if noise else [])
    runs = [(s, c) for s in N.NOISE_SEEDS for c in N.NOISE_COUNTERS]
    if (T, B, Z, A) == N.DIRECTED_CASE and eps:
        runs += [(N.DIRECTED_SEED, N.DIRECTED_ZERO_BITS[0]), (N.DIRECTED_SEED, N.DIRECTED_ALL_ONES[0])]
    bad = []
    for seed, ctr in runs:
        advance = int(ctr < 2 ** 63 - 1)
        state, out = _state(ctr, 0), Outputs(T, B, W, A, Z, eps, noise)
        _begin(dev, out, T, B, B, W, A, Z, state, seed, advance)
        torch.cuda.synchronize()
        got = out.read()
        tag = f"begin {mode} {T}x{B} Z{Z} A{A} seed {seed:#x} ctr {ctr:#x}"
        assert state[:2].tolist() == [ctr + advance, advance] and not bool(state[2:].any()), tag
        _gather_equal(got, ref, tag)
        bad += _check(_noise_rows(got, seed, ctr, streams), tag)
        if ctr == N.DIRECTED_ALL_ONES[0] and seed == N.DIRECTED_SEED:
            q = N.DIRECTED_ALL_ONES[1]
            assert got["eps"][4 * q] == 0.0 and got["eps"][4 * q + 1] == 0.0, got["eps"][4 * q:4 * q + 4]
        if ctr == N.DIRECTED_ZERO_BITS[0] and seed == N.DIRECTED_SEED:
            q = N.DIRECTED_ZERO_BITS[1]
            r64, _, e32 = N.reference(seed, ctr, 0, T * B * Z)
            pair = got["eps"][4 * q:4 * q + 2].astype(np.float64)
            print(f"NG | {tag} | extreme pair | {np.abs(pair - r64[4 * q:4 * q + 2]).max() / np.abs(r64).max():.2e} | {e32:.2e} | {N.bound(e32):.2e}")
            assert np.abs(pair - r64[4 * q:4 * q + 2]).max() <= N.bound(e32) * np.abs(r64).max() and abs(np.hypot(*pair) - N.R_MAX) <= 2.0 * N.bound(e32) * N.R_MAX
    assert not bad, bad


# ---- b. tickets and self-advance ---------------------------------------------------------------------------------------------------------------
def _ticket_inputs(T, B, W, A, Z):
    R_ = N.CAPPED_R if (T, B, W, A, Z) == N.CAPPED_CASE else N.ticket_rows(B)
    return R_, N.gather_inputs(T, R_, B, W, A, slots=N.TICKET_S0 + N.TICKET_LAUNCHES, slot=N.TICKET_S0, family="plain", tag=3)


def _after_launch(got, inp, state, k, T, B, Z, A, tag, advanced=True):
    """what must hold after launch k of a chain that started at (TICKET_C0, TICKET_S0)"""
    c, s = N.TICKET_C0 + k, N.TICKET_S0 + k
    assert state[:2].tolist() == [c + int(advanced), s + int(advanced)] and not bool(state[2:].any()), (tag, k, state[:3].tolist())
    _gather_equal(got, N.gather(inp, inp["perm"][s * B:(s + 1) * B]), (tag, k))
    return _check(_noise_rows(got, N.DIRECTED_SEED, c, (("eps", 0), ("noise", 1))), f"{tag} launch {k}")


@pytest.mark.parametrize("T,B,W,A,Z", N.TICKET_CASES + (N.CAPPED_CASE,), ids=[f"grid{g}" for g in N.TICKET_GRIDS] + ["grid8192-capped"])
def test_tickets_and_self_advance(T, B, W, A, Z):
    """four consecutive launches on one state at grids of 1, 2, 63, 64, 65, 127, 128, 129 workgroups and at the cap: after each the counter and the slot are
    one further and every ticket word is back at zero, the rows are the next slice of the permutation and the noise is the next counter's (the counter
    crosses 2^32 on the way); with advance = 0 the state is untouched and a repeat gives the same bits"""
    R_, inp = _ticket_inputs(T, B, W, A, Z)
    dev, tag = _upload(inp), f"tickets grid {N.grid(T, B, W, A, Z)}"
    state, bad = _state(N.TICKET_C0, N.TICKET_S0), []
    for k in range(N.TICKET_LAUNCHES):
        out = Outputs(T, B, W, A, Z, True, True)
        _begin(dev, out, T, R_, B, W, A, Z, state, N.DIRECTED_SEED)
        torch.cuda.synchronize()
        got = out.read()
        bad += _after_launch(got, inp, state, k, T, B, Z, A, tag)
        first = got if k == 0 else first
    state[0], state[1] = N.TICKET_C0, N.TICKET_S0
    before = state.clone()
    for _ in range(2):
        out = Outputs(T, B, W, A, Z, True, True)
        _begin(dev, out, T, R_, B, W, A, Z, state, N.DIRECTED_SEED, advance=0)
        torch.cuda.synchronize()
        again = out.read()
        assert torch.equal(state, before)
        assert all(N.same_bits(again[k], first[k]) for k in first), tag
    assert not bad, bad


@contextlib.contextmanager
def _capture(graph):
    gc.collect()
    enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            yield
    finally:
        if enabled:
            gc.enable()


def test_captured_launch_replays_and_advances_itself():
    """the launch captured as a graph of one kernel node and replayed three times without host input: every replay reads the next slot and counter"""
    T, B, W, A, Z = N.TICKET_CASES[N.TICKET_GRIDS.index(65)]
    R_, inp = _ticket_inputs(T, B, W, A, Z)
    dev = _upload(inp)
    state, out = _state(N.TICKET_C0, N.TICKET_S0), Outputs(T, B, W, A, Z, True, True)
    _begin(dev, out, T, R_, B, W, A, Z, state, N.DIRECTED_SEED, advance=0)          # (the kernel's code is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with _capture(graph):
        _begin(dev, out, T, R_, B, W, A, Z, state, N.DIRECTED_SEED)
    torch.cuda.synchronize()
    assert state[:2].tolist() == [N.TICKET_C0, N.TICKET_S0]          # a capture launches nothing
    bad = []
    for k in range(3):
        for b in out.buf.values():
            b[:-TAIL] = float("nan")
        graph.replay()
        torch.cuda.synchronize()
        bad += _after_launch(out.read(), inp, state, k, T, B, Z, A, "tickets graph replay")
    assert not bad, bad


# ---- c. the gather, bit for bit ---------------------------------------------------------------------------------------------------------------
_WA = tuple((W, A) for W in N.GATHER_W for A in N.GATHER_A)


@pytest.mark.parametrize("W,A", _WA, ids=_ids(_WA))
def test_gather_entries_bit_for_bit(W, A):
    """tmjx_gather_normalize, tmjx_gather_minibatch and tmjx_minibatch_begin (slot 2 of a longer permutation, no draws) at B in {1, 77}, R in {1, B, 300},
    T in {1, 5}, the hard family (columns with std = 1e-6, values up to 1e6): all seven outputs equal to the float32 numpy gather to the bit.  The
    slice holds row R - 1, row 0 and a duplicate; the slices in front of it hold other rows"""
    L = hip.lib()
    for T, R_, B, W_, A_ in N.gather_cases():
        if (W_, A_) != (W, A):
            continue
        tag = f"gather T{T} R{R_} B{B} W{W} A{A}"
        inp = N.gather_inputs(T, R_, B, W, A)
        dev = _upload(inp)
        sl = slice(N.GATHER_SLOT * B, (N.GATHER_SLOT + 1) * B)
        ref = N.gather(inp, inp["perm"][sl])
        idx = dev["perm"][sl]          # (a view: the slice's first element, 8-byte aligned)
        # tmjx_gather_normalize: the observations, and the bootstrap observation as its T = 1 form
        o1, o2 = _guard(T * B * W), _guard(B * W)
        hip.check(L.tmjx_gather_normalize(_p(dev["obs"]), _p(idx), _p(dev["mean"]), _p(dev["std"]), _p(o1), T, R_, B, W, _st()), "tmjx_gather_normalize")
        hip.check(L.tmjx_gather_normalize(_p(dev["next_last"]), _p(idx), _p(dev["mean"]), _p(dev["std"]), _p(o2), 1, R_, B, W, _st()), "tmjx_gather_normalize")
        # tmjx_gather_minibatch: the slice passed as idx
        out_g = Outputs(T, B, W, A, 1, False, False)
        hip.check(L.tmjx_gather_minibatch(*(_p(dev[k]) for k in ("obs", "next_last", "raw_action") + N.SCALARS), _p(idx), _p(dev["mean"]), _p(dev["std"]),
                                          *(C.c_void_p(out_g.ptr(k)) for k in ("obs_n", "next_n", "raw_action_g", "scalars_g")), T, R_, B, W, A, _st()), "tmjx_gather_minibatch")
        # tmjx_minibatch_begin: the slot from the state
        state, out_b = _state(9, N.GATHER_SLOT), Outputs(T, B, W, A, 1, False, False)
        _begin(dev, out_b, T, R_, B, W, A, 1, state, advance=0)
        torch.cuda.synchronize()
        assert _intact(o1, T * B * W) and _intact(o2, B * W), tag
        assert N.same_bits(o1[:T * B * W].cpu().numpy().reshape(T, B, W), ref["obs_n"]) and N.same_bits(o2[:B * W].cpu().numpy().reshape(B, W), ref["next_n"]), tag
        _gather_equal(out_g.read(), ref, tag + " gather_minibatch")
        _gather_equal(out_b.read(), ref, tag + " minibatch_begin")
        assert state[:2].tolist() == [9, N.GATHER_SLOT] and not bool(state[2:].any())


# ---- d. the bf16 twin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 8], ids=["ld=W", "ld=W+8"])
@pytest.mark.parametrize("T,R_,B,W", N.BF16_CASES, ids=_ids(N.BF16_CASES))
def test_bf16_twin_is_round_to_nearest_even(T, R_, B, W, pad):
    """mean 0 and std 1, so obs_n is the observation to the bit; planted: ties with an even and an odd upper half, the tie that rounds to infinity, both
    infinities, a NaN.  The twin equals the integer round-to-nearest-even of obs_n (NaN for NaN), its columns beyond W and its tail keep their sentinel,
    and the float32 outputs are bit-equal to the launch without a twin"""
    A, Z = 3, 5
    inp = N.bf16_inputs(T, R_, B, W)
    dev = _upload(inp)
    ref = N.gather(inp, inp["perm"][N.GATHER_SLOT * B:(N.GATHER_SLOT + 1) * B])
    res = []
    for ld16 in (None, W + pad):
        state, out = _state(2 ** 32 + 7, N.GATHER_SLOT), Outputs(T, B, W, A, Z, True, True, ld16)
        _begin(dev, out, T, R_, B, W, A, Z, state, N.DIRECTED_SEED)
        torch.cuda.synchronize()
        res.append(out.read())
        assert state[:2].tolist() == [2 ** 32 + 8, N.GATHER_SLOT + 1] and not bool(state[2:].any())
    plain, twin = res
    for k in plain:
        assert N.same_bits(plain[k], twin[k]), k
    obs_n = twin["obs_n"].reshape(T * B, W)
    nan = np.isnan(obs_n)
    assert N.same_bits(obs_n[~nan], ref["obs_n"].reshape(T * B, W)[~nan]) and (nan == np.isnan(ref["obs_n"].reshape(T * B, W))).all()
    want = N.bf16_rne(obs_n).reshape(T * B, W)
    assert (N.bf16_is_nan(twin["twin"]) == nan).all() and (N.bf16_is_nan(want) == nan).all()
    assert (twin["twin"][~nan] == want[~nan]).all(), int((twin["twin"][~nan] != want[~nan]).sum())
    bits = obs_n.view(np.uint32)
    assert (bits == 0x3F808000).any() and (bits == 0x3F818000).any() and (T * B * W < 48 or ((bits == 0x7F7F8000).any() and nan.any() and np.isinf(obs_n).any()))
    assert not _check(_noise_rows(twin, N.DIRECTED_SEED, 2 ** 32 + 7, (("eps", 0), ("noise", 1))), f"bf16 twin {T}x{B}x{W} ld {W + pad}")


# ---- e. the acting path ----------------------------------------------------------------------------------------------------------------------
def _t64(a, *shape):
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(*shape)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("n,Z", N.ACT_LATENT_CASES, ids=_ids(N.ACT_LATENT_CASES))
def test_latent_concat_draws_stream_2(n, Z, fam):
    """eps == NULL: element (e, c) of the latent noise is draw e Z + c of stream 2 at the state's counter; x against the float64 reference of
    tests/row_kernels_ref.py fed with the float64 draws (the float32 restatement with the float32 draws); the state is left alone.  plain: the noise
    implied by x, (x - mean) / exp(logvar / 2), also matches draw for draw"""
    obs_w, ref_w = N.ACT_OBS_W, N.ACT_REF_W
    stride = Z + obs_w - ref_w + N.ACT_PAD
    inp = R.latent_inputs(fam, n, Z, obs_w, stride)
    fc2, obs, mo, so = (inp[k].to(DEV).contiguous() for k in ("fc2", "obs", "mean_o", "std_o"))
    bad = []
    for seed in N.ACT_SEEDS:
        for ctr in N.ACT_COUNTERS:
            e64, e32_, _ = N.reference(seed, ctr, N.STREAM_ACT_LATENT, n * Z)
            r64 = R.latent_concat(dict(inp, eps=_t64(e64, n, Z)), Z, obs_w, ref_w, stride, True)
            r32 = R.latent_concat(dict(inp, eps=_t64(e32_, n, Z)), Z, obs_w, ref_w, stride, True, torch.float32)
            state, x = torch.tensor([ctr, 0], dtype=torch.int64, device=DEV), _guard(n * stride)
            hip.check(hip.lib().tmjx_latent_concat(_p(fc2), None, _p(obs), _p(x), n, Z, obs_w, ref_w, obs_w, 1, _p(mo), _p(so), stride, seed, _p(state), _st()),
                      "tmjx_latent_concat")
            torch.cuda.synchronize()
            assert _intact(x, n * stride) and state.tolist() == [ctr, 0]
            x = x[:n * stride].view(n, stride).cpu()
            assert bool(torch.isfinite(x).all()) and bool((x[:, Z + obs_w - ref_w:] == 0).all())
            tag = f"latent {fam} {n} Z{Z} seed {seed:#x} ctr {ctr:#x}"
            rows = [("x", R.array_error(x, r64), R.array_error(r32, r64)), ("latent", R.array_error(x[:, :Z], r64[:, :Z]), R.array_error(r32[:, :Z], r64[:, :Z]))]
            if fam == "plain":
                f = inp["fc2"].double()
                implied = lambda t: ((t[:, :Z].double() - f[:, :Z]) / torch.exp(f[:, Z:] / 2.0)).reshape(-1).numpy()  # noqa: E731
                rows.append(("implied eps", N.array_error(implied(x), e64), N.array_error(implied(r32), e64)))
            bad += _check(rows, tag)
    assert not bad, bad


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("n,A", N.ACT_ACTION_CASES, ids=_ids(N.ACT_ACTION_CASES))
def test_sample_action_draws_stream_3(n, A, fam):
    """noise == NULL: element (e, a) of the action noise is draw e A + a of stream 3 at the state's counter; raw, action_t and logp against the float64
    reference fed with the float64 draws; the counter advances by exactly one per call and the ticket word is back at 0, at one-wave and 256-thread
    blocks.  plain: the noise implied by raw, (raw - loc) / scale, also matches draw for draw"""
    inp = R.action_inputs(fam, n, A)
    logits = inp["logits"].to(DEV).contiguous()
    bad = []
    for seed in N.ACT_SEEDS:
        for ctr in N.ACT_COUNTERS:
            z64, z32, _ = N.reference(seed, ctr, N.STREAM_ACT_ACTION, n * A)
            r64, r32 = R.sample_action(dict(inp, noise=_t64(z64, n, A))), R.sample_action(dict(inp, noise=_t64(z32, n, A)), torch.float32)
            state = torch.tensor([ctr, 0], dtype=torch.int64, device=DEV)
            raw, act, logp = _guard(n * A), _guard(n * A), _guard(n)
            hip.check(hip.lib().tmjx_sample_action(_p(logits), None, _p(raw), _p(act), _p(logp), n, A, seed, _p(state), _st()), "tmjx_sample_action")
            torch.cuda.synchronize()
            assert _intact(raw, n * A) and _intact(act, n * A) and _intact(logp, n) and state.tolist() == [ctr + 1, 0]
            got = {"raw": raw[:n * A].view(n, A).cpu(), "action_t": act[:n * A].view(A, n).cpu(), "logp": logp[:n].cpu()}
            assert all(bool(torch.isfinite(v).all()) for v in got.values())
            rows = [(k, R.array_error(got[k], r64[k]), R.array_error(r32[k], r64[k])) for k in ("raw", "action_t", "logp")]
            if fam == "plain":
                lg = inp["logits"].double()
                implied = lambda t: ((t.double() - lg[:, :A]) / (R.softplus(lg[:, A:]) + R.MIN_STD)).reshape(-1).numpy()  # noqa: E731
                rows.append(("implied noise", N.array_error(implied(got["raw"]), z64), N.array_error(implied(r32["raw"]), z64)))
            bad += _check(rows, f"action {fam} {n}x{A} seed {seed:#x} ctr {ctr:#x}")
    assert not bad, bad
