"""The float64 reference of the wavelet spectrogram (include/tmjx.h: tmjx_spectrogram; DESIGN.md "Spectrogram"), a float32 numpy restatement of the
kernel's evaluation order, the cases and the checks that tests/test_spectrogram_cpu.py (host emulation) and tests/test_gpu_spectrogram.py (C-ABI)
share.  A `backend` is analysis.pca.HipBackend or the emulation's stand-in: `wavelet_bank`, `spectrogram`, `asarray`, `to_numpy`.

The error bound, per output, against the float64 definition evaluated with the unrounded tables and the unrounded mean:

    |A - A64| <= (3 L + 8) u S + 4 u |m|,    u = 2^-24,  L = the taps in range,  S = (2 / G) sum_tau g[tau] |xt[t + tau]|  (>= A64).

Derivation (first order in u; L u <= 2^-11 for L <= 8193, so the second-order terms are below a thousandth of the first).  The kernel forms
re = sum wr32[tau] xt32[t + tau] as one float32 FMA chain in ascending tau.  Each product carries the rounding of the table entry (u), of the
subtraction xt32 = fl(x - m32) (u) and the chain adds at most L u of its own (the standard bound of a recursive sum of L terms, one rounding per
FMA): |re - re64'| <= (L + 2) u sum |wr| |xt|, and likewise im with wi.  Because wr^2 + wi^2 = g^2 in every term, Minkowski's inequality gives
sqrt(dre^2 + dim^2) <= (L + 2) u sum g |xt|, so the modulus moves by at most (L + 2) u (G / 2) S.  The square root's argument fma(re, re, im im)
carries two roundings (2 u relative, halved by the root), the root one, the product with 2 none, the division one: 3 u A <= 3 u S.  G is a
difference of float64 prefix sums rounded once: u A <= u S (a float32 accumulation of G in ascending order, which the bound is written to admit,
would cost (L - 1) u S instead: (L + 2) + (L - 1) + 3 + 1 <= 3 L + 8 either way).  Last, xt32 is taken about m32 = fl(m64), off by at most
u |m| in every tap: the modulus moves by at most (2 / G) sum g u |m| = 2 u |m|, doubled for the float64 sums behind m64 and the cancellation
in x - m.  Total: (L + 2 + 3 + 1) u S + 4 u |m| <= (3 L + 8) u S + 2^-22 |m|.  Zero products from rows outside the sequence leave a chain's bits
as they are, so L counts the taps in range only.
For output = log the bound is the amplitude bound over max(A64, floor) (the slope of ln, to first order; where both sides sit on the floor the
error is 0) plus 4 u |ln| for logf (within 2 ulp on both targets) and the rounding of its argument.
"""
from __future__ import annotations

import functools
import math

import numpy as np

U24 = 2.0 ** -24
RATE = 50.0
f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731
f64 = lambda a: np.ascontiguousarray(a, np.float64)      # noqa: E731


def dyadic(f_min, f_max, n):
    return f_min * (f_max / f_min) ** (np.arange(n) / (n - 1)) if n > 1 else np.array([float(f_min)])


DEFAULT_BANK = dyadic(1.0, 25.0, 25)
FIVE = dyadic(1.0, 25.0, 5)
# (lengths, C, frequencies): the smallest shapes at which the tiling can go wrong
EDGE = ((1, 2, 5, 63, 64, 65, 129, 400), 3, FIVE)
CHANNEL_CASES = tuple(((37, 150), C, np.array([3.0, 12.5])) for C in (1, 3, 64, 65, 67, 130))
F1 = ((40, 200), 2, np.array([5.0]))
F64 = ((40, 200), 2, dyadic(2.0, 25.0, 64))
PRODUCT = ((249,) * 4, 67, DEFAULT_BANK)


def seq_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


@functools.lru_cache(None)
def _signal(lengths, C, seed):
    r = np.random.default_rng(seed)
    n = int(sum(lengths))
    t = np.arange(n)[:, None]
    x = 3.0 + r.standard_normal((1, C)) + np.sin(2 * np.pi * (2.0 + 4.0 * r.random((1, C))) * t / RATE + 6.28 * r.random((1, C))) + 0.3 * r.standard_normal((n, C))
    x = f32(x)
    x.setflags(write=False)
    return x


def signal(case, seed=5):
    return _signal(tuple(case[0]), case[1], seed)


def tables64(freqs, rate=RATE, omega0=5.0, support=4.0):
    """[(R, g, wr, wi)] float64, tau = -R .. R, as the header defines them."""
    out = []
    for f in f64(freqs):
        sigma = omega0 * rate / (2.0 * math.pi * f)
        R = int(math.ceil(support * sigma))
        tau = np.arange(-R, R + 1, dtype=np.float64)
        g = np.exp(-tau * tau / (2.0 * sigma * sigma))
        ph = 2.0 * math.pi * f * tau / rate
        out.append((R, g, g * np.cos(ph), -g * np.sin(ph)))
    return out


def _toeplitz(w, R, T):
    """M [t, t'] = w[t' - t] for |t' - t| <= R, else 0."""
    d = np.arange(T)[None, :] - np.arange(T)[:, None]
    return np.where(np.abs(d) <= R, w[np.clip(d + R, 0, 2 * R)], 0.0)


def spectrogram64(x, lengths, freqs, detrend=True, log=False, floor=1e-3, rate=RATE, omega0=5.0, support=4.0):
    """The definition in float64 -> (out [n, F C], coverage [n, F], bound [n, F C]): the outputs, and the error bound of every one."""
    x, tabs = f64(x), tables64(freqs, rate, omega0, support)
    (n, C), F = x.shape, len(tabs)
    out, cov, bound = np.zeros((n, F * C)), np.zeros((n, F)), np.zeros((n, F * C))
    seq = seq_of(lengths)
    for s0, s1 in zip(seq[:-1], seq[1:]):
        T = s1 - s0
        m = x[s0:s1].mean(0) if detrend else np.zeros(C)
        xt = x[s0:s1] - m
        for j, (R, g, wr, wi) in enumerate(tabs):
            Mg = _toeplitz(g, R, T)
            G, L = Mg.sum(1), (Mg > 0).sum(1)
            re, im = _toeplitz(wr, R, T) @ xt, _toeplitz(wi, R, T) @ xt
            A = 2.0 * np.sqrt(re * re + im * im) / G[:, None]
            S = 2.0 * (Mg @ np.abs(xt)) / G[:, None]
            b = (3 * L[:, None] + 8) * U24 * S + 2.0 ** -22 * np.abs(m)[None, :]
            if log:
                v = np.log(np.maximum(A, floor))
                b = b / np.maximum(A, floor) + 4 * U24 * np.abs(v)
                A = v
            out[s0:s1, j * C:(j + 1) * C], bound[s0:s1, j * C:(j + 1) * C], cov[s0:s1, j] = A, b, G / g.sum()
    return out, cov, bound


def _fma32(a, b, c):
    """fl32(a b + c) through float64: the product is exact there, the sum is rounded twice (to 53 bits, then to 24)."""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def spectrogram32(x, lengths, freqs, detrend=True, log=False, floor=1e-3, variant=None, rate=RATE, omega0=5.0, support=4.0):
    """The kernel's evaluation order in float32 numpy (csrc/spectrogram_core.h): the mean from four interleaved float64 row classes, xt = x - m in
    float32, re and im as FMA chains in ascending tau over the float32 tables, G a difference of float64 prefix sums rounded once,
    A = 2 sqrt(fma(re, re, im im)) / G.  variant: None, or one of three deliberate mistakes: "shift" (the window one tap late), "no_renorm" (the whole
    envelope's sum for G), "mean_left_in"."""
    x, tabs = f32(x), tables64(freqs, rate, omega0, support)
    (n, C), F = x.shape, len(tabs)
    out, cov = np.zeros((n, F * C), np.float32), np.zeros((n, F), np.float32)
    seq = seq_of(lengths)
    for s0, s1 in zip(seq[:-1], seq[1:]):
        T = s1 - s0
        xs = x[s0:s1]
        if detrend and variant != "mean_left_in":
            cls = [f64(xs[h::4]).cumsum(0)[-1] if T > h else np.zeros(C) for h in range(4)]      # (cumsum: a sum in row order)
            m = ((((cls[0] + cls[1]) + cls[2]) + cls[3]) / float(T)).astype(np.float32)
            xt = (xs - m[None, :]).astype(np.float32)
        else:
            xt = xs
        t = np.arange(T)
        for j, (R, g, wr, wi) in enumerate(tabs):
            g32, wr32, wi32 = f32(g), f32(wr), f32(wi)
            P = np.concatenate([[0.0], f64(g32).cumsum()])
            re, im = np.zeros((T, C), np.float32), np.zeros((T, C), np.float32)
            sh = 1 if variant == "shift" else 0
            for tau in range(-R, R + 1):
                lo_t, hi_t = max(0, -(tau + sh)), min(T, T - (tau + sh))      # the rows whose tap lies inside the sequence
                if lo_t >= hi_t:
                    continue
                src = xt[lo_t + tau + sh:hi_t + tau + sh]
                re[lo_t:hi_t] = _fma32(wr32[tau + R], src, re[lo_t:hi_t])
                im[lo_t:hi_t] = _fma32(wi32[tau + R], src, im[lo_t:hi_t])
            lo, hi = np.maximum(-R, -t), np.minimum(R, T - 1 - t)
            G = (P[hi + R + 1] - P[lo + R]).astype(np.float32)
            Gall = np.float32(P[2 * R + 1])
            den = np.full(T, Gall, np.float32) if variant == "no_renorm" else G
            mod = np.sqrt(_fma32(re, re, (im * im).astype(np.float32)))
            A = ((np.float32(2.0) * mod).astype(np.float32) / den[:, None]).astype(np.float32)
            if log:
                A = np.log(np.maximum(A, np.float32(floor))).astype(np.float32)
            out[s0:s1, j * C:(j + 1) * C], cov[s0:s1, j] = A, (G / Gall).astype(np.float32)
    return out, cov


@functools.lru_cache(None)
def _reference(lengths, C, freqs, detrend, log, seed=5):
    return spectrogram64(_signal(lengths, C, seed), lengths, np.array(freqs), detrend, log)


def reference(case, detrend=True, log=False):
    """The float64 reference of a case, computed once and shared."""
    return _reference(tuple(case[0]), case[1], tuple(float(f) for f in case[2]), detrend, log)


def worst_ratio(out, cov, ref):
    r_out, r_cov, bound = ref
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, np.abs(f64(out) - r_out) / np.where(bound > 0, bound, 1.0), np.where(f64(out) == r_out, 0.0, np.inf))
    return float(ratio.max()), float(np.abs(f64(cov) - r_cov).max())


def check(out, cov, ref, what=""):
    """Every output within its bound, every coverage within 4 u (a float64 difference rounded once, a division)."""
    out, cov = np.asarray(out), np.asarray(cov)
    assert out.shape == ref[0].shape and cov.shape == ref[1].shape and out.dtype == np.float32 and cov.dtype == np.float32, (what, out.shape, cov.shape)
    assert np.isfinite(out).all() and np.isfinite(cov).all(), what
    ratio, cerr = worst_ratio(out, cov, ref)
    print(f"[spectrogram] {what}: worst error / bound {ratio:.4f}, coverage error {cerr:.3e}")
    assert ratio <= 1.0, (what, ratio)
    assert cerr <= 4 * U24, (what, cerr)
    return ratio


def run(backend, case, detrend=True, log=False, x=None, out=None):
    lengths, C, freqs = case
    x = signal(case) if x is None else x
    bank, offset, radius = backend.wavelet_bank(RATE, freqs)
    o, c = backend.spectrogram(backend.asarray(x), seq_of(lengths), bank, offset, radius, detrend, log, 1e-3, out)
    return backend.to_numpy(o), backend.to_numpy(c)


def check_bank(backend):
    """The host bank builder against the float64 tables: the radii, the offsets, every entry within half an ulp plus libm's float64 error."""
    for freqs in (FIVE, DEFAULT_BANK, F64[2], np.array([25.0]), np.array([0.05])):      # (0.05 Hz: a radius of 3184)
        bank, offset, radius = backend.wavelet_bank(RATE, freqs)
        tabs = tables64(freqs)
        assert list(radius) == [t[0] for t in tabs] and offset[0] == 0 and list(np.diff(offset)) == [3 * (2 * t[0] + 1) for t in tabs]
        assert bank.dtype == np.float32 and bank.shape == (offset[-1],)
        for j, (R, g, wr, wi) in enumerate(tabs):
            want = np.concatenate([g, wr, wi])
            got = bank[offset[j]:offset[j + 1]]
            assert np.abs(f64(got) - want).max() <= U24 * 1.001 and got[R] == 1.0 and got[2 * R + 1 + R] == 1.0 and got[2 * (2 * R + 1) + R] == 0.0
    assert list(backend.wavelet_bank(RATE, FIVE)[2]) == [160, 72, 32, 15, 7]


def sinusoid(j, n=1000):
    t = np.arange(n)
    return f32(3.0 + np.sin(2 * np.pi * DEFAULT_BANK[j] * t / RATE + 0.4))[:, None]


def check_analysis(out, cov, j, what="", exact=True):
    """A unit sinusoid with offset 3 at bank frequency j (f_j <= rate / 4) of the default bank: A = 1 in the interior at column j, the argmax over the
    frequencies is j, coverage is 1 where the window fits (exactly in the kernel, whose interior G is the whole
    sum; to 1e-12 in the float64 reference, which adds in another order) and between 0.5 and 0.65 at row 0."""
    radius = np.array([t[0] for t in tables64(DEFAULT_BANK)])
    n = out.shape[0]
    R = radius[j]
    inner = slice(R, n - R)
    err = float(np.abs(f64(out[inner, j]) - 1.0).max())
    print(f"[spectrogram] {what}: frequency {j} ({DEFAULT_BANK[j]:.3f} Hz): interior |A - 1| <= {err:.2e}, coverage at row 0 {cov[0].min():.3f} .. {cov[0].max():.3f}")
    assert err <= 1e-4, (what, j, err)
    full = slice(radius.max(), n - radius.max())
    assert (np.argmax(out[full], 1) == j).all(), (what, j)
    for k, Rk in enumerate(radius):
        assert (np.abs(f64(cov[Rk:n - Rk, k]) - 1.0) <= (0.0 if exact else 1e-12)).all() and (cov[:Rk, k] < 1.0).all() and (cov[n - Rk:, k] < 1.0).all(), (what, k)
    assert (cov[0] >= 0.5).all() and (cov[0] <= 0.65).all() and (cov[-1] >= 0.5).all() and (cov[-1] <= 0.65).all(), (what, cov[0])


def check_length_one(backend, what=""):
    """A sequence of one row: exactly 0 with detrend on (the row is its own mean), 2 |x| within the bound with it off."""
    case = ((1, 1, 7, 1), 3, FIVE)
    x = signal(case)
    out, cov = run(backend, case, True)
    for row in (0, 1, 9):
        assert (out[row] == 0.0).all() and (cov[row] > 0).all(), (what, row, out[row])
    out, cov = run(backend, case, False)
    ref = reference(case, False)
    check(out, cov, ref, f"{what}, sequences of one row, detrend off")
    for row in (0, 1, 9):
        assert np.abs(f64(out[row]).reshape(5, 3) - 2.0 * np.abs(f64(x[row]))[None, :]).max() <= ref[2][row].max(), (what, row)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_bits(backend, what=""):
    """Two runs give the same bits; a sequence's rows and coverage have the same bits alone, first, last, and between two sequences of NaN, whose
    own outputs are NaN."""
    lengths, C, freqs = (150,), 3, FIVE
    mid = signal((lengths, C, freqs), seed=11)
    other = signal(((70,), C, freqs), seed=12)
    nan = np.full((70, C), np.nan, np.float32)
    for detrend, log in ((True, False), (False, True)):
        alone = run(backend, (lengths, C, freqs), detrend, log, x=mid)
        again = run(backend, (lengths, C, freqs), detrend, log, x=mid)
        for a, b in zip(alone, again):
            np.testing.assert_array_equal(bits(a), bits(b))
        first = run(backend, ((150, 70), C, freqs), detrend, log, x=np.concatenate([mid, other]))
        last = run(backend, ((70, 150), C, freqs), detrend, log, x=np.concatenate([other, mid]))
        between = run(backend, ((70, 150, 70), C, freqs), detrend, log, x=np.concatenate([nan, mid, nan]))
        for got, rows in ((first, slice(0, 150)), (last, slice(70, 220)), (between, slice(70, 220))):
            for g, a in zip(got, alone):
                np.testing.assert_array_equal(bits(g[rows]), bits(a), err_msg=f"{what}: detrend {detrend}, log {log}")
        assert np.isnan(between[0][:70]).all() and np.isnan(between[0][220:]).all() and np.isfinite(between[0][70:220]).all(), what
        assert np.isfinite(between[1]).all()


# ---------------------------------------------------------------------------------------------------------------- the feature earns its place
@functools.lru_cache(None)
def planted():
    """Rate 50, 8 segments of 250 rows alternating between 2 Hz and 6 Hz, 3 channels of unit amplitude with random phases, Gaussian noise of 0.1
    -> (x [2000, 3] float32, truth [2000])."""
    r = np.random.default_rng(0)
    xs, truth = [], []
    t = np.arange(250)[:, None]
    for seg in range(8):
        f = 2.0 if seg % 2 == 0 else 6.0
        xs.append(np.sin(2 * np.pi * f * t / RATE + 2 * np.pi * r.random((1, 3))) + 0.1 * r.standard_normal((250, 3)))
        truth += [seg % 2] * 250
    x = f32(np.concatenate(xs))
    x.setflags(write=False)
    return x, np.array(truth)


PLANTED_BANK = dyadic(1.0, 12.5, 12)


def agreement(labels, truth):
    a = float((np.asarray(labels) == truth).mean())
    return max(a, 1.0 - a)


def check_planted(backend, what=""):
    """2-means on the raw samples finds the segments at chance (at most 0.6 of the rows: the float64 definition with a plain 2-means measured 0.502);
    on the spectrogram amplitudes it finds at least 0.95 of them (measured 0.998 there)."""
    from track_mjx_amd.analysis import cluster
    from track_mjx_amd.analysis.spectrogram import Spectrogram
    x, truth = planted()
    raw = agreement(cluster.KMeans(2, n_init=4, seed=0, backend=backend).fit(np.array(x)).labels_, truth)
    sp = Spectrogram(RATE, frequencies=PLANTED_BANK, backend=backend)
    feats, cov = sp.transform(np.array(x), [2000])
    assert feats.shape == (2000, 36) and cov.shape == (2000, 12) and sp.columns_.shape == (36, 2) and list(sp.columns_[4]) == [1, 1]
    amp = agreement(cluster.KMeans(2, n_init=4, seed=0, backend=backend).fit(feats).labels_, truth)
    sl = Spectrogram(RATE, frequencies=PLANTED_BANK, output="log", backend=backend)
    lg = agreement(cluster.KMeans(2, n_init=4, seed=0, backend=backend).fit(sl.transform(np.array(x), [2000])[0]).labels_, truth)
    print(f"[spectrogram] {what}: 2-means agrees with the planted segments on {raw:.3f} of the raw rows, {amp:.3f} of the amplitude rows, {lg:.3f} of the log rows")
    assert raw <= 0.6, (what, raw)
    assert amp >= 0.95, (what, amp)


# ---------------------------------------------------------------------------------------------------------------- command line
def clip_files(tmp_path, lengths=(90, 70, 110)):
    """Three small synthetic clip_<i>.h5 with ctrl [T - 1, 4], qposes_rollout [T, 9] (the last two columns swing at 2 Hz in the first half of a clip
    and at 6 Hz in the second), activations/intention [T - 1, 6], a [T - 1] metric and meta -> the directory."""
    from track_mjx_amd import h5lite
    r = np.random.default_rng(3)
    for clip, T in zip((0, 3, 4), lengths):
        t = np.arange(T)[:, None]
        f = np.where(t < T // 2, 2.0, 6.0)
        q = np.concatenate([r.standard_normal((T, 7)), np.sin(2 * np.pi * f * t / RATE + r.random((1, 2)))], 1) + 0.05 * r.standard_normal((T, 9))
        h5lite.write_tree(str(tmp_path / f"clip_{clip}.h5"), {
            "ctrl": f32(r.standard_normal((T - 1, 4))), "qposes_rollout": f32(q), "activations": {"intention": f32(r.standard_normal((T - 1, 6)))},
            "rollout_metrics": {"pos_reward": f32(r.random(T - 1))}, "meta": {"clip_idx": np.int64(clip), "model": "mlp"}})
    return str(tmp_path)


def check_cli(tmp_path, backend, capsys):
    """The tool end to end: the files it writes, projections=, the clustering, HMM and PCA tools on its output unchanged, usage errors return 2."""
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import cluster, hmm, pca
    from track_mjx_amd.analysis import spectrogram as SP
    (tmp_path / "clips").mkdir()
    rollouts, lengths = clip_files(tmp_path / "clips"), {0: 90, 3: 70, 4: 110}
    out = str(tmp_path / "spec")
    base = [f"rollouts={rollouts}", "rate=50"]
    assert SP.main(base + ["source=qposes_rollout", "cols=7:", "f_min=1", "f_max=25", "n_freqs=6", "output=log", f"out={out}"], backend=backend) == 0
    assert "[spectrogram] qposes_rollout[7:]: 270 rows x 2 channels from 3 clips at 6 frequencies" in capsys.readouterr().out
    for c, T in lengths.items():
        with h5lite.File(f"{out}/clip_{c}.h5") as h:
            feat, cov, fr = (np.asarray(h[k][()]) for k in ("activations/spectrogram", "spectrogram_coverage", "frequencies"))
            meta = {k: h["spectrogram_meta"][k][()] for k in ("source", "cols", "rate", "omega0", "support", "detrend", "output", "floor", "n_channels")}
            assert int(np.asarray(h["meta"]["clip_idx"][()])) == c and bytes(h["meta"]["model"][()]) == b"mlp"
        assert feat.shape == (T, 12) and feat.dtype == np.float32 and cov.shape == (T, 6) and cov.dtype == np.float32 and np.isfinite(feat).all()
        np.testing.assert_allclose(fr, dyadic(1.0, 25.0, 6), rtol=1e-12)
        assert bytes(meta["source"]) == b"qposes_rollout" and bytes(meta["cols"]) == b"7:" and bytes(meta["output"]) == b"log"
        assert float(meta["rate"]) == 50.0 and float(meta["omega0"]) == 5.0 and float(meta["support"]) == 4.0 and int(meta["detrend"]) == 1
        assert float(meta["floor"]) == 1e-3 and int(meta["n_channels"]) == 2 and (cov > 0).all() and (cov <= 1).all()
    # ctrl has one row fewer than the poses
    out2 = str(tmp_path / "spec_ctrl")
    assert SP.main(base + ["source=ctrl", "n_freqs=4", f"out={out2}"], backend=backend) == 0
    with h5lite.File(f"{out2}/clip_3.h5") as h:
        assert np.asarray(h["activations/spectrogram"][()]).shape == (69, 16)
    # the leading components of a layer, from a pca.h5
    pca_file = str(tmp_path / "pca.h5")
    assert pca.main([f"rollouts={rollouts}", "feature=intention", "n_components=3", f"out={pca_file}"], backend=backend) == 0
    out3 = str(tmp_path / "spec_pca")
    assert SP.main(base + [f"projections={pca_file}", "cols=:2", "n_freqs=5", f"out={out3}"], backend=backend) == 0
    with h5lite.File(f"{out3}/clip_4.h5") as h:
        assert np.asarray(h["activations/spectrogram"][()]).shape == (109, 10) and bytes(h["spectrogram_meta"]["projections"][()]) == b"pca.h5"
    capsys.readouterr()
    # the motif tools take the directory unchanged
    assert cluster.main([f"rollouts={out}", "feature=spectrogram", "k=2", "n_init=2", f"out={tmp_path / 'clusters.h5'}"], backend=backend) == 0
    assert "270 samples x 12 features from 3 clips into 2 motifs" in capsys.readouterr().out
    with h5lite.File(str(tmp_path / "clusters.h5")) as h:
        lab = np.asarray(h["labels"]["clip_4"][()])
    inner = np.r_[10:45, 65:100]      # away from the clip's edges and from the switch at row 55
    assert lab.shape == (110,) and agreement(lab[inner], np.r_[np.zeros(35), np.ones(35)]) >= 0.9
    assert hmm.main([f"rollouts={out}", "feature=spectrogram", "k=2", "n_init=1", "max_iter=5", f"out={tmp_path / 'hmm.h5'}"], backend=backend) == 0
    assert pca.main([f"rollouts={out}", "feature=spectrogram", "n_components=2", f"out={tmp_path / 'pca_spec.h5'}"], backend=backend) == 0
    capsys.readouterr()
    assert SP.main(base + ["source=activations/intention", "n_freqs=64", "f_min=5", f"out={out2}"], backend=backend) == 0      # 64 x 6 = 384 columns
    capsys.readouterr()
    # refusals: exit status 2 with a message
    wide = str(tmp_path / "wide")
    (tmp_path / "wideclips").mkdir()
    h5lite.write_tree(str(tmp_path / "wideclips" / "clip_0.h5"), {"ctrl": np.zeros((30, 41), np.float32)})
    for argv, word in (([f"rollouts={tmp_path / 'wideclips'}", "rate=50", "source=ctrl", f"out={wide}"], "cols="),      # 25 x 41 = 1025 columns
                       (base + ["source=velocity", f"out={wide}"], "unknown source"),
                       (base + ["source=qposes_rollout", "cols=9:", f"out={wide}"], "selects no column"),
                       (base + ["source=qposes_rollout", "cols=x", f"out={wide}"], "expected a:b"),
                       (base + ["source=ctrl", "f_max=26", f"out={wide}"], "rate / 2"),
                       (base + ["source=rollout_metrics/pos_reward", f"out={wide}"], "expected [T, C]"),
                       (base + ["source=activations/decoder/layer_9", f"out={wide}"], "decoder/layer_9"),
                       (base + ["source=ctrl", "output=power", f"out={wide}"], "amplitude or log"),
                       (base + ["source=ctrl", "detrend=maybe", f"out={wide}"], "true or false"),
                       (base + ["source=ctrl", "f_min=0.001", f"out={wide}"], "4096")):
        assert SP.main(argv, backend=backend) == 2, argv
        err = capsys.readouterr().err
        assert "[spectrogram]" in err and word in err, (argv, err)
    for word in ("cols=", "n_freqs=", "projections="):      # the ways out of the width limit are named
        SP.main([f"rollouts={tmp_path / 'wideclips'}", "rate=50", "source=ctrl", f"out={wide}"], backend=backend)
        assert word in capsys.readouterr().err
    for argv in ([f"rollouts={rollouts}", "source=ctrl", f"out={wide}"], base + ["source=ctrl"], base + ["source=ctrl", f"out={wide}", "colour=red"], base + [f"out={wide}"]):
        assert SP.main(argv, backend=backend) == 2      # no rate=, no out=, an unknown option, neither source= nor projections=
        assert "usage:" in capsys.readouterr().err
    import os
    assert not os.path.exists(wide)
