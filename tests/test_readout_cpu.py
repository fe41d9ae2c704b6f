"""The linear readout on the CPU: the host emulation of the kernel bodies (tests/hostemu/readout_emu.cpp),
called through the shared analysis backend (tests/hostemu/analysis_emu.py), under the checks tests/test_gpu_readout.py
applies to the kernels (the float64 reference of tests/readout_ref.py at the first four cases, the bit-level properties, the refusals), the product
library's refusals (no GPU is touched), analysis.readout on synthetic roll-outs through the emulation backend, the command-line tool, and the
emulation as a stand-alone program under the sanitizers."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import pca_ref as PR
from tests import readout_ref as R
from tests.hostemu import analysis_emu as E
from track_mjx_amd import hip
from track_mjx_amd.analysis import readout as RO

ROOT = Path(__file__).resolve().parents[1]
B = E.B
MID = R.CPU_CASES[1]      # 513 + 129 rows, 129 -> 38, three penalties: the case of the bit-level checks


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(None)
def run(case):
    return R.run_case(case, B)


@pytest.mark.parametrize("case", R.CPU_CASES)
def test_emu_against_float64(case):
    (mean_x, comp, var, mean_y, z), w, preds, r2, _ = run(case)
    R.check_case(case, w, preds, r2, "emulation")
    xtr, ytr = R.case_data(case)[:2]
    pm, pc, pv, _ = B.fit_wide(xtr)                               # the PCA part: tmjx_pca_fit_wide's bits
    for u, v in ((mean_x, pm), (comp, pc), (var, pv)):
        np.testing.assert_array_equal(bits(u), bits(v))
    if case[2] <= hip.PCA_MAX_D:                                     # and, up to 128 features, the narrow fit's
        for u, v in zip((mean_x, comp, var), B.fit(xtr)[:3]):
            np.testing.assert_array_equal(bits(u), bits(v))
    m64 = ytr.astype(np.float64).mean(0)
    assert (np.abs(mean_y - m64) <= 2.0 ** -24 * np.abs(m64)).all()  # float64 sums, rounded once


def test_two_calls_give_the_same_bits():
    xtr, ytr, xte, yte = R.case_data(MID)
    (mean_x, comp, var, mean_y, z), w, _, _, (sse, sst) = run(MID)
    again = B.readout_fit(xtr.copy(), ytr.copy())
    np.testing.assert_array_equal(bits(again[4]), bits(z))
    w2 = B.readout_weights(comp, var, z, R.lambdas_of(var, R.CASES[MID]))
    np.testing.assert_array_equal(bits(w2), bits(w))
    sse2, sst2 = B.readout_score(xte, yte, mean_x, w, mean_y)
    np.testing.assert_array_equal(bits(sse2), bits(sse))
    np.testing.assert_array_equal(bits(sst2), bits(sst))


def strided(a, pad_left, pad_right):
    buf = np.full((a.shape[0], a.shape[1] + pad_left + pad_right), 1e6, np.float32)
    buf[:, pad_left:pad_left + a.shape[1]] = a
    return buf[:, pad_left:pad_left + a.shape[1]]


def test_row_strides_give_the_dense_bits_and_ldo_is_respected():
    xtr, ytr, xte, yte = R.case_data(MID)
    (mean_x, comp, var, mean_y, z), w, preds, _, (sse, sst) = run(MID)
    xs, ys, xts, yts = strided(xtr, 3, 2), strided(ytr, 1, 6), strided(xte, 4, 1), strided(yte, 2, 2)
    assert B.asarray(xs) is xs and xs.strides[0] == 4 * (MID[2] + 5)               # no copy
    got = B.readout_fit(xs, ys)
    for u, v in zip(got[:5], (mean_x, comp, var, mean_y, z)):
        np.testing.assert_array_equal(bits(u), bits(v))
    sse2, sst2 = B.readout_score(xts, yts, mean_x, w, mean_y)
    np.testing.assert_array_equal(bits(sse2), bits(sse))
    np.testing.assert_array_equal(bits(sst2), bits(sst))
    m = MID[3]
    out = np.full((xte.shape[0], m + 3), -5.0, np.float32)
    E.over("tmjx_readout_predict", out=out[:, :m], ldo=m + 3).readout_predict(xts, mean_x, w[1], mean_y)
    np.testing.assert_array_equal(bits(out[:, :m]), bits(preds[1]))
    assert (out[:, m:] == -5.0).all()


def test_predict_reproduces_the_score_and_one_penalty_equals_its_row():
    xtr, ytr, xte, yte = R.case_data(MID)
    (mean_x, comp, var, mean_y, z), w, preds, _, (sse, sst) = run(MID)
    for i in range(w.shape[0]):
        host_sse, host_sst = R.sse_sst(yte, preds[i])
        assert (np.abs(sse[i] - host_sse) <= R.FLOOR * host_sse).all(), np.abs(sse[i] / host_sse - 1).max()
        assert (np.abs(sst - host_sst) <= R.FLOOR * host_sst).all()
        one = B.readout_score(xte, yte, mean_x, w[i:i + 1], mean_y)
        np.testing.assert_array_equal(bits(one[0][0]), bits(sse[i]))
        np.testing.assert_array_equal(bits(one[1]), bits(sst))


def test_a_constant_target_scores_nan():
    x = PR.make_data(90, 20, 3.0, 2)
    y = np.stack([x[:, 0] * 2.0, np.full(90, 4.0, np.float32)], 1).astype(np.float32)
    r = RO.Ridge((0.01, 1.0), backend=B).fit(x[:60], y[:60])
    r2 = r.score(x[60:], y[60:])
    assert r2.shape == (2, 2) and np.isnan(r2[:, 1]).all() and r2[0, 0] > 0.99 > r2[1, 0] and r.best_index_ == 0      # (alpha = 1 shrinks)


# ------------------------------------------------------------------------------------------------------------------ refusals
REFUSALS_FIT = (({"d": 0}, "d must be >= 1 .got 0."), ({"d": 1025, "ldx": 1025}, "d = 1025 exceeds the readout limit of 1024"), ({"m": 0}, "m must be >= 1 .got 0."),
                ({"m": 513, "ldy": 513}, "m = 513 exceeds the readout limit of 512"), ({"n": 1}, "n >= 2 rows .got 1."), ({"ldx": 11}, "ldx = 11 is smaller than d = 12"),
                ({"ldy": 2}, "ldy = 2 is smaller than m = 3"), ({"misalign": True}, "16-byte aligned"))


@pytest.mark.parametrize("library", ["emulation", "product"])
def test_fit_refusals_of_both_libraries(library):
    """The same marshalling and the same substitutes against the emulation and against the product library (which refuses before any launch)."""
    x, y = PR.make_data(8, 12), PR.make_data(8, 3, seed=1)
    on = B if library == "emulation" else E.product()
    for over, msg in REFUSALS_FIT:
        with pytest.raises(ValueError, match=msg):
            E.over("tmjx_readout_fit", on=on, **over).readout_fit(x, y)


def test_emu_refusals():
    x, y = PR.make_data(8, 12), PR.make_data(8, 3, seed=1)
    mean_x, comp, var, mean_y, z, _ = B.readout_fit(x, y)
    for lam, msg in (([0.0], r"lambda\[0\] = 0"), ([1.0, -2.0], r"lambda\[1\] = -2"), ([float("nan")], r"lambda\[0\] = .*nan"), ([float("inf")], r"lambda\[0\] = inf")):
        with pytest.raises(ValueError, match=msg + ".* must be finite and > 0"):
            B.readout_weights(comp, var, z, lam)
    with pytest.raises(ValueError, match="n_lambda = 0 penalties: a call takes 1 .. 16"):
        B.readout_weights(comp, var, z, [])
    with pytest.raises(ValueError, match="n_lambda = 17 penalties"):
        B.readout_weights(comp, var, z, np.ones(17))
    w = B.readout_weights(comp, var, z, [0.1, 1.0])
    with pytest.raises(ValueError, match="a prediction needs n >= 1 rows .got 0."):
        E.over("tmjx_readout_predict", n=0).readout_predict(x, mean_x, w[0], mean_y)
    with pytest.raises(ValueError, match="ldo = 2 is smaller than m = 3"):
        E.over("tmjx_readout_predict", ldo=2).readout_predict(x, mean_x, w[0], mean_y)
    with pytest.raises(ValueError, match="ldx = 11 is smaller than d = 12"):
        E.over("tmjx_readout_predict", ldx=11).readout_predict(x, mean_x, w[0], mean_y)
    with pytest.raises(ValueError, match="a readout score needs n >= 2 rows .got 1."):
        E.over("tmjx_readout_score", n=1).readout_score(x, y, mean_x, w, mean_y)
    with pytest.raises(ValueError, match="ldy = 2 is smaller than m = 3"):
        E.over("tmjx_readout_score", ldy=2).readout_score(x, y, mean_x, w, mean_y)
    with pytest.raises(ValueError, match="n_lambda = 17"):
        E.over("tmjx_readout_score", n_lambda=17).readout_score(x, y, mean_x, w, mean_y)
    with pytest.raises(ValueError, match="16-byte aligned"):
        E.over("tmjx_readout_score", misalign=True).readout_score(x, y, mean_x, w, mean_y)
    with pytest.raises(ValueError, match="n_lambda = 0 penalties"):
        E.over("tmjx_readout_score", n_lambda=0).readout_score(x, y, mean_x, w, mean_y)
    with pytest.raises(ValueError, match="ldx = 11 is smaller than d = 12"):
        E.over("tmjx_readout_score", ldx=11).readout_score(x, y, mean_x, w, mean_y)
    for call in (lambda **k: E.over("tmjx_readout_predict", **k).readout_predict(x, mean_x, w[0], mean_y),
                 lambda **k: E.over("tmjx_readout_score", **k).readout_score(x, y, mean_x, w, mean_y),
                 lambda **k: E.over("tmjx_readout_weights", **k).readout_weights(comp, var, z, [0.1, 1.0])):
        with pytest.raises(ValueError, match="d must be >= 1 .got 0."):
            call(d=0)
        with pytest.raises(ValueError, match="d = 1025 exceeds the readout limit of 1024"):
            call(d=1025)
        with pytest.raises(ValueError, match="m must be >= 1 .got 0."):
            call(m=0)
        with pytest.raises(ValueError, match="m = 513 exceeds the readout limit of 512"):
            call(m=513)
    with pytest.raises(ValueError, match=r"lambda\[0\] = 1e-50 must be finite and > 0 as a float32"):      # (it is rounded to float32: 0)
        B.readout_weights(comp, var, z, [1e-50])
    with pytest.raises(ValueError, match=r"lambda\[0\] = 1e\+39 must be finite and > 0 as a float32"):
        B.readout_weights(comp, var, z, [1e39])
    L, info, p = E.lib(), hip.PcaInfo(), x.ctypes.data
    assert L.tmjx_readout_fit(p, 8, 12, 12, None, 3, 3, p, p, p, p, p, p, C.byref(info), None) != 0 and b"null argument" in L.tmjx_last_error()
    assert L.tmjx_readout_predict(p, 8, 12, 12, p, None, p, 3, p, 3, None) != 0 and b"null argument" in L.tmjx_last_error()
    assert L.tmjx_readout_score(p, 8, 12, 12, p, 3, 3, p, p, p, 2, None, p, p, None) != 0 and b"null argument" in L.tmjx_last_error()
    assert L.tmjx_readout_workspace(8, 12, 3, 2, None) != 0 and b"null argument" in L.tmjx_last_error()
    bad = x.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match="did not converge|non-finite"):       # the PCA part's refusal passes through
        B.readout_fit(bad, y)
    wide_bad = PR.make_data(40, 130).copy()
    wide_bad[3, 77] = np.nan
    with pytest.raises(ValueError, match="tmjx_pca_fit_wide: the covariance is non-finite"):
        B.readout_fit(wide_bad, PR.make_data(40, 3, seed=1))


def test_library_refuses_before_any_launch():
    """The product library's own checks (no GPU is touched: the dummy pointers are never dereferenced), and its workspace sizes."""
    L = hip.lib()
    one, info, floats = C.c_void_p(1 << 20), hip.PcaInfo(), C.c_int64(0)
    lam = (C.c_double * 17)(*([1.0] * 17))

    def fit(n=8, d=12, ldx=12, m=3, ldy=3, x=one, ws=one, inf=C.byref(info)):
        return L.tmjx_readout_fit(x, n, d, ldx, one, m, ldy, one, one, one, one, one, ws, inf, None)

    def predict(n=8, d=12, ldx=12, m=3, ldo=3, w=one):
        return L.tmjx_readout_predict(one, n, d, ldx, one, w, one, m, one, ldo, None)

    def score(n=8, d=12, ldx=12, m=3, ldy=3, nl=2, sse=one, ws=one):
        return L.tmjx_readout_score(one, n, d, ldx, one, m, ldy, one, one, one, nl, sse, one, ws, None)

    def weights(d=12, m=3, nl=2, lams=lam, w=one):
        return L.tmjx_readout_weights(one, one, one, d, m, lams, nl, w, None)

    odd = C.c_void_p((1 << 20) + 4)
    for call, word in ((lambda: fit(d=0), b"d must be >= 1 (got 0)"), (lambda: fit(d=1025, ldx=1025), b"d = 1025 exceeds the readout limit of 1024"),
                       (lambda: fit(m=0), b"m must be >= 1 (got 0)"), (lambda: fit(m=513, ldy=513), b"m = 513 exceeds the readout limit of 512"),
                       (lambda: fit(n=1), b"n >= 2 rows (got 1)"), (lambda: fit(ldx=11), b"ldx = 11 is smaller than d = 12"),
                       (lambda: fit(ldy=2), b"ldy = 2 is smaller than m = 3"), (lambda: fit(x=None), b"null argument"), (lambda: fit(inf=None), b"null argument"),
                       (lambda: fit(ws=odd), b"16-byte aligned"),
                       (lambda: predict(n=0), b"n >= 1 rows (got 0)"), (lambda: predict(ldo=2), b"ldo = 2 is smaller than m = 3"),
                       (lambda: predict(ldx=11), b"ldx = 11"), (lambda: predict(d=1025, ldx=1025), b"d = 1025"), (lambda: predict(m=513, ldo=513), b"m = 513"),
                       (lambda: predict(w=None), b"null argument"),
                       (lambda: score(n=1), b"n >= 2 rows (got 1)"), (lambda: score(nl=0), b"n_lambda = 0 penalties"), (lambda: score(nl=17), b"n_lambda = 17 penalties"),
                       (lambda: score(ldy=2), b"ldy = 2"), (lambda: score(ldx=11), b"ldx = 11"), (lambda: score(sse=None), b"null argument"),
                       (lambda: score(ws=odd), b"16-byte aligned"), (lambda: score(m=513, ldy=513), b"m = 513"),
                       (lambda: weights(nl=0), b"n_lambda = 0"), (lambda: weights(nl=17), b"n_lambda = 17"), (lambda: weights(d=1025), b"d = 1025"),
                       (lambda: weights(w=None), b"null argument"), (lambda: weights(lams=None), b"null argument"),
                       (lambda: weights(lams=(C.c_double * 2)(1.0, 0.0)), b"lambda[1] = 0"), (lambda: weights(lams=(C.c_double * 2)(-1.0, 1.0)), b"lambda[0] = -1"),
                       (lambda: weights(lams=(C.c_double * 2)(float("nan"), 1.0)), b"must be finite and > 0"),
                       (lambda: weights(lams=(C.c_double * 2)(1.0, float("inf"))), b"lambda[1] = inf"),
                       (lambda: weights(lams=(C.c_double * 2)(1e-50, 1.0)), b"lambda[0] = 1e-50 must be finite and > 0 as a float32"),
                       (lambda: score(d=1025, ldx=1025), b"d = 1025"), (lambda: score(d=0), b"d must be >= 1 (got 0)"), (lambda: weights(m=513), b"m = 513"),
                       (lambda: weights(m=0), b"m must be >= 1 (got 0)"), (lambda: predict(m=0), b"m must be >= 1 (got 0)")):
        assert call() == -22 and word in L.tmjx_last_error(), (word, L.tmjx_last_error())
    for args, word in (((1, 12, 3, 2), b"n >= 2"), ((8, 1025, 3, 2), b"d = 1025"), ((8, 12, 513, 2), b"m = 513"), ((8, 12, 3, 17), b"n_lambda = 17")):
        assert L.tmjx_readout_workspace(*args, C.byref(floats)) == -22 and word in L.tmjx_last_error()
    assert L.tmjx_readout_workspace(8, 12, 3, 2, None) == -22
    for args in ((8, 12, 3, 2), (300, 60, 5, 1), (513, 129, 38, 3), (4200, 257, 130, 2), (210_000, 1024, 74, 8), (1_000_000, 1024, 512, 16)):
        assert L.tmjx_readout_workspace(*args, C.byref(floats)) == 0 and floats.value == E.workspace("tmjx_readout_workspace", *args) and floats.value % 4 == 0
    print(f"workspace of 1 000 000 x 1024 -> 512 under 16 penalties: {4 * floats.value / 2 ** 20:.0f} MiB")
    assert 4 * floats.value <= 512 * 2 ** 20


def test_workspace_of_n_rows_covers_every_smaller_call():
    """tmjx_readout_workspace promises a buffer for calls of UP TO n rows, and the number of super-chunks is not monotone in n: 16 chunks of 256 rows
    are 16 super-chunks, 17 chunks are 9 of two.  The size of n rows must reach the end of the layout of every n' <= n, for the fit and for the
    score.  The layouts depend on n' through its chunk count only, so n' = 256 k and 256 k + 1 stand for all of them."""
    L, floats = hip.lib(), C.c_int64(0)
    assert hip.PCA_WIDE_MAX_SUPER == 16
    ns = (2, 255, 256, 257, 4095, 4096, 4097, 4352, 4353, 8192, 8193, 8448, 12_289, 57_600, 57_601)
    smaller = sorted({2, *(256 * k for k in range(1, 227)), *(256 * k + 1 for k in range(1, 226))})
    for d, m, nl in ((1, 512, 1), (4, 512, 1), (25, 512, 16), (128, 74, 8), (129, 38, 3), (1024, 74, 8), (1024, 512, 16)):
        ends = [(n2, max(E.readout_extents(n2, d, m, nl))) for n2 in smaller]
        for n in ns:
            have = E.workspace("tmjx_readout_workspace", n, d, m, nl)
            assert L.tmjx_readout_workspace(n, d, m, nl, C.byref(floats)) == 0 and floats.value == have
            worst = max((e, n2) for n2, e in ends if n2 <= n)
            assert have >= worst[0], f"workspace({n}, {d}, {m}, {nl}) = {have} floats, a call of {worst[1]} rows reaches {worst[0]}"
    fit_end, score_end = E.readout_extents(4096, 1, 512, 1)      # the case that showed it: 17 chunks sized, 16 scored
    assert E.workspace("tmjx_readout_workspace", 4352, 1, 512, 1) >= score_end > E.readout_extents(4352, 1, 512, 1)[0] and fit_end <= score_end


@pytest.mark.parametrize("d", (1, 4, 130))
def test_calls_of_fewer_rows_stay_inside_a_workspace_of_more(d):
    """A fit and a score of 4096 rows (16 super-chunks) in a buffer of exactly tmjx_readout_workspace(4352 rows: 9 super-chunks) floats: the guard
    behind it comes back untouched and the results have the bits of the calls in buffers of their own."""
    m, rng = 512 if d < 130 else 40, np.random.default_rng(5)
    x = PR.make_data(4096, d, 3.0, 4)
    y = (x[:, :1] * rng.standard_normal(m) + rng.standard_normal((4096, m))).astype(np.float32)
    own = B.readout_fit(x, y)
    got = E.over("tmjx_readout_fit", ws_rows=4352).readout_fit(x, y)
    for u, v in zip(got[:5], own[:5]):
        np.testing.assert_array_equal(bits(u), bits(v))
    mean_x, comp, var, mean_y, z, _ = own
    w = B.readout_weights(comp, var, z, [float(var.sum()) / d])
    sse, sst = B.readout_score(x, y, mean_x, w, mean_y)
    sse2, sst2 = E.over("tmjx_readout_score", ws_rows=4352).readout_score(x, y, mean_x, w, mean_y)
    np.testing.assert_array_equal(bits(sse2), bits(sse))
    np.testing.assert_array_equal(bits(sst2), bits(sst))
    if d < 130:      # the guard does see a buffer that is too small (at d = 130 the fit's part is the larger one even for 256 rows)
        with pytest.raises(AssertionError, match="wrote behind its workspace"):
            E.over("tmjx_readout_score", ws_rows=256).readout_score(x, y, mean_x, w, mean_y)


def test_abi_declares_the_readout_entry_points():
    names = ("tmjx_readout_workspace", "tmjx_readout_fit", "tmjx_readout_weights", "tmjx_readout_predict", "tmjx_readout_score")
    assert set(names) <= set(hip.EXPORTS) and any(p.name == "tmjx_readout.hip" for p in hip.SOURCES)
    header = (ROOT / "include" / "tmjx.h").read_text()
    core = (ROOT / "track_mjx_amd" / "csrc" / "readout_core.h").read_text()
    for text in names + (f"#define READOUT_MAX_M {hip.READOUT_MAX_M}", f"#define READOUT_MAX_L {hip.READOUT_MAX_L}"):
        assert text in header
    assert f"#define READOUT_MAX_M {hip.READOUT_MAX_M}" in core and f"#define READOUT_MAX_L {hip.READOUT_MAX_L}" in core
    from track_mjx_amd.analysis import pca as P
    for name in ("readout_fit", "readout_weights", "readout_predict", "readout_score"):
        assert callable(getattr(P.HipBackend, name))


def test_emulation_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """The emulation's own main, built with AddressSanitizer and UBSan (a host program: no preload, no Python), runs clean on a strided 300 x 140 -> 70
    problem with a ragged score block."""
    exe = E.build_main("readout", tmp_path / "readout_emu", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "checksum" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr
    assert "300 x 140 -> 70" in out.stdout


# ------------------------------------------------------------------------------------------------------------------ Python and the tool
def test_ridge_class():
    case = R.CPU_CASES[0]
    xtr, ytr, xte, yte = R.case_data(case)
    f64 = R.fit(xtr, ytr, (0.01, 1.0, 100.0))
    r = RO.Ridge((0.01, 1.0, 100.0), backend=B).fit(strided(xtr, 2, 3), ytr)
    d, m = case[2], case[3]
    assert r.coef_.shape == (3, d, m) and r.intercept_.shape == (3, m) and r.components_.shape == (d, d) and r.n_samples_ == 300
    np.testing.assert_allclose(r.lambdas_, f64["lambdas"], rtol=1e-5)
    np.testing.assert_allclose(r.explained_variance_, f64["variance"], rtol=1e-4, atol=1e-6)
    mid = r.predict(xte)                                              # before a score: the middle penalty
    np.testing.assert_array_equal(mid, r.predict(xte, 1))
    np.testing.assert_allclose(mid, xte.astype(np.float64) @ r.coef_[1] + r.intercept_[1], rtol=0, atol=2e-4)
    r2 = r.score(xte, yte)
    assert r2.shape == (3, m) and r2.dtype == np.float64 and r.best_index_ == int(np.argmax(r2.mean(1)))
    np.testing.assert_array_equal(r.predict(xte), r.predict(xte, r.best_index_))
    p64 = R.predict(xte, f64["mean_x"], f64["W"][0], f64["mean_y"])
    assert np.abs(r2[0] - R.r2(yte, p64)).max() < 1e-4
    with pytest.raises(ValueError, match="expected 60 features, got 59"):
        r.predict(xte[:, :59])
    with pytest.raises(ValueError, match="index = 3 of 3 penalties"):
        r.predict(xte, 3)
    with pytest.raises(ValueError, match="not fitted"):
        RO.Ridge(backend=B).predict(xte)
    for bad in ((0.0,), (1.0, -1.0), (float("nan"),), (float("inf"),)):
        with pytest.raises(ValueError, match="every alpha must be finite and > 0"):
            RO.Ridge(bad, backend=B)
    with pytest.raises(ValueError, match="17 penalties given"):
        RO.Ridge(np.ones(17), backend=B)
    with pytest.raises(ValueError, match="zero total variance"):
        RO.Ridge(backend=B).fit(np.tile(xtr[:1], (10, 1)), ytr[:10])
    with pytest.raises(ValueError, match="x has 300 rows, y has 299"):
        RO.Ridge(backend=B).fit(xtr, ytr[:299])
    one = RO.Ridge((0.01, 1.0, 100.0), backend=B).fit(xtr, ytr[:, 2])      # a single target series [n] is a [n, 1] target
    assert one.coef_.shape == (3, d, 1) and one.n_targets_ == 1
    col = RO.Ridge((0.01, 1.0, 100.0), backend=B).fit(xtr, ytr[:, 2:3])
    np.testing.assert_array_equal(bits(one.coef_), bits(col.coef_))
    np.testing.assert_array_equal(bits(one.score(xte, yte[:, 2])), bits(col.score(xte, yte[:, 2:3])))


NBODY = 4


def rollouts(n_clips=6, T=41, seed=7, permute=False, nbody=NBODY):
    """Synthetic roll-out dicts with an exact linear map planted from activations/intention (16 wide, spectrum 0.9^j) to every target."""
    rng = np.random.default_rng(seed)
    a_ctrl, a_q, a_f = (rng.standard_normal((16, k)) for k in (5, 9, 6 * nbody))
    out = []
    for c in range(n_clips):
        lat = PR.make_data(T - 1, 16, 0.5, seed + c, decay=0.9)
        frames = np.concatenate([lat, PR.make_data(1, 16, 0.5, seed + 100 + c, decay=0.9)])      # a per-frame series has one row more
        perm = rng.permutation(T - 1) if permute else np.arange(T - 1)
        out.append({"ctrl": (lat @ a_ctrl + 1.0)[perm].astype(np.float32), "qposes_rollout": (frames @ a_q - 2.0).astype(np.float32),
                    "joint_forces": (lat @ a_f).reshape(T - 1, nbody, 6).astype(np.float32), "state_rewards": (frames @ a_q[:, 0]).astype(np.float32),
                    "rollout_metrics": {"pos_distances": (frames @ a_q[:, 1]).astype(np.float32)},
                    "activations": {"intention": lat, "decoder": {"layer_0": np.tanh(lat @ a_ctrl).astype(np.float32)}}})
    return out


def test_fit_rollouts_reads_out_a_planted_map():
    rolls = rollouts()
    r = RO.fit_rollouts(rolls, "intention", "ctrl", alphas=(1e-4,), holdout=3, backend=B)
    assert r.train_clips_ == [0, 1, 3, 4] and r.test_clips_ == [2, 5]             # exactly the positions 2 and 5 are held out
    assert r.n_samples_ == 4 * 40 and r.r2_.shape == (1, 5) and r.best_index_ == 0
    lat = lambda clips: np.concatenate([rolls[c]["activations"]["intention"] for c in clips])      # noqa: E731
    ctrl = lambda clips: np.concatenate([rolls[c]["ctrl"] for c in clips])                          # noqa: E731
    xtr, ytr, xte, yte = lat(r.train_clips_), ctrl(r.train_clips_), lat(r.test_clips_), ctrl(r.test_clips_)
    f64 = R.fit(xtr, ytr, (1e-4,))
    r64 = R.r2(yte, R.predict(xte, f64["mean_x"], f64["W"][0], f64["mean_y"]))
    print("held-out R2:", r.r2_[0], "float64:", r64)
    assert (r64 >= 0.999).all()                                                   # the precondition: the reference reads the map out
    assert (r.r2_[0] >= 0.999).all()
    shuffled = RO.fit_rollouts(rollouts(permute=True), "intention", "ctrl", alphas=(1e-4,), holdout=3, backend=B)
    print("rows permuted across time: mean R2", shuffled.r2_.mean())
    assert shuffled.r2_.mean() < 0.1


def test_fit_rollouts_targets_rows_and_columns():
    rolls = rollouts()
    kw = dict(alphas=(1e-4,), holdout=3, backend=B)
    q = RO.fit_rollouts(rolls, "intention", "qposes_rollout", target_cols="2:", **kw)        # T rows against T - 1: target[t], nothing dropped
    assert q.n_targets_ == 7 and q.n_samples_ == 4 * 40 and (q.r2_ >= 0.999).all()
    q1 = RO.fit_rollouts(rolls, "intention", "qposes_rollout", lag=1, **kw)                    # target[t + 1]: another frame's, still a partner for every row
    assert q1.n_samples_ == 4 * 40 and q1.r2_.mean() < 0.5
    lagged = RO.fit_rollouts(rolls, "intention", "ctrl", lag=1, **kw)                          # T - 1 rows: lag 1 drops one row per clip
    assert lagged.n_samples_ == 4 * 39 and [f.shape[0] for f in lagged.test_features_] == [39, 39]
    jf = RO.fit_rollouts(rolls, "intention", "joint_forces", **kw)
    assert jf.n_targets_ == 6 * NBODY and (jf.r2_ >= 0.999).all()                              # [T - 1, nbody, 6] flattened
    assert RO.fit_rollouts(rolls, "intention", "state_rewards", **kw).n_targets_ == 1
    assert (RO.fit_rollouts(rolls, "intention", "rollout_metrics/pos_distances", **kw).r2_ >= 0.999).all()
    layer = RO.fit_rollouts(rolls, "intention", "activations/decoder/layer_0", **kw)
    assert layer.n_targets_ == 5 and 0.3 < layer.r2_.mean() < 1.0                              # a tanh of the map: linear only in part
    with pytest.raises(ValueError, match="joint_forces is 516 wide: a readout takes up to 512 targets, pick columns with target_cols=a:b"):
        RO.fit_rollouts(rollouts(T=6, nbody=86), "intention", "joint_forces", **kw)
    assert RO.fit_rollouts(rollouts(T=6, nbody=86), "intention", "joint_forces", target_cols="0:12", alphas=(1.0,), holdout=3, backend=B).n_targets_ == 12
    with pytest.raises(ValueError, match="at least two clips"):
        RO.fit_rollouts(rolls[:1], "intention", "ctrl", **kw)
    with pytest.raises(ValueError, match="leaves no test clip"):
        RO.fit_rollouts(rolls[:2], "intention", "ctrl", **kw)
    with pytest.raises(ValueError, match="lag must be 0 or 1"):
        RO.fit_rollouts(rolls, "intention", "ctrl", lag=2, **kw)
    with pytest.raises(ValueError, match="target_cols = 9: selects no column of 5"):
        RO.fit_rollouts(rolls, "intention", "ctrl", target_cols="9:", **kw)
    with pytest.raises(KeyError, match="unknown target 'torques'"):
        RO.fit_rollouts(rolls, "intention", "torques", **kw)
    with pytest.raises(KeyError, match="has no sensor_readings"):
        RO.fit_rollouts(rolls, "intention", "sensor_readings", **kw)


def test_tool_round_trips_through_h5lite(tmp_path, capsys):
    from track_mjx_amd import h5lite
    rolls = rollouts()
    (tmp_path / "in").mkdir()
    ids = (0, 2, 3, 7, 11, 12)
    for c, r in zip(ids, rolls):
        h5lite.write_tree(tmp_path / "in" / f"clip_{c}.h5", r)
    out = tmp_path / "fit" / "readout.h5"
    args = [f"rollouts={tmp_path / 'in'}", "feature=intention", "target=qposes_rollout", "target_cols=2:", "alphas=1e-4,1e-2,1", "holdout=3", f"out={out}"]
    assert RO.main(args, backend=B) == 0
    line = capsys.readouterr().out
    assert "intention -> qposes_rollout: 160 samples x 16 features -> 7 targets, 4 training and 2 held-out clips" in line and "best alpha 0.0001" in line
    want = RO.fit_rollouts(tmp_path / "in", "intention", "qposes_rollout", (1e-4, 1e-2, 1.0), 3, target_cols="2:", backend=B)
    with h5lite.File(out) as h:
        np.testing.assert_array_equal(h["alphas"][()], [1e-4, 1e-2, 1.0])
        np.testing.assert_array_equal(h["lambdas"][()], want.lambdas_)
        np.testing.assert_array_equal(h["r2"][()], want.r2_)
        np.testing.assert_array_equal(h["r2_mean"][()], want.r2_.mean(1))
        assert int(h["best_index"][()]) == 0 and h["r2"][()].shape == (3, 7)
        np.testing.assert_array_equal(h["coef"][()], want.coef_[0])
        np.testing.assert_array_equal(h["intercept"][()], want.intercept_[0])
        np.testing.assert_array_equal(h["mean_x"][()], want.mean_)
        np.testing.assert_array_equal(h["mean_y"][()], want.mean_y_)
        assert bytes(h["feature"][()]).decode() == "intention" and bytes(h["target"][()]).decode() == "qposes_rollout"
        np.testing.assert_array_equal(h["train_clips"][()], [0, 2, 7, 11])
        np.testing.assert_array_equal(h["test_clips"][()], [3, 12])
        pred = h["predictions/clip_12"][()]
        assert pred.shape == (40, 7) and h["predictions/clip_3"][()].shape == (40, 7)
        np.testing.assert_array_equal(pred, want.predict(want.test_features_[1]))
        assert np.abs(pred - rolls[5]["qposes_rollout"][:40, 2:]).max() < 1e-2
    assert RO.main([f"rollouts={tmp_path / 'in'}", "feature=decoder/layer_9", "target=ctrl", f"out={out}"], backend=B) == 2
    assert "has no activations/decoder/layer_9" in capsys.readouterr().err
    assert RO.main([f"rollouts={tmp_path / 'in'}", "feature=intention", "target=sensor_readings", f"out={out}"], backend=B) == 2
    assert "has no sensor_readings" in capsys.readouterr().err
    assert RO.main([f"rollouts={tmp_path / 'in'}", "feature=intention", f"out={out}"], backend=B) == 2
    assert "usage:" in capsys.readouterr().err
