"""The readout kernels (csrc/tmjx_readout.hip) against the float64 reference (tests/readout_ref.py) at the five cases of DESIGN.md "Readout": the
weights under kappa_lambda max(d, 8) 2^-23, the held-out predictions and R^2 under 30 x the float32 numpy twin's error; the bit-level properties
(the PCA part's bits, repeatability, row strides, ldo, predict against the score, one penalty against its row), the refusals, `Ridge` on device
tensors and the command-line tool.  The measured values are in DESIGN.md "Readout"."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import pca_ref as PR
from tests import readout_ref as R
from track_mjx_amd import hip
from track_mjx_amd.analysis import pca as P
from track_mjx_amd.analysis import readout as RO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MID = R.GPU_CASES[1]


def backend():
    return P.HipBackend(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(None)
def run(case):
    return R.run_case(case, backend())


@pytest.mark.parametrize("case", R.GPU_CASES)
def test_against_float64(case):
    (mean_x, comp, var, mean_y, z), w, preds, r2, _ = run(case)
    R.check_case(case, w, preds, r2, "kernel")
    b = backend()
    x = b.asarray(R.case_data(case)[0])
    for u, v in zip((mean_x, comp, var), b.fit_wide(x)[:3]):            # the PCA part: tmjx_pca_fit_wide's bits
        np.testing.assert_array_equal(bits(u), bits(v))
    if case[2] <= hip.PCA_MAX_D:                                       # and, up to 128 features, tmjx_pca_fit's
        for u, v in zip((mean_x, comp, var), b.fit(x)[:3]):
            np.testing.assert_array_equal(bits(u), bits(v))


def test_two_calls_give_the_same_bits():
    b = backend()
    xtr, ytr, xte, yte = (b.asarray(a) for a in R.case_data(MID))
    (mean_x, comp, var, mean_y, z), w, _, _, (sse, sst) = run(MID)
    np.testing.assert_array_equal(bits(b.readout_fit(xtr, ytr)[4]), bits(z))
    np.testing.assert_array_equal(bits(b.readout_weights(comp, var, z, R.lambdas_of(var, R.CASES[MID]))), bits(w))
    sse2, sst2 = b.readout_score(xte, yte, mean_x, w, mean_y)
    np.testing.assert_array_equal(bits(sse2), bits(sse))
    np.testing.assert_array_equal(bits(sst2), bits(sst))


def strided(a, pad_left, pad_right):
    buf = torch.full((a.shape[0], a.shape[1] + pad_left + pad_right), 1e6, dtype=torch.float32, device=DEV)
    buf[:, pad_left:pad_left + a.shape[1]] = torch.from_numpy(np.array(a))
    return buf[:, pad_left:pad_left + a.shape[1]]


def test_row_strides_give_the_dense_bits_and_ldo_is_respected():
    b, L = backend(), hip.lib()
    xtr, ytr, xte, yte = R.case_data(MID)
    (mean_x, comp, var, mean_y, z), w, preds, _, (sse, sst) = run(MID)
    xs, ys, xts, yts = strided(xtr, 3, 2), strided(ytr, 1, 6), strided(xte, 4, 1), strided(yte, 2, 2)
    assert b.asarray(xs).data_ptr() == xs.data_ptr() and xs.stride(0) == MID[2] + 5      # no copy
    got = b.readout_fit(xs, ys)
    for u, v in zip(got[:5], (mean_x, comp, var, mean_y, z)):
        np.testing.assert_array_equal(bits(u), bits(v))
    sse2, sst2 = b.readout_score(xts, yts, mean_x, w, mean_y)
    np.testing.assert_array_equal(bits(sse2), bits(sse))
    np.testing.assert_array_equal(bits(sst2), bits(sst))
    n, d, m = xte.shape[0], MID[2], MID[3]
    out = torch.full((n, m + 3), -5.0, dtype=torch.float32, device=DEV)
    mx, w1, my = (torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (mean_x, w[1], mean_y))
    hip.check(L.tmjx_readout_predict(xts.data_ptr(), n, d, xts.stride(0), mx.data_ptr(), w1.data_ptr(), my.data_ptr(), m, out.data_ptr(), m + 3, None),
              "tmjx_readout_predict")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(out[:, :m].cpu().numpy()), bits(preds[1]))
    assert (out[:, m:] == -5.0).all()


def test_predict_reproduces_the_score_and_one_penalty_equals_its_row():
    b = backend()
    xte, yte = R.case_data(MID)[2:]
    (mean_x, comp, var, mean_y, z), w, preds, _, (sse, sst) = run(MID)
    xt, yt = b.asarray(xte), b.asarray(yte)
    for i in range(w.shape[0]):
        host_sse, host_sst = R.sse_sst(yte, preds[i])
        assert (np.abs(sse[i] - host_sse) <= R.FLOOR * host_sse).all(), np.abs(sse[i] / host_sse - 1).max()
        assert (np.abs(sst - host_sst) <= R.FLOOR * host_sst).all()
        one = b.readout_score(xt, yt, mean_x, w[i:i + 1], mean_y)
        np.testing.assert_array_equal(bits(one[0][0]), bits(sse[i]))
        np.testing.assert_array_equal(bits(one[1]), bits(sst))


def test_calls_of_fewer_rows_stay_inside_a_workspace_of_more():
    """tmjx_readout_workspace covers calls of UP TO n rows: a fit and a score of 4096 rows (16 super-chunks) in a buffer of exactly the size of 4352
    rows (9 super-chunks of two chunks) leave the guard behind it untouched and give the bits of calls in buffers of their own."""
    L, b, rng = hip.lib(), backend(), np.random.default_rng(5)
    n, d, m, guard = 4096, 4, 512, 1 << 16
    xh = PR.make_data(n, d, 3.0, 4)
    yh = (xh[:, :1] * rng.standard_normal(m) + rng.standard_normal((n, m))).astype(np.float32)
    x, y = b.asarray(xh), b.asarray(yh)
    mean_x, comp, var, mean_y, z, _ = b.readout_fit(x, y)
    w = b.readout_weights(comp, var, z, [float(var.sum()) / d])
    sse, sst = b.readout_score(x, y, mean_x, w, mean_y)
    floats, info = C.c_int64(0), hip.PcaInfo()
    hip.check(L.tmjx_readout_workspace(4352, d, m, 1, C.byref(floats)), "tmjx_readout_workspace")
    size = int(floats.value)
    ws = torch.full((size + guard,), -7.25, dtype=torch.float32, device=DEV)
    o = [torch.empty(s, dtype=torch.float32, device=DEV) for s in ((d,), (d, d), (d,), (m,), (d, m))]
    hip.check(L.tmjx_readout_fit(x.data_ptr(), n, d, x.stride(0), y.data_ptr(), m, y.stride(0), *(t.data_ptr() for t in o), ws.data_ptr(), C.byref(info), None),
              "tmjx_readout_fit")
    assert (ws[size:] == -7.25).all()
    for u, v in zip(o, (mean_x, comp, var, mean_y, z)):
        np.testing.assert_array_equal(bits(u.cpu().numpy()), bits(v))
    wd = torch.as_tensor(np.ascontiguousarray(w), device=DEV)
    out = torch.empty(m + m, dtype=torch.float64, device=DEV)
    hip.check(L.tmjx_readout_score(x.data_ptr(), n, d, x.stride(0), y.data_ptr(), m, y.stride(0), o[0].data_ptr(), wd.data_ptr(), o[3].data_ptr(), 1,
                                   out.data_ptr(), out.data_ptr() + 8 * m, ws.data_ptr(), None), "tmjx_readout_score")
    torch.cuda.synchronize()
    assert (ws[size:] == -7.25).all()
    np.testing.assert_array_equal(bits(out[:m].cpu().numpy()), bits(sse[0]))
    np.testing.assert_array_equal(bits(out[m:].cpu().numpy()), bits(sst))


def test_refusals_launch_nothing():
    L, b = hip.lib(), backend()
    x, y = b.asarray(PR.make_data(8, 12)), b.asarray(PR.make_data(8, 3, seed=1))
    floats, info = C.c_int64(0), hip.PcaInfo()
    hip.check(L.tmjx_readout_workspace(8, 12, 3, 2, C.byref(floats)), "tmjx_readout_workspace")
    ws = torch.full((int(floats.value),), 3.0, device=DEV)
    outs = [torch.full((12 * 12,), 7.0, device=DEV) for _ in range(5)]
    sse = torch.full((2 * 3 + 3,), 7.0, dtype=torch.float64, device=DEV)
    o, lam = [t.data_ptr() for t in outs], (C.c_double * 17)(*([1.0] * 17))

    def fit(n=8, d=12, ldx=12, m=3, ldy=3, xp=x.data_ptr(), wsp=ws.data_ptr(), inf=C.byref(info)):
        return L.tmjx_readout_fit(xp, n, d, ldx, y.data_ptr(), m, ldy, *o, wsp, inf, None)

    def predict(n=8, d=12, ldx=12, m=3, ldo=3, w=o[1]):
        return L.tmjx_readout_predict(x.data_ptr(), n, d, ldx, o[0], w, o[3], m, o[4], ldo, None)

    def score(n=8, d=12, ldx=12, m=3, ldy=3, nl=2, ssep=sse.data_ptr(), wsp=ws.data_ptr()):
        return L.tmjx_readout_score(x.data_ptr(), n, d, ldx, y.data_ptr(), m, ldy, o[0], o[1], o[3], nl, ssep, sse.data_ptr() + 48, wsp, None)

    def weights(d=12, m=3, nl=2, lams=lam, w=o[1]):
        return L.tmjx_readout_weights(o[1], o[2], o[4], d, m, lams, nl, w, None)

    for call, word in ((lambda: fit(d=0), b"d must be >= 1 (got 0)"), (lambda: fit(d=1025, ldx=1025), b"d = 1025 exceeds the readout limit of 1024"),
                       (lambda: fit(m=0), b"m must be >= 1 (got 0)"), (lambda: fit(m=513, ldy=513), b"m = 513 exceeds the readout limit of 512"),
                       (lambda: fit(n=1), b"n >= 2 rows (got 1)"), (lambda: fit(ldx=11), b"ldx = 11 is smaller than d = 12"),
                       (lambda: fit(ldy=2), b"ldy = 2 is smaller than m = 3"), (lambda: fit(xp=None), b"null argument"), (lambda: fit(inf=None), b"null argument"),
                       (lambda: fit(wsp=ws.data_ptr() + 4), b"16-byte aligned"),
                       (lambda: predict(n=0), b"n >= 1 rows (got 0)"), (lambda: predict(ldo=2), b"ldo = 2 is smaller than m = 3"),
                       (lambda: predict(ldx=11), b"ldx = 11"), (lambda: predict(d=1025, ldx=1025), b"d = 1025"), (lambda: predict(m=513, ldo=513), b"m = 513"),
                       (lambda: predict(w=None), b"null argument"),
                       (lambda: score(n=1), b"n >= 2 rows (got 1)"), (lambda: score(nl=0), b"n_lambda = 0 penalties"), (lambda: score(nl=17), b"n_lambda = 17 penalties"),
                       (lambda: score(ldy=2), b"ldy = 2"), (lambda: score(ldx=11), b"ldx = 11"), (lambda: score(ssep=None), b"null argument"),
                       (lambda: score(wsp=ws.data_ptr() + 4), b"16-byte aligned"),
                       (lambda: weights(nl=0), b"n_lambda = 0"), (lambda: weights(nl=17), b"n_lambda = 17"), (lambda: weights(d=1025), b"d = 1025"),
                       (lambda: weights(m=513), b"m = 513"), (lambda: weights(w=None), b"null argument"), (lambda: weights(lams=None), b"null argument"),
                       (lambda: weights(lams=(C.c_double * 2)(1.0, 0.0)), b"lambda[1] = 0"), (lambda: weights(lams=(C.c_double * 2)(-1.0, 1.0)), b"lambda[0] = -1"),
                       (lambda: weights(lams=(C.c_double * 2)(float("nan"), 1.0)), b"must be finite and > 0"),
                       (lambda: weights(lams=(C.c_double * 2)(1.0, float("inf"))), b"lambda[1] = inf")):
        assert call() == -22 and word in L.tmjx_last_error(), (word, L.tmjx_last_error())
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in outs) and (sse == 7.0).all() and (ws == 3.0).all()      # nothing was written
    bad = PR.make_data(40, 130).copy()
    bad[3, 77] = np.nan
    with pytest.raises(hip.TmjxError, match="tmjx_pca_fit_wide: the covariance is non-finite"):      # the PCA part's refusal passes through
        b.readout_fit(b.asarray(bad), b.asarray(PR.make_data(40, 3, seed=1)))
    with pytest.raises(ValueError, match="zero total variance"):
        RO.Ridge(device=DEV).fit(np.tile(PR.make_data(1, 12), (10, 1)), PR.make_data(10, 3, seed=1))


def test_ridge_on_device_tensors():
    case = R.GPU_CASES[0]
    xtr, ytr, xte, yte = R.case_data(case)
    alphas = (0.01, 1.0, 100.0)
    f64 = R.fit(xtr, ytr, alphas)
    buf = torch.full((300, 70), 1e6, dtype=torch.float32, device=DEV)
    buf[:, 4:64] = torch.from_numpy(xtr.copy())
    r = RO.Ridge(alphas, device=DEV).fit(buf[:, 4:64], torch.from_numpy(ytr.copy()).to(DEV))      # a strided view, kept as it is
    assert r.coef_.shape == (3, 60, 5) and r.intercept_.shape == (3, 5) and r.components_.shape == (60, 60) and r.n_samples_ == 300
    np.testing.assert_allclose(r.lambdas_, f64["lambdas"], rtol=1e-5)
    np.testing.assert_allclose(r.explained_variance_, f64["variance"], rtol=1e-4, atol=1e-6)
    xt = torch.from_numpy(xte.copy()).to(DEV)
    mid = r.predict(xt)
    assert isinstance(mid, torch.Tensor) and mid.shape == (70, 5)
    np.testing.assert_array_equal(mid.cpu().numpy(), r.predict(xte, 1))                          # numpy in, numpy out; the middle penalty before a score
    r2 = r.score(xt, torch.from_numpy(yte.copy()).to(DEV))
    assert r2.shape == (3, 5) and r.best_index_ == int(np.argmax(r2.mean(1)))
    for i in range(3):
        assert np.abs(r2[i] - R.r2(yte, R.predict(xte, f64["mean_x"], f64["W"][i], f64["mean_y"]))).max() < 1e-4
    np.testing.assert_array_equal(r.predict(xt).cpu().numpy(), r.predict(xte, r.best_index_))


def test_tool_on_synthetic_clips(tmp_path, capsys):
    from track_mjx_amd import h5lite
    rng = np.random.default_rng(7)
    a = rng.standard_normal((16, 9))
    (tmp_path / "in").mkdir()
    clips = {}
    for c in (0, 1, 4, 5, 8, 9):
        lat = PR.make_data(40, 16, 0.5, 7 + c, decay=0.9)
        frames = np.concatenate([lat, PR.make_data(1, 16, 0.5, 107 + c, decay=0.9)])
        clips[c] = {"qposes_rollout": (frames @ a - 2.0).astype(np.float32), "activations": {"intention": lat}}
        h5lite.write_tree(tmp_path / "in" / f"clip_{c}.h5", clips[c])
    out = tmp_path / "readout.h5"
    assert RO.main([f"rollouts={tmp_path / 'in'}", "feature=intention", "target=qposes_rollout", "target_cols=2:", "alphas=1e-4,1", "holdout=3", f"out={out}"]) == 0
    assert "160 samples x 16 features -> 7 targets, 4 training and 2 held-out clips" in capsys.readouterr().out
    want = RO.fit_rollouts(tmp_path / "in", "intention", "qposes_rollout", (1e-4, 1.0), 3, target_cols="2:", device=DEV)
    with h5lite.File(out) as h:
        np.testing.assert_array_equal(h["r2"][()], want.r2_)
        np.testing.assert_array_equal(h["coef"][()], want.coef_[0])
        np.testing.assert_array_equal(h["test_clips"][()], [4, 9])
        assert int(h["best_index"][()]) == 0 and (h["r2"][()][0] >= 0.999).all()
        pred = h["predictions/clip_9"][()]
        assert pred.shape == (40, 7) and np.abs(pred - clips[9]["qposes_rollout"][:40, 2:]).max() < 1e-2
    assert RO.main([f"rollouts={tmp_path / 'in'}", "feature=intention", "target=ctrl", f"out={out}"]) == 2
    assert "has no ctrl" in capsys.readouterr().err
