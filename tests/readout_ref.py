"""Float64 numpy restatement of the linear readout, written from DESIGN.md "Readout" (not from the kernels), with the data generator, the cases and
the acceptance checks the CPU and GPU tests share.  The same code in float32 is the baseline the tests print and scale two bounds by."""
from __future__ import annotations

import functools

import numpy as np

from tests import pca_ref as P

EPS = P.EPS
FLOOR = 16 * EPS
# (n_train, n_test, d, m, offset, seed) -> alphas
CASES = {(300, 70, 60, 5, 3.0, 0): (0.01,),                                   # the narrow path, L m below one tile
         (513, 129, 129, 38, 3.0, 0): (0.01, 0.1, 1.0),                        # the first wide d, three chunks with a ragged last one, a ragged test block
         (130, 64, 192, 74, 3.0, 0): (0.03, 0.1, 1.0, 10.0),                   # n < d: a rank-deficient covariance; L m = 296 crosses tiles
         (4200, 1000, 257, 130, 100.0, 0): (0.1, 1.0),                         # super-chunks of two; m crosses 128; the offset a one-pass moment fails
         (2100, 500, 1024, 17, 3.0, 0): (1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0)}      # the size limit, L = 8 (GPU only)
CPU_CASES = tuple(CASES)[:4]
GPU_CASES = tuple(CASES)


# ------------------------------------------------------------------------------------------------------------------ data
def make_xy(n_train, n_test, d, m, offset, seed):
    """x float32 [n, d] (pca_ref.make_data) and y float32 [n, m] = x_c W0 + noise of half the signal's spread + a per-target offset, n = n_train + n_test."""
    n = n_train + n_test
    x = P.make_data(n, d, offset, seed)
    rng = np.random.default_rng(seed + 1000)
    w0 = rng.standard_normal((d, m)) / np.sqrt(np.arange(1, d + 1))[:, None]
    xc = x.astype(np.float64) - x.astype(np.float64).mean(0)
    sig = xc @ w0
    y = sig + 0.5 * sig.std(0) * rng.standard_normal((n, m)) + 10.0 * rng.standard_normal(m)
    return x, y.astype(np.float32)


@functools.lru_cache(None)
def case_data(case):
    x, y = make_xy(*case)
    for a in (x, y):
        a.setflags(write=False)
    nt = case[0]
    return x[:nt], y[:nt], x[nt:], y[nt:]


# ------------------------------------------------------------------------------------------------------------------ the maths
def fit(x, y, alphas, dtype=np.float64):
    """-> dict: mean_x, mean_y, components [d, d] (rows), variance [d] (clamped at 0, descending), C [d, m], Z [d, m], lambdas [L], W [L, d, m]."""
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    n, d = x.shape
    mean_x, mean_y = x.mean(0, dtype=dtype), y.mean(0, dtype=dtype)
    xc, yc = x - mean_x, y - mean_y
    cov, c = (xc.T @ xc) / dtype(n - 1), (xc.T @ yc) / dtype(n - 1)
    lam, vec = np.linalg.eigh(cov)
    order = np.argsort(-lam, kind="stable")
    s, v = np.maximum(lam[order], 0), vec.T[order]
    z = v @ c
    lambdas = np.asarray(alphas, np.float64) * float(s.astype(np.float64).sum()) / d
    w = np.stack([v.T @ (z / (s + dtype(l))[:, None]) for l in lambdas])
    return {"mean_x": mean_x, "mean_y": mean_y, "components": v, "variance": s, "C": c, "Z": z, "lambdas": lambdas, "W": w}


def predict(x, mean_x, w, mean_y, dtype=np.float64):
    return (np.asarray(x).astype(dtype) - np.asarray(mean_x).astype(dtype)) @ np.asarray(w).astype(dtype) + np.asarray(mean_y).astype(dtype)


def sse_sst(y, yhat):
    """sse [m] of one prediction, sst [m] about the float64 column mean of y; both float64."""
    y64 = np.asarray(y, np.float64)
    return ((y64 - np.asarray(yhat, np.float64)) ** 2).sum(0), ((y64 - y64.mean(0)) ** 2).sum(0)


def r2(y, yhat):
    sse, sst = sse_sst(y, yhat)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sst > 0, 1.0 - sse / sst, np.nan)


def lambdas_of(variance, alphas):
    v = np.asarray(variance, np.float64)
    return np.asarray(alphas, np.float64) * v.sum() / v.shape[0]


def kappa(variance64, lam):
    return float((variance64.max() + lam) / (variance64.min() + lam))


def pred_error(yhat, yhat64):
    """The largest per-column ||yhat - yhat64|| / ||yhat64 - mean(yhat64)|| over the rows."""
    a, b = np.asarray(yhat, np.float64), np.asarray(yhat64, np.float64)
    return float((np.linalg.norm(a - b, axis=0) / np.linalg.norm(b - b.mean(0), axis=0)).max())


@functools.lru_cache(None)
def case_reference(case):
    """The float64 fit, its held-out predictions [L, nt, m] and R^2 [L, m], kappa per penalty, and the float32 numpy twin's three errors per penalty."""
    xtr, ytr, xte, yte = case_data(case)
    alphas = CASES[case]
    f64, f32 = fit(xtr, ytr, alphas), fit(xtr, ytr, alphas, np.float32)
    L = len(alphas)
    p64 = np.stack([predict(xte, f64["mean_x"], f64["W"][i], f64["mean_y"]) for i in range(L)])
    p32 = np.stack([predict(xte, f32["mean_x"], f32["W"][i], f32["mean_y"], np.float32) for i in range(L)])
    r64, r32 = np.stack([r2(yte, p) for p in p64]), np.stack([r2(yte, p) for p in p32])
    base = [{"w": float(np.linalg.norm(f32["W"][i] - f64["W"][i]) / np.linalg.norm(f64["W"][i])), "pred": pred_error(p32[i], p64[i]),
             "r2": float(np.abs(r32[i] - r64[i]).max())} for i in range(L)]
    kap = [kappa(f64["variance"], l) for l in f64["lambdas"]]
    return f64, p64, r64, kap, base


def check_case(case, w, preds, r2_got, what=""):
    """The acceptance of DESIGN.md "Readout" for one case: w [L, d, m], preds [L, n_test, m] and r2_got [L, m] of the code under test.  Every value is
    printed beside the float32 numpy twin's before anything is asserted.  -> the measured values per penalty."""
    f64, p64, r64, kap, base = case_reference(case)
    d, b = case[2], P.bound(case[2])
    got = []
    for i, alpha in enumerate(CASES[case]):
        g = {"w": float(np.linalg.norm(np.asarray(w[i], np.float64) - f64["W"][i]) / np.linalg.norm(f64["W"][i])), "pred": pred_error(preds[i], p64[i]),
             "r2": float(np.abs(np.asarray(r2_got[i], np.float64) - r64[i]).max())}
        got.append(g)
        print(f"{what} {case} alpha {alpha:g}: kappa b {kap[i] * b:.2e}; " + ", ".join(f"{k} {g[k]:.2e} (float32 numpy {base[i][k]:.1e})" for k in g) +
              f"; R2 {np.nanmean(r64[i]):.4f}")
    for i in range(len(got)):
        kb = kap[i] * b
        assert kb <= 0.1, (i, kb)                                        # a precondition on the input, not on the kernel
        assert got[i]["w"] <= kb, ("w", i, got[i]["w"], kb)
        assert got[i]["pred"] <= max(30 * base[i]["pred"], FLOOR), ("pred", i, got[i]["pred"], base[i]["pred"])
        assert got[i]["r2"] <= max(30 * base[i]["r2"], FLOOR), ("r2", i, got[i]["r2"], base[i]["r2"])
        assert got[i]["r2"] <= 3 * kb, ("r2", i, got[i]["r2"], 3 * kb)
    return got


def run_case(case, b):
    """One case through the backend methods `readout_fit` / `readout_weights` / `readout_predict` / `readout_score` of b -> (fit outputs, w, preds, r2)."""
    xtr, ytr, xte, yte = case_data(case)
    xa, ya, xt, yt = (b.asarray(a) for a in (xtr, ytr, xte, yte))
    mean_x, comp, var, mean_y, z, info = b.readout_fit(xa, ya)
    assert info.converged == 1
    w = b.readout_weights(comp, var, z, lambdas_of(var, CASES[case]))
    sse, sst = b.readout_score(xt, yt, mean_x, w, mean_y)
    preds = np.stack([np.asarray(b.to_numpy(b.readout_predict(xt, mean_x, w[i], mean_y))) for i in range(w.shape[0])])
    return (mean_x, comp, var, mean_y, z), w, preds, 1.0 - sse / sst[None, :], (sse, sst)
