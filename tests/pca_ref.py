"""Float64 numpy restatement of the PCA fit, the transform and the progression panel, written from DESIGN.md "PCA" (not from the kernels), with the
data generator and the metrics the CPU and GPU tests share."""
from __future__ import annotations

import functools

import numpy as np

EPS = 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------------ data
def make_data(n: int, d: int, offset: float = 3.0, seed: int = 0, decay: float = 0.7) -> np.ndarray:
    """float32 [n, d]: Gaussian rows whose covariance has the spectrum decay^j in a random orthonormal basis, plus `offset` on every column."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    z = rng.standard_normal((n, d)) * np.sqrt(decay ** np.arange(d))
    return (z @ q.T + offset).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ fit / transform
def sign_rows(v: np.ndarray) -> np.ndarray:
    """Each row's largest-magnitude coefficient positive, the lowest index winning a tie."""
    j = np.argmax(np.abs(v), axis=1)      # (argmax returns the first maximum)
    s = np.sign(v[np.arange(v.shape[0]), j])
    s[s == 0] = 1.0
    return v * s[:, None]


def fit(x, dtype=np.float64):
    """(mean [d], components [d, d] rows, variance [d]) of x's rows: two-pass covariance with divisor n - 1, symmetric eigen-decomposition, variances
    clamped at 0 and descending, unit rows with the sign convention.  dtype=float32: the same in float32 (the baseline the tests print)."""
    x = np.asarray(x).astype(dtype)
    n = x.shape[0]
    mean = x.mean(0, dtype=dtype)
    xc = x - mean
    cov = (xc.T @ xc) / dtype(n - 1)
    lam, vec = np.linalg.eigh(cov)
    order = np.argsort(-lam, kind="stable")
    return mean, sign_rows(vec.T[order]), np.maximum(lam[order], 0)


def covariance64(x):
    x = np.asarray(x, np.float64)
    xc = x - x.mean(0)
    return xc.T @ xc / (x.shape[0] - 1)


def transform(x, mean, components):
    return (np.asarray(x, np.float64) - np.asarray(mean, np.float64)) @ np.asarray(components, np.float64).T


def bound(d: int) -> float:
    """max(d, 8) * 2^-23: the worst-case backward error of a stable symmetric eigensolver in float32 at this size."""
    return max(d, 8) * EPS


def fit_metrics(x, mean, components, variance) -> dict:
    """The four fit metrics of a result against the float64 reference on the same float32 input."""
    m64, _, l64 = fit(x)
    c64 = covariance64(x)
    v, lam = np.asarray(components, np.float64), np.asarray(variance, np.float64)
    lmax = max(l64[0], np.finfo(np.float64).tiny)
    return {"eig": float(np.abs(lam - l64).max() / lmax),
            "resid": float(np.linalg.norm(c64 @ v.T - v.T * lam[None, :], axis=0).max() / lmax),
            "orth": float(np.abs(v @ v.T - np.eye(v.shape[0])).max()),
            "mean": float((np.abs(np.asarray(mean, np.float64) - m64) / np.maximum(np.abs(m64), 1.0)).max())}


def top_k(n: int, d: int) -> int:
    return min(4, d, n - 1)


def eigengap(variance64, k: int) -> float:
    """The smallest gap between consecutive eigenvalues among the top k + 1 (a missing one counts as 0), relative to the largest."""
    lam = np.concatenate([np.asarray(variance64, np.float64), [0.0]])[:k + 1]
    return float((lam[:-1] - lam[1:]).min() / lam[0])


def projection_error(x, proj, k: int) -> float:
    m64, v64, _ = fit(x)
    p64 = transform(x, m64, v64[:k])
    return float(np.abs(np.asarray(proj, np.float64)[:, :k] - p64).max() / np.abs(p64).max())


def fit_cases(rows_per_wg: int):
    """(n, d, offset, seed) of the fit tests: the smallest problems, sizes around the 16-wide tiles, 64 and the 128 limit, one and several row
    chunks, and the offset-100 case a one-pass variance fails.  The seeds give a top-5 eigengap >= 0.05 (asserted from the reference)."""
    return ((2, 1, 3.0, 0), (2, 3, 3.0, 0), (3, 2, 3.0, 0), (63, 60, 3.0, SEED_63_60), (65, 64, 3.0, 0), (129, 65, 3.0, 0),
            (rows_per_wg + 1, 127, 3.0, 0), (3 * rows_per_wg + 7, 128, 3.0, 0), (1025, 60, 100.0, 0))


SEED_63_60 = 5


@functools.lru_cache(None)
def case_data(n, d, offset, seed):
    x = make_data(n, d, offset, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(None)
def case_reference(n, d, offset, seed):
    """(float64 fit, top k, eigengap, the float32 numpy baseline's metrics and projection error) of a case, computed once."""
    x = case_data(n, d, offset, seed)
    f64, k = fit(x), top_k(n, d)
    m32, c32, v32 = fit(x, np.float32)
    base = fit_metrics(x, m32, c32, v32)
    base["proj"] = projection_error(x, (x - m32) @ c32[:k].T, k)
    return f64, k, eigengap(f64[2], k), base


def check_fit(x, mean, components, variance, proj, case, what=""):
    """Every fit metric of a result under max(d, 8) 2^-23, the projections under that over the eigengap, the signs exactly."""
    n, d = x.shape
    (m64, c64, l64), k, gap, base = case_reference(*case)
    got, b = fit_metrics(x, mean, components, variance), bound(d)
    got["proj"] = projection_error(x, proj, k)
    print(f"{what} {case}: bound {b:.3e}, gap {gap:.3f}; " + ", ".join(f"{key} {got[key]:.2e} (float32 numpy {base[key]:.1e})" for key in got))
    assert gap >= 0.05, gap                                      # a precondition on the input, not on the kernel
    for key in ("eig", "resid", "orth", "mean"):
        assert got[key] <= b, (key, got[key], b)
    assert got["proj"] <= b / gap, (got["proj"], b / gap)
    comp = np.asarray(components)
    np.testing.assert_array_equal(comp, sign_rows(comp))         # the convention, exactly
    assert (np.sum(comp[:k].astype(np.float64) * c64[:k], 1) > 0.9).all()      # and the same axes as the reference, signs included
    assert (np.diff(np.asarray(variance)) <= 0).all() and (np.asarray(variance) >= 0).all()
    return got


# ------------------------------------------------------------------------------------------------------------------ the panel
NEAR = 1e-3      # pixels: a pixel whose float64 distance to a line, marker or the terminated line is this close to its threshold is not compared


def style_dict(st) -> dict:
    """A hip.StripStyle as plain numbers."""
    return {"margins": (st.margin_left, st.margin_right, st.margin_top, st.margin_bottom), "hw": float(st.line_half_width), "radius": float(st.marker_radius),
            "colour": [tuple(st.colour[c][:3]) for c in range(8)], "background": tuple(st.background[:3]), "axes": tuple(st.axes[:3]),
            "terminated": tuple(st.terminated[:3])}


def _seg_dist(cx, cy, ax, ay, bx, by):
    ex, ey, wx, wy = bx - ax, by - ay, cx - ax, cy - ay
    u = np.clip((wx * ex + wy * ey) / (ex * ex + ey * ey), 0.0, 1.0)
    return np.hypot(wx - u * ex, wy - u * ey)


def panel(proj, frame_idx, flags, k, ymin, ymax, window, style: dict, W, H):
    """(rgba uint8 [F, H, W, 4], near bool [F, H, W]) from the panel geometry of DESIGN.md "PCA", every pixel against every segment in float64."""
    proj = np.asarray(proj, np.float64)
    T = proj.shape[0]
    ml, mr, mt, mb = style["margins"]
    x0, x1, y0, y1 = ml, W - mr, mt, H - mb
    ymin, ymax, hw, rad = float(np.float32(ymin)), float(np.float32(ymax)), float(np.float32(style["hw"])), float(np.float32(style["radius"]))
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    cx, cy = px + 0.5, py + 0.5
    inside = (px >= x0) & (px < x1) & (py >= y0) & (py < y1)
    frame = inside & ((px == x0) | (px == x1 - 1) | (py == y0) | (py == y1 - 1))
    sx, sy = (x1 - x0) / window, (y1 - y0) / (ymax - ymin)
    out = np.zeros((len(frame_idx), H, W, 4), np.uint8)
    near = np.zeros((len(frame_idx), H, W), bool)
    for f, i in enumerate(frame_idx):
        i = int(min(max(i, 0), T))
        xa = 0.0 if i <= window else float(i - window)
        X = lambda t: x0 + (t - xa) * sx          # noqa: E731
        Y = lambda v: y1 - (v - ymin) * sy        # noqa: E731
        img = np.empty((H, W, 3), np.uint8)
        img[:] = style["background"]
        img[frame] = style["axes"]                # the 1-px frame of the plot rectangle, under the curves
        nr = np.zeros((H, W), bool)
        for c in range(k):                        # lines: later components over earlier ones
            for t in range(i - 1):
                v0, v1 = proj[t, c], proj[t + 1, c]
                if not (np.isfinite(v0) and np.isfinite(v1)):
                    continue
                dist = _seg_dist(cx, cy, X(t), Y(v0), X(t + 1), Y(v1))
                img[inside & (dist <= hw)] = style["colour"][c]
                nr |= np.abs(dist - hw) < NEAR
        if i >= 1:
            for c in range(k):                    # markers over lines: a filled disc at the last drawn point
                v = proj[i - 1, c]
                if np.isfinite(v):
                    dist = np.hypot(cx - X(i - 1), cy - Y(v))
                    img[inside & (dist <= rad)] = style["colour"][c]
                    nr |= np.abs(dist - rad) < NEAR
        if int(flags[f]) & 1:                     # the terminated line over both
            dist = np.abs(cx - X(i))
            img[inside & (dist <= hw)] = style["terminated"]
            nr |= np.abs(dist - hw) < NEAR
        out[f, ..., :3], out[f, ..., 3] = img, 255
        near[f] = nr & inside
    return out, near


# the panel scenes of the CPU and GPU tests: T = 12, one curve steeper than the plot, one NaN sample
PANEL_SIZES = ((96, 64), (161, 97))
PANEL_KS = (1, 3, 8)
PANEL_WINDOWS = (5, 530)
PANEL_FRAMES = (0, 1, 2, 5, 6, 11, 12)
PANEL_YLIM = (-2.2, 2.2)


def panel_projections() -> np.ndarray:
    rng = np.random.default_rng(5)
    p = (rng.standard_normal((12, 8)) * np.array([1.0, 0.8, 0.6, 0.5, 0.4, 0.3, 0.25, 0.2])).astype(np.float32)
    p[:, 2] = (np.where(np.arange(12) % 2 == 0, -1.0, 1.0) * (6.0 + 2.0 * rng.random(12))).astype(np.float32)      # steeper than the plot: leaves it at both ends every step
    p[4, 1] = np.nan
    return p


def panel_style(W, H):
    from track_mjx_amd.analysis import pca as P
    return P.strip_style(W, H, line_half_width=0.8, marker_radius=2.6, margins=(W // 10, W // 16, H // 12, H // 8))


@functools.lru_cache(None)
def panel_reference(size, k, window):
    W, H = size
    flags = np.zeros(len(PANEL_FRAMES), np.uint8)
    flags[-1] = 1
    return panel(panel_projections(), PANEL_FRAMES, flags, k, *PANEL_YLIM, window, style_dict(panel_style(W, H)), W, H)


def check_panel(got, size, k, window, what=""):
    ref, near = panel_reference(size, k, window)
    share = near.reshape(near.shape[0], -1).mean(1).max()
    bad = (got != ref).any(-1) & ~near
    print(f"{what} {size} k={k} window={window}: {int(bad.sum())} pixels differ, at most {100 * share:.3f} % of a panel's pixels excluded")
    assert share <= 1e-3, share
    assert got.shape == ref.shape and not bad.any(), np.argwhere(bad)[:10]
