"""Linear readout of behaviour from recorded activations on the GPU: ridge regression in the PCA's eigenbasis (csrc/tmjx_readout.hip; DESIGN.md "Readout").

How much of a behavioural variable (joint angles, controls, contact forces, sensor readings, another layer) can be read out linearly from a recorded
layer?  One fit gives the layer's PCA and, for every penalty of a sweep, the ridge weights W = V^T diag(1 / (s + lambda)) V C_xy; whole clips are
held out and scored by R^2.

    python -m track_mjx_amd.analysis.readout rollouts=<dir of clip_<i>.h5> feature=decoder/layer_0 target=qposes_rollout [target_cols=7:]
        [alphas=1e-3,1e-2,1e-1,1] [holdout=5] [lag=0] out=<readout.h5>

writes alphas, lambdas, r2 [L, M], r2_mean [L], best_index, coef and intercept of the best penalty, mean_x, mean_y, feature, target, train_clips,
test_clips and predictions/clip_<i> [T', M] of the held-out clips.
"""
from __future__ import annotations

import sys

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import resolve
from .recorded import by_clip, columns, feature_of, rollout_features, target_of

CLI_OPTIONS = ("rollouts", "out", "feature", "target", "target_cols", "alphas", "holdout", "lag")
USAGE = ("usage: python -m track_mjx_amd.analysis.readout rollouts=<dir of clip_<i>.h5> feature=<layer> target=<recorded array> [target_cols=a:b] "
         "[alphas=1e-3,1e-2,1e-1,1] [holdout=5] [lag=0] out=<readout.h5>")
DEFAULT_ALPHAS = (1e-3, 1e-2, 1e-1, 1.0, 10.0)


class Ridge:
    """Ridge regression from [n, d] rows (d <= 1024) to [n, m] targets (m <= 512) for every penalty of `alphas` at once.  A penalty is given relative
    to the mean variance of the features: lambda_i = alpha_i sum(variance) / d.  `fit(x, y)`, `score(x, y)` -> float64 [L, M] R^2 (NaN where a
    target is constant over the rows scored), `predict(x, index=None)` (by default the penalty with the best mean R^2 of the last `score`, before any
    score the middle one).  After a fit: `coef_` [L, D, M], `intercept_` [L, M], `lambdas_`, `alphas_`, and the PCA's `mean_`, `components_` [D, D],
    `explained_variance_` [D]: one fit serves both analyses.  Inputs: numpy arrays, or torch device tensors (a row stride is kept)."""

    def __init__(self, alphas=DEFAULT_ALPHAS, device="cuda", backend=None):
        a = np.atleast_1d(np.asarray(alphas, np.float64))
        if a.ndim != 1 or not 1 <= a.shape[0] <= _hip.READOUT_MAX_L:
            raise ValueError(f"{a.size} penalties given: a sweep takes 1 .. {_hip.READOUT_MAX_L}")
        if not (np.isfinite(a) & (a > 0)).all():
            raise ValueError(f"every alpha must be finite and > 0 (got {a.tolist()}): alpha = 0 is not a ridge, and a rank-deficient layer needs one")
        self.alphas_ = a
        self._b = resolve(backend, device)

    @staticmethod
    def _columns(y):
        return y[:, None] if getattr(y, "ndim", 2) == 1 else y      # a single target series [n] -> [n, 1]

    def fit(self, x, y):
        xa, ya = self._b.asarray(x), self._b.asarray(self._columns(y))
        if xa.shape[0] != ya.shape[0]:
            raise ValueError(f"x has {xa.shape[0]} rows, y has {ya.shape[0]}")
        mean_x, comp, var, mean_y, z, info = self._b.readout_fit(xa, ya)
        d = int(xa.shape[1])
        total = float(var.astype(np.float64).sum())
        if not total > 0.0:
            raise ValueError("the features have zero total variance (every row is the same): there is nothing to regress on")
        self.lambdas_ = self.alphas_ * total / d
        self.coef_ = self._b.readout_weights(comp, var, z, self.lambdas_)
        self.mean_, self.components_, self.explained_variance_, self.mean_y_ = mean_x, comp, var, mean_y
        self.intercept_ = (mean_y.astype(np.float64)[None, :] - np.einsum("d,ldm->lm", mean_x.astype(np.float64), self.coef_.astype(np.float64))).astype(np.float32)
        self.n_samples_, self.n_features_, self.n_targets_, self.n_sweeps_ = int(xa.shape[0]), d, int(ya.shape[1]), int(info.sweeps)
        self.r2_, self.best_index_ = None, None
        return self

    def _fitted(self, xa):
        if not hasattr(self, "coef_"):
            raise ValueError("this Ridge is not fitted")
        if xa.shape[1] != self.n_features_:
            raise ValueError(f"expected {self.n_features_} features, got {xa.shape[1]}")

    def score(self, x, y):
        xa, ya = self._b.asarray(x), self._b.asarray(self._columns(y))
        self._fitted(xa)
        if ya.shape[1] != self.n_targets_ or ya.shape[0] != xa.shape[0]:
            raise ValueError(f"expected targets [{xa.shape[0]}, {self.n_targets_}], got {tuple(ya.shape)}")
        sse, sst = self._b.readout_score(xa, ya, self.mean_, self.coef_, self.mean_y_)
        with np.errstate(divide="ignore", invalid="ignore"):
            r2 = np.where(sst[None, :] > 0.0, 1.0 - sse / sst[None, :], np.nan)
        self.r2_ = r2
        means = np.array([np.nanmean(r) if np.isfinite(r).any() else -np.inf for r in r2])
        self.best_index_ = int(np.argmax(means))
        return r2

    def predict(self, x, index=None):
        xa = self._b.asarray(x)
        self._fitted(xa)
        L = self.coef_.shape[0]
        i = (self.best_index_ if self.best_index_ is not None else L // 2) if index is None else int(index)
        if not 0 <= i < L:
            raise ValueError(f"index = {i} of {L} penalties")
        out = self._b.readout_predict(xa, self.mean_, self.coef_[i], self.mean_y_)
        return self._b.to_numpy(out) if isinstance(x, np.ndarray) else out


def _align(feat, targ, lag: int, where: str):
    """Rows of one roll-out: activation row t is paired with target[t + lag], and the rows without a partner are dropped.  A per-frame series (T rows
    against the T - 1 steps) has a partner for every row at either lag; a per-step one (T - 1 rows) is used as it is at lag 0 and loses its last
    row at lag 1."""
    t1 = feat.shape[0]
    if targ.shape[0] not in (t1, t1 + 1):
        raise ValueError(f"{where}: the target has {targ.shape[0]} rows, the feature {t1}")
    rows = min(t1, targ.shape[0] - lag)
    return feat[:rows], targ[lag:lag + rows]


def fit_rollouts(rollouts, feature: str, target: str, alphas=DEFAULT_ALPHAS, holdout: int = 5, lag: int = 0, target_cols=None, device="cuda", backend=None):
    """Fit a `Ridge` from `feature` (as recorded.feature_of resolves it) to `target` over the training clips and score it on the held-out ones: of the sorted
    clip list, the positions p with p % holdout == holdout - 1.  `rollouts`: a directory of clip_<i>.h5, or a list of roll-out dicts.
    -> the fitted Ridge with r2_ [L, M], best_index_, train_clips_, test_clips_ (clip numbers; list positions for dicts), feature_, target_, and
    test_features_ (the held-out clips' feature rows, for predictions)."""
    holdout, lag = int(holdout), int(lag)
    if holdout < 2:
        raise ValueError(f"holdout must be >= 2 (got {holdout})")
    if lag not in (0, 1):
        raise ValueError(f"lag must be 0 or 1 (got {lag})")
    ids, pairs = rollout_features(rollouts, lambda r, _, where: (feature_of(r, feature, where), target_of(r, target, where)))
    if len(ids) < 2:
        raise ValueError(f"a held-out score needs at least two clips (got {len(ids)})")
    if len({f.shape[1] for f, _ in pairs}) != 1 or len({t.shape[1] for _, t in pairs}) != 1:
        raise ValueError(f"{feature} or {target} has different widths across roll-outs")
    sl = columns(target_cols, pairs[0][1].shape[1])
    width = len(range(*sl.indices(pairs[0][1].shape[1])))
    if width > _hip.READOUT_MAX_M:
        raise ValueError(f"{target} is {width} wide: a readout takes up to {_hip.READOUT_MAX_M} targets, pick columns with target_cols=a:b")
    rows = [_align(f, t[:, sl], lag, f"clip {c}") for c, (f, t) in zip(ids, pairs)]
    test = [p for p in range(len(ids)) if p % holdout == holdout - 1]
    train = [p for p in range(len(ids)) if p % holdout != holdout - 1]
    if not test or not train:
        raise ValueError(f"holdout = {holdout} over {len(ids)} clips leaves no {'test' if not test else 'training'} clip")
    ridge = Ridge(alphas, device=device, backend=backend)
    cat = lambda ps, k: np.ascontiguousarray(np.concatenate([rows[p][k] for p in ps], 0), np.float32)      # noqa: E731
    ridge.fit(cat(train, 0), cat(train, 1))
    ridge.score(cat(test, 0), cat(test, 1))
    ridge.train_clips_, ridge.test_clips_ = [ids[p] for p in train], [ids[p] for p in test]
    ridge.feature_, ridge.target_, ridge.test_features_ = feature, target, [rows[p][0] for p in test]
    return ridge


def main(argv=None, backend=None) -> int:
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out", "feature", "target"), USAGE)
    if opts is None:
        return 2
    try:
        alphas = tuple(float(v) for v in opts["alphas"].split(",")) if "alphas" in opts else DEFAULT_ALPHAS
        r = fit_rollouts(opts["rollouts"], opts["feature"], opts["target"], alphas, int(opts.get("holdout", 5)), int(opts.get("lag", 0)),
                         opts.get("target_cols"), backend=backend)
    except (KeyError, ValueError) as e:
        return cli.report("readout", e)
    best = r.best_index_
    r2_mean = np.array([np.nanmean(v) if np.isfinite(v).any() else np.nan for v in r.r2_])
    cli.write(opts["out"], {"alphas": r.alphas_, "lambdas": r.lambdas_, "r2": r.r2_, "r2_mean": r2_mean, "best_index": np.int64(best), "coef": r.coef_[best],
                            "intercept": r.intercept_[best], "mean_x": r.mean_, "mean_y": r.mean_y_, "feature": r.feature_, "target": r.target_,
                            "train_clips": np.asarray(r.train_clips_, np.int64), "test_clips": np.asarray(r.test_clips_, np.int64),
                            "predictions": by_clip(r.test_clips_, [r.predict(f) for f in r.test_features_])})
    print(f"[readout] {r.feature_} -> {r.target_}: {r.n_samples_} samples x {r.n_features_} features -> {r.n_targets_} targets, {len(r.train_clips_)} training and "
          f"{len(r.test_clips_)} held-out clips; held-out R2 by alpha " + ", ".join(f"{a:g}: {v:.4f}" for a, v in zip(r.alphas_, r2_mean)) +
          f"; best alpha {r.alphas_[best]:g}; wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
