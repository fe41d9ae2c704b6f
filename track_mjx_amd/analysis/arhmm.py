"""An autoregressive hidden Markov model of recorded signals on the GPU (csrc/tmjx_arhmm.hip; DESIGN.md "Autoregressive sequence model"): the time
steps of every clip assigned to motifs that are told apart by how the signal MOVES.  Every state is its own linear law
x_t ~ A_1 x_(t-1) + .. + A_L x_(t-L) + b with diagonal noise (the AR-HMM of MoSeq, there run on about 10 principal components with 3 lags); two
motifs may occupy the same region and differ only in how they traverse it.  The transition matrix, the forward-backward pass, the Viterbi path and
the ethogram summaries are the Gaussian HMM's (analysis.hmm).

    python -m track_mjx_amd.analysis.arhmm rollouts=<dir of clip_<i>.h5> [feature=intention | projections=<pca.h5> n_components=10] k=32 lags=3 [warmup=]
                                           [ridge=1] [kappa=0] [prior=0.1] [seed=0] [n_init=4] [max_iter=50] [tol=1e-4] [holdout=0] [rate=]
                                           [posteriors=false] out=<arhmm.h5>

The signal is up to 32 wide: a recorded feature that narrow, or the leading n_components of a pca.h5 written by analysis.pca (projections=).  The
first `warmup` rows of every clip (default: lags) are conditioned on, not scored.  The file holds what an hmm.h5 holds (means, variances, transmat,
startprob, loglik, loglik_per_step_train / _heldout PER SCORED ROW, n_iter, converged, feature, clips, seed, counts, transitions, dwell_mean,
init_dwell_mean, labels/clip_<i>, confidence/clip_<i>, gamma/clip_<i> with posteriors=true, centroids = means, so `python -m
track_mjx_amd.analysis.rollout ... intervene_centroids=<arhmm.h5>` takes it) and weights [K, D, L D + 1] (column l D + c multiplies feature c at lag
l + 1, the last column is the intercept, in coordinates centred on `center`), center [D], lags, warmup, status [K] (0 updated, 1 light, 2 singular
at the last M-step), n_singular, and with rate=<Hz> eig_modulus and eig_freq_hz [K, L D]: the eigenvalues of every state's companion matrix, by
descending modulus: whether the motif oscillates, and at what rate.
"""
from __future__ import annotations

import sys

import numpy as np

from .. import hip as _hip
from . import cli
from . import hmm as _hmm
from .recorded import feature_of, rollout_features, seq_start, signals

CLI_OPTIONS = ("rollouts", "out", "feature", "projections", "n_components", "k", "lags", "warmup", "ridge", "kappa", "prior", "seed", "n_init", "max_iter", "tol",
               "holdout", "rate", "posteriors")
USAGE = ("usage: python -m track_mjx_amd.analysis.arhmm rollouts=<dir of clip_<i>.h5> [feature=intention | projections=<pca.h5> n_components=10] k=32 lags=3 "
         "[warmup=] [ridge=1] [kappa=0] [prior=0.1] [seed=0] [n_init=4] [max_iter=50] [tol=1e-4] [holdout=0] [rate=] [posteriors=false] out=<arhmm.h5>")


def _too_wide(d):
    return (f"{d} features: the autoregressive HMM takes up to {_hip.ARHMM_MAX_D}; project the layer first (python -m track_mjx_amd.analysis.pca ... "
            f"out=<pca.h5>) and pass projections=<pca.h5> n_components=10")


def companion_eigenvalues(weights, d: int, lags: int):
    """The eigenvalues [K, L D] of every state's companion matrix [[A_1 .. A_L], [I 0]], by descending modulus (host numpy)."""
    k, ld = weights.shape[0], lags * d
    out = np.zeros((k, ld), np.complex128)
    for j in range(k if ld else 0):
        comp = np.zeros((ld, ld))
        comp[:d] = np.asarray(weights[j][:, :ld], np.float64)
        comp[d:, :ld - d] = np.eye(ld - d)
        ev = np.linalg.eigvals(comp)
        out[j] = ev[np.argsort(-np.abs(ev), kind="stable")]
    return out


class ARHMM(_hmm.GaussianHMM):
    """EM for a hidden Markov model with autoregressive emissions over [n, d] rows in sequences of `lengths`, d <= 32, lags <= 4, lags d <= 128,
    n_states <= 128.  The surface of GaussianHMM: `fit`, `predict`, `predict_proba`, `score`, `score_sequences`, and after a fit `means_` (every
    state's weighted mean of x), `vars_` [K, D] (the noise), `transmat_`, `startprob_`, `loglik_`, `n_iter_`, `converged_`, `labels_`, `counts_`,
    `gamma_`, `init_labels_`, plus `weights_` [K, D, L D + 1], `center_` [D] (the float32 column mean, fixed before the fit), `status_` [K] and
    `n_scored_`.  warmup=None scores every row that has its lags; ridge counts pseudo-rows: the penalty on every regressor column but the
    intercept is ridge x the mean column variance.  The initialisation is GaussianHMM's, so deterministic: k-means labels, one-hot gamma, the
    moments and one solve from zero weights, the transitions from the label counts.  States are numbered by descending Viterbi count."""

    def __init__(self, n_states: int, lags: int = 1, warmup=None, ridge: float = 1.0, max_iter: int = 50, tol: float = 1e-4, prior: float = 0.1,
                 kappa: float = 0.0, min_var=None, n_init: int = 4, seed: int = 0, device="cuda", backend=None):
        if not 0 <= int(lags) <= _hip.ARHMM_MAX_LAGS:
            raise ValueError(f"lags must be in 0 .. {_hip.ARHMM_MAX_LAGS} (got {lags})")
        if warmup is not None and int(warmup) < int(lags):
            raise ValueError(f"warmup = {warmup} is smaller than lags = {lags}")
        if not float(ridge) >= 0.0:
            raise ValueError(f"ridge must be >= 0 (got {ridge})")
        super().__init__(n_states, max_iter=max_iter, tol=tol, prior=prior, kappa=kappa, min_var=min_var, n_init=n_init, seed=seed, device=device,
                         backend=backend)
        self.lags, self.warmup, self.ridge = int(lags), int(lags) if warmup is None else int(warmup), float(ridge)

    def _scored(self, seq):
        return int(np.maximum(np.diff(seq) - self.warmup, 0).sum())

    def fit(self, x, lengths):
        b, k, L, R = self._b, self.n_states, self.lags, self.warmup
        xa = b.asarray(x)
        n, d = (int(v) for v in xa.shape)
        seq = seq_start(lengths, n)
        if k > n:
            raise ValueError(f"n_states = {k} exceeds the {n} rows")
        if d > _hip.ARHMM_MAX_D:
            raise ValueError(_too_wide(d))
        if L * d > 128:
            raise ValueError(f"lags x features = {L * d} exceeds the 128 lagged regressor columns the autoregressive HMM takes")
        x64 = np.asarray(b.to_numpy(xa), np.float64)
        colvar = float(x64.var(0).mean())
        self.min_var_ = 1e-3 * colvar if self.min_var is None else self.min_var
        self.ridge_ = self.ridge * colvar
        center = x64.mean(0).astype(np.float32)
        p = L * d + 1
        km, onehot, A, pi = self._start(xa, seq)
        moments, weight = b.arhmm_moments(xa, seq, L, R, center, onehot)
        W, var, _, _ = b.arhmm_solve(moments, weight, d, L, center, np.zeros((k, d, p), np.float32),
                                     np.full((k, d), max(colvar, self.min_var_, 1e-30), np.float32), self.ridge_, self.min_var_, 0.5)
        W, var, A, pi, gamma, labels, status, info = b.arhmm_fit(xa, seq, L, R, center, W, var, A, pi, self.max_iter, self.tol, self.prior, self.kappa, self.ridge_,
                                                                 self.min_var_, _hmm.MIN_WEIGHT)
        # every state's weighted mean of x over the scored rows, from the moments of the final posteriors (a state without weight: the centre)
        moments, weight = b.arhmm_moments(xa, seq, L, R, center, gamma)
        with np.errstate(divide="ignore", invalid="ignore"):
            shift = np.where(weight[:, None] > 0, moments[:, p:, p - 1] / weight[:, None], 0.0)
        mu = (center.astype(np.float64)[None, :] + shift).astype(np.float32)
        order = self._fitted(mu, var, A, pi, gamma, labels, info, km.labels_, seq, d)
        self.weights_, self.status_, self.n_singular_, self.center_ = np.ascontiguousarray(W[order]), np.ascontiguousarray(status[order]), int(info.n_singular), center
        self.n_scored_ = self._scored(seq)
        return self

    def _logb(self, x, lengths):
        if not hasattr(self, "weights_"):
            raise ValueError("this ARHMM is not fitted")
        xa = self._b.asarray(x)
        if xa.shape[1] != self.n_features_:
            raise ValueError(f"expected {self.n_features_} features, got {xa.shape[1]}")
        seq = seq_start(lengths, int(xa.shape[0]))
        return self._b.arhmm_emission(xa, seq, self.lags, self.warmup, self.center_, self.weights_, self.vars_), seq

    def scored_rows(self, lengths) -> int:
        return max(self._scored(seq_start(lengths, sum(lengths))), 1)

    def eigenvalues(self):
        """[K, L D] complex: the eigenvalues of every state's companion matrix, by descending modulus."""
        return companion_eigenvalues(self.weights_, self.n_features_, self.lags)


def _read(rollouts, feature, projections, n_components):
    """-> (clip numbers, [T_j, D] float32 signals, the name they go by): the recorded feature, or the leading n_components of the projections of a
    pca.h5."""
    if projections is None:
        ids, feats = rollout_features(rollouts, lambda r, _, where: feature_of(r, feature, where), feature, "fit")
        if feats[0].shape[1] > _hip.ARHMM_MAX_D:
            raise ValueError(f"{feature}: " + _too_wide(feats[0].shape[1]))
        return ids, [np.ascontiguousarray(f, np.float32) for f in feats], feature
    if not 1 <= int(n_components) <= _hip.ARHMM_MAX_D:
        raise ValueError(f"n_components must be in 1 .. {_hip.ARHMM_MAX_D} (got {n_components})")
    ids, sigs, _ = signals(rollouts, "projections", None, projections)
    if sigs[0].shape[1] < int(n_components):
        raise ValueError(f"{projections} holds {sigs[0].shape[1]} components, n_components = {n_components} asked")
    return ids, [np.ascontiguousarray(s[:, :int(n_components)], np.float32) for s in sigs], "projections"


def fit_rollouts(rollouts, feature: str = "intention", k: int = 32, lags: int = 3, warmup=None, ridge: float = 1.0, max_iter: int = 50, tol: float = 1e-4,
                 prior: float = 0.1, kappa: float = 0.0, n_init: int = 4, seed: int = 0, holdout: int = 0, projections=None, n_components: int = 10,
                 device="cuda", backend=None):
    """Fit `feature` (up to 32 wide), or the leading n_components of `projections` (a pca.h5), over the roll-outs, each one sequence.  With
    holdout = h >= 2 the clips at the positions p, p % h == h - 1, are left out of the fit and scored.
    -> (arhmm, feats): as analysis.hmm.fit_rollouts; the likelihoods per step are per SCORED row."""
    return _hmm.fit_split(lambda: _read(rollouts, feature, projections, n_components),
                          lambda: ARHMM(k, lags=lags, warmup=warmup, ridge=ridge, max_iter=max_iter, tol=tol, prior=prior, kappa=kappa, n_init=n_init, seed=seed,
                                        device=device, backend=backend), holdout)


def main(argv=None, backend=None) -> int:
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out", "k"), USAGE, lambda o: not ("feature" in o and "projections" in o))
    if opts is None:
        return 2
    try:
        k, seed, lags = int(opts["k"]), int(opts.get("seed", 0)), int(opts.get("lags", 3))
        warmup = int(opts["warmup"]) if opts.get("warmup", "") != "" else None
        rate = float(opts["rate"]) if opts.get("rate", "") != "" else None
        if rate is not None and not rate > 0.0:
            raise ValueError(f"rate must be > 0 (got {rate})")
        posteriors = cli.flag(opts, "posteriors")
        m, feats = fit_rollouts(opts["rollouts"], opts.get("feature", "intention"), k, lags, warmup, float(opts.get("ridge", 1.0)), int(opts.get("max_iter", 50)),
                                float(opts.get("tol", 1e-4)), float(opts.get("prior", 0.1)), float(opts.get("kappa", 0.0)), int(opts.get("n_init", 4)), seed,
                                int(opts.get("holdout", 0)), opts.get("projections"), int(opts.get("n_components", 10)), backend=backend)
        tree = _hmm.fitted_tree(m, feats, seed, posteriors)
    except (KeyError, ValueError) as e:
        return cli.report("arhmm", e)
    tree.update({"weights": m.weights_, "center": m.center_, "lags": np.int64(m.lags), "warmup": np.int64(m.warmup), "status": np.asarray(m.status_, np.int32),
                 "n_singular": np.int64(m.n_singular_)})
    if rate is not None:
        ev = m.eigenvalues()
        tree["eig_modulus"], tree["eig_freq_hz"] = np.abs(ev), np.abs(np.angle(ev)) * rate / (2.0 * np.pi)
    cli.write(opts["out"], tree)
    print(f"[arhmm] {m.feature_}: {m.n_samples_} samples x {m.n_features_} features from {len(m.train_)} clips into {k} states of {m.lags} lags, "
          + _hmm.summary_tail(m, tree, "scored step", opts["out"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
