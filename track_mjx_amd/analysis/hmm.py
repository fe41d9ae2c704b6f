"""A hidden Markov model of recorded activations on the GPU (csrc/tmjx_hmm.hip; DESIGN.md "Sequence model"): the time steps of every clip assigned
to motifs that persist.  The states are Gaussian with diagonal covariance, their transition matrix is fitted, the ethogram of a clip is its Viterbi
path, and the likelihood of held-out clips tells how many states the data support.

    python -m track_mjx_amd.analysis.hmm rollouts=<dir of clip_<i>.h5> [feature=intention] k=32 [kappa=0] [prior=0.1] [seed=0] [n_init=4] [max_iter=50]
                                         [tol=1e-4] [holdout=0] [posteriors=false] out=<hmm.h5>

writes means, variances [K, D], transmat [K, K], startprob [K], loglik (the training clips), loglik_per_step_train, loglik_per_step_heldout (with
holdout=h the clips at the positions p, p % h == h - 1, of the sorted list are left out of the fit and scored), n_iter, converged, feature, clips,
seed, counts, transitions, dwell_mean (analysis.cluster.segment_summary of the Viterbi labels), init_dwell_mean (the same of the k-means labels the
fit started from: what the smoothing did), labels/clip_<i> int32 [T - 1], confidence/clip_<i> float32 [T - 1] (the posterior of the label),
gamma/clip_<i> [T - 1, K] with posteriors=true, and centroids = means, so that `python -m track_mjx_amd.analysis.rollout ...
intervene_centroids=<hmm.h5>` takes the file as it takes a clusters.h5.  States are numbered by descending count over the fitted clips: state 0 is
the commonest.
"""
from __future__ import annotations

import os
import sys

import numpy as np

from .. import hip as _hip
from . import cluster as _cluster
from . import pca as _pca
from .utils import rollout_features

CLI_OPTIONS = ("rollouts", "out", "feature", "k", "kappa", "prior", "seed", "n_init", "max_iter", "tol", "holdout", "posteriors")
MIN_WEIGHT = 1e-3      # a state holding less than this many expected rows keeps its emission parameters


def _seq_start(lengths, n):
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if lengths.size == 0 or (lengths < 1).any() or int(lengths.sum()) != n:
        raise ValueError(f"lengths must be positive and sum to the {n} rows (got {lengths.size} lengths summing to {int(lengths.sum())})")
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


class GaussianHMM:
    """EM for a hidden Markov model with diagonal Gaussian emissions over [n, d] rows in sequences of `lengths`, d <= 1024, n_states <= 128: `fit`,
    `predict` (Viterbi), `predict_proba` (the posteriors gamma), `score` (the total log likelihood), `score_sequences` (one per sequence), and
    after a fit `means_`, `vars_` [K, D], `transmat_` [K, K], `startprob_` [K], `loglik_`, `n_iter_`, `converged_`, `labels_` [n] int32,
    `counts_` [K], `init_labels_` (the k-means labels the fit started from, in the k-means' numbering).  prior and kappa are Dirichlet
    pseudo-counts of the transition rows (kappa on the diagonal: a sticky model); min_var=None floors the variances at 1e-3 x the mean column variance.
    The initialisation is deterministic: cluster.KMeans(n_states, n_init, seed=seed) on the same rows, the moments of its clusters, its transition
    counts.  States are numbered by descending Viterbi count (equal counts keep their order).  Every run gives the same bits."""

    def __init__(self, n_states: int, max_iter: int = 50, tol: float = 1e-4, prior: float = 0.1, kappa: float = 0.0, min_var=None, n_init: int = 4,
                 seed: int = 0, device="cuda", backend=None):
        if not 1 <= int(n_states) <= _hip.HMM_MAX_K:
            raise ValueError(f"n_states must be in 1 .. {_hip.HMM_MAX_K} (got {n_states})")
        if int(max_iter) < 1 or int(n_init) < 1 or not float(tol) >= 0.0 or not float(prior) >= 0.0 or not float(kappa) >= 0.0:
            raise ValueError(f"max_iter and n_init must be >= 1 and tol, prior, kappa >= 0 (got {max_iter}, {n_init}, {tol}, {prior}, {kappa})")
        if min_var is not None and not float(min_var) >= 0.0:
            raise ValueError(f"min_var must be >= 0 (got {min_var})")
        self.n_states, self.max_iter, self.tol, self.prior, self.kappa = int(n_states), int(max_iter), float(tol), float(prior), float(kappa)
        self.min_var, self.n_init, self.seed = None if min_var is None else float(min_var), int(n_init), int(seed)
        self._b = _pca.HipBackend(device) if backend is None else backend

    def fit(self, x, lengths):
        b, k = self._b, self.n_states
        xa = b.asarray(x)
        n, d = (int(v) for v in xa.shape)
        seq = _seq_start(lengths, n)
        if k > n:
            raise ValueError(f"n_states = {k} exceeds the {n} rows")
        if d > _hip.HMM_MAX_D:
            raise ValueError(f"{d} features: the HMM takes up to {_hip.HMM_MAX_D}")
        colvar = float(np.asarray(b.to_numpy(xa), np.float64).var(0).mean())
        self.min_var_ = 1e-3 * colvar if self.min_var is None else self.min_var
        km = _cluster.KMeans(k, n_init=self.n_init, seed=self.seed, backend=b).fit(xa)
        lab0 = km.labels_
        cut = [lab0[s:e] for s, e in zip(seq[:-1], seq[1:])]
        onehot = np.zeros((n, k), np.float32)
        onehot[np.arange(n), lab0] = 1.0
        mu, var, _ = b.hmm_mstep(xa, onehot, km.cluster_centers_, np.full((k, d), max(colvar, self.min_var_, 1e-30), np.float32), self.min_var_, 0.5)
        _, trans, _ = _cluster.segment_summary(cut, k)
        first = np.bincount(lab0[seq[:-1]], minlength=k).astype(np.float64)
        A, pi = b.hmm_transitions(trans.astype(np.float64), first, self.prior, self.kappa, np.full((k, k), 1.0 / k, np.float32), np.full(k, 1.0 / k, np.float32))
        mu, var, A, pi, gamma, labels, info = b.hmm_fit(xa, seq, mu, var, A, pi, self.max_iter, self.tol, self.prior, self.kappa, self.min_var_, MIN_WEIGHT)
        counts = np.bincount(labels, minlength=k)
        order = np.argsort(-counts, kind="stable")      # descending count, equal counts in their original order
        rank = np.empty(k, np.int64)
        rank[order] = np.arange(k)
        self.means_, self.vars_ = np.ascontiguousarray(mu[order]), np.ascontiguousarray(var[order])
        self.transmat_, self.startprob_ = np.ascontiguousarray(A[order][:, order]), np.ascontiguousarray(pi[order])
        self.labels_, self.counts_, self.gamma_ = rank[labels].astype(np.int32), counts[order].astype(np.int64), np.ascontiguousarray(gamma[:, order])
        self.loglik_, self.n_iter_, self.converged_ = float(info.loglik), int(info.n_iter), bool(info.converged)
        self.init_labels_, self.n_samples_, self.n_features_, self.seq_start_ = lab0, n, d, seq
        return self

    def _logb(self, x, lengths):
        if not hasattr(self, "means_"):
            raise ValueError("this GaussianHMM is not fitted")
        xa = self._b.asarray(x)
        if xa.shape[1] != self.n_features_:
            raise ValueError(f"expected {self.n_features_} features, got {xa.shape[1]}")
        return self._b.hmm_emission(xa, self.means_, self.vars_), _seq_start(lengths, int(xa.shape[0]))

    def predict(self, x, lengths):
        logb, seq = self._logb(x, lengths)
        return self._b.hmm_viterbi(logb, seq, self.transmat_, self.startprob_)[0]

    def predict_proba(self, x, lengths):
        logb, seq = self._logb(x, lengths)
        return self._b.hmm_forward_backward(logb, seq, self.transmat_, self.startprob_)[0]

    def score_sequences(self, x, lengths):
        logb, seq = self._logb(x, lengths)
        return self._b.hmm_forward_backward(logb, seq, self.transmat_, self.startprob_)[3]

    def score(self, x, lengths):
        logb, seq = self._logb(x, lengths)
        return self._b.hmm_forward_backward(logb, seq, self.transmat_, self.startprob_)[4]


def fit_rollouts(rollouts, feature: str = "intention", k: int = 32, max_iter: int = 50, tol: float = 1e-4, prior: float = 0.1, kappa: float = 0.0,
                 n_init: int = 4, seed: int = 0, holdout: int = 0, device="cuda", backend=None):
    """Fit `feature` (up to 1024 wide) over the roll-outs, each one sequence.  `rollouts`: a directory of clip_<i>.h5, or a list of roll-out dicts.
    With holdout = h >= 2 the clips at the positions p, p % h == h - 1, are left out of the fit and scored.
    -> (hmm, feats): feats[j] float32 [T_j, D] of roll-out j; hmm.clips_ are the clip numbers, hmm.train_ / hmm.heldout_ the positions fitted / scored,
    hmm.loglik_per_step_train_ / hmm.loglik_per_step_heldout_ (None without held-out clips)."""
    holdout = int(holdout)
    if holdout < 0 or holdout == 1:
        raise ValueError(f"holdout must be 0 (no clip held out) or >= 2 (got {holdout})")
    ids, feats = rollout_features(rollouts, lambda r, _, where: _pca._feature_of(r, feature, where), feature, "fit")
    held = [p for p in range(len(ids)) if holdout and p % holdout == holdout - 1]
    train = [p for p in range(len(ids)) if p not in held]
    if not train or (holdout and not held):
        raise ValueError(f"holdout = {holdout} over {len(ids)} clips leaves no {'training' if not train else 'held-out'} clip")
    hmm = GaussianHMM(k, max_iter=max_iter, tol=tol, prior=prior, kappa=kappa, n_init=n_init, seed=seed, device=device, backend=backend)
    hmm.fit(np.concatenate([feats[p] for p in train], 0), [feats[p].shape[0] for p in train])
    hmm.clips_, hmm.feature_, hmm.train_, hmm.heldout_ = ids, feature, train, held
    hmm.loglik_per_step_train_ = hmm.loglik_ / hmm.n_samples_
    hmm.loglik_per_step_heldout_ = None
    if held:
        lens = [feats[p].shape[0] for p in held]
        hmm.loglik_per_step_heldout_ = hmm.score(np.concatenate([feats[p] for p in held], 0), lens) / sum(lens)
    return hmm, feats


def main(argv=None, backend=None) -> int:
    from .. import h5lite
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = dict(a.split("=", 1) for a in argv if "=" in a and a.split("=", 1)[0] in CLI_OPTIONS)
    if any(o not in opts for o in ("rollouts", "out", "k")) or len(opts) != len(argv):
        print("usage: python -m track_mjx_amd.analysis.hmm rollouts=<dir of clip_<i>.h5> [feature=intention] k=32 [kappa=0] [prior=0.1] [seed=0] [n_init=4] "
              "[max_iter=50] [tol=1e-4] [holdout=0] [posteriors=false] out=<hmm.h5>", file=sys.stderr)
        return 2
    feature = opts.get("feature", "intention")
    try:
        k, seed = int(opts["k"]), int(opts.get("seed", 0))
        posteriors = opts.get("posteriors", "false").lower()
        if posteriors not in ("true", "false"):
            raise ValueError(f"posteriors must be true or false (got {opts['posteriors']})")
        hmm, feats = fit_rollouts(opts["rollouts"], feature, k, int(opts.get("max_iter", 50)), float(opts.get("tol", 1e-4)), float(opts.get("prior", 0.1)),
                                  float(opts.get("kappa", 0.0)), int(opts.get("n_init", 4)), seed, int(opts.get("holdout", 0)), backend=backend)
        lens = [f.shape[0] for f in feats]
        allx = np.concatenate(feats, 0)
        labels, gamma = hmm.predict(allx, lens), hmm.predict_proba(allx, lens)
    except (KeyError, ValueError) as e:
        print(f"[hmm] {e.args[0] if e.args else e}", file=sys.stderr)
        return 2
    ends = np.cumsum(lens)
    cut = lambda a: [a[e - t:e] for e, t in zip(ends, lens)]      # noqa: E731
    lab, gam = cut(labels), cut(gamma)
    counts, trans, dwell = _cluster.segment_summary(lab, k)
    _, _, dwell0 = _cluster.segment_summary([hmm.init_labels_[s:e] for s, e in zip(hmm.seq_start_[:-1], hmm.seq_start_[1:])], k)
    tree = {"means": hmm.means_, "variances": hmm.vars_, "transmat": hmm.transmat_, "startprob": hmm.startprob_, "centroids": hmm.means_,
            "loglik": np.float64(hmm.loglik_), "loglik_per_step_train": np.float64(hmm.loglik_per_step_train_), "n_iter": np.int64(hmm.n_iter_),
            "converged": np.int64(hmm.converged_), "feature": feature, "clips": np.asarray(hmm.clips_, np.int64), "seed": np.int64(seed),
            "counts": counts, "transitions": trans, "dwell_mean": dwell, "init_dwell_mean": dwell0,
            "labels": {f"clip_{c}": np.asarray(v, np.int32) for c, v in zip(hmm.clips_, lab)},
            "confidence": {f"clip_{c}": np.ascontiguousarray(g[np.arange(len(v)), v], np.float32) for c, v, g in zip(hmm.clips_, lab, gam)}}
    if hmm.loglik_per_step_heldout_ is not None:
        tree["loglik_per_step_heldout"] = np.float64(hmm.loglik_per_step_heldout_)
    if posteriors == "true":
        tree["gamma"] = {f"clip_{c}": np.ascontiguousarray(g, np.float32) for c, g in zip(hmm.clips_, gam)}
    os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
    h5lite.write_tree(opts["out"], tree)
    occ, occ0 = counts > 0, dwell0 > 0
    held = "" if hmm.loglik_per_step_heldout_ is None else f", {hmm.loglik_per_step_heldout_:.4f} on {len(hmm.heldout_)} held-out clips"
    print(f"[hmm] {feature}: {hmm.n_samples_} samples x {hmm.n_features_} features from {len(hmm.train_)} clips into {k} states, {hmm.n_iter_} iterations"
          f"{'' if hmm.converged_ else ' (not converged)'}, loglik per step {hmm.loglik_per_step_train_:.4f}{held}; mean dwell "
          f"{float(dwell[occ].mean()):.2f} steps (k-means start: {float(dwell0[occ0].mean()):.2f}); wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
