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

import sys

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import resolve
from .cluster import KMeans, segment_summary
from .recorded import by_clip, feature_of, number_by_count, rollout_features, seq_start, split

CLI_OPTIONS = ("rollouts", "out", "feature", "k", "kappa", "prior", "seed", "n_init", "max_iter", "tol", "holdout", "posteriors")
USAGE = ("usage: python -m track_mjx_amd.analysis.hmm rollouts=<dir of clip_<i>.h5> [feature=intention] k=32 [kappa=0] [prior=0.1] [seed=0] [n_init=4] "
         "[max_iter=50] [tol=1e-4] [holdout=0] [posteriors=false] out=<hmm.h5>")
MIN_WEIGHT = 1e-3      # a state holding less than this many expected rows keeps its emission parameters


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
        self._b = resolve(backend, device)

    def _start(self, xa, seq):
        """The deterministic start both models share: -> (the k-means, its labels as one-hot posteriors [n, K], the transition matrix and start
        probabilities from its label counts)."""
        b, k, n = self._b, self.n_states, int(xa.shape[0])
        km = KMeans(k, n_init=self.n_init, seed=self.seed, backend=b).fit(xa)
        lab0 = km.labels_
        onehot = np.zeros((n, k), np.float32)
        onehot[np.arange(n), lab0] = 1.0
        _, trans, _ = segment_summary([lab0[s:e] for s, e in zip(seq[:-1], seq[1:])], k)
        first = np.bincount(lab0[seq[:-1]], minlength=k).astype(np.float64)
        A, pi = b.hmm_transitions(trans.astype(np.float64), first, self.prior, self.kappa, np.full((k, k), 1.0 / k, np.float32), np.full(k, 1.0 / k, np.float32))
        return km, onehot, A, pi

    def _fitted(self, mu, var, A, pi, gamma, labels, info, lab0, seq, d):
        """Keep a fit's result with the states numbered by descending Viterbi count; -> the permutation `order`."""
        order, rank, self.counts_ = number_by_count(labels, self.n_states)
        self.means_, self.vars_ = np.ascontiguousarray(mu[order]), np.ascontiguousarray(var[order])
        self.transmat_, self.startprob_ = np.ascontiguousarray(A[order][:, order]), np.ascontiguousarray(pi[order])
        self.labels_, self.gamma_ = rank[labels].astype(np.int32), np.ascontiguousarray(gamma[:, order])
        self.loglik_, self.n_iter_, self.converged_ = float(info.loglik), int(info.n_iter), bool(info.converged)
        self.init_labels_, self.n_samples_, self.n_features_, self.seq_start_ = lab0, int(labels.shape[0]), d, seq
        return order

    def fit(self, x, lengths):
        b, k = self._b, self.n_states
        xa = b.asarray(x)
        n, d = (int(v) for v in xa.shape)
        seq = seq_start(lengths, n)
        if k > n:
            raise ValueError(f"n_states = {k} exceeds the {n} rows")
        if d > _hip.HMM_MAX_D:
            raise ValueError(f"{d} features: the HMM takes up to {_hip.HMM_MAX_D}")
        colvar = float(np.asarray(b.to_numpy(xa), np.float64).var(0).mean())
        self.min_var_ = 1e-3 * colvar if self.min_var is None else self.min_var
        km, onehot, A, pi = self._start(xa, seq)
        mu, var, _ = b.hmm_mstep(xa, onehot, km.cluster_centers_, np.full((k, d), max(colvar, self.min_var_, 1e-30), np.float32), self.min_var_, 0.5)
        mu, var, A, pi, gamma, labels, info = b.hmm_fit(xa, seq, mu, var, A, pi, self.max_iter, self.tol, self.prior, self.kappa, self.min_var_, MIN_WEIGHT)
        self._fitted(mu, var, A, pi, gamma, labels, info, km.labels_, seq, d)
        return self

    def _logb(self, x, lengths):
        if not hasattr(self, "means_"):
            raise ValueError("this GaussianHMM is not fitted")
        xa = self._b.asarray(x)
        if xa.shape[1] != self.n_features_:
            raise ValueError(f"expected {self.n_features_} features, got {xa.shape[1]}")
        return self._b.hmm_emission(xa, self.means_, self.vars_), seq_start(lengths, int(xa.shape[0]))

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

    def scored_rows(self, lengths) -> int:
        """The rows of sequences of `lengths` that a likelihood counts: what a likelihood per step is divided by."""
        return int(sum(lengths))


def fit_split(read, make, holdout):
    """The fit both sequence models run over roll-outs: `read()` -> (clip numbers, features, the feature's name), `make()` -> the model.  With
    holdout = h >= 2 the clips at the positions p, p % h == h - 1, are left out of the fit and scored.  -> (model, feats); the model gains
    clips_, feature_, train_, heldout_ and loglik_per_step_train_ / _heldout_ (None without held-out clips), per row of model.scored_rows."""
    holdout = int(holdout)
    if holdout < 0 or holdout == 1:
        raise ValueError(f"holdout must be 0 (no clip held out) or >= 2 (got {holdout})")
    ids, feats, feature = read()
    held = [p for p in range(len(ids)) if holdout and p % holdout == holdout - 1]
    train = [p for p in range(len(ids)) if p not in held]
    if not train or (holdout and not held):
        raise ValueError(f"holdout = {holdout} over {len(ids)} clips leaves no {'training' if not train else 'held-out'} clip")
    model = make()
    lens = [feats[p].shape[0] for p in train]
    model.fit(np.concatenate([feats[p] for p in train], 0), lens)
    model.clips_, model.feature_, model.train_, model.heldout_ = ids, feature, train, held
    model.loglik_per_step_train_ = model.loglik_ / model.scored_rows(lens)
    model.loglik_per_step_heldout_ = None
    if held:
        lens = [feats[p].shape[0] for p in held]
        model.loglik_per_step_heldout_ = model.score(np.concatenate([feats[p] for p in held], 0), lens) / model.scored_rows(lens)
    return model, feats


def fit_rollouts(rollouts, feature: str = "intention", k: int = 32, max_iter: int = 50, tol: float = 1e-4, prior: float = 0.1, kappa: float = 0.0,
                 n_init: int = 4, seed: int = 0, holdout: int = 0, device="cuda", backend=None):
    """Fit `feature` (up to 1024 wide) over the roll-outs, each one sequence.  `rollouts`: a directory of clip_<i>.h5, or a list of roll-out dicts.
    With holdout = h >= 2 the clips at the positions p, p % h == h - 1, are left out of the fit and scored.
    -> (hmm, feats): feats[j] float32 [T_j, D] of roll-out j; hmm.clips_ are the clip numbers, hmm.train_ / hmm.heldout_ the positions fitted / scored,
    hmm.loglik_per_step_train_ / hmm.loglik_per_step_heldout_ (None without held-out clips)."""
    return fit_split(lambda: (*rollout_features(rollouts, lambda r, _, where: feature_of(r, feature, where), feature, "fit"), feature),
                     lambda: GaussianHMM(k, max_iter=max_iter, tol=tol, prior=prior, kappa=kappa, n_init=n_init, seed=seed, device=device, backend=backend), holdout)


def fitted_tree(model, feats, seed, posteriors: bool):
    """What hmm.h5 and arhmm.h5 share, from a fitted model and the features of every clip."""
    k, lens = model.n_states, [f.shape[0] for f in feats]
    allx = np.concatenate(feats, 0)
    lab, gam = split(model.predict(allx, lens), lens), split(model.predict_proba(allx, lens), lens)
    counts, trans, dwell = segment_summary(lab, k)
    _, _, dwell0 = segment_summary([model.init_labels_[s:e] for s, e in zip(model.seq_start_[:-1], model.seq_start_[1:])], k)
    tree = {"means": model.means_, "variances": model.vars_, "transmat": model.transmat_, "startprob": model.startprob_, "centroids": model.means_,
            "loglik": np.float64(model.loglik_), "loglik_per_step_train": np.float64(model.loglik_per_step_train_), "n_iter": np.int64(model.n_iter_),
            "converged": np.int64(model.converged_), "feature": model.feature_, "clips": np.asarray(model.clips_, np.int64), "seed": np.int64(seed),
            "counts": counts, "transitions": trans, "dwell_mean": dwell, "init_dwell_mean": dwell0, "labels": by_clip(model.clips_, lab, np.int32),
            "confidence": by_clip(model.clips_, [g[np.arange(len(v)), v] for v, g in zip(lab, gam)], np.float32)}
    if model.loglik_per_step_heldout_ is not None:
        tree["loglik_per_step_heldout"] = np.float64(model.loglik_per_step_heldout_)
    if posteriors:
        tree["gamma"] = by_clip(model.clips_, gam, np.float32)
    return tree


def summary_tail(model, tree, per: str, out) -> str:
    """The end of the summary line both tools print: the likelihoods per step, the dwell times, the file."""
    dwell, dwell0 = tree["dwell_mean"], tree["init_dwell_mean"]
    held = "" if model.loglik_per_step_heldout_ is None else f", {model.loglik_per_step_heldout_:.4f} on {len(model.heldout_)} held-out clips"
    return (f"{model.n_iter_} iterations{'' if model.converged_ else ' (not converged)'}, loglik per {per} {model.loglik_per_step_train_:.4f}{held}; mean dwell "
            f"{float(dwell[tree['counts'] > 0].mean()):.2f} steps (k-means start: {float(dwell0[dwell0 > 0].mean()):.2f}); wrote {out}")


def main(argv=None, backend=None) -> int:
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out", "k"), USAGE)
    if opts is None:
        return 2
    try:
        k, seed = int(opts["k"]), int(opts.get("seed", 0))
        posteriors = cli.flag(opts, "posteriors")
        hmm, feats = fit_rollouts(opts["rollouts"], opts.get("feature", "intention"), k, int(opts.get("max_iter", 50)), float(opts.get("tol", 1e-4)),
                                  float(opts.get("prior", 0.1)), float(opts.get("kappa", 0.0)), int(opts.get("n_init", 4)), seed, int(opts.get("holdout", 0)),
                                  backend=backend)
        tree = fitted_tree(hmm, feats, seed, posteriors)
    except (KeyError, ValueError) as e:
        return cli.report("hmm", e)
    cli.write(opts["out"], tree)
    print(f"[hmm] {hmm.feature_}: {hmm.n_samples_} samples x {hmm.n_features_} features from {len(hmm.train_)} clips into {k} states, "
          + summary_tail(hmm, tree, "step", opts["out"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
