"""k-means of recorded activations on the GPU (csrc/tmjx_kmeans.hip; DESIGN.md "Clustering"): the time steps of every clip clustered into motifs,
the ethogram of each clip, how often each motif occurs and which follows which.

    python -m track_mjx_amd.analysis.cluster rollouts=<dir of clip_<i>.h5> [feature=intention] k=32 [seed=0] [n_init=4] [max_iter=100] [tol=1e-4]
                                             out=<clusters.h5>

writes centroids [K, D], counts [K], transitions [K, K], dwell_mean [K], inertia, n_iter, feature, clips, seed, labels/clip_<i> int32 [T - 1] and
distances/clip_<i> float32 [T - 1] (the squared distance to the motif's centroid).  Motifs are numbered by descending count: motif 0 is the
commonest.  `python -m track_mjx_amd.analysis.rollout ... intervene_centroids=<clusters.h5>` takes the centroids as directions to push along.
"""
from __future__ import annotations

import sys

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import resolve
from .recorded import by_clip, feature_of, number_by_count, rollout_features, split

CLI_OPTIONS = ("rollouts", "out", "feature", "k", "seed", "n_init", "max_iter", "tol")
USAGE = ("usage: python -m track_mjx_amd.analysis.cluster rollouts=<dir of clip_<i>.h5> [feature=intention] k=32 [seed=0] [n_init=4] [max_iter=100] "
         "[tol=1e-4] out=<clusters.h5>")


class KMeans:
    """Lloyd's k-means with k-means++ seeding of [n, d] rows, d <= 1024, into n_clusters <= 256: `fit`, `predict`, `fit_predict`, and after a fit
    `cluster_centers_` [K, D], `labels_` [n] int32, `distances_` [n] float32 (squared, to the row's centroid), `inertia_`, `n_iter_`, `counts_` [K].
    The seeding uniforms are np.random.default_rng(seed).random((n_init, K)); the restart with the lowest inertia wins, the earlier one on a tie.
    Clusters are numbered by descending count (equal counts keep their order): cluster 0 is the commonest.  Inputs: numpy arrays, or torch device
    tensors (a row stride is fine).  Every run gives the same bits."""

    def __init__(self, n_clusters: int, n_init: int = 4, max_iter: int = 100, tol: float = 1e-4, seed: int = 0, device="cuda", backend=None):
        if not 1 <= int(n_clusters) <= _hip.KMEANS_MAX_K:
            raise ValueError(f"n_clusters must be in 1 .. {_hip.KMEANS_MAX_K} (got {n_clusters})")
        if int(n_init) < 1 or int(max_iter) < 1 or not float(tol) >= 0.0:
            raise ValueError(f"n_init and max_iter must be >= 1 and tol >= 0 (got {n_init}, {max_iter}, {tol})")
        self.n_clusters, self.n_init, self.max_iter, self.tol, self.seed = int(n_clusters), int(n_init), int(max_iter), float(tol), int(seed)
        self._b = resolve(backend, device)

    def fit(self, x):
        xa = self._b.asarray(x)
        n, d = (int(v) for v in xa.shape)
        k = self.n_clusters
        if k > n:
            raise ValueError(f"n_clusters = {k} exceeds the {n} rows")
        if d > _hip.KMEANS_MAX_D:
            raise ValueError(f"{d} features: k-means takes up to {_hip.KMEANS_MAX_D}")
        u = np.random.default_rng(self.seed).random((self.n_init, k))
        best = None
        for r in range(self.n_init):
            cen, self.seed_index_ = self._b.kmeans_seed(xa, k, u[r])
            cen, labels, dist2, info = self._b.kmeans_fit(xa, cen, self.max_iter, self.tol)
            if best is None or float(info.inertia) < best[3]:
                best = (cen, labels, dist2, float(info.inertia), int(info.n_iter), r)
        cen, labels, dist2, self.inertia_, self.n_iter_, self.best_init_ = best
        order, rank, self.counts_ = number_by_count(labels, k)
        self.cluster_centers_ = np.ascontiguousarray(cen[order])
        self.labels_, self.distances_ = rank[labels].astype(np.int32), dist2
        self.n_samples_, self.n_features_ = n, d
        return self

    def predict(self, x):
        if not hasattr(self, "cluster_centers_"):
            raise ValueError("this KMeans is not fitted")
        xa = self._b.asarray(x)
        if xa.shape[1] != self.n_features_:
            raise ValueError(f"expected {self.n_features_} features, got {xa.shape[1]}")
        return self._b.kmeans_assign(xa, self.cluster_centers_)[0]

    def fit_predict(self, x):
        return self.fit(x).labels_


def segment_summary(labels_per_clip, k: int):
    """-> (counts [K] int64; transitions [K, K] int64: the pairs t -> t + 1 inside a clip, never across a clip boundary; dwell_mean [K] float64: the
    mean run length in steps, 0 for a motif that never occurs)."""
    counts, trans, runs = np.zeros(k, np.int64), np.zeros((k, k), np.int64), np.zeros(k, np.int64)
    for lab in labels_per_clip:
        lab = np.asarray(lab, np.int64).reshape(-1)
        if lab.size == 0:
            continue
        if lab.min() < 0 or lab.max() >= k:
            raise ValueError(f"a label outside 0 .. {k - 1}")
        counts += np.bincount(lab, minlength=k)
        np.add.at(trans, (lab[:-1], lab[1:]), 1)
        starts = np.concatenate([[True], lab[1:] != lab[:-1]])
        runs += np.bincount(lab[starts], minlength=k)
    dwell = np.divide(counts, runs, out=np.zeros(k, np.float64), where=runs > 0)
    return counts, trans, dwell


def fit_rollouts(rollouts, feature: str = "intention", k: int = 32, n_init: int = 4, max_iter: int = 100, tol: float = 1e-4, seed: int = 0, device="cuda",
                 backend=None):
    """Cluster `feature` (up to 1024 wide) over every roll-out.  `rollouts`: a directory of clip_<i>.h5, or a list of roll-out dicts.
    -> (kmeans, labels, distances): labels[j] int32 [T_j] and distances[j] float32 [T_j] of roll-out j; kmeans.clips_ are the clip numbers."""
    ids, feats = rollout_features(rollouts, lambda r, _, where: feature_of(r, feature, where), feature, "cluster")
    km = KMeans(k, n_init=n_init, max_iter=max_iter, tol=tol, seed=seed, device=device, backend=backend)
    km.fit(km._b.asarray(np.concatenate(feats, 0)))
    km.clips_, km.feature_ = ids, feature
    lens = [f.shape[0] for f in feats]
    return km, split(km.labels_, lens), split(km.distances_, lens)


def main(argv=None, backend=None) -> int:
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out", "k"), USAGE)
    if opts is None:
        return 2
    feature = opts.get("feature", "intention")
    try:
        k, seed = int(opts["k"]), int(opts.get("seed", 0))
        km, labels, dists = fit_rollouts(opts["rollouts"], feature, k, int(opts.get("n_init", 4)), int(opts.get("max_iter", 100)), float(opts.get("tol", 1e-4)),
                                         seed, backend=backend)
    except (KeyError, ValueError) as e:
        return cli.report("cluster", e)
    counts, trans, dwell = segment_summary(labels, k)
    cli.write(opts["out"], {"centroids": km.cluster_centers_, "counts": counts, "transitions": trans, "dwell_mean": dwell, "inertia": np.float64(km.inertia_),
                            "n_iter": np.int64(km.n_iter_), "feature": feature, "clips": np.asarray(km.clips_, np.int64), "seed": np.int64(seed),
                            "labels": by_clip(km.clips_, labels, np.int32), "distances": by_clip(km.clips_, dists, np.float32)})
    top = ", ".join(f"{c}" for c in counts[:5])
    print(f"[cluster] {feature}: {km.n_samples_} samples x {km.n_features_} features from {len(labels)} clips into {k} motifs, {km.n_iter_} iterations "
          f"(restart {km.best_init_} of {km.n_init}), inertia {km.inertia_:.6g}; the commonest motifs hold {top} steps; mean dwell "
          f"{float(dwell[counts > 0].mean()):.2f} steps; wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
