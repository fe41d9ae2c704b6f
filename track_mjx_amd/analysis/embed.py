"""A behaviour map of recorded features on the GPU (csrc/tmjx_tsne.hip; DESIGN.md "Behaviour map"): the time steps of every clip embedded in two
dimensions by exact t-SNE, the density of the map, its watershed regions, and the region of every time step.

    python -m track_mjx_amd.analysis.embed rollouts=<dir of clip_<i>.h5> [feature=intention] [perplexity=30] [max_train=20000] [n_iter=750]
                                           [grid=256] [sigma=<in map units>] out=<map.h5>

`rollouts` is a roll-out directory or a spectrogram directory (analysis.spectrogram writes the same clip_<i>.h5 layout).  Writes
embedding/clip_<i> float32 [T - 1, 2], train_index, kl, density [G, G], regions int32 [G, G], extent [4], labels/clip_<i> int32 [T - 1],
counts [K], transitions [K, K], dwell_mean [K] (analysis.cluster.segment_summary), centroids [K, D] (the mean feature row of every region),
feature and clips.  Regions are numbered by descending count of time steps: region 0 is the commonest.
`python -m track_mjx_amd.analysis.rollout ... intervene_centroids=<map.h5>` takes the file as it takes a clusters.h5.
"""
from __future__ import annotations

import sys

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import resolve
from .cluster import segment_summary
from .recorded import by_clip, feature_of, rollout_features, split

CLI_OPTIONS = ("rollouts", "out", "feature", "perplexity", "max_train", "n_iter", "grid", "sigma")
USAGE = ("usage: python -m track_mjx_amd.analysis.embed rollouts=<dir of clip_<i>.h5> [feature=intention] [perplexity=30] [max_train=20000] [n_iter=750] "
         "[grid=256] [sigma=<in map units>] out=<map.h5>")
INIT_STD = 1e-4


def symmetric_csr(idx, p):
    """P = (Pc + Pc^T) / 2n from the neighbour lists idx [n, k] and the conditional rows p [n, k] -> (row_ptr int32 [n + 1], col int32 [nnz] ascending
    in a row, val float32 [nnz]).  Float32, in a fixed order: the pair (i, j) is p_ij + p_ji (the entry of the lower row first) over 2n.  An index
    outside [0, n) is dropped."""
    idx, p = np.asarray(idx, np.int64), np.asarray(p, np.float32)
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols, vals = idx.reshape(-1), p.reshape(-1)
    ok = (cols >= 0) & (cols < n)
    rows, cols, vals = rows[ok], cols[ok], vals[ok]
    key = np.concatenate([rows * n + cols, cols * n + rows])
    val = np.concatenate([vals, vals])
    order = np.argsort(key, kind="stable")
    key, val = key[order], val[order]
    first = np.concatenate([[True], key[1:] != key[:-1]]) if key.size else np.zeros(0, bool)
    starts = np.flatnonzero(first)
    total = np.add.reduceat(val, starts).astype(np.float32) if key.size else val      # (at most two terms a pair: one float32 add)
    ukey = key[starts]
    row_ptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(ukey // n, minlength=n), out=row_ptr[1:])
    return row_ptr, (ukey % n).astype(np.int32), (total / np.float32(2 * n)).astype(np.float32)


class TSNE:
    """Exact t-SNE of [n, d] rows, d <= 1024, in two dimensions: `fit`, `transform`, and after a fit `embedding_` [n_train, 2] float32, `train_index_`
    (the rows that trained), `kl_`, `beta_` [n_train], `n_iter_`.  Every s-th row trains, s the smallest stride that leaves at most `max_train`
    (<= 65536) rows; each has k = min(3 perplexity, n_train - 1, 128) exact neighbours; the start is the first two principal components scaled to a
    standard deviation of 1e-4: no random numbers, the same bits on every run.  `transform` places rows at the affinity-weighted mean of their
    nearest training rows.  Inputs: numpy arrays, or torch device tensors (a row stride is fine)."""

    def __init__(self, perplexity: float = 30, n_iter: int = 750, exaggeration: float = 12, exaggeration_iters: int = 250, eta="auto", max_train: int = 20000,
                 momentum_early: float = 0.5, momentum_late: float = 0.8, min_gain: float = 0.01, device="cuda", backend=None):
        if not float(perplexity) >= 1.0 or int(n_iter) < 0 or int(exaggeration_iters) < 0 or not float(exaggeration) > 0:
            raise ValueError(f"perplexity must be >= 1, n_iter and exaggeration_iters >= 0, exaggeration > 0 (got {perplexity}, {n_iter}, {exaggeration_iters}, "
                             f"{exaggeration})")
        if not 2 <= int(max_train) <= _hip.TSNE_MAX_N:
            raise ValueError(f"max_train must be in 2 .. {_hip.TSNE_MAX_N} (got {max_train})")
        if eta != "auto" and not float(eta) > 0:
            raise ValueError(f"eta must be 'auto' or positive (got {eta})")
        self.perplexity, self.n_iter, self.exaggeration, self.exaggeration_iters = float(perplexity), int(n_iter), float(exaggeration), int(exaggeration_iters)
        self.eta, self.max_train, self.min_gain = eta, int(max_train), float(min_gain)
        self.momentum_early, self.momentum_late = float(momentum_early), float(momentum_late)
        self._b = resolve(backend, device)

    def _neighbours(self, n_train):
        k = min(int(3 * self.perplexity), n_train - 1, _hip.TSNE_MAX_K)
        if not self.perplexity < k:
            raise ValueError(f"perplexity = {self.perplexity:g} needs more than {k} neighbours ({n_train} training rows, at most {_hip.TSNE_MAX_K} neighbours)")
        return k

    def initial(self, xt):
        """The start: the first two principal components of the training rows, scaled so that the first has standard deviation 1e-4."""
        b = self._b
        mean, comp, _, _ = b.fit_wide(xt)
        proj = np.asarray(b.to_numpy(b.transform_wide(xt, mean, comp[:2])), np.float64)
        if proj.shape[1] < 2:
            proj = np.concatenate([proj, np.zeros((proj.shape[0], 2 - proj.shape[1]))], 1)
        std = proj[:, 0].std()
        return np.ascontiguousarray(proj / (std if std > 0 else 1.0) * INIT_STD, np.float32)

    def fit(self, x, lengths=None):
        b = self._b
        xa = b.asarray(x)
        n_all, d = (int(v) for v in xa.shape)
        if lengths is not None and int(np.sum(lengths)) != n_all:
            raise ValueError(f"lengths sum to {int(np.sum(lengths))}, x has {n_all} rows")
        if d > _hip.TSNE_MAX_D:
            raise ValueError(f"{d} features: the behaviour map takes up to {_hip.TSNE_MAX_D}")
        s = -(-n_all // self.max_train)
        xt = xa[::s]
        n = int(xt.shape[0])
        if n < 3:
            raise ValueError(f"{n} training rows: the behaviour map needs at least 3")
        k = self._neighbours(n)
        idx, dist2 = b.knn(xt, None, k, exclude_self=True)
        p, beta = b.tsne_affinities(dist2, self.perplexity)
        self.csr_ = symmetric_csr(idx, p)
        eta = max(n / self.exaggeration / 4.0, 50.0) if self.eta == "auto" else float(self.eta)
        y, _, _, info = b.tsne_fit(self.initial(xt), self.csr_, self.n_iter, self.exaggeration, min(self.exaggeration_iters, self.n_iter), self.momentum_early,
                                   self.momentum_late, eta, self.min_gain)
        self.embedding_, self.train_index_, self.kl_, self.beta_ = y, np.arange(0, n_all, s, dtype=np.int64), float(info.kl), beta
        self.z_, self.n_iter_, self.eta_, self.n_neighbours_, self.info_ = float(info.z), int(info.n_iter), eta, k, info
        self._train, self.n_features_, self.n_samples_ = xt, d, n_all
        return self

    def transform(self, x):
        """-> [m, 2] float32: every row at the affinity-weighted mean of its k nearest training rows on the map."""
        if not hasattr(self, "embedding_"):
            raise ValueError("this TSNE is not fitted")
        b = self._b
        xa = b.asarray(x)
        if xa.shape[1] != self.n_features_:
            raise ValueError(f"expected {self.n_features_} features, got {xa.shape[1]}")
        idx, dist2 = b.knn(self._train, xa, self.n_neighbours_)
        p, _ = b.tsne_affinities(dist2, self.perplexity)
        return b.tsne_place(idx, p, self.embedding_)

    def fit_transform(self, x, lengths=None):
        """The map position of every row of x: the embedding for the rows that trained, the placement for the others."""
        out = self.fit(x, lengths).transform(x)
        out[self.train_index_] = self.embedding_
        return out


# ---------------------------------------------------------------------------------------------------------------- the map (host numpy)
def density_map(y, grid: int = 256, sigma: float | None = None, extent=None):
    """-> (density float64 [grid, grid], extent (x0, x1, y0, y1), counts int64 [grid, grid]).  counts is the histogram of the points y [n, 2]
    (cell [iy, ix]), density its separable Gaussian blur with standard deviation sigma in map units (default: 1/32 of the larger span), in points per
    cell: it sums to n, the default extent being the data's box padded by the kernel's reach."""
    y = np.asarray(y, np.float64)
    if y.ndim != 2 or y.shape[1] != 2 or y.shape[0] < 1 or int(grid) < 2:
        raise ValueError(f"expected points [n, 2] and grid >= 2 (got shape {y.shape}, grid {grid})")
    lo, hi = y.min(0), y.max(0)
    span = float(max(hi[0] - lo[0], hi[1] - lo[1], 1e-12))
    sigma = span / 32.0 if sigma is None else float(sigma)
    if not sigma > 0:
        raise ValueError(f"sigma must be positive (got {sigma})")
    if extent is None:
        # the kernel reaches 4 sigma: pad by that and one cell of the padded box, so that no mass leaves the grid
        pad = 4.0 * sigma
        side = (span + 2 * pad) * (1.0 + 4.0 / grid)
        cx, cy = 0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1])
        extent = (cx - side / 2, cx + side / 2, cy - side / 2, cy + side / 2)
    x0, x1, y0, y1 = (float(v) for v in extent)
    dx, dy = (x1 - x0) / grid, (y1 - y0) / grid
    counts = np.zeros((grid, grid), np.int64)
    np.add.at(counts, cells(y, grid, extent), 1)
    out = counts.astype(np.float64)
    for axis, step in ((1, dx), (0, dy)):
        r = int(np.ceil(4.0 * sigma / step))
        t = np.arange(-r, r + 1) * step
        kern = np.exp(-0.5 * (t / sigma) ** 2)
        kern /= kern.sum()
        out = np.apply_along_axis(lambda v: np.convolve(v, kern, mode="same"), axis, out)
    return out, (x0, x1, y0, y1), counts


def cells(y, grid: int, extent):
    """-> (iy, ix): the cell of every point, clipped to the grid."""
    y = np.asarray(y, np.float64)
    x0, x1, y0, y1 = extent
    ix = np.clip(np.floor((y[:, 0] - x0) / (x1 - x0) * grid).astype(np.int64), 0, grid - 1)
    iy = np.clip(np.floor((y[:, 1] - y0) / (y1 - y0) * grid).astype(np.int64), 0, grid - 1)
    return iy, ix


def watershed(density, counts=None):
    """-> regions int32 [G, H]: every cell of positive density goes to the local maximum that steepest ascent over its 8 neighbours reaches (the
    greatest neighbour; among equal values, its own included, the first in row-major order, so that a plateau is one maximum); a cell of density
    <= 0 is -1.  Regions are numbered by descending weight, equal weights in row-major order of their maxima: the weight of a region is the sum of `counts`
    (the time steps per cell) over it, or of the density without counts."""
    d = np.asarray(density, np.float64)
    G, H = d.shape
    pad = np.full((G + 2, H + 2), -np.inf)
    pad[1:-1, 1:-1] = d
    best, arg = d.copy(), np.arange(G * H, dtype=np.int64).reshape(G, H)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di == 0 and dj == 0:
                continue
            nb = pad[1 + di:1 + di + G, 1 + dj:1 + dj + H]
            ii, jj = np.arange(G)[:, None] + di, np.arange(H)[None, :] + dj
            better = (nb > best) | ((nb == best) & (ii * H + jj < arg))
            best = np.where(better, nb, best)
            arg = np.where(better, ii * H + jj, arg)
    ptr = arg.reshape(-1)
    while True:
        nxt = ptr[ptr]
        if (nxt == ptr).all():
            break
        ptr = nxt
    live = (d > 0).reshape(-1)
    weight = (np.asarray(counts, np.float64) if counts is not None else d).reshape(-1)
    roots = np.unique(ptr[live])
    mass = np.array([weight[live & (ptr == r)].sum() for r in roots])
    order = np.argsort(-mass, kind="stable")
    number = np.full(G * H, -1, np.int64)
    number[roots[order]] = np.arange(len(roots))
    out = np.where(live, number[ptr], -1)
    return out.reshape(G, H).astype(np.int32)


def region_labels(regions, y, extent):
    """-> int32 [n]: the region of every point."""
    iy, ix = cells(y, regions.shape[0], extent)
    return np.asarray(regions)[iy, ix].astype(np.int32)


def map_rollouts(rollouts, feature: str = "intention", perplexity: float = 30, max_train: int = 20000, n_iter: int = 750, grid: int = 256, sigma=None,
                 device="cuda", backend=None):
    """Embed `feature` (up to 1024 wide) over every roll-out and cut the map into regions.  `rollouts`: a directory of clip_<i>.h5, or a list of
    roll-out dicts.  -> (tsne, result): result has embedding[j] [T_j, 2] and labels[j] int32 [T_j] of roll-out j, density, regions, extent, counts,
    transitions, dwell_mean and centroids; tsne.clips_ are the clip numbers."""
    ids, feats = rollout_features(rollouts, lambda r, _, where: feature_of(r, feature, where), feature, "embed")
    x, lens = np.concatenate(feats, 0), [f.shape[0] for f in feats]
    tsne = TSNE(perplexity, n_iter=n_iter, max_train=max_train, device=device, backend=backend)
    emb = np.asarray(tsne.fit_transform(x, lens), np.float32)
    tsne.clips_, tsne.feature_ = ids, feature
    density, extent, hist = density_map(emb, grid, sigma)
    regions = watershed(density, hist)
    labels = region_labels(regions, emb, extent)
    K = int(regions.max()) + 1
    counts, trans, dwell = segment_summary(split(labels, lens), K)
    x64 = np.asarray(x, np.float64)
    centroids = np.stack([x64[labels == j].mean(0) if counts[j] else np.zeros(x.shape[1]) for j in range(K)]).astype(np.float32)
    return tsne, {"embedding": split(emb, lens), "labels": split(labels, lens), "density": density, "regions": regions, "extent": np.asarray(extent, np.float64),
                  "counts": counts, "transitions": trans, "dwell_mean": dwell, "centroids": centroids}


def main(argv=None, backend=None) -> int:
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out"), USAGE)
    if opts is None:
        return 2
    feature = opts.get("feature", "intention")
    try:
        tsne, res = map_rollouts(opts["rollouts"], feature, float(opts.get("perplexity", 30)), int(opts.get("max_train", 20000)), int(opts.get("n_iter", 750)),
                                 int(opts.get("grid", 256)), float(opts["sigma"]) if "sigma" in opts else None, backend=backend)
    except (KeyError, ValueError) as e:
        return cli.report("embed", e)
    cli.write(opts["out"], {"embedding": by_clip(tsne.clips_, res["embedding"], np.float32), "train_index": tsne.train_index_, "kl": np.float64(tsne.kl_),
                            "density": res["density"], "regions": res["regions"], "extent": res["extent"], "labels": by_clip(tsne.clips_, res["labels"], np.int32),
                            "counts": res["counts"], "transitions": res["transitions"], "dwell_mean": res["dwell_mean"], "centroids": res["centroids"],
                            "feature": feature, "clips": np.asarray(tsne.clips_, np.int64), "perplexity": np.float64(tsne.perplexity)})
    print(f"[embed] {feature}: {tsne.n_samples_} samples x {tsne.n_features_} features from {len(res['labels'])} clips, {len(tsne.train_index_)} trained "
          f"({tsne.n_neighbours_} neighbours, {tsne.n_iter_} iterations, kl {tsne.kl_:.4f}); {len(res['counts'])} regions, the commonest hold "
          f"{', '.join(str(c) for c in res['counts'][:5])} steps; wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
