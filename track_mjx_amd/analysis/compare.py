"""How two recorded representations relate, on the GPU: linear CKA, the correlation of representational dissimilarity matrices and canonical
correlations (csrc/tmjx_compare.hip; DESIGN.md "Representation comparison").

Two networks (MLP against LSTM decoder, a new encoder on a frozen decoder, with and without domain randomisation), two layers of one network, or
a layer against the kinematics or the motif labels of the same time steps: rows are paired by clip and time step, and every pair of features
gets a linear CKA (every paired row) and the Pearson correlation of the two dissimilarity matrices' upper triangles (a sorted sample of rows
without replacement, at most 32 768: the all-pairs kernel writes neither matrix).  One pair can also get its canonical correlations.

    python -m track_mjx_amd.analysis.compare a=<dir of clip_<i>.h5> [b=<dir>] features_a=intention,decoder/layer_0 [features_b=...]
        [cols_a=a:b] [cols_b=a:b] [labels=<clusters.h5>] [metric=correlation] [max_rows=20000] [seed=0] [cca=intention:intention] [var_keep=0.99]
        out=<compare.h5>

A feature is anything analysis.pca takes as a feature or analysis.readout as a target (`qposes_rollout` with cols=7:, `ctrl`,
`rollout_metrics/<name>`, ...); `b` omitted compares side a with itself, and features_b omitted repeats features_a.  Writes features_a,
features_b, clips, rows, row_index, cka [A, B], rdm_corr [A, B], rdm_metric and, for the cca= pair, rho, svcca, directions_a, directions_b, kx, ky
and feature, mean, components [r, d1] (the orthonormalised directions_a), so that analysis.rollout intervene_pca=<compare.h5> projects out of
network a the subspace it shares with network b.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import resolve
from .recorded import columns, feature_of, labels_file, rollout_features, target_of

CLI_OPTIONS = ("a", "b", "features_a", "features_b", "cols_a", "cols_b", "labels", "metric", "max_rows", "seed", "cca", "var_keep", "out")
USAGE = ("usage: python -m track_mjx_amd.analysis.compare a=<dir of clip_<i>.h5> [b=<dir>] features_a=<f1,f2,...> [features_b=...] [cols_a=a:b] [cols_b=a:b] "
         "[labels=<clusters.h5>] [metric=correlation|euclidean|sqeuclidean] [max_rows=20000] [seed=0] [cca=<fa>:<fb>] [var_keep=0.99] out=<compare.h5>")
METRICS = {"sqeuclidean": _hip.COMPARE_SQEUCLIDEAN, "euclidean": _hip.COMPARE_EUCLIDEAN, "correlation": _hip.COMPARE_CORRELATION, "labels": _hip.COMPARE_LABEL}
LABELS = "labels"      # the name of the motif-label feature that labels= adds to side a


def cka_of(norms) -> float:
    """Linear CKA from tmjx_cka_linear's three norms; NaN, with a warning, where a side has no variance."""
    xy, xx, yy = (float(v) for v in norms)
    if not (xx > 0.0 and yy > 0.0):
        warnings.warn("linear CKA of a representation without variance is undefined: NaN", RuntimeWarning, stacklevel=2)
        return float("nan")
    return xy / np.sqrt(xx * yy)


def pearson_of(sums, n: int) -> float:
    """The Pearson correlation of the two dissimilarity matrices' upper triangles from tmjx_rdm_corr's five sums over the n (n - 1) / 2 pairs; NaN,
    with a warning, where a matrix is constant."""
    sx, sy, sxx, syy, sxy = (float(v) for v in sums)
    pairs = n * (n - 1) / 2.0
    vx, vy, cov = sxx - sx * sx / pairs, syy - sy * sy / pairs, sxy - sx * sy / pairs
    if not (vx > 0.0 and vy > 0.0):
        warnings.warn("a dissimilarity matrix is constant: its correlation is undefined: NaN", RuntimeWarning, stacklevel=2)
        return float("nan")
    return cov / np.sqrt(vx * vy)


def orthonormal_rows(directions) -> np.ndarray:
    """The float64 Gram-Schmidt orthonormalisation, in order, of the rows of `directions` (twice through, for the rounding of the first pass); a row
    inside the span of the rows before it comes out as zeros."""
    q = np.array(directions, np.float64)
    for i in range(q.shape[0]):
        scale = np.linalg.norm(q[i])
        for _ in range(2):
            for j in range(i):
                q[i] -= (q[i] @ q[j]) * q[j]
        norm = np.linalg.norm(q[i])
        q[i] = q[i] / norm if norm > 1e-12 * scale and norm > 0.0 else 0.0
    return q


class Comparison:
    """Measures between [n, d1] and [n, d2] rows of the same n time steps (d <= 1024): `cka(x, y)`, `rdm_corr(x, y, metric_x, metric_y)` (n <=
    32 768; metrics by name: sqeuclidean, euclidean, correlation, labels) and `cca(x, y, var_keep, max_rank)` -> (rho, a, b) with `kx_`, `ky_`,
    `sweeps_` set.  Inputs: numpy arrays, or torch device tensors (a row stride is kept)."""

    def __init__(self, device="cuda", backend=None):
        self._b = resolve(backend, device)

    def _rows(self, x):
        return self._b.asarray(x[:, None] if getattr(x, "ndim", 2) == 1 else x)

    def cka_norms(self, x, y):
        return self._b.cka_linear(self._rows(x), self._rows(y))

    def cka(self, x, y) -> float:
        return cka_of(self.cka_norms(x, y))

    def rdm_sums(self, x, y, metric_x="correlation", metric_y="correlation"):
        for m in (metric_x, metric_y):
            if m not in METRICS:
                raise ValueError(f"unknown metric {m!r}: one of {', '.join(METRICS)}")
        xa, ya = self._rows(x), self._rows(y)
        if xa.shape[0] > _hip.COMPARE_MAX_N:
            raise ValueError(f"{xa.shape[0]} rows: the dissimilarity matrices take up to {_hip.COMPARE_MAX_N} (sample them)")
        return self._b.rdm_corr(xa, METRICS[metric_x], ya, METRICS[metric_y])

    def rdm_corr(self, x, y, metric_x="correlation", metric_y="correlation") -> float:
        return pearson_of(self.rdm_sums(x, y, metric_x, metric_y), int(np.shape(x)[0]))

    def cca(self, x, y, var_keep=0.99, max_rank=_hip.COMPARE_MAX_RANK):
        rho, a, b, info = self._b.cca(self._rows(x), self._rows(y), var_keep, max_rank)
        self.kx_, self.ky_, self.sweeps_ = int(info.kx), int(info.ky), int(info.sweeps)
        self.pca_ms_, self.cross_ms_, self.svd_ms_ = float(info.pca_ms), float(info.cross_ms), float(info.svd_ms)
        return rho, a, b


def _series_of(rollout, name: str, where: str) -> np.ndarray:
    """A feature of analysis.pca or a target of analysis.readout of one roll-out, [rows, D] float32."""
    try:
        return feature_of(rollout, name, where)
    except KeyError as first:
        try:
            return target_of(rollout, name, where)
        except KeyError:
            raise first from None


def _metric_for(name: str, width: int, metric: str) -> str:
    """The metric a feature gets: labels for the motif labels, the tool's metric otherwise (Euclidean where one column cannot be correlated)."""
    if name == LABELS:
        return "labels"
    return "euclidean" if metric == "correlation" and width < 2 else metric


def _side(rollouts, names, cols, labels_of=None):
    """-> {clip: [the [T, D] float32 series of every name]}; `labels_of`: {clip: int labels [T]} adds the LABELS feature."""
    def read(r, clip, where):
        out = []
        for name in names:
            if name == LABELS:
                if clip not in labels_of:
                    raise KeyError(f"the labels file has no clip_{clip}")
                out.append(np.asarray(labels_of[clip], np.float32).reshape(-1, 1))
                continue
            a = _series_of(r, name, where)
            out.append(np.ascontiguousarray(a[:, columns(cols, a.shape[1])]))
        return out
    ids, items = rollout_features(rollouts, read, None, "compare")
    return dict(zip(ids, items))


def compare_rollouts(a, b=None, features_a=("intention",), features_b=None, cols_a=None, cols_b=None, labels=None, metric="correlation", max_rows=20000,
                     seed=0, cca=None, var_keep=0.99, device="cuda", backend=None) -> dict:
    """Compare every feature of side `a` with every feature of side `b` (a directory of clip_<i>.h5 or a list of roll-out dicts each; b=None: side
    a itself).  Rows are paired by clip and time step: the clips present on both sides, the first min(T_a, T_b) rows of each, and within a side
    the rows every feature has (a per-frame series such as qposes_rollout drops its extra last row).  -> the dict the command line writes."""
    if metric not in METRICS or metric == "labels":
        raise ValueError(f"metric = {metric!r}: one of sqeuclidean, euclidean, correlation")
    max_rows = int(max_rows)
    if max_rows > _hip.COMPARE_MAX_N:
        raise ValueError(f"max_rows = {max_rows} exceeds the {_hip.COMPARE_MAX_N} rows the dissimilarity matrices take")
    if max_rows < 3:
        raise ValueError(f"max_rows must be >= 3 (got {max_rows})")
    fa = [f for f in features_a if f]
    fb = list(fa) if features_b is None else [f for f in features_b if f]
    if labels is not None:
        fa = fa + [LABELS]
    if not fa or not fb:
        raise ValueError("no feature to compare")
    lab = None if labels is None else (labels_file(labels) if isinstance(labels, (str, os.PathLike)) else dict(labels))
    side_a = _side(a, fa, cols_a, lab)
    side_b = side_a if b is None and fb == fa and cols_b == cols_a else _side(a if b is None else b, fb, cols_b, lab)
    clips = sorted(set(side_a) & set(side_b))
    if not clips:
        raise ValueError("the two sides share no clip")
    rows_a, rows_b, counts = [[] for _ in fa], [[] for _ in fb], []
    for c in clips:
        t = min(min(s.shape[0] for s in side_a[c]), min(s.shape[0] for s in side_b[c]))
        counts.append(t)
        for k, s in enumerate(side_a[c]):
            rows_a[k].append(s[:t])
        for k, s in enumerate(side_b[c]):
            rows_b[k].append(s[:t])
    xa = [np.ascontiguousarray(np.concatenate(r, 0), np.float32) for r in rows_a]
    xb = [np.ascontiguousarray(np.concatenate(r, 0), np.float32) for r in rows_b]
    n = int(sum(counts))
    if n < 3:
        raise ValueError(f"{n} paired rows: a comparison needs at least 3")
    for name, x in zip(fa + fb, xa + xb):
        if x.shape[1] > _hip.COMPARE_MAX_D:
            raise ValueError(f"{name} is {x.shape[1]} wide: a comparison takes up to {_hip.COMPARE_MAX_D} features, pick columns with cols_a / cols_b")
    cmp_ = Comparison(device=device, backend=backend)
    bk = cmp_._b
    index = np.sort(np.random.default_rng(int(seed)).choice(n, size=min(max_rows, n), replace=False)).astype(np.int64)
    da, db = [bk.asarray(x) for x in xa], [bk.asarray(x) for x in xb]
    sa, sb = [bk.asarray(x[index]) for x in xa], [bk.asarray(x[index]) for x in xb]
    cka, rdm = np.full((len(fa), len(fb)), np.nan), np.full((len(fa), len(fb)), np.nan)
    for i, na in enumerate(fa):
        for j, nb in enumerate(fb):
            if na != LABELS:      # (CKA of integer labels means nothing: NaN)
                cka[i, j] = cka_of(bk.cka_linear(da[i], db[j]))
            ma, mb = _metric_for(na, xa[i].shape[1], metric), _metric_for(nb, xb[j].shape[1], metric)
            rdm[i, j] = pearson_of(bk.rdm_corr(sa[i], METRICS[ma], sb[j], METRICS[mb]), index.shape[0])
    out = {"features_a": ",".join(fa), "features_b": ",".join(fb), "clips": np.asarray(clips, np.int64), "rows": np.asarray(counts, np.int64),
           "row_index": index, "cka": cka, "rdm_corr": rdm, "rdm_metric": metric}
    if cca:
        na, _, nb = str(cca).partition(":")
        nb = nb or na
        if na not in fa or nb not in fb or na == LABELS:
            raise ValueError(f"cca = {cca}: expected <a feature of side a>:<a feature of side b> (of {', '.join(fa)} : {', '.join(fb)})")
        i, j = fa.index(na), fb.index(nb)
        rho, wa, wb = cmp_.cca(da[i], db[j], float(var_keep))
        out.update({"rho": rho, "svcca": np.float64(rho.astype(np.float64).mean()), "directions_a": wa, "directions_b": wb, "kx": np.int64(cmp_.kx_),
                    "ky": np.int64(cmp_.ky_), "feature": na, "mean": xa[i].astype(np.float64).mean(0).astype(np.float32),
                    "components": orthonormal_rows(wa).astype(np.float32), "cca_features": f"{na}:{nb}"})
    return out


def main(argv=None, backend=None) -> int:
    opts = cli.parse(argv, CLI_OPTIONS, ("a", "features_a", "out"), USAGE)
    if opts is None:
        return 2
    try:
        res = compare_rollouts(opts["a"], opts.get("b"), opts["features_a"].split(","), opts["features_b"].split(",") if "features_b" in opts else None,
                               opts.get("cols_a"), opts.get("cols_b"), opts.get("labels"), opts.get("metric", "correlation"), int(opts.get("max_rows", 20000)),
                               int(opts.get("seed", 0)), opts.get("cca"), float(opts.get("var_keep", 0.99)), backend=backend)
    except (KeyError, ValueError) as e:
        return cli.report("compare", e)
    cli.write(opts["out"], res)
    fa, fb = res["features_a"].split(","), res["features_b"].split(",")
    best = ", ".join(f"{a} ~ {fb[int(np.nanargmax(res['cka'][i]))]} {np.nanmax(res['cka'][i]):.3f}" for i, a in enumerate(fa) if np.isfinite(res["cka"][i]).any())
    tail = f"; cca {res['cca_features']}: {res['kx']} x {res['ky']} kept, svcca {float(res['svcca']):.4f}" if "rho" in res else ""
    print(f"[compare] {len(fa)} x {len(fb)} features over {int(res['rows'].sum())} paired rows of {len(res['clips'])} clips, {res['row_index'].shape[0]} rows "
          f"in the dissimilarity matrices ({res['rdm_metric']}); best CKA {best}{tail}; wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
