"""PCA of recorded activations on the GPU (csrc/tmjx_pca.hip; DESIGN.md "PCA").

Reference: track_mjx/analysis/render.py fits sklearn's PCA on a recorded feature (the intention, ctrl or a layer) over many clips and plots the
first components of one clip against the timestep.  Here the fit is two passes over the rows and, for features up to 128 wide, one workgroup of
Jacobi rotations; wider features (the 256- to 1024-wide layers, the LSTM carry), up to 1024, go through block Jacobi on the covariance in global
memory (csrc/tmjx_pca_wide.hip), whose inner solver is that same workgroup.

    python -m track_mjx_amd.analysis.pca rollouts=<dir of clip_<i>.h5> [feature=intention] [n_components=4] out=<pca.h5>

writes mean, components, explained_variance, explained_variance_ratio, feature, n_samples, clips and projections/clip_<i> [T - 1, K];
`python -m track_mjx_amd.analysis.render ... pca=<pca.h5>` draws them beside the frames.
"""
from __future__ import annotations

import sys

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import HipBackend, resolve      # noqa: F401  (analysis/backend.py: the calls of every analysis; tests and tools take pca.HipBackend)
from .recorded import by_clip, feature_of, rollout_features, split

CLI_OPTIONS = ("rollouts", "out", "feature", "n_components")
USAGE = "usage: python -m track_mjx_amd.analysis.pca rollouts=<dir of clip_<i>.h5> [feature=intention] [n_components=4] out=<pca.h5>"
# the first eight of matplotlib's default colour cycle (what the reference's curves get), then background, axes, "terminated" line
STRIP_COLOURS = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194), (127, 127, 127))


def strip_style(width: int, height: int, line_half_width: float = 1.0, marker_radius: float = 3.0, colours=STRIP_COLOURS, background=(255, 255, 255),
                axes=(0, 0, 0), terminated=(255, 0, 0), margins=None) -> _hip.StripStyle:
    """tmjx_strip_style_t: `margins` (left, right, top, bottom) in pixels, by default a sixteenth of the panel on every side (at least 2)."""
    st = _hip.StripStyle()
    mx, my = max(int(width) // 16, 2), max(int(height) // 16, 2)
    st.margin_left, st.margin_right, st.margin_top, st.margin_bottom = (mx, mx, my, my) if margins is None else (int(v) for v in margins)
    st.line_half_width, st.marker_radius = float(line_half_width), float(marker_radius)
    for c in range(8):
        st.colour[c][:] = [*colours[c % len(colours)], 255]
    st.background[:], st.axes[:], st.terminated[:] = [*background, 255], [*axes, 255], [*terminated, 255]
    return st


class PCA:
    """Principal components of [n, d] rows, d <= 1024: `fit`, `transform`, `fit_transform`, and after a fit `mean_` [D], `components_` [K, D] (unit rows,
    descending variance, the largest-magnitude coefficient of each positive), `explained_variance_` [K], `explained_variance_ratio_` [K] (zeros when
    the total variance is 0), `n_samples_`, `n_sweeps_` (Jacobi sweeps; above 128 features the block sweeps, also in `n_block_sweeps_`, which is 0
    for a narrow fit).  Features wider than 128 go through the backend's `fit_wide` / `transform_wide` where it has them.  Inputs: numpy arrays, or torch device tensors (a row stride is fine: activations are
    stored as column slices of wider buffers).  `transform` returns numpy for numpy, a device tensor for a tensor."""

    def __init__(self, n_components: int | None = None, device="cuda", backend=None):
        if n_components is not None and int(n_components) < 1:
            raise ValueError(f"n_components must be >= 1 (got {n_components})")
        self.n_components = None if n_components is None else int(n_components)
        self._b = resolve(backend, device)

    def fit(self, x):
        xa = self._b.asarray(x)
        n, d = (int(v) for v in xa.shape)
        k = min(n, d) if self.n_components is None else self.n_components
        if k > d:
            raise ValueError(f"n_components = {k} exceeds the {d} features")
        wide = d > _hip.PCA_MAX_D and hasattr(self._b, "fit_wide")
        mean, comp, var, info = self._b.fit_wide(xa) if wide else self._b.fit(xa)
        total = float(var.astype(np.float64).sum())
        self.mean_, self.components_, self.explained_variance_ = mean, np.ascontiguousarray(comp[:k]), var[:k].copy()
        self.explained_variance_ratio_ = (var[:k].astype(np.float64) / total).astype(np.float32) if total > 0.0 else np.zeros(k, np.float32)
        self.n_samples_, self.n_features_, self.n_sweeps_, self.off_rel_ = n, d, int(info.sweeps), float(info.off_rel)
        self.moments_ms_, self.jacobi_ms_, self.n_block_sweeps_ = float(info.moments_ms), float(info.jacobi_ms), int(info.sweeps) if wide else 0
        return self

    def transform(self, x):
        if not hasattr(self, "components_"):
            raise ValueError("this PCA is not fitted")
        xa = self._b.asarray(x)
        if xa.shape[1] != self.n_features_:
            raise ValueError(f"expected {self.n_features_} features, got {xa.shape[1]}")
        wide = self.n_features_ > _hip.PCA_MAX_D and hasattr(self._b, "transform_wide")
        out = self._b.transform_wide(xa, self.mean_, self.components_) if wide else self._b.transform(xa, self.mean_, self.components_)
        return self._b.to_numpy(out) if isinstance(x, np.ndarray) else out

    def fit_transform(self, x):
        return self.fit(x).transform(x)


def fit_rollouts(rollouts, feature: str = "intention", n_components: int | None = None, device="cuda", backend=None):
    """Fit one PCA on `feature` (up to 1024 wide) over every roll-out and project each.  `rollouts`: a directory of clip_<i>.h5, or a list of roll-out dicts.
    -> (pca, projections): projections[j] float32 [T_j, K] of roll-out j; pca.clips_ are the clip numbers (the list positions for dicts)."""
    ids, feats = rollout_features(rollouts, lambda r, _, where: feature_of(r, feature, where), feature, "fit")
    pca = PCA(n_components, device=device, backend=backend)
    x = pca._b.asarray(np.concatenate(feats, 0))
    proj = pca._b.to_numpy(pca.fit(x).transform(x))
    pca.clips_, pca.feature_ = ids, feature
    return pca, split(proj, [f.shape[0] for f in feats])


def main(argv=None, backend=None) -> int:
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out"), USAGE)
    if opts is None:
        return 2
    feature = opts.get("feature", "intention")
    try:
        pca, proj = fit_rollouts(opts["rollouts"], feature, int(opts.get("n_components", 4)), backend=backend)
    except (KeyError, ValueError) as e:
        return cli.report("pca", e)
    cli.write(opts["out"], {"mean": pca.mean_, "components": pca.components_, "explained_variance": pca.explained_variance_,
                            "explained_variance_ratio": pca.explained_variance_ratio_, "feature": feature, "n_samples": np.int64(pca.n_samples_),
                            "clips": np.asarray(pca.clips_, np.int64), "projections": by_clip(pca.clips_, proj)})
    ratio = ", ".join(f"{100 * r:.1f}%" for r in pca.explained_variance_ratio_)
    print(f"[pca] {feature}: {pca.n_samples_} samples x {pca.n_features_} features from {len(proj)} clips, {pca.n_sweeps_} sweeps; explained variance "
          f"{ratio}; wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
