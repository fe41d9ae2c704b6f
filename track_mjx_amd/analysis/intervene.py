"""Activation interventions in checkpoint roll-outs: remove, clamp, scale or drive a subspace (or single units) of one layer while the animal runs.

An `Intervention` names a target activation of the roll-out's policy step and a linear edit of it; analysis.rollout.create_rollout_generator(...,
intervention=) and replay_latents(..., intervention=) run it as ONE more launch of the step's launch list, tmjx_intervene (include/tmjx.h; DESIGN.md
"Interventions"), directly behind the launch that produces the target.  Row r at control step t, when window[0] <= t < window[1] and dose != 0:

    subspace:  p_k = sum_j (h_j - c_j) v_kj;   h'_j = h_j + dose sum_k ((g_k - 1) p_k + o_k) v_kj
    units:     h'_j = h_j + dose ((g_j - 1)(h_j - c_j) + o_j)          for the listed units j

gain 0, offset 0 projects the subspace out (or silences the units to the centre); gain 0, offset s clamps the coordinates to s; gain 1, offset s
stimulates; gain g scales.  The directions are orthonormalised (float64 modified Gram-Schmidt, in the order given: direction k becomes the part of
row k orthogonal to the rows before it), so gain / offset k refer to the orthonormal direction k.

Targets: intention, encoder/layer_<i>, decoder/layer_<i>, hidden_state/h:<k> (LSTM policies; the replay decoder has no encoder).

CLI:  python -m track_mjx_amd.analysis.intervene baseline=<dir of clip_<i>.h5> perturbed=<dir of clip_<i>.h5> out=<effect.h5>
      host-side numpy over the two roll-outs: per clip present in both, the mean state_rewards of each and their difference, the first step at
      which qposes_rollout differs (-1: never), the per-step root-position and joint-angle distance, the difference of each recorded metric's
      mean; the perturbed files' `intervention` group is written through.
"""
from __future__ import annotations

import os
import re
import sys

import numpy as np

from ..hip import INTERVENE_MAX_K as MAX_K, INTERVENE_MAX_W as MAX_W

T_END = 2 ** 31 - 1
RANK_TOL = 1e-6
SUPPORTED = "intention, encoder/layer_<i>, decoder/layer_<i>, hidden_state/h:<k> (LSTM policies)"
_TARGET = re.compile(r"intention|(encoder|decoder)/layer_\d+|hidden_state/h:\d+")
CLI_OPTIONS = ("intervene_pca", "intervene_components", "intervene_readout", "intervene_centroids", "intervene_columns", "intervene_units", "intervene_mean", "intervene_gain",
               "intervene_offset", "intervene_window", "intervene_dose")


def check_target(target: str) -> str:
    target = str(target)
    if not _TARGET.fullmatch(target):
        raise ValueError(f"intervention target {target!r} is not supported; supported: {SUPPORTED}")
    return target


def orthonormalise(directions) -> np.ndarray:
    """float32 [K, w] orthonormal rows spanning the rows given, by modified Gram-Schmidt in float64 (twice: the second pass removes what rounding left);
    ValueError where a row's part orthogonal to the rows before it is below RANK_TOL of the row's norm."""
    v = np.array(directions, dtype=np.float64, ndmin=2)
    if v.ndim != 2 or not np.isfinite(v).all():
        raise ValueError("directions must be a finite [K, w] array")
    K, w = v.shape
    if not 1 <= K <= MAX_K or not 1 <= w <= MAX_W:
        raise ValueError(f"directions [{K}, {w}]: an intervention takes 1 .. {MAX_K} directions of 1 .. {MAX_W} features")
    q = np.zeros_like(v)
    for k in range(K):
        norm0 = np.linalg.norm(v[k])
        r = v[k].copy()
        for _ in range(2):
            for i in range(k):
                r -= (q[i] @ r) * q[i]
        pivot = np.linalg.norm(r)
        if norm0 == 0 or pivot < RANK_TOL * norm0:
            raise ValueError(f"directions have rank below {K}: row {k} lies in the span of the rows before it (pivot {pivot:.3e} against a norm of {norm0:.3e})")
        q[k] = r / pivot
    return q.astype(np.float32)


def _slice(spec, n: int, what: str) -> list:
    """"a:b" | "i,j,k" | "i" -> indices below n."""
    spec = str(spec).strip()
    if ":" in spec:
        a, _, b = spec.partition(":")
        idx = list(range(int(a or 0), int(b) if b else n))
    else:
        idx = [int(c) for c in spec.split(",") if c.strip()]
    if not idx or min(idx) < 0 or max(idx) >= n:
        raise ValueError(f"{what}={spec!r} selects {idx[:5]}{'..' if len(idx) > 5 else ''} of {n}")
    return idx


def _text(v) -> str:
    return bytes(v).decode() if isinstance(v, (bytes, np.bytes_)) else str(v)


class InterventionBuffers:
    """The device buffers of one intervention for the n rows of one launch list (what LaunchList.intervene reads)."""

    def __init__(self, spec: "Intervention", n: int, w: int, device, window, dose):
        import torch
        from .. import hip
        self.spec, self.n, self.w = spec, int(n), int(w)
        dev = torch.device(device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)      # noqa: E731
        self.dirs = self.proj = None
        self.K = self.ldv = self.ldp = 0
        if spec.mode == "subspace":
            if spec.directions.shape[1] != self.w:
                raise ValueError(f"the intervention's directions are {spec.directions.shape[1]} wide, the target {spec.target} is {self.w} wide")
            self.mode, self.K, self.ldv, self.ldp = hip.INTERVENE_SUBSPACE, spec.K, self.w, spec.K
            self.dirs = up(spec.directions, np.float32)
            self.proj = torch.zeros((self.n, self.K), dtype=torch.float32, device=dev)
            gain, offset = spec.gain, spec.offset
        else:
            if max(spec.units) >= self.w:
                raise ValueError(f"unit {max(spec.units)} outside the {self.w} units of {spec.target}")
            self.mode = hip.INTERVENE_UNITS
            gain, offset = np.ones(self.w, np.float32), np.zeros(self.w, np.float32)
            gain[spec.units], offset[spec.units] = spec.gain, spec.offset
        if spec.center is not None and spec.center.shape[0] != self.w:
            raise ValueError(f"the intervention's center has {spec.center.shape[0]} entries, the target {spec.target} is {self.w} wide")
        self.center = None if spec.center is None else up(spec.center, np.float32)
        self.gain, self.offset = up(gain, np.float32), up(offset, np.float32)
        window = np.asarray(window, np.int64).reshape(self.n, 2)
        self.dose, self.t_on, self.t_off = up(np.asarray(dose).reshape(self.n), np.float32), up(window[:, 0], np.int32), up(window[:, 1], np.int32)


class Intervention:
    """One linear edit of one activation.  mode "subspace": directions [K <= 16, w <= 1024] (orthonormalised here; a set of rank below K is
    refused), gain / offset a scalar or one per direction; mode "units": units = the unit indices, gain / offset a scalar or one per listed unit.
    center [w] or None (0).  window = (t_on, t_off) in control steps (t_off None: to the end) and dose: one value, or one per clip of a
    generate_rollout / replay_latents call."""

    def __init__(self, target, mode, directions=None, units=None, center=None, gain=0.0, offset=0.0, window=(0, None), dose=1.0):
        self.target = check_target(target)
        if mode not in ("subspace", "units"):
            raise ValueError(f"mode must be 'subspace' or 'units', not {mode!r}")
        self.mode = mode
        if mode == "subspace":
            if directions is None or units is not None:
                raise ValueError("a subspace intervention takes directions=[K, w] (and no units)")
            self.directions = orthonormalise(directions)
            self.K, self.units, count, what = self.directions.shape[0], None, self.directions.shape[0], "direction"
        else:
            if units is None or directions is not None:
                raise ValueError("a units intervention takes units=[indices] (and no directions)")
            u = np.atleast_1d(np.asarray(units))
            if u.ndim != 1 or u.size == 0 or not np.issubdtype(u.dtype, np.integer) or u.min() < 0 or u.max() >= MAX_W or len(set(u.tolist())) != u.size:
                raise ValueError(f"units must be distinct indices in 0 .. {MAX_W - 1}")
            self.units, self.directions, self.K, count, what = u.astype(np.int64), None, 0, u.size, "listed unit"
        self.center = None if center is None else np.ascontiguousarray(center, np.float32).reshape(-1)
        if self.center is not None and mode == "subspace" and self.center.shape[0] != self.directions.shape[1]:
            raise ValueError(f"center has {self.center.shape[0]} entries, the directions {self.directions.shape[1]} features")

        def per(v, name):
            v = np.atleast_1d(np.asarray(v, np.float64)).ravel()
            if v.size not in (1, count) or not np.isfinite(v).all():
                raise ValueError(f"{name}: {v.size} values for {count} {what}s (one finite value, or one per {what})")
            return np.full(count, v[0], np.float32) if v.size == 1 else v.astype(np.float32)
        self.gain, self.offset = per(gain, "gain"), per(offset, "offset")
        self.window, self.dose = window, dose
        self._parsed(window, dose)      # (a malformed window / dose fails here, not in the first roll-out)

    @staticmethod
    def _parsed(window, dose):
        rows = np.atleast_2d(np.asarray(window, object))
        if rows.ndim != 2 or rows.shape[1] != 2:
            raise ValueError("window must be (t_on, t_off) or one such pair per clip (t_off None: to the end)")
        win = np.array([[int(a or 0), T_END if b is None else int(b)] for a, b in rows], np.int64)
        if (win < 0).any() or (win > T_END).any():
            raise ValueError("window: steps must be in 0 .. 2^31 - 1")
        d = np.atleast_1d(np.asarray(dose, np.float64)).ravel()
        if d.size == 0 or not np.isfinite(d).all():
            raise ValueError("dose must be finite")
        return win, d.astype(np.float32)

    def per_clip(self, total: int, window=None, dose=None):
        """(window int64 [total, 2], dose float32 [total]) for a generate_rollout call of `total` clips: one value, or one per clip."""
        win, d = self._parsed(self.window if window is None else window, self.dose if dose is None else dose)
        if win.shape[0] not in (1, int(total)):
            raise ValueError(f"window: {win.shape[0]} values for {total} clips (one value, or one per clip)")
        if d.size not in (1, int(total)):
            raise ValueError(f"dose: {d.size} values for {total} clips (one value, or one per clip)")
        return np.broadcast_to(win, (int(total), 2)).copy(), np.broadcast_to(d, (int(total),)).copy()

    def buffers(self, n: int, w: int, device, window, dose) -> InterventionBuffers:
        return InterventionBuffers(self, n, w, device, window, dose)

    def record(self, window, dose, projection=None) -> dict:
        """The `intervention` group of one batch's result: [n] leading axes on window / dose / projection, the rest repeated per clip."""
        n = len(dose)
        rep = lambda a: np.broadcast_to(a, (n, *np.shape(a))).copy()      # noqa: E731
        out = {"target": np.array([self.target.encode()] * n), "mode": np.array([self.mode.encode()] * n), "gain": rep(self.gain), "offset": rep(self.offset),
               "window": np.asarray(window, np.int64), "dose": np.asarray(dose, np.float32)}
        if self.mode == "subspace":
            out["directions"] = rep(self.directions)
            if projection is not None:
                out["projection"] = projection
        else:
            out["units"] = rep(self.units)
        if self.center is not None:
            out["center"] = rep(self.center)
        return out

    # ------------------------------------------------------------------------------------------------ constructors from analysis files
    @classmethod
    def from_pca(cls, path, components="0:2", **kw):
        """Target, directions and center from a pca.h5 (analysis.pca: `feature`, `components` [k, d] rows, `mean`)."""
        from .. import h5lite
        f = h5lite.File(str(path))
        comp = np.asarray(f["components"][()], np.float64)
        idx = _slice(components, comp.shape[0], "components")
        return cls(_text(f["feature"][()]), "subspace", directions=comp[idx], center=np.asarray(f["mean"][()], np.float32), **kw)

    @classmethod
    def from_readout(cls, path, columns="0:3", **kw):
        """Target, directions and center from a readout.h5 (analysis.readout: the columns of `coef` [d, m], `mean_x`, `feature`)."""
        from .. import h5lite
        f = h5lite.File(str(path))
        coef = np.asarray(f["coef"][()], np.float64)
        idx = _slice(columns, coef.shape[1], "columns")
        return cls(_text(f["feature"][()]), "subspace", directions=coef[:, idx].T, center=np.asarray(f["mean_x"][()], np.float32), **kw)

    @classmethod
    def from_centroids(cls, path, columns="0:3", **kw):
        """Target, directions and center from a clusters.h5 (analysis.cluster: `centroids` [k, d], `feature`): the rows `columns` of
        centroids - mean(centroids) are the directions, the mean of the centroids the center."""
        from .. import h5lite
        f = h5lite.File(str(path))
        cen = np.asarray(f["centroids"][()], np.float64)
        idx = _slice(columns, cen.shape[0], "columns")
        mean = cen.mean(0)
        return cls(_text(f["feature"][()]), "subspace", directions=(cen - mean)[idx], center=mean.astype(np.float32), **kw)

    @classmethod
    def units(cls, target, indices, center=None, **kw):      # noqa: F811  (the instance attribute `units` shadows it on instances only)
        """A units-mode intervention; center: None (0), an array [w], or the path of a pca.h5 of the same feature (its `mean`)."""
        if isinstance(center, (str, os.PathLike)):
            from .. import h5lite
            f = h5lite.File(str(center))
            if _text(f["feature"][()]) != str(target):
                raise ValueError(f"{center}: the PCA of {_text(f['feature'][()])!r}, the intervention targets {target!r}")
            center = np.asarray(f["mean"][()], np.float32)
        return cls(target, "units", units=indices, center=center, **kw)


# ---------------------------------------------------------------------------------------------------------------- roll-out CLI options
def from_cli(opts: dict):
    """The Intervention of the roll-out command line's intervene_* options (analysis.rollout), or None; (window, dose) stay per-clip lists for
    per_clip.  ValueError: a usage error."""
    given = [k for k in ("intervene_pca", "intervene_readout", "intervene_centroids", "intervene_units") if k in opts]
    if not given:
        extra = [k for k in CLI_OPTIONS if k in opts]
        if extra:
            raise ValueError(f"{', '.join(extra)}: no intervention is given (intervene_pca= | intervene_readout= | intervene_centroids= | intervene_units=)")
        return None
    if len(given) > 1:
        raise ValueError(f"exactly one of intervene_pca / intervene_readout / intervene_centroids / intervene_units may be given (got {', '.join(given)})")
    src = given[0]
    for opt, owners in (("intervene_components", ("intervene_pca",)), ("intervene_columns", ("intervene_readout", "intervene_centroids")),
                        ("intervene_mean", ("intervene_units",))):
        if opt in opts and src not in owners:
            raise ValueError(f"{opt} goes with {owners[0]}=" + "".join(f" or {o}=" for o in owners[1:]))
    floats = lambda k, d: [float(x) for x in str(opts[k]).split(",") if x.strip()] if k in opts else d      # noqa: E731
    kw = dict(gain=floats("intervene_gain", 0.0), offset=floats("intervene_offset", 0.0), dose=floats("intervene_dose", 1.0))
    if "intervene_window" in opts:
        a, sep, b = str(opts["intervene_window"]).partition(":")
        if not sep:
            raise ValueError("intervene_window=a:b")
        kw["window"] = (int(a or 0), int(b) if b else None)
    try:
        if src == "intervene_pca":
            return Intervention.from_pca(opts[src], opts.get("intervene_components", "0:2"), **kw)
        if src == "intervene_readout":
            return Intervention.from_readout(opts[src], opts.get("intervene_columns", "0:3"), **kw)
        if src == "intervene_centroids":
            return Intervention.from_centroids(opts[src], opts.get("intervene_columns", "0:3"), **kw)
        target, sep, idx = str(opts[src]).rpartition(":")
        if target.startswith("hidden_state/h") and target.count(":") == 0:      # hidden_state/h:<k>:i,j
            raise ValueError("intervene_units=hidden_state/h:<k>:i,j,k")
        if not sep or not idx:
            raise ValueError("intervene_units=<target>:i,j,k")
        return Intervention.units(target, [int(c) for c in idx.split(",") if c.strip()], center=opts.get("intervene_mean"), **kw)
    except (OSError, KeyError) as e:
        raise ValueError(f"{src}: {e}") from e


# ---------------------------------------------------------------------------------------------------------------- effect summary
def effect_summary(baseline: str, perturbed: str) -> dict:
    """{clip_<i>: {...}} over the clips present in both directories."""
    from .utils import load_from_h5py
    ids = lambda d: {int(m.group(1)) for m in (re.fullmatch(r"clip_(\d+)\.h5", f) for f in os.listdir(d)) if m}      # noqa: E731
    both = sorted(ids(baseline) & ids(perturbed))
    if not both:
        raise ValueError(f"no clip_<i>.h5 present in both {baseline} and {perturbed}")
    out = {}
    for c in both:
        b, p = (load_from_h5py(os.path.join(d, f"clip_{c}.h5")) for d in (baseline, perturbed))
        qb, qp = np.asarray(b["qposes_rollout"], np.float32), np.asarray(p["qposes_rollout"], np.float32)
        if qb.shape != qp.shape:
            raise ValueError(f"clip_{c}.h5: qposes_rollout {qb.shape} against {qp.shape}")
        differs = (qb.view(np.uint32) != qp.view(np.uint32)).any(axis=1)
        rb, rp = float(np.mean(b["state_rewards"], dtype=np.float64)), float(np.mean(p["state_rewards"], dtype=np.float64))
        one = {"reward_mean_baseline": np.float64(rb), "reward_mean_perturbed": np.float64(rp), "reward_mean_difference": np.float64(rp - rb),
               "first_divergence": np.int64(int(np.argmax(differs)) if differs.any() else -1),
               "root_distance": np.linalg.norm(qp[:, :3].astype(np.float64) - qb[:, :3], axis=1),
               "joint_distance": np.linalg.norm(qp[:, 7:].astype(np.float64) - qb[:, 7:], axis=1)}
        mb, mp = b.get("rollout_metrics"), p.get("rollout_metrics")
        if isinstance(mb, dict) and isinstance(mp, dict):
            one["metric_mean_difference"] = {k: np.float64(np.mean(mp[k], dtype=np.float64) - np.mean(mb[k], dtype=np.float64)) for k in mb if k in mp}
        if "intervention" in p:
            one["intervention"] = p["intervention"]
        out[f"clip_{c}"] = one
    return out


def main(argv=None) -> int:
    from . import cli
    from .utils import to_tree
    opts = cli.parse(argv, ("baseline", "perturbed", "out"), ("baseline", "perturbed", "out"),
                     "usage: python -m track_mjx_amd.analysis.intervene baseline=<dir of clip_<i>.h5> perturbed=<dir of clip_<i>.h5> out=<effect.h5>")
    if opts is None:
        return 2
    try:
        tree = effect_summary(opts["baseline"], opts["perturbed"])
    except (OSError, KeyError, ValueError) as e:
        return cli.report("intervene", e)
    cli.write(opts["out"], to_tree(tree))
    d = [int(v["first_divergence"]) for v in tree.values()]
    dr = [float(v["reward_mean_difference"]) for v in tree.values()]
    print(f"[intervene] {len(tree)} clips; diverged: {sum(x >= 0 for x in d)} (first step: {min([x for x in d if x >= 0], default=-1)}); "
          f"mean reward difference {np.mean(dr):+.6f}; wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
