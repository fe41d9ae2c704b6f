"""What an analysis tool reads from recorded roll-outs, and how it turns the concatenated rows of many clips back into per-clip results: the one
copy of what pca, cluster, hmm, arhmm, embed, readout, compare, spectrogram, jacobian and dynamics share.  Host numpy; no backend call."""
from __future__ import annotations

import os
import re

import numpy as np

from .. import h5lite

PLAIN_TARGETS = ("ctrl", "qposes_rollout", "qposes_ref", "state_rewards", "joint_forces", "sensor_readings")


# ---------------------------------------------------------------------------------------------------------------- reading
def rollout_features(rollouts, read, name=None, verb=None):
    """What the analysis tools take of a set of roll-outs.  `rollouts`: a directory of clip_<i>.h5 (read in numeric order), or a list of roll-out
    dicts; `read(rollout, clip, where)` -> the [T, D] feature of one (an open h5lite file or a dict), or a tuple that starts with it.
    -> (clip numbers: the list positions for dicts, [what `read` returned]).  With `verb` ("fit", "cluster", ...) an empty set is an error; with
    `name` the features must all have one width."""
    if isinstance(rollouts, (str, os.PathLike)):
        ids = sorted(int(m.group(1)) for m in (re.fullmatch(r"clip_(\d+)\.h5", f) for f in os.listdir(rollouts)) if m)
        if verb is not None and not ids:
            raise ValueError(f"no clip_<i>.h5 in {rollouts}")
        items = []
        for c in ids:
            with h5lite.File(os.path.join(rollouts, f"clip_{c}.h5")) as h:
                items.append(read(h, c, f"clip_{c}.h5"))
    else:
        ids = list(range(len(rollouts)))
        if verb is not None and not ids:
            raise ValueError(f"no roll-outs to {verb}")
        items = [read(r, j, f"roll-out {j}") for j, r in enumerate(rollouts)]
    if name is not None:
        widths = {(i[0] if isinstance(i, tuple) else i).shape[1] for i in items}
        if len(widths) != 1:
            raise ValueError(f"{name} has different widths across roll-outs: {sorted(widths)}")
    return ids, items


def _array(node, dtype=None):
    return np.asarray(node if isinstance(node, (np.ndarray, list, tuple)) else node[()], dtype)      # (an h5lite dataset reads with [()])


def feature_of(rollout, feature: str, where: str) -> np.ndarray:
    """The recorded feature of one roll-out as [T, D]: `ctrl`, or a path under activations/ (intention, decoder/layer_0, hidden_state/h, ...)."""
    node, path = rollout, ([feature] if feature == "ctrl" else ["activations", *[p for p in feature.split("/") if p]])
    for part in path:
        try:
            node = node[part]
        except (KeyError, IndexError, TypeError):
            raise KeyError(f"{where} has no {'/'.join(path)}" + (" (roll it out with log_activations=true)" if feature != "ctrl" else "")) from None
    if hasattr(node, "keys"):
        raise KeyError(f"{where}: {'/'.join(path)} is a group ({', '.join(node.keys())}), not a recorded array")
    a = _array(node, np.float32)
    if a.ndim < 2:
        raise ValueError(f"{where}: {'/'.join(path)} has shape {a.shape}, expected [T, D]")
    return a.reshape(-1, a.shape[-1])


def target_of(rollout, target: str, where: str) -> np.ndarray:
    """The recorded target of one roll-out as [rows, M] float32: one of PLAIN_TARGETS, rollout_metrics/<name> or activations/<path>."""
    if target.startswith("activations/"):
        return feature_of(rollout, target[len("activations/"):], where)
    parts = [p for p in target.split("/") if p]
    if not (target in PLAIN_TARGETS or (len(parts) == 2 and parts[0] == "rollout_metrics")):
        raise KeyError(f"unknown target {target!r}: one of {', '.join(PLAIN_TARGETS)}, rollout_metrics/<name> or activations/<path>")
    node = rollout
    for part in parts:
        try:
            node = node[part]
        except (KeyError, IndexError, TypeError):
            raise KeyError(f"{where} has no {target}" + (" (roll it out with log_sensors=true)" if target in ("joint_forces", "sensor_readings") else "")) from None
    if hasattr(node, "keys"):
        raise KeyError(f"{where}: {target} is a group ({', '.join(node.keys())}), not a recorded array")
    a = _array(node, np.float32)
    if a.ndim < 1:
        raise ValueError(f"{where}: {target} is a scalar")
    return a.reshape(a.shape[0], -1)      # (joint_forces [T - 1, nbody, 6] -> [T - 1, 6 nbody]; a [T] series -> [T, 1])


def columns(spec, width: int, name: str = "target_cols") -> slice:
    """The column slice of an "a:b" option (None or "": every column); `name` is the option the refusals speak of."""
    if spec is None or spec == "":
        return slice(0, width)
    m = re.fullmatch(r"(-?\d*):(-?\d*)", str(spec))
    if not m:
        raise ValueError(f"{name} = {spec!r}: expected a:b")
    sl = slice(int(m.group(1)) if m.group(1) else None, int(m.group(2)) if m.group(2) else None)
    if len(range(*sl.indices(width))) < 1:
        raise ValueError(f"{name} = {spec} selects no column of {width}")
    return sl


def tree(node):
    """An h5lite group as nested dicts of numpy arrays."""
    if hasattr(node, "keys"):
        return {k: tree(node[k]) for k in node.keys()}
    v = node[()]
    return bytes(v) if isinstance(v, (bytes, bytearray, np.bytes_)) else np.asarray(v)


def meta_of(rollout):
    """The roll-out's meta tree (of an open h5lite file: read into dicts), or None."""
    if isinstance(rollout, h5lite.File):
        return tree(rollout["meta"]) if "meta" in rollout else None
    return rollout.get("meta") if hasattr(rollout, "get") else None


def aligned_of(rollout, rows: int, where: str):
    """The roll-out's `aligned` flags as bool [rows] (set on a step that ended with a re-alignment: the roll-out zeroed the carry behind it), or
    None where it recorded none.  Flags for another number of rows are refused."""
    try:
        node = rollout["aligned"]
        aligned = np.asarray(node if isinstance(node, np.ndarray) else node[()]).reshape(-1) != 0
    except (KeyError, IndexError, TypeError):
        return None
    if aligned.shape[0] != rows:
        raise ValueError(f"{where}: aligned has {aligned.shape[0]} rows, intention {rows}")
    return aligned


def seq_start(lengths, n: int) -> np.ndarray:
    """int32 [S + 1]: the first row of every sequence and n, for sequences of `lengths` that tile the n rows."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if lengths.size == 0 or (lengths < 1).any() or int(lengths.sum()) != n:
        raise ValueError(f"lengths must be positive and sum to the {n} rows (got {lengths.size} lengths summing to {int(lengths.sum())})")
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def signals(rollouts, source: str, cols, projections):
    """-> (clip numbers, [T_j, C] float32 signals, the roll-outs' meta trees or None): the columns `cols` of a recorded series (target_of's
    names), or of the projections/clip_<i> of a pca.h5."""
    if projections is None:
        parts = [p for p in str(source).split("/") if p]
        if not (source in PLAIN_TARGETS or str(source).startswith("activations/") or (len(parts) == 2 and parts[0] == "rollout_metrics")):
            raise KeyError(f"unknown source {source!r}: one of {', '.join(PLAIN_TARGETS)}, rollout_metrics/<name> or activations/<path>")
    proj = None
    if projections is not None:
        with h5lite.File(projections) as h:
            if "projections" not in h:
                raise KeyError(f"{projections} has no projections group (write it with analysis.pca)")
            proj = {int(k.split("_")[1]): np.asarray(h["projections"][k][()], np.float32) for k in h["projections"].keys()}

    def one(r, clip, where):
        if proj is not None:
            if clip not in proj:
                raise KeyError(f"{projections} has no projections/clip_{clip}")
            a = proj[clip]
        else:
            a = target_of(r, source, where)
            node = r
            for part in [p for p in source.split("/") if p]:
                node = node[part]
            raw = np.shape(node if isinstance(node, (np.ndarray, list, tuple)) else node[()])
            if len(raw) < 2:      # (as feature_of resolves a feature: a [T] series is not a set of channels)
                raise ValueError(f"{where}: {source} has shape {tuple(raw)}, expected [T, C]")
        return np.ascontiguousarray(a[:, columns(cols, a.shape[1], "cols")], np.float32)

    ids, items = rollout_features(rollouts, lambda r, clip, where: (one(r, clip, where), meta_of(r)), source, "transform")
    sigs, metas = [s for s, _ in items], [m for _, m in items]
    if any(s.ndim != 2 or s.shape[0] < 1 for s in sigs):
        raise ValueError(f"{source}: expected [T, C] with T >= 1")
    return ids, sigs, metas


# ---------------------------------------------------------------------------------------------------------------- labels
def labels_file(path) -> dict:
    """{clip: int labels [T]} of the labels group of a clusters.h5, hmm.h5, arhmm.h5 or map.h5."""
    with h5lite.File(str(path)) as h:
        if "labels" not in h:
            raise KeyError(f"{path} has no labels group (write it with analysis.cluster, hmm, arhmm or embed)")
        return {int(k.split("_", 1)[1]): np.asarray(h["labels"][k][()]).reshape(-1) for k in h["labels"].keys()}


def labels_for_rows(labels, ids, lens) -> np.ndarray:
    """int64 [sum(lens)]: the label of every row of the clips `ids` with `lens` rows.  `labels`: a file labels_file reads, or {clip: int labels};
    labels beyond a clip's rows are dropped, a clip without labels or with too few is refused."""
    lab = labels_file(labels) if isinstance(labels, (str, os.PathLike)) else {int(k): np.asarray(v).reshape(-1) for k, v in dict(labels).items()}
    flat = []
    for c, t in zip(ids, lens):
        if c not in lab:
            raise KeyError(f"the labels file has no clip_{c}")
        if lab[c].shape[0] < t:
            raise ValueError(f"the labels of clip_{c} hold {lab[c].shape[0]} rows, the roll-out {t}")
        flat.append(lab[c][:t])
    return np.concatenate(flat).astype(np.int64)


def number_by_count(labels, k: int):
    """Number k motifs by descending count, equal counts in their original order: -> (order [k]: the old number of every new one, rank [k]: the new
    number of every old one, counts int64 [k] in the new numbering).  A motif without a row keeps a number."""
    counts = np.bincount(labels, minlength=k)
    order = np.argsort(-counts, kind="stable")
    rank = np.empty(k, np.int64)
    rank[order] = np.arange(k)
    return order, rank, counts[order].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- rows back into clips
def split(a, lens) -> list:
    """The rows of `a` cut back into clips of `lens` rows."""
    ends = np.cumsum(lens)
    return [a[e - t:e] for e, t in zip(ends, lens)]


def by_clip(ids, values, dtype=None) -> dict:
    """{clip_<c>: value}: the group a tool writes per clip."""
    return {f"clip_{c}": v if dtype is None else np.asarray(v, dtype) for c, v in zip(ids, values)}


def scatter_per_clip(a, rows, total: int, ids, lens) -> dict:
    """{clip_<c>: float32 [T_c, ...]} of a series evaluated at `rows` of the `total` concatenated rows only: NaN in the other rows."""
    full = np.full((total, *a.shape[1:]), np.nan, np.float32)
    full[rows] = a
    return by_clip(ids, split(full, lens))
