"""Saving and loading roll-out pytrees as HDF5 — mirror of track_mjx/analysis/utils.py:10-95 (save_to_h5py, recursive_dict_to_h5py,
load_from_h5py, recursive_load_from_h5py).  h5py is not in this image: files are written by h5lite.write_tree and read by h5lite.File.

Mapping (recursive_dict_to_h5py): dict -> group, list / tuple -> group with members "0" .. "n-1", array / tensor / scalar / bytes / str ->
dataset, None -> skipped.  Loading turns a group whose members are all digits back into a list (an empty group too, as the reference does)."""
from __future__ import annotations

import os
import re
from pathlib import Path

import numpy as np

from .. import h5lite


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


def _to_tree(data):
    if data is None:
        return None
    if isinstance(data, tuple):
        data = list(data)
    if isinstance(data, dict):
        out = {}
        for k, v in data.items():
            t = _to_tree(v)
            if t is not None:
                out[str(k)] = t
        return out
    if isinstance(data, list):
        out = {}
        for i, v in enumerate(data):
            t = _to_tree(v)
            if t is not None:
                out[str(i)] = t
        return out
    if hasattr(data, "detach"):                       # torch tensors
        data = data.detach().cpu().numpy()
    if isinstance(data, (int, float, bool, str, bytes, np.bytes_, np.ndarray, np.generic)):
        return data
    raise TypeError(f"save_to_h5py: unsupported type {type(data).__name__}")


def _nest(tree: dict, group_path: str) -> dict:
    for part in reversed([p for p in group_path.split("/") if p]):
        tree = {part: tree}
    return tree


def save_to_h5py(file_path: str | Path, data, group_path: str = "/") -> None:
    """Write `data` (a pytree) to a new file, rooted at `group_path`."""
    tree = _to_tree(data)
    if not isinstance(tree, dict):
        parts = [p for p in group_path.split("/") if p]
        if not parts:
            raise ValueError("save_to_h5py: a single array needs a group_path naming the dataset")
        tree = _nest({parts[-1]: tree}, "/".join(parts[:-1]))
    else:
        tree = _nest(tree, group_path)
    h5lite.write_tree(str(file_path), tree)


def _load(node):
    if isinstance(node, h5lite.Dataset):
        return node[()]
    keys = list(node.keys())
    if all(k.isdigit() for k in keys):
        return [_load(node[k]) for k in sorted(keys, key=int)]
    return {k: _load(node[k]) for k in keys}


def load_from_h5py(file_path: str | Path, group_path: str = "/"):
    """The pytree under `group_path` (recursive_load_from_h5py)."""
    f = h5lite.File(str(file_path))
    node = f if group_path.strip("/") == "" else f[group_path]
    return _load(node)
