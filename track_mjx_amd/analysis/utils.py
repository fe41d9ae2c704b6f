"""Saving and loading roll-out pytrees as HDF5 — mirror of track_mjx/analysis/utils.py:10-95 (save_to_h5py, recursive_dict_to_h5py,
load_from_h5py, recursive_load_from_h5py).  h5py is not in this image: files are written by h5lite.write_tree and read by h5lite.File.

Mapping (recursive_dict_to_h5py): dict -> group, list / tuple -> group with members "0" .. "n-1", array / tensor / scalar / bytes / str ->
dataset, None -> skipped.  Loading turns a group whose members are all digits back into a list (an empty group too, as the reference does)."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from .. import h5lite


def to_tree(data):
    if data is None:
        return None
    if isinstance(data, tuple):
        data = list(data)
    if isinstance(data, dict):
        out = {}
        for k, v in data.items():
            t = to_tree(v)
            if t is not None:
                out[str(k)] = t
        return out
    if isinstance(data, list):
        out = {}
        for i, v in enumerate(data):
            t = to_tree(v)
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
    tree = to_tree(data)
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
