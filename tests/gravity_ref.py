"""Shared by the per-env gravity tests: the model blob with its `gravity` entry replaced ON THE HOST — what a handle (or the oracle) for one
gravity vector is created from, and what the RAND kernel with that vector as an env's gravity must reproduce bit for bit (the physics reads
gravity in one place and no derived model constant depends on it) — and the gravity set the tests use."""
from __future__ import annotations

import numpy as np

from track_mjx_amd import blob as _blob


def f32(v) -> np.ndarray:
    """`v` rounded to float32 and widened again: what a float32 table column and a float64 blob entry can both hold exactly."""
    return np.asarray(v, np.float32).astype(np.float64)


def model_gravity(blob: bytes) -> np.ndarray:
    return np.asarray(_blob.unpack(blob)["gravity"], dtype=np.float64).reshape(3)


def tilted(g0, scale: float, tilt_deg: float, toward) -> np.ndarray:
    """scale |g0| along g0's direction tilted by `tilt_deg` toward the horizontal direction `toward` (x, y): formed in float32."""
    g0 = np.asarray(g0, np.float64)
    mag = np.linalg.norm(g0)
    h = np.array([toward[0], toward[1], 0.0]) / np.hypot(toward[0], toward[1])
    t = np.deg2rad(tilt_deg)
    return f32(scale * mag * (np.cos(t) * g0 / mag + np.sin(t) * h))


def gravity_set(g0) -> list:
    """The six gravities of the tests: g0, 0.5 g0, 1.5 g0, |g0| tilted 10 deg toward +x, 20 deg toward -y, 0.38 |g0| tilted 5 deg toward
    (+x, +y).  Every member is float32-representable: formed in float32, returned as float64(float32(x))."""
    g0 = f32(g0)
    return [g0, f32(np.float32(0.5) * g0.astype(np.float32)), f32(np.float32(1.5) * g0.astype(np.float32)), tilted(g0, 1.0, 10.0, (1, 0)),
            tilted(g0, 1.0, 20.0, (0, -1)), tilted(g0, 0.38, 5.0, (1, 1))]


def gravity_blob(blob: bytes, g) -> bytes:
    """`blob` with its `gravity` entry set to `g` (3 values, stored in the blob's float64)."""
    e = _blob.unpack(blob)
    e["gravity"] = np.asarray(g, dtype=np.float64).reshape(3).copy()
    return _blob.pack(e)


def gravity_table(G, per: int) -> np.ndarray:
    """[3][len(G) * per] float32, rows gx | gy | gz: `per` consecutive envs for each member of `G`."""
    return np.ascontiguousarray(np.repeat(np.asarray(G, np.float32).reshape(-1, 3), per, axis=0).T)
