"""Shared by the domain-randomisation tests: the model blob with its constants scaled ON THE HOST — what a handle (or the oracle) for one
(friction, actuator, damping) triple is created from, and what the RAND kernel with that triple as an env's scales must reproduce."""
from __future__ import annotations

import numpy as np

from track_mjx_amd import blob as _blob

TRIPLES_G1 = ((1.0, 1.0, 1.0), (0.6, 1.0, 1.0), (1.0, 0.7, 1.0), (1.3, 1.2, 1.8))     # (friction, actuator, damping)


def scaled_blob(blob: bytes, friction: float = 1.0, actuator: float = 1.0, damping: float = 1.0) -> bytes:
    """`blob` with con_friction[:, 0] (sliding friction), act_gain and act_bias[:, 0:2] (the affine bias pair, where the model has one) and
    dof_damping multiplied by the three scales (the entry names tools/compile_model.py writes).  The product is formed in float32, as the
    kernel forms it from its float32 constant and float32 scale, and stored in the blob's float64; all scales 1: `blob` itself."""
    if friction == 1.0 and actuator == 1.0 and damping == 1.0:
        return blob
    e = _blob.unpack(blob)

    def mul(a, s):
        return (np.asarray(a, np.float32) * np.float32(s)).astype(np.float64)

    fr = np.array(e["con_friction"], dtype=np.float64).reshape(-1, 3)
    fr[:, 0] = mul(fr[:, 0], friction)
    e["con_friction"] = fr.ravel()
    e["act_gain"] = mul(e["act_gain"], actuator)
    if "act_bias" in e:
        b = np.array(e["act_bias"], dtype=np.float64).reshape(-1, 3)
        b[:, 0] = mul(b[:, 0], actuator); b[:, 1] = mul(b[:, 1], actuator)
        e["act_bias"] = b.ravel()
    e["dof_damping"] = mul(e["dof_damping"], damping)
    return _blob.pack(e)


def scales_table(triples, per: int) -> np.ndarray:
    """[3][len(triples) * per] float32: `per` consecutive envs for each triple."""
    return np.ascontiguousarray(np.repeat(np.asarray(triples, np.float32), per, axis=0).T)
