"""The affine actuator bias of the position-actuator rodent (walker.BLOBS (False, 0.8)) restated in float64 numpy, and the substitution
that lets the unmodified oracle — which computes force = gain * act and ignores the blob's `act_bias` — produce the affine model's
physics for ONE substep:

    act' = act + (b0 + b1 * length(qpos)) / gain      =>      gain * act' = gain * act + b0 + b1 * length

(all 38 rodent gains are positive).  The oracle's forces, qacc, qvel and qpos of that substep are then exactly the affine model's; only
its `act` output is off (the filter advances act' instead of act), so `act` is checked against the filter formula instead (next_act).
"""
from __future__ import annotations

import numpy as np

from tests.common import PHYS_ROWS, rel_err
from track_mjx_amd import config as _config
from track_mjx_amd import walker as _walker

POS_OVERRIDES = ["walker_config.torque_actuators=false", "walker_config.rescale_factor=0.8"]


def position_config():
    """`--config-name rodent-sps-per-actor walker_config.torque_actuators=false walker_config.rescale_factor=0.8`."""
    return _config.load_config(name="rodent-sps-per-actor", overrides=POS_OVERRIDES)


def position_walker():
    cfg = position_config()
    return _walker.Rodent(**cfg["walker_config"]), cfg


class Actuation:
    """float64 actuator tables of a walker's blob."""

    def __init__(self, model):
        dims = model["dims"]
        nv, nu, njnt = int(dims[3]), int(dims[4]), int(dims[1])
        self.nu, self.nv = nu, nv
        self.moment = np.asarray(model["act_moment"], np.float64).reshape(nu, nv)
        self.gain = np.asarray(model["act_gain"], np.float64)
        self.tau = np.asarray(model["act_tau"], np.float64)
        self.ctrlrange = np.asarray(model["act_ctrlrange"], np.float64).reshape(nu, 2)
        b = np.asarray(model["act_bias"], np.float64).reshape(nu, 3) if "act_bias" in model else np.zeros((nu, 3))
        self.b0, self.b1, self.b2 = b[:, 0], b[:, 1], b[:, 2]
        # qpos address of every hinge dof (the free joint's dofs carry no actuator moment)
        jt, qa, da = (np.asarray(model[k]) for k in ("jnt_type", "jnt_qposadr", "jnt_dofadr"))
        self.dof_qpos = np.full(nv, -1)
        for j in range(njnt):
            if jt[j] == 3:
                self.dof_qpos[da[j]] = qa[j]

    def length(self, qpos):
        """actuator_length [nu] (or [nu, n] for qpos [nq, n]) = moment . qpos of the driven hinge dofs."""
        qpos = np.asarray(qpos, np.float64)
        hinge = self.dof_qpos >= 0
        return self.moment[:, hinge] @ qpos[self.dof_qpos[hinge]]

    def force(self, act, qpos):
        act = np.asarray(act, np.float64)
        L = self.length(qpos)
        sh = (slice(None),) + (None,) * (act.ndim - 1)
        return self.gain[sh] * act + self.b0[sh] + self.b1[sh] * L

    def qfrc_actuator(self, act, qpos):
        return self.moment.T @ self.force(act, qpos)

    def substituted_act(self, act, qpos):
        act = np.asarray(act, np.float64)
        sh = (slice(None),) + (None,) * (act.ndim - 1)
        return act + (self.b0[sh] + self.b1[sh] * self.length(qpos)) / self.gain[sh]

    def next_act(self, act, ctrl, h):
        """The filter (MJX dyntype filter + Euler): act + (clip(ctrl) - act) / tau * h."""
        act, ctrl = np.asarray(act, np.float64), np.asarray(ctrl, np.float64)
        sh = (slice(None),) + (None,) * (act.ndim - 1)
        c = np.clip(ctrl, self.ctrlrange[:, 0][sh], self.ctrlrange[:, 1][sh])
        return act + (c - act) / np.maximum(self.tau[sh], 1e-15) * h


def oracle_substep(O, A: Actuation, st: dict, ctrl):
    """One substep of the oracle O from the state rows `st` (float64 vectors, PHYS_ROWS) with the bias substituted into act.
    Returns {"qpos", "qvel"} of the affine model."""
    d = O.new_data(st["qpos"], st["qvel"])
    for k in PHYS_ROWS:
        O.set(d, k, st[k])
    O.set(d, "act", A.substituted_act(st["act"], st["qpos"]))
    O.step(d, np.asarray(ctrl, np.float64))
    return {k: O.get(d, k) for k in ("qpos", "qvel")}


def collect(errs, got, res64, res32):
    for k in ("qpos", "qvel"):
        errs[k][0].append(rel_err(got[k], res64[k])); errs[k][1].append(rel_err(res32[k], res64[k]))
