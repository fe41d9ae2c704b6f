"""float64 numpy restatement of the recording kernel's sensor stage (csrc/wave_physics.h: tmw_sensor_stage), for the tests.

Written from MuJoCo's published semantics, independently of the kernel's data layout: forward kinematics (tools/compile_model.fk), cdof,
cvel / cdof_dot (mj_comVel), cacc (mj_rnePostConstraint), the site sensors (mj_objectVelocity / mj_objectAcceleration with flg_local),
subtree_linvel (mj_subtreeVel) and cfrc_ext (mj_rnePostConstraint's contact part: the pyramid rows decoded to the contact frame, rotated to
world, taken about subtree_com[body_rootid]; minus on geom 1's body, plus on geom 2's, the world body skipped).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
from compile_model import fk, quat_to_mat  # noqa: E402


def model_dict(entries) -> dict:
    """Blob entries (track_mjx_amd/blob.py) -> the shapes this module and compile_model.fk use."""
    e = entries
    nbody, njnt, nq, nv, nu, ncon = (int(x) for x in e["dims"])
    m = dict(nbody=nbody, njnt=njnt, nq=nq, nv=nv, nu=nu, ncon=ncon)
    for k in ("body_parentid", "body_rootid", "body_jntadr", "body_jntnum", "body_dofadr", "body_dofnum", "jnt_type", "jnt_bodyid",
              "jnt_qposadr", "jnt_dofadr", "dof_bodyid", "dof_jntid", "dof_parentid", "con_body1", "con_body2"):
        m[k] = np.asarray(e[k], int)
    for k, w in (("body_pos", 3), ("body_quat", 4), ("body_ipos", 3), ("jnt_pos", 3), ("jnt_axis", 3), ("con_friction", 3)):
        m[k] = np.asarray(e[k], float).reshape(-1, w)
    m["body_mass"], m["qpos0"], m["gravity"] = np.asarray(e["body_mass"], float), np.asarray(e["qpos0"], float), np.asarray(e["gravity"], float)
    m["nlim"] = int(np.sum(e["jnt_limited"]))
    if "sensor_type" in e:
        m["sensor_type"], m["sensor_objid"], m["sensor_adr"] = (np.asarray(e[k], int) for k in ("sensor_type", "sensor_objid", "sensor_adr"))
        m["site_bodyid"] = np.asarray(e["site_bodyid"], int)
        m["site_pos"], m["site_quat"] = np.asarray(e["site_pos"], float).reshape(-1, 3), np.asarray(e["site_quat"], float).reshape(-1, 4)
    return m


def _cross_motion(u, v):
    return np.concatenate([np.cross(u[:3], v[:3]), np.cross(u[:3], v[3:]) + np.cross(u[3:], v[:3])])


def kinematics(m, qpos):
    """xpos, xmat, xipos, subtree_com (per body: the point about which that body's com-based quantities are taken), cdof."""
    xpos, xquat, xanchor, xaxis = fk(m, qpos)
    nb = m["nbody"]
    xmat = np.array([quat_to_mat(q) for q in xquat])
    xipos = xpos + np.einsum("bij,bj->bi", xmat, m["body_ipos"])
    mass = m["body_mass"]
    root = m["body_rootid"]
    scom = np.zeros((nb, 3))
    for r in set(root[1:].tolist()):
        sub = [b for b in range(1, nb) if root[b] == r]
        M = mass[sub].sum()
        scom[r] = (mass[sub, None] * xipos[sub]).sum(0) / M if M > 1e-15 else xipos[r]
    com_of = scom[root]                              # per body: subtree_com[body_rootid[b]]
    cdof = np.zeros((m["nv"], 6))
    for j in range(m["njnt"]):
        b, d = m["jnt_bodyid"][j], m["jnt_dofadr"][j]
        c = com_of[b]
        if m["jnt_type"][j] == 0:
            for k in range(3):
                cdof[d + k, 3 + k] = 1.0
                ax = xmat[b][:, k]
                cdof[d + 3 + k] = np.concatenate([ax, np.cross(ax, c - xpos[b])])
        else:
            cdof[d] = np.concatenate([xaxis[j], np.cross(xaxis[j], c - xanchor[j])])
    return dict(xpos=xpos, xmat=xmat, xipos=xipos, com_of=com_of, cdof=cdof)


def velocities(m, cdof, qvel, qacc):
    """cvel, cdof_dot (mj_comVel) and cacc (mj_rnePostConstraint) of every body."""
    nb = m["nbody"]
    cvel, cacc = np.zeros((nb, 6)), np.zeros((nb, 6))
    cacc[0, 3:] = -m["gravity"]
    cdd = np.zeros_like(cdof)
    for b in range(1, nb):
        p = m["body_parentid"][b]
        cv = cvel[p].copy()
        for j in range(m["body_jntadr"][b], m["body_jntadr"][b] + m["body_jntnum"][b]) if m["body_jntnum"][b] else []:
            d = m["jnt_dofadr"][j]
            if m["jnt_type"][j] == 0:
                cv = cv + cdof[d:d + 3].T @ qvel[d:d + 3]
                for k in range(3, 6):
                    cdd[d + k] = _cross_motion(cv, cdof[d + k])
                cv = cv + cdof[d + 3:d + 6].T @ qvel[d + 3:d + 6]
            else:
                cdd[d] = _cross_motion(cv, cdof[d])
                cv = cv + cdof[d] * qvel[d]
        cvel[b] = cv
        ca = cacc[p].copy()
        d0, nd = m["body_dofadr"][b], m["body_dofnum"][b]
        for d in range(d0, d0 + nd) if nd else []:
            ca += cdd[d] * qvel[d] + cdof[d] * qacc[d]
        cacc[b] = ca
    return cvel, cdd, cacc


def contact_forces(m, efc_force, con_pos, con_frame):
    """World-frame force [ncon, 3] of every contact from its four pyramid rows (MJX row order: limits, then four rows per contact)."""
    nl, nc = m["nlim"], m["ncon"]
    f = np.asarray(efc_force, float)[nl:nl + 4 * nc].reshape(nc, 4)
    mu = m["con_friction"][:, 0]
    fn, f1, f2 = f.sum(1), (f[:, 0] - f[:, 1]) * mu, (f[:, 2] - f[:, 3]) * mu
    fr = np.asarray(con_frame, float).reshape(nc, 3, 3)
    return fr[:, 0] * fn[:, None] + fr[:, 1] * f1[:, None] + fr[:, 2] * f2[:, None]


def sensors(m, qpos, qvel, qacc, efc_force, con_pos, con_frame):
    """(sensordata [nsensordata], cfrc_ext [nbody, 6]) of one env."""
    kin = kinematics(m, np.asarray(qpos, float))
    cvel, _, cacc = velocities(m, kin["cdof"], np.asarray(qvel, float), np.asarray(qacc, float))
    nb = m["nbody"]
    F = contact_forces(m, efc_force, con_pos, con_frame)
    P = np.asarray(con_pos, float).reshape(-1, 3)
    cfrc = np.zeros((nb, 6))
    for c in range(m["ncon"]):
        for b, sg in ((m["con_body1"][c], -1.0), (m["con_body2"][c], 1.0)):
            if b == 0:
                continue
            cfrc[b, :3] += sg * np.cross(P[c] - kin["com_of"][b], F[c])
            cfrc[b, 3:] += sg * F[c]
    sd = []
    for t, o in zip(m.get("sensor_type", []), m.get("sensor_objid", [])):
        if t == 3:
            sub = [k for k in range(o, nb) if _in_subtree(m, k, o)]
            mass = m["body_mass"][sub]
            v = np.array([cvel[k, 3:] - np.cross(kin["xipos"][k] - kin["com_of"][k], cvel[k, :3]) for k in sub])
            sd.append((mass[:, None] * v).sum(0) / max(mass.sum(), 1e-15))
            continue
        b = m["site_bodyid"][o]
        R = kin["xmat"][b] @ quat_to_mat(m["site_quat"][o])
        d = kin["xpos"][b] + kin["xmat"][b] @ m["site_pos"][o] - kin["com_of"][b]
        w, v = R.T @ cvel[b, :3], R.T @ (cvel[b, 3:] - np.cross(d, cvel[b, :3]))
        if t == 0:
            sd.append(R.T @ (cacc[b, 3:] - np.cross(d, cacc[b, :3])) + np.cross(w, v))
        else:
            sd.append(v if t == 1 else w)
    return (np.concatenate(sd) if sd else np.zeros(0)), cfrc


def _in_subtree(m, k, root):
    while k > 0:
        if k == root:
            return True
        k = m["body_parentid"][k]
    return False
