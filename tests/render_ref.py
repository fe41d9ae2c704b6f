"""Float64 restatement of the roll-out renderer (DESIGN.md "Rendering"), written from its definitions: kinematics as tools/compile_model.fk,
pinhole rays, the five analytic ray intersections, headlight shading, the floor checker and the one-layer ghost composite.  `dtype=np.float32`
runs the same expressions in float32: the error of that run against the float64 run is what the tests derive their bounds from.

Nothing here reads track_mjx_amd/csrc.  Conventions restated:
  primitive record, REC = 20 floats: centre [3], rotation world-from-local row-major [9], size [3], rgb [3], type + 256 * id (int32 bits),
      ghost flag (int32 bits, 0 | 1);  types are the compiler's GEOM_* codes (plane 0, sphere 2, capsule 3, ellipsoid 4, box 6)
  camera record, CAM = 16 floats: origin [3], X [3], Y [3], Z [3], tan(fovy / 2), 3 unused;  the camera looks along -Z, +X right, +Y up
  pixel (column i, row j from the top) + offset (u, v) in [0, 1]^2:
      x = (2 (i + u) / W - 1) tan(fovy / 2) W / H,  y = (1 - 2 (j + v) / H) tan(fovy / 2),  d = normalise(x X + y Y - Z)
  a convex primitive is hit where the ray ENTERS it at t > 0 (a camera inside a primitive does not see it); a plane from either side at t > 0
  shade s = 0.3 + 0.7 |n . d|;  opaque colour rgb s;  floor (every plane) checker of CHECKER_CELL in world xy of the hit point;  miss = SKY
  ghost: colour GHOST_RGB s, alpha GHOST_ALPHA, composited once over what lies behind when its nearest hit is nearer than the opaque hit
  uint8 level = floor(clip(c, 0, 1) 255 + 0.5)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))
import compile_model as cm  # noqa: E402

REC, CAM = 20, 16
PLANE, SPHERE, CAPSULE, ELLIPSOID, BOX = 0, 2, 3, 4, 6
CHECKER_CELL = 0.5
CHECKER_A, CHECKER_B = (0.1, 0.2, 0.3), (0.2, 0.3, 0.4)
SKY = (0.4, 0.6, 0.8)
GHOST_RGB, GHOST_ALPHA = (0.8, 0.8, 0.8), 0.2
MODE_FIXED, MODE_TRACK, MODE_TRACKCOM = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------------ model
def model_of(entries) -> dict:
    """walker.model (flat blob entries) -> the dict tools/compile_model.fk reads, plus the render tables."""
    e = entries
    nbody, njnt = int(e["dims"][0]), int(e["dims"][1])
    m = dict(nbody=nbody, njnt=njnt, nq=int(e["dims"][2]))
    for k in ("body_parentid", "body_jntadr", "body_jntnum", "jnt_type", "jnt_qposadr"):
        m[k] = np.asarray(e[k], int)
    for k, w in (("body_pos", 3), ("body_quat", 4), ("body_ipos", 3), ("jnt_pos", 3), ("jnt_axis", 3)):
        m[k] = np.asarray(e[k], np.float64).reshape(-1, w)
    m["body_mass"], m["qpos0"] = np.asarray(e["body_mass"], np.float64), np.asarray(e["qpos0"], np.float64)
    n = len(e["rgeom_type"])
    m["rgeom_body"], m["rgeom_type"] = np.asarray(e["rgeom_body"], int), np.asarray(e["rgeom_type"], int)
    for k, w in (("size", 3), ("pos", 3), ("quat", 4), ("rgba", 4)):
        m[f"rgeom_{k}"] = np.asarray(e[f"rgeom_{k}"], np.float64).reshape(n, w)
    moving = np.zeros(nbody, bool)      # below a free joint: what the ghost instance draws
    for b in range(1, nbody):
        free = any(m["jnt_type"][j] == cm.JNT_FREE for j in range(m["body_jntadr"][b], m["body_jntadr"][b] + m["body_jntnum"][b])) \
            if m["body_jntnum"][b] else False
        moving[b] = free or moving[m["body_parentid"][b]]
    m["body_moving"] = moving
    return m


def _q2m(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=q.dtype)


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], dtype=a.dtype)


def fk(m, qpos, dtype=np.float64):
    """tools/compile_model.fk's body frames with every operand and result in `dtype` (float64: cm.fk's numbers to the last bit)."""
    T = dtype
    qpos = np.asarray(qpos, T)
    nb = m["nbody"]
    xpos, xquat = np.zeros((nb, 3), T), np.tile(np.array([1, 0, 0, 0], T), (nb, 1))
    for b in range(1, nb):
        p = m["body_parentid"][b]
        pos = xpos[p] + _q2m(xquat[p]) @ m["body_pos"][b].astype(T)
        quat = _qmul(xquat[p], m["body_quat"][b].astype(T))
        for j in range(m["body_jntadr"][b], m["body_jntadr"][b] + m["body_jntnum"][b]) if m["body_jntnum"][b] else []:
            a = m["jnt_qposadr"][j]
            if m["jnt_type"][j] == cm.JNT_FREE:
                pos = qpos[a:a + 3].copy()
                q = qpos[a + 3:a + 7]
                quat = q / np.sqrt((q * q).sum(dtype=T))
            else:
                anchor = _q2m(quat) @ m["jnt_pos"][j].astype(T) + pos
                ang = (qpos[a] - T(m["qpos0"][a])) * T(0.5)
                quat = _qmul(quat, np.concatenate([[np.cos(ang)], m["jnt_axis"][j].astype(T) * np.sin(ang)]).astype(T))
                pos = anchor - _q2m(quat) @ m["jnt_pos"][j].astype(T)
        xpos[b], xquat[b] = pos, quat / np.sqrt((quat * quat).sum(dtype=T))
    return xpos, xquat


def pose_prims(m, qpos, qpos_ghost=None, dtype=np.float64):
    """World-space primitive table [P][REC] of one frame: every visible geom at `qpos`, then (ghost) the geoms of the moving tree at
    `qpos_ghost` with id + visible count and the ghost flag."""
    T = dtype
    nvis = len(m["rgeom_type"])
    out = []
    for inst, q in enumerate([qpos] if qpos_ghost is None else [qpos, qpos_ghost]):
        xpos, xquat = fk(m, q, T)
        for g in range(nvis):
            b = m["rgeom_body"][g]
            if inst and not m["body_moving"][b]:
                continue
            Rb = _q2m(xquat[b])
            r = np.zeros(REC, T)
            r[0:3] = xpos[b] + Rb @ m["rgeom_pos"][g].astype(T)
            r[3:12] = (Rb @ _q2m(m["rgeom_quat"][g].astype(T))).ravel()
            r[12:15], r[15:18] = m["rgeom_size"][g], m["rgeom_rgba"][g, :3]
            r[18], r[19] = m["rgeom_type"][g] + 256 * (g + inst * nvis), inst      # kept as numbers here; pack_prims writes the int32 bits
            out.append(r)
    return np.array(out)


def n_prims(m, ghost: bool) -> int:
    return len(m["rgeom_type"]) + (int(m["body_moving"][m["rgeom_body"]].sum()) if ghost else 0)


def subtree_com(m, qpos, body, dtype=np.float64):
    T = dtype
    xpos, xquat = fk(m, qpos, T)
    tot, acc = T(0), np.zeros(3, T)
    for b in range(body, m["nbody"]):
        a = b
        while a > body:
            a = m["body_parentid"][a]
        if a != body:
            continue
        tot = tot + T(m["body_mass"][b])
        acc = acc + T(m["body_mass"][b]) * (xpos[b] + _q2m(xquat[b]) @ m["body_ipos"][b].astype(T))
    return acc / tot


def camera_record(m, cam, qpos, dtype=np.float64):
    """cam: {body, mode, offset, quat, fovy}.  trackcom: origin = subtree_com(body) + offset, axes = quat (world, fixed); fixed: the body frame
    applied to (offset, quat)."""
    T = dtype
    r = np.zeros(CAM, T)
    off, quat = np.asarray(cam["offset"], T), np.asarray(cam["quat"], T)
    if cam["mode"] == MODE_TRACKCOM:
        r[0:3] = subtree_com(m, qpos, cam["body"], T) + off
        A = _q2m(quat)
    elif cam["mode"] == MODE_FIXED:
        xpos, xquat = fk(m, qpos, T)
        Rb = _q2m(xquat[cam["body"]])
        r[0:3] = xpos[cam["body"]] + Rb @ off
        A = Rb @ _q2m(quat)
    else:
        raise NotImplementedError("camera mode track")
    r[3:6], r[6:9], r[9:12] = A[:, 0], A[:, 1], A[:, 2]
    r[12] = T(np.tan(np.float64(cam["fovy"]) * np.pi / 360.0))
    return r


def named_camera(walker, name) -> dict:
    c = walker.cameras()[name]
    code = {"fixed": MODE_FIXED, "track": MODE_TRACK, "trackcom": MODE_TRACKCOM}[c["mode"]]
    track = code == MODE_TRACKCOM
    return dict(body=c["body"], mode=code, offset=c["off0"] if track else c["pos"], quat=c["wquat0"] if track else c["quat"], fovy=c["fovy"])


def pack_prims(prims) -> np.ndarray:
    """[..., REC] numbers -> the float32 records the C-ABI takes (words 18, 19 as int32 bits)."""
    p = np.asarray(prims)
    out = np.ascontiguousarray(p, np.float32)
    iv = out.view(np.int32)
    iv[..., 18] = np.rint(p[..., 18]).astype(np.int32)
    iv[..., 19] = np.rint(p[..., 19]).astype(np.int32)
    return out


# ------------------------------------------------------------------------------------------------------------------ rays
def rays(cam, W, H, offset=(0.5, 0.5), dtype=np.float64, corners=False):
    """Rays through pixel + offset of every pixel [H * W]; corners=True: through the (H + 1) * (W + 1) pixel corners instead."""
    T = dtype
    cam = np.asarray(cam, T)
    if corners:
        offset = (0.0, 0.0)
    i, j = np.meshgrid(np.arange(W + int(corners), dtype=T), np.arange(H + int(corners), dtype=T))
    th = cam[12]
    x = (T(2) * (i + T(offset[0])) / T(W) - T(1)) * (th * T(W) / T(H))
    y = (T(1) - T(2) * (j + T(offset[1])) / T(H)) * th
    d = x[..., None] * cam[3:6] + y[..., None] * cam[6:9] - cam[9:12]
    d = d / np.sqrt((d * d).sum(-1, dtype=T))[..., None]
    return np.broadcast_to(cam[0:3], d.shape).reshape(-1, 3).astype(T), d.reshape(-1, 3).astype(T)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _sphere(oc, d, r):
    """Entry root from the point of closest approach; returns (t or inf, |n . d|)."""
    tca = -_dot(oc, d)
    q = oc + tca[:, None] * d
    h2 = r * r - _dot(q, q)
    t = tca - np.sqrt(np.maximum(h2, 0))
    ok = (h2 >= 0) & (t > 0)
    nd = np.abs(_dot(oc + t[:, None] * d, d)) / r
    return np.where(ok, t, np.inf).astype(oc.dtype), nd


def intersect(rec, o, d):
    """One primitive against N rays: (t [N] with inf = miss, |n . d| [N])."""
    T = o.dtype.type
    c, R, size = rec[0:3].astype(T), rec[3:12].reshape(3, 3).astype(T), rec[12:15].astype(T)
    typ = int(round(float(rec[18]))) % 256
    oc = o - c
    with np.errstate(all="ignore"):
        if typ == SPHERE:
            return _sphere(oc, d, size[0])
        if typ == PLANE:
            n = R[:, 2]
            den = d @ n
            t = -(oc @ n) / den
            ok = (den != 0) & (t > 0)
            return np.where(ok, t, np.inf).astype(T), np.abs(den)
        ol, dl = oc @ R, d @ R      # local = R^T world
        if typ == ELLIPSOID:
            os_, ds_ = ol / size, dl / size
            A = _dot(ds_, ds_)
            tca = -_dot(os_, ds_) / A
            q = os_ + tca[:, None] * ds_
            h2 = (T(1) - _dot(q, q)) / A
            t = tca - np.sqrt(np.maximum(h2, 0))
            ok = (h2 >= 0) & (t > 0)
            g = (ol + t[:, None] * dl) / (size * size)
            nd = np.abs(_dot(g, dl)) / np.sqrt(_dot(g, g))
            return np.where(ok, t, np.inf).astype(T), nd
        if typ == CAPSULE:
            r, hh = size[0], size[1]
            A = dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1]
            tca = -(ol[:, 0] * dl[:, 0] + ol[:, 1] * dl[:, 1]) / A
            qx, qy = ol[:, 0] + tca * dl[:, 0], ol[:, 1] + tca * dl[:, 1]
            h2 = (r * r - (qx * qx + qy * qy)) / A
            ts = tca - np.sqrt(np.maximum(h2, 0))
            z = ol[:, 2] + ts * dl[:, 2]
            ok = (A > 0) & (h2 >= 0) & (ts > 0) & (np.abs(z) <= hh)
            t = np.where(ok, ts, np.inf).astype(T)
            nd = np.abs((ol[:, 0] + ts * dl[:, 0]) * dl[:, 0] + (ol[:, 1] + ts * dl[:, 1]) * dl[:, 1]) / r
            for sgn in (1.0, -1.0):
                oc2 = ol.copy()
                oc2[:, 2] = oc2[:, 2] - T(sgn) * hh
                t2, nd2 = _sphere(oc2, dl, r)
                better = t2 < t
                t, nd = np.where(better, t2, t), np.where(better, nd2, nd)
            return t, nd
        if typ == BOX:
            inv = T(1) / dl
            t1, t2 = (-size - ol) * inv, (size - ol) * inv
            lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
            tn = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
            tf = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
            ok = (tn <= tf) & (tn > 0)
            nd = np.where(lo[:, 0] >= tn, np.abs(dl[:, 0]), np.where(lo[:, 1] >= tn, np.abs(dl[:, 1]), np.abs(dl[:, 2])))
            return np.where(ok, tn, np.inf).astype(T), nd
    raise NotImplementedError(f"primitive type {typ}")


def trace(prims, o, d):
    """Nearest opaque and nearest ghost hit of N rays over the table (first record wins a tie):
    dict t_o, k_o (record index, -1 = miss), nd_o, t_g, k_g, nd_g."""
    N, T = len(o), o.dtype.type
    res = {}
    for tag in ("o", "g"):
        res["t_" + tag], res["k_" + tag], res["nd_" + tag] = np.full(N, np.inf, T), np.full(N, -1), np.zeros(N, T)
    for k, rec in enumerate(prims):
        tag = "g" if int(round(float(rec[19]))) else "o"
        t, nd = intersect(rec, o, d)
        better = t < res["t_" + tag]
        res["t_" + tag] = np.where(better, t, res["t_" + tag])
        res["k_" + tag] = np.where(better, k, res["k_" + tag])
        res["nd_" + tag] = np.where(better, nd, res["nd_" + tag])
    return res


def shade(prims, o, d, tr):
    """Float colour [N, 3], depth [N] and reported id [N] from a trace."""
    T = o.dtype.type
    prims = np.asarray(prims)
    N = len(o)
    col = np.broadcast_to(np.array(SKY, T), (N, 3)).copy()
    hit = tr["k_o"] >= 0
    k = np.where(hit, tr["k_o"], 0)
    s = T(0.3) + T(0.7) * tr["nd_o"]
    rgb = prims[k, 15:18].astype(T)
    plane = (np.rint(prims[k, 18]).astype(int) % 256) == PLANE
    with np.errstate(all="ignore"):
        p = o + np.where(hit, tr["t_o"], 0)[:, None].astype(T) * d
        cells = np.floor(p[:, 0] / T(CHECKER_CELL)) + np.floor(p[:, 1] / T(CHECKER_CELL))
        par = np.where(cells - T(2) * np.floor(T(0.5) * cells) != 0, 1, 0)
    rgb = np.where(plane[:, None], np.where(par[:, None] == 1, np.array(CHECKER_B, T), np.array(CHECKER_A, T)), rgb)
    col = np.where(hit[:, None], rgb * s[:, None], col).astype(T)
    front = (tr["k_g"] >= 0) & (tr["t_g"] < tr["t_o"])
    gs = T(0.3) + T(0.7) * tr["nd_g"]
    gcol = np.array(GHOST_RGB, T) * gs[:, None]
    col = np.where(front[:, None], T(GHOST_ALPHA) * gcol + T(1 - GHOST_ALPHA) * col, col).astype(T)
    depth = np.where(front, tr["t_g"], tr["t_o"])
    ids = np.rint(prims[:, 18]).astype(np.int64) // 256
    gid = np.where(front, ids[np.where(front, tr["k_g"], 0)], np.where(hit, ids[k], -1))
    return col, depth, gid


def to_u8(col):
    return np.floor(np.clip(col, 0, 1) * col.dtype.type(255) + col.dtype.type(0.5)).astype(np.uint8)


def render(prims, cam, W, H, dtype=np.float64, offset=(0.5, 0.5)):
    """One frame: dict rgb uint8 [H, W, 3], depth [H, W], geom_id [H, W], k_o / k_g (record indices, -1 = none) [H, W], blended bool [H, W]."""
    o, d = rays(cam, W, H, offset, dtype)
    tr = trace(prims, o, d)
    col, depth, gid = shade(prims, o, d, tr)
    sh = (H, W)
    return dict(rgb=to_u8(col).reshape(H, W, 3), depth=depth.reshape(sh), geom_id=gid.reshape(sh), k_o=tr["k_o"].reshape(sh), k_g=tr["k_g"].reshape(sh),
                blended=((tr["k_g"] >= 0) & (tr["t_g"] < tr["t_o"])).reshape(sh))


def interior(prims, cam, W, H, centre=None):
    """Pixels whose float64 (opaque record, ghost record) pair is the same at the centre and at the four corners."""
    c = render(prims, cam, W, H) if centre is None else centre
    o, d = rays(cam, W, H, corners=True)      # every corner once: it is shared by up to four pixels
    tr = trace(prims, o, d)
    ko, kg = tr["k_o"].reshape(H + 1, W + 1), tr["k_g"].reshape(H + 1, W + 1)
    ok = np.ones((H, W), bool)
    for dj, di in ((0, 0), (0, 1), (1, 0), (1, 1)):
        ok &= (ko[dj:dj + H, di:di + W] == c["k_o"]) & (kg[dj:dj + H, di:di + W] == c["k_g"])
    return ok
