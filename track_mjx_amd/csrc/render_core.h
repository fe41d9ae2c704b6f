// csrc/render_core.h — the bodies of the roll-out renderer (DESIGN.md "Rendering"): Stage A poses the model's visible primitives (walker and
// optional ghost) and the frame's camera; Stage B casts one ray per pixel against the frame's primitive table.  TM_DEV functions that also compile
// on the host (tests/hostemu/render_emu.cpp), like wave_align.h.  The render tables live in RModel, a table of their own: DModel has none of them.
//
//   primitive record, TMR_REC = 20 floats: centre [3], rotation world-from-local row-major [9], size [3], rgb [3], type | id << 8 (int bits),
//       ghost flag (int bits);  types: the model compiler's GEOM_* codes
//   camera record, TMR_CAM = 16 floats: origin [3], X [3], Y [3], Z [3], tan(fovy / 2), 3 unused;  the camera looks along -Z, +X right, +Y up
//   body frame of the pose stage's scratch, TMR_BODY = 8 floats: position [3], quaternion [4], 1 unused
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef TM_DEV
#define TM_DEV __device__ __forceinline__
#endif

#define TMR_REC 20
#define TMR_CAM 16
#define TMR_BODY 8
#define TMR_MAXB 72     // bodies
#define TMR_MAXJ 76     // joints
#define TMR_MAXQ 76
#define TMR_MAXG 128    // visible geoms
#define TMR_MAXP 256    // primitives of one frame (walker + ghost): the LDS table of k_render_rays
#define TMR_PLANE 0
#define TMR_SPHERE 2
#define TMR_CAPSULE 3
#define TMR_ELLIPSOID 4
#define TMR_BOX 6
#define TMR_MODE_FIXED 0
#define TMR_MODE_TRACK 1
#define TMR_MODE_TRACKCOM 2
// shading constants (DESIGN.md "Rendering")
#define TMR_CHECKER_CELL 0.5f
#define TMR_CHECKER_A0 0.1f
#define TMR_CHECKER_A1 0.2f
#define TMR_CHECKER_A2 0.3f
#define TMR_CHECKER_B0 0.2f
#define TMR_CHECKER_B1 0.3f
#define TMR_CHECKER_B2 0.4f
#define TMR_SKY0 0.4f
#define TMR_SKY1 0.6f
#define TMR_SKY2 0.8f
#define TMR_GHOST_GREY 0.8f
#define TMR_GHOST_ALPHA 0.2f

struct RModel {
  int nbody, njnt, nq, ngeom, nghost;      // ngeom: visible geoms; nghost: those on the moving tree (what the ghost instance draws)
  int body_parentid[TMR_MAXB], body_jntadr[TMR_MAXB], body_jntnum[TMR_MAXB], body_nsub[TMR_MAXB];
  float body_pos[TMR_MAXB][3], body_quat[TMR_MAXB][4], body_mass[TMR_MAXB], body_ipos[TMR_MAXB][3];
  int jnt_type[TMR_MAXJ], jnt_qposadr[TMR_MAXJ];
  float jnt_pos[TMR_MAXJ][3], jnt_axis[TMR_MAXJ][3], qpos0[TMR_MAXQ];
  int g_body[TMR_MAXG], g_type[TMR_MAXG], g_ghost_slot[TMR_MAXG];      // g_ghost_slot: index among the ghost's records, -1 = not drawn
  float g_size[TMR_MAXG][3], g_pos[TMR_MAXG][3], g_quat[TMR_MAXG][4], g_rgb[TMR_MAXG][3];
};
// the camera as the kernels take it (tmjx_camera_t with the field of view as tan(fovy / 2))
struct RCamera { int body, mode; float offset[3], quat[4], tanhalf; };

TM_DEV int tmr_bits(float f) { int i; __builtin_memcpy(&i, &f, 4); return i; }
TM_DEV float tmr_float(int i) { float f; __builtin_memcpy(&f, &i, 4); return f; }
TM_DEV float tmr_dot(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
TM_DEV void tmr_q2m(float *m, const float *q) {
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2.f * (x * y - w * z); m[2] = 2.f * (x * z + w * y);
  m[3] = 2.f * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2.f * (y * z - w * x);
  m[6] = 2.f * (x * z - w * y); m[7] = 2.f * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
TM_DEV void tmr_qmul(float *o, const float *a, const float *b) {
  const float w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const float y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}
TM_DEV void tmr_qnorm(float *q) {
  const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
// o = p + M v
TM_DEV void tmr_mulv(float *o, const float *M, const float *v, const float *p) {
  const float x = M[0] * v[0] + M[1] * v[1] + M[2] * v[2], y = M[3] * v[0] + M[4] * v[1] + M[5] * v[2], z = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
  o[0] = p[0] + x; o[1] = p[1] + y; o[2] = p[2] + z;
}

// ------------------------------------------------------------------------------------------------------------------ Stage A
// One (frame, instance): the body tree at `qpos` (tools/compile_model.fk: a free joint's quaternion normalised, hinges about jnt_axis at jnt_pos)
// into `body` [nbody][TMR_BODY], then the instance's records into the frame's table `prims`; instance 0 also writes the camera record.
TM_DEV void tmr_pose(const RModel &m, const float *qpos, int inst, float *body, float *prims, const RCamera &cam, float *camrec) {
  body[0] = body[1] = body[2] = 0.f; body[3] = 1.f; body[4] = body[5] = body[6] = body[7] = 0.f;
  for (int b = 1; b < m.nbody; b++) {
    const float *pf = body + m.body_parentid[b] * TMR_BODY;
    float pq[4] = {pf[3], pf[4], pf[5], pf[6]}, R[9], pos[3], quat[4];
    tmr_q2m(R, pq);
    tmr_mulv(pos, R, m.body_pos[b], pf);
    tmr_qmul(quat, pq, m.body_quat[b]);
    for (int j = m.body_jntadr[b], je = j + m.body_jntnum[b]; j < je; j++) {
      const int a = m.jnt_qposadr[j];
      if (m.jnt_type[j] == 0) {
        pos[0] = qpos[a]; pos[1] = qpos[a + 1]; pos[2] = qpos[a + 2];
        quat[0] = qpos[a + 3]; quat[1] = qpos[a + 4]; quat[2] = qpos[a + 5]; quat[3] = qpos[a + 6];
        tmr_qnorm(quat);
      } else {
        float anchor[3], Rq[9], rj[3];
        const float zero[3] = {0.f, 0.f, 0.f};
        tmr_q2m(Rq, quat);
        tmr_mulv(anchor, Rq, m.jnt_pos[j], pos);
        const float half = 0.5f * (qpos[a] - m.qpos0[a]), sn = sinf(half);
        const float rot[4] = {cosf(half), m.jnt_axis[j][0] * sn, m.jnt_axis[j][1] * sn, m.jnt_axis[j][2] * sn};
        tmr_qmul(quat, quat, rot);
        tmr_q2m(Rq, quat);
        tmr_mulv(rj, Rq, m.jnt_pos[j], zero);
        pos[0] = anchor[0] - rj[0]; pos[1] = anchor[1] - rj[1]; pos[2] = anchor[2] - rj[2];
      }
    }
    tmr_qnorm(quat);
    float *f = body + b * TMR_BODY;
    f[0] = pos[0]; f[1] = pos[1]; f[2] = pos[2]; f[3] = quat[0]; f[4] = quat[1]; f[5] = quat[2]; f[6] = quat[3]; f[7] = 0.f;
  }
  for (int g = 0; g < m.ngeom; g++) {
    const int slot = inst ? m.g_ghost_slot[g] : g;
    if (slot < 0) continue;
    const float *f = body + m.g_body[g] * TMR_BODY;
    const float bq[4] = {f[3], f[4], f[5], f[6]};
    float Rb[9], Rg[9];
    tmr_q2m(Rb, bq);
    tmr_q2m(Rg, m.g_quat[g]);
    float *r = prims + (inst ? m.ngeom + slot : slot) * TMR_REC;
    tmr_mulv(r, Rb, m.g_pos[g], f);
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) r[3 + 3 * i + k] = Rb[3 * i] * Rg[k] + Rb[3 * i + 1] * Rg[3 + k] + Rb[3 * i + 2] * Rg[6 + k];
    for (int k = 0; k < 3; k++) { r[12 + k] = m.g_size[g][k]; r[15 + k] = m.g_rgb[g][k]; }
    r[18] = tmr_float(m.g_type[g] | ((g + inst * m.ngeom) << 8));
    r[19] = tmr_float(inst);
  }
  if (inst) return;
  float A[9], org[3];
  if (cam.mode == TMR_MODE_TRACKCOM) {      // origin = subtree_com(body) + offset, world axes fixed (bodies are numbered depth first)
    float tot = 0.f, acc[3] = {0.f, 0.f, 0.f};
    for (int b = cam.body, be = cam.body + m.body_nsub[cam.body]; b < be; b++) {
      const float *f = body + b * TMR_BODY;
      const float bq[4] = {f[3], f[4], f[5], f[6]};
      float Rb[9], c[3];
      tmr_q2m(Rb, bq);
      tmr_mulv(c, Rb, m.body_ipos[b], f);
      tot += m.body_mass[b];
      acc[0] += m.body_mass[b] * c[0]; acc[1] += m.body_mass[b] * c[1]; acc[2] += m.body_mass[b] * c[2];
    }
    org[0] = acc[0] / tot + cam.offset[0]; org[1] = acc[1] / tot + cam.offset[1]; org[2] = acc[2] / tot + cam.offset[2];
    tmr_q2m(A, cam.quat);
  } else {      // fixed: the body frame applied to (offset, quat)
    const float *f = body + cam.body * TMR_BODY;
    const float bq[4] = {f[3], f[4], f[5], f[6]};
    float Rb[9], Rc[9];
    tmr_q2m(Rb, bq);
    tmr_q2m(Rc, cam.quat);
    tmr_mulv(org, Rb, cam.offset, f);
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) A[3 * i + k] = Rb[3 * i] * Rc[k] + Rb[3 * i + 1] * Rc[3 + k] + Rb[3 * i + 2] * Rc[6 + k];
  }
  for (int k = 0; k < 3; k++) { camrec[k] = org[k]; camrec[3 + k] = A[3 * k]; camrec[6 + k] = A[3 * k + 1]; camrec[9 + k] = A[3 * k + 2]; }
  camrec[12] = cam.tanhalf; camrec[13] = camrec[14] = camrec[15] = 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ Stage B
// ray of pixel (column i, row j from the top) through its centre
TM_DEV void tmr_ray(const float *cam, int i, int j, int W, int H, float *o, float *d) {
  const float th = cam[12];
  const float x = (2.f * ((float)i + 0.5f) / (float)W - 1.f) * (th * (float)W / (float)H);
  const float y = (1.f - 2.f * ((float)j + 0.5f) / (float)H) * th;
  float v[3];
  for (int k = 0; k < 3; k++) { o[k] = cam[k]; v[k] = x * cam[3 + k] + y * cam[6 + k] - cam[9 + k]; }
  const float n = sqrtf(tmr_dot(v, v));
  d[0] = v[0] / n; d[1] = v[1] / n; d[2] = v[2] / n;
}

// Entry root of a sphere of radius r at the origin, solved from the ray's point of closest approach (oc + tca d is perpendicular to d: no
// cancellation between |oc|^2 ~ 1 m^2 and r^2 ~ 1 cm^2).  t = inf on a miss; nd = |n . d|.
TM_DEV void tmr_sphere(const float *oc, const float *d, float r, float &t, float &nd) {
  const float tca = -tmr_dot(oc, d);
  const float q[3] = {oc[0] + tca * d[0], oc[1] + tca * d[1], oc[2] + tca * d[2]};
  const float h2 = r * r - tmr_dot(q, q);
  const float te = tca - sqrtf(fmaxf(h2, 0.f));
  const float p[3] = {oc[0] + te * d[0], oc[1] + te * d[1], oc[2] + te * d[2]};
  nd = fabsf(tmr_dot(p, d)) / r;
  t = (h2 >= 0.f && te > 0.f) ? te : INFINITY;
}

// One record against one ray.  `typ` is the record's type (wave-uniform in the kernel: one branch per record, no divergence but the hit test).
TM_DEV void tmr_intersect(const float *r, int typ, const float *o, const float *d, float &t, float &nd) {
  const float oc[3] = {o[0] - r[0], o[1] - r[1], o[2] - r[2]};
  if (typ == TMR_SPHERE) { tmr_sphere(oc, d, r[12], t, nd); return; }
  if (typ == TMR_PLANE) {      // normal = the local z axis (third column)
    const float n[3] = {r[5], r[8], r[11]};
    const float den = tmr_dot(d, n), tp = -tmr_dot(oc, n) / den;
    nd = fabsf(den);
    t = (den != 0.f && tp > 0.f) ? tp : INFINITY;
    return;
  }
  // local = R^T world
  const float ol[3] = {r[3] * oc[0] + r[6] * oc[1] + r[9] * oc[2], r[4] * oc[0] + r[7] * oc[1] + r[10] * oc[2], r[5] * oc[0] + r[8] * oc[1] + r[11] * oc[2]};
  const float dl[3] = {r[3] * d[0] + r[6] * d[1] + r[9] * d[2], r[4] * d[0] + r[7] * d[1] + r[10] * d[2], r[5] * d[0] + r[8] * d[1] + r[11] * d[2]};
  if (typ == TMR_ELLIPSOID) {      // the unit sphere in size-scaled coordinates
    const float os[3] = {ol[0] / r[12], ol[1] / r[13], ol[2] / r[14]}, ds[3] = {dl[0] / r[12], dl[1] / r[13], dl[2] / r[14]};
    const float A = tmr_dot(ds, ds), tca = -tmr_dot(os, ds) / A;
    const float q[3] = {os[0] + tca * ds[0], os[1] + tca * ds[1], os[2] + tca * ds[2]};
    const float h2 = (1.f - tmr_dot(q, q)) / A;
    const float te = tca - sqrtf(fmaxf(h2, 0.f));
    const float g[3] = {(ol[0] + te * dl[0]) / (r[12] * r[12]), (ol[1] + te * dl[1]) / (r[13] * r[13]), (ol[2] + te * dl[2]) / (r[14] * r[14])};
    nd = fabsf(tmr_dot(g, dl)) / sqrtf(tmr_dot(g, g));
    t = (h2 >= 0.f && te > 0.f) ? te : INFINITY;
    return;
  }
  if (typ == TMR_CAPSULE) {      // radius size[0], half length size[1] along local z: the cylinder side, then the two cap spheres
    const float rad = r[12], hh = r[13];
    const float A = dl[0] * dl[0] + dl[1] * dl[1], tca = -(ol[0] * dl[0] + ol[1] * dl[1]) / A;
    const float qx = ol[0] + tca * dl[0], qy = ol[1] + tca * dl[1];
    const float h2 = (rad * rad - (qx * qx + qy * qy)) / A;
    const float ts = tca - sqrtf(fmaxf(h2, 0.f));
    const float z = ol[2] + ts * dl[2];
    t = (A > 0.f && h2 >= 0.f && ts > 0.f && fabsf(z) <= hh) ? ts : INFINITY;
    nd = fabsf((ol[0] + ts * dl[0]) * dl[0] + (ol[1] + ts * dl[1]) * dl[1]) / rad;
    float t2, nd2;
    const float oa[3] = {ol[0], ol[1], ol[2] - hh};
    tmr_sphere(oa, dl, rad, t2, nd2);
    if (t2 < t) { t = t2; nd = nd2; }
    const float ob[3] = {ol[0], ol[1], ol[2] + hh};
    tmr_sphere(ob, dl, rad, t2, nd2);
    if (t2 < t) { t = t2; nd = nd2; }
    return;
  }
  {      // box: slabs
    float lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
      const float inv = 1.f / dl[k], t1 = (-r[12 + k] - ol[k]) * inv, t2 = (r[12 + k] - ol[k]) * inv;
      lo[k] = fminf(t1, t2); hi[k] = fmaxf(t1, t2);
    }
    const float tn = fmaxf(fmaxf(lo[0], lo[1]), lo[2]), tf = fminf(fminf(hi[0], hi[1]), hi[2]);
    nd = lo[0] >= tn ? fabsf(dl[0]) : (lo[1] >= tn ? fabsf(dl[1]) : fabsf(dl[2]));
    t = (tn <= tf && tn > 0.f) ? tn : INFINITY;
  }
}

struct RHit { float t_o, nd_o, t_g, nd_g; int k_o, k_g; };      // nearest opaque / nearest ghost record (k: record index, -1 = none)

#if defined(__HIP_DEVICE_COMPILE__)
#define TMR_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)      // a value every lane of the wave holds: lets the type switch be a scalar branch
#else
#define TMR_UNIFORM(x) (x)
#endif
TM_DEV void tmr_trace(const float *prims, int P, const float *o, const float *d, RHit &h) {
  h.t_o = h.t_g = INFINITY; h.nd_o = h.nd_g = 0.f; h.k_o = h.k_g = -1;
  for (int k = 0; k < P; k++) {
    const float *r = prims + k * TMR_REC;
    const int typ = TMR_UNIFORM(tmr_bits(r[18])) & 255, ghost = TMR_UNIFORM(tmr_bits(r[19]));
    float t, nd;
    tmr_intersect(r, typ, o, d, t, nd);
    if (ghost) { if (t < h.t_g) { h.t_g = t; h.nd_g = nd; h.k_g = k; } }
    else if (t < h.t_o) { h.t_o = t; h.nd_o = nd; h.k_o = k; }
  }
}

// colour (packed r | g << 8 | b << 16 | 255 << 24), depth and reported id of one traced pixel
TM_DEV uint32_t tmr_shade(const float *prims, const RHit &h, const float *o, const float *d, float &depth, int &gid) {
  float c[3] = {TMR_SKY0, TMR_SKY1, TMR_SKY2};
  depth = h.t_o; gid = -1;
  if (h.k_o >= 0) {
    const float *r = prims + h.k_o * TMR_REC;
    const int w = tmr_bits(r[18]);
    const float s = 0.3f + 0.7f * h.nd_o;
    float rgb[3] = {r[15], r[16], r[17]};
    if ((w & 255) == TMR_PLANE) {      // two-colour checker in world xy of the hit point
      const float px = o[0] + h.t_o * d[0], py = o[1] + h.t_o * d[1];
      const float cells = floorf(px / TMR_CHECKER_CELL) + floorf(py / TMR_CHECKER_CELL);
      const bool odd = cells - 2.f * floorf(0.5f * cells) != 0.f;
      rgb[0] = odd ? TMR_CHECKER_B0 : TMR_CHECKER_A0; rgb[1] = odd ? TMR_CHECKER_B1 : TMR_CHECKER_A1; rgb[2] = odd ? TMR_CHECKER_B2 : TMR_CHECKER_A2;
    }
    c[0] = rgb[0] * s; c[1] = rgb[1] * s; c[2] = rgb[2] * s;
    gid = w >> 8;
  }
  if (h.k_g >= 0 && h.t_g < h.t_o) {      // the ghost, once, over what lies behind it
    const float g = TMR_GHOST_GREY * (0.3f + 0.7f * h.nd_g);
    for (int k = 0; k < 3; k++) c[k] = TMR_GHOST_ALPHA * g + (1.f - TMR_GHOST_ALPHA) * c[k];
    depth = h.t_g;
    gid = tmr_bits(prims[h.k_g * TMR_REC + 18]) >> 8;
  }
  uint32_t out = 255u << 24;
  for (int k = 0; k < 3; k++) out |= (uint32_t)floorf(fminf(fmaxf(c[k], 0.f), 1.f) * 255.f + 0.5f) << (8 * k);
  return out;
}
