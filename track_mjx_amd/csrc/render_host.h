// csrc/render_host.h — host side of the renderer: model blob -> RModel (render_core.h) and the blob's named cameras, with every index checked
// here so that the kernels never are handed one out of range.  Plain C++ (no HIP): the test-only host emulation shares it.
#pragma once
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/tmjx.h"
#include "model_host.h"
#include "render_core.h"

namespace tmjx_host {

struct RNamedCamera { std::string name; int body, mode; float pos[3], quat[4], fovy, off0[3], wquat0[4]; };
struct RenderTables { RModel m; std::vector<RNamedCamera> cams; };

// false + empty `err`: the blob has no render tables (no rgeom_type entry); false + message: malformed tables
inline bool build_rmodel(const void *blob, size_t nbytes, RenderTables &out, std::string &err) {
  err.clear();
  Reader R{blob, nbytes, ""};
  const int ng = R.count("rgeom_type");
  if (ng < 0) return false;
  RModel &m = out.m;
  memset(&m, 0, sizeof(RModel));
  int dims[6];
  if (!R.ints("dims", dims, 6)) { err = R.err; return false; }
  m.nbody = dims[0]; m.njnt = dims[1]; m.nq = dims[2]; m.ngeom = ng;
  if (m.nbody < 1 || m.nbody > TMR_MAXB || m.njnt < 0 || m.njnt > TMR_MAXJ || m.nq < 0 || m.nq > TMR_MAXQ || ng < 1 || ng > TMR_MAXG) {
    err = "render tables: the model exceeds the renderer's compiled-in maximum dimensions"; return false;
  }
  bool ok = R.ints("body_parentid", m.body_parentid, m.nbody) && R.ints("body_jntadr", m.body_jntadr, m.nbody) &&
            R.ints("body_jntnum", m.body_jntnum, m.nbody) && R.floats("body_pos", &m.body_pos[0][0], m.nbody * 3) &&
            R.floats("body_quat", &m.body_quat[0][0], m.nbody * 4) && R.floats("body_mass", m.body_mass, m.nbody) &&
            R.floats("body_ipos", &m.body_ipos[0][0], m.nbody * 3) && R.ints("jnt_type", m.jnt_type, m.njnt) &&
            R.ints("jnt_qposadr", m.jnt_qposadr, m.njnt) && R.floats("jnt_pos", &m.jnt_pos[0][0], m.njnt * 3) &&
            R.floats("jnt_axis", &m.jnt_axis[0][0], m.njnt * 3) && R.floats("qpos0", m.qpos0, m.nq) &&
            R.ints("rgeom_body", m.g_body, ng) && R.ints("rgeom_type", m.g_type, ng) && R.floats("rgeom_size", &m.g_size[0][0], ng * 3) &&
            R.floats("rgeom_pos", &m.g_pos[0][0], ng * 3) && R.floats("rgeom_quat", &m.g_quat[0][0], ng * 4);
  std::vector<float> rgba((size_t)ng * 4);
  ok = ok && R.floats("rgeom_rgba", rgba.data(), ng * 4);
  if (!ok) { err = "render tables: " + R.err; return false; }
  std::vector<int> moving(m.nbody, 0);
  for (int b = 1; b < m.nbody; b++) {
    if (m.body_parentid[b] < 0 || m.body_parentid[b] >= b) { err = "render tables: bodies must come after their parents"; return false; }
    const int j0 = m.body_jntadr[b], nj = m.body_jntnum[b];
    if (nj < 0 || (nj > 0 && (j0 < 0 || j0 + nj > m.njnt))) { err = "render tables: body joint range out of bounds"; return false; }
    moving[b] = moving[m.body_parentid[b]];
    for (int j = j0; j < j0 + nj; j++) {
      const int t = m.jnt_type[j], a = m.jnt_qposadr[j];
      if (t != 0 && t != 3) { err = "render tables: only free and hinge joints are posed"; return false; }
      if (a < 0 || a + (t == 0 ? 7 : 1) > m.nq) { err = "render tables: joint qpos address out of range"; return false; }
      if (t == 0) moving[b] = 1;
    }
  }
  m.body_jntnum[0] = 0;
  for (int b = 0; b < m.nbody; b++) {      // subtree = [b, b + nsub): needs depth-first numbering, checked by counting descendants
    int nsub = 1, total = 1;
    for (int c = b + 1; c < m.nbody; c++) {
      bool desc = false;
      for (int a = c; a > b; a = m.body_parentid[a]) if (m.body_parentid[a] == b) { desc = true; break; }
      if (desc) { total++; if (c == b + nsub) nsub++; }
    }
    if (total != nsub) { err = "render tables: body numbering is not depth-first"; return false; }
    m.body_nsub[b] = nsub;
  }
  m.nghost = 0;
  for (int g = 0; g < ng; g++) {
    const int t = m.g_type[g];
    if (m.g_body[g] < 0 || m.g_body[g] >= m.nbody) { err = "rgeom_body: body id out of range"; return false; }
    if (t != TMR_PLANE && t != TMR_SPHERE && t != TMR_CAPSULE && t != TMR_ELLIPSOID && t != TMR_BOX) {
      err = "rgeom_type: geom type " + std::to_string(t) + " is not rendered (plane, sphere, capsule, ellipsoid, box)"; return false;
    }
    for (int k = 0; k < 3; k++) m.g_rgb[g][k] = rgba[(size_t)g * 4 + k];
    m.g_ghost_slot[g] = moving[m.g_body[g]] ? m.nghost++ : -1;
  }
  if (m.ngeom + m.nghost > TMR_MAXP) { err = "render tables: more than " + std::to_string(TMR_MAXP) + " primitives per frame with the ghost"; return false; }
  // cameras (optional)
  out.cams.clear();
  const int nc = R.count("rcam_body");
  if (nc > 0) {
    std::vector<int> name((size_t)nc * 32), body(nc), mode(nc);
    std::vector<float> pos(nc * 3), quat(nc * 4), fovy(nc), off0(nc * 3), wq0(nc * 4);
    ok = R.ints("rcam_name", name.data(), nc * 32) && R.ints("rcam_body", body.data(), nc) && R.ints("rcam_mode", mode.data(), nc) &&
         R.floats("rcam_pos", pos.data(), nc * 3) && R.floats("rcam_quat", quat.data(), nc * 4) && R.floats("rcam_fovy", fovy.data(), nc) &&
         R.floats("rcam_off0", off0.data(), nc * 3) && R.floats("rcam_wquat0", wq0.data(), nc * 4);
    if (!ok) { err = "render tables: " + R.err; return false; }
    for (int i = 0; i < nc; i++) {
      RNamedCamera c;
      for (int k = 0; k < 32 && name[(size_t)i * 32 + k] > 0 && name[(size_t)i * 32 + k] < 256; k++) c.name.push_back((char)name[(size_t)i * 32 + k]);
      if (body[i] < 0 || body[i] >= m.nbody || mode[i] < 0 || mode[i] > 2) { err = "rcam_body / rcam_mode: value out of range for camera " + c.name; return false; }
      c.body = body[i]; c.mode = mode[i]; c.fovy = fovy[i];
      for (int k = 0; k < 3; k++) { c.pos[k] = pos[i * 3 + k]; c.off0[k] = off0[i * 3 + k]; }
      for (int k = 0; k < 4; k++) { c.quat[k] = quat[i * 4 + k]; c.wquat0[k] = wq0[i * 4 + k]; }
      out.cams.push_back(c);
    }
  }
  return true;
}

// ---- argument checks of the C-ABI (include/tmjx.h: tmjx_render_*), shared with the host emulation: "" = fine, else the message
static_assert(TMJX_CAMERA_FIXED == TMR_MODE_FIXED && TMJX_CAMERA_TRACK == TMR_MODE_TRACK && TMJX_CAMERA_TRACKCOM == TMR_MODE_TRACKCOM,
              "include/tmjx.h and csrc/render_core.h disagree");
inline std::string render_check_camera(const RModel &m, const tmjx_camera_t *cam, RCamera &out) {
  if (!cam) return "null camera";
  if (cam->body < 0 || cam->body >= m.nbody) return "camera body " + std::to_string(cam->body) + " is out of range";
  if (cam->mode == TMJX_CAMERA_TRACK) return "camera mode track is not rendered (fixed and trackcom are)";
  if (cam->mode != TMJX_CAMERA_FIXED && cam->mode != TMJX_CAMERA_TRACKCOM) return "unknown camera mode " + std::to_string(cam->mode);
  if (!(cam->fovy > 0.f && cam->fovy < 180.f)) return "camera fovy must be in (0, 180) degrees";
  const float n2 = cam->quat[0] * cam->quat[0] + cam->quat[1] * cam->quat[1] + cam->quat[2] * cam->quat[2] + cam->quat[3] * cam->quat[3];
  if (!(fabsf(n2 - 1.f) < 1e-3f)) return "camera quaternion is not of unit length";
  if (cam->mode == TMJX_CAMERA_TRACKCOM) {
    float tot = 0.f;
    for (int b = cam->body; b < cam->body + m.body_nsub[cam->body]; b++) tot += m.body_mass[b];
    if (!(tot > 0.f)) return "a trackcom camera needs a body whose subtree has mass";
  }
  out.body = cam->body; out.mode = cam->mode;
  for (int k = 0; k < 3; k++) out.offset[k] = cam->offset[k];
  for (int k = 0; k < 4; k++) out.quat[k] = cam->quat[k];
  out.tanhalf = (float)tan((double)cam->fovy * 3.14159265358979323846 / 360.0);
  return "";
}
inline std::string render_check_frames(int F, int F_ghost, const float *qpos, const float *qpos_ghost) {
  if (F < 1) return "F must be >= 1 (got " + std::to_string(F) + ")";
  if (!qpos) return "null qpos";
  if (qpos_ghost && F_ghost != F) return "ghost frames: " + std::to_string(F_ghost) + " frames against " + std::to_string(F) + " of the walker";
  if (F > (1 << 20)) return "more than 2^20 frames in one call";
  return "";
}
inline std::string render_check_image(int W, int H) {
  if (W < 1 || H < 1) return "W and H must be >= 1 (got " + std::to_string(W) + " x " + std::to_string(H) + ")";
  if (W > 16384 || H > 16384) return "image larger than 16384 x 16384";
  return "";
}
inline std::string render_check_rays(const float *prims, const float *cams, int F, int P, int W, int H, const void *rgba, const void *depth, const void *geom_id) {
  if (F < 1) return "F must be >= 1 (got " + std::to_string(F) + ")";
  std::string e = render_check_image(W, H);
  if (!e.empty()) return e;
  if (P < 1 || P > TMR_MAXP) return "1 .. " + std::to_string(TMR_MAXP) + " primitives per frame (got " + std::to_string(P) + ")";
  if (!prims || !cams || !rgba) return "null argument";
  if (((uintptr_t)prims & 15) || (((uintptr_t)cams | (uintptr_t)rgba | (uintptr_t)depth | (uintptr_t)geom_id) & 3))
    return "prims must be 16-byte aligned, the other buffers 4-byte aligned";
  return "";
}
inline void render_info(const RenderTables &t, int F, int ghost, tmjx_render_info_t *out) {
  const RModel &r = t.m;
  out->ngeom = r.ngeom; out->ncam = (int)t.cams.size(); out->rec_floats = TMR_REC; out->cam_floats = TMR_CAM;
  out->nprim = r.ngeom + (ghost ? r.nghost : 0);
  out->prims_offset = (int64_t)F * TMR_CAM;
  out->workspace_floats = (int64_t)F * TMR_CAM + (int64_t)F * out->nprim * TMR_REC + (int64_t)F * (ghost ? 2 : 1) * r.nbody * TMR_BODY;
}
inline std::string render_find_camera(const RenderTables &t, const char *name, tmjx_camera_t *out) {
  std::string have;
  for (const RNamedCamera &c : t.cams) {
    have += (have.empty() ? "" : ", ") + c.name;
    if (c.name != name) continue;
    if (c.mode == TMR_MODE_TRACK) return std::string("camera ") + name + ": mode track is not rendered (fixed and trackcom are)";
    const bool com = c.mode == TMR_MODE_TRACKCOM;      // trackcom: what the camera has at qpos0 (world offset from the subtree com, world axes)
    out->body = c.body; out->mode = c.mode; out->fovy = c.fovy;
    for (int k = 0; k < 3; k++) out->offset[k] = com ? c.off0[k] : c.pos[k];
    for (int k = 0; k < 4; k++) out->quat[k] = com ? c.wquat0[k] : c.quat[k];
    return "";
  }
  return std::string("unknown camera '") + name + "' (the model has: " + (have.empty() ? "none" : have) + ")";
}
#define TMR_NO_TABLES "the handle has no render tables: its blob carries no rgeom_* entries (the model's <stem>.render.tmjx.txt side file)"

}  // namespace tmjx_host
