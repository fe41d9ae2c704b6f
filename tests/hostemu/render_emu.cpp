// tests/hostemu/render_emu.cpp — TEST-ONLY host emulation of the renderer's C-ABI (include/tmjx.h: tmjx_render_*): the kernel bodies of
// csrc/render_core.h and the argument checks of csrc/render_host.h compiled with g++, one loop iteration where the GPU has one thread.  Built
// like the other emulations; nothing in track_mjx_amd/ loads it.  With -DRENDER_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   render_emu <packed model blob> — renders qpos0 with a ghost from every named camera at 33 x 17, and the tables again through the Stage B
//   entry point at 1 x 1, and prints a checksum.
#define TM_HOST_EMU 1
#define TM_DEV static inline
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../track_mjx_amd/csrc/render_host.h"

using namespace tmjx_host;
static std::string g_err;
static int fail(const std::string &e) { g_err = e; return -22; }
#define EMU_TRY(expr) do { const std::string e_ = (expr); if (!e_.empty()) return fail(e_); } while (0)

struct RenderEmu { bool has; RenderTables t; };

extern "C" {
const char *remu_last_error() { return g_err.c_str(); }
RenderEmu *remu_create(const void *blob, size_t n) {
  RenderEmu *h = new RenderEmu();
  h->has = build_rmodel(blob, n, h->t, g_err);
  if (!h->has && !g_err.empty()) { delete h; return nullptr; }
  return h;
}
void remu_destroy(RenderEmu *h) { delete h; }
int remu_info(const RenderEmu *h, int F, int ghost, tmjx_render_info_t *out) {
  if (!h->has) return fail(TMR_NO_TABLES);
  if (F < 1) return fail("F must be >= 1 (got " + std::to_string(F) + ")");
  render_info(h->t, F, ghost, out);
  return 0;
}
int remu_camera(const RenderEmu *h, const char *name, tmjx_camera_t *out) {
  if (!h->has) return fail(TMR_NO_TABLES);
  EMU_TRY(render_find_camera(h->t, name, out));
  return 0;
}
static void pose(const RenderEmu *h, const float *qpos, const float *qg, int F, const RCamera &cam, float *ws) {
  const RModel &m = h->t.m;
  const int ninst = qg ? 2 : 1, P = m.ngeom + (qg ? m.nghost : 0);
  float *cams = ws, *prims = ws + (size_t)F * TMR_CAM, *bodies = prims + (size_t)F * P * TMR_REC;
  for (int tid = 0; tid < F * ninst; tid++) {
    const int f = tid / ninst, inst = tid % ninst;
    tmr_pose(m, (inst ? qg : qpos) + (size_t)f * m.nq, inst, bodies + (size_t)tid * m.nbody * TMR_BODY, prims + (size_t)f * P * TMR_REC, cam,
             cams + (size_t)f * TMR_CAM);
  }
}
static int rays(const float *prims, const float *cams, int F, int P, int W, int H, uint8_t *rgba, float *depth, int32_t *gid) {
  EMU_TRY(render_check_rays(prims, cams, F, P, W, H, rgba, depth, gid));
  for (int f = 0; f < F; f++)
    for (int py = 0; py < H; py++)
      for (int px = 0; px < W; px++) {
        float o[3], d[3], dep;
        int id;
        RHit hit;
        const float *tab = prims + (size_t)f * P * TMR_REC;
        tmr_ray(cams + (size_t)f * TMR_CAM, px, py, W, H, o, d);
        tmr_trace(tab, P, o, d, hit);
        const uint32_t c = tmr_shade(tab, hit, o, d, dep, id);
        const size_t at = ((size_t)f * H + py) * W + px;
        memcpy(rgba + 4 * at, &c, 4);
        if (depth) depth[at] = dep;
        if (gid) gid[at] = id;
      }
  return 0;
}
int remu_pose(const RenderEmu *h, const float *qpos, const float *qg, int F, int Fg, const tmjx_camera_t *cam, float *ws) {
  if (!h->has) return fail(TMR_NO_TABLES);
  RCamera rc;
  EMU_TRY(render_check_frames(F, Fg, qpos, qg));
  EMU_TRY(render_check_camera(h->t.m, cam, rc));
  if (!ws || ((uintptr_t)ws & 15)) return fail("the workspace must be a 16-byte aligned buffer of the info call's size");
  pose(h, qpos, qg, F, rc, ws);
  return 0;
}
int remu_prims(const float *prims, const float *cams, int F, int P, int W, int H, uint8_t *rgba, float *depth, int32_t *gid) {
  return rays(prims, cams, F, P, W, H, rgba, depth, gid);
}
int remu_render(const RenderEmu *h, const float *qpos, const float *qg, int F, int Fg, const tmjx_camera_t *cam, int W, int H, float *ws, uint8_t *rgba,
                float *depth, int32_t *gid) {
  if (!h->has) return fail(TMR_NO_TABLES);
  RCamera rc;
  EMU_TRY(render_check_frames(F, Fg, qpos, qg));
  EMU_TRY(render_check_camera(h->t.m, cam, rc));
  if (!ws || ((uintptr_t)ws & 15)) return fail("the workspace must be a 16-byte aligned buffer of the info call's size");
  const int P = h->t.m.ngeom + (qg ? h->t.m.nghost : 0);
  EMU_TRY(render_check_rays(ws + (size_t)F * TMR_CAM, ws, F, P, W, H, rgba, depth, gid));
  pose(h, qpos, qg, F, rc, ws);
  return rays(ws + (size_t)F * TMR_CAM, ws, F, P, W, H, rgba, depth, gid);
}
}  // extern "C"

#ifdef RENDER_EMU_MAIN
int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: render_emu <packed model blob>\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<unsigned char> blob;
  unsigned char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
  fclose(f);
  RenderEmu *h = remu_create(blob.data(), blob.size());
  if (!h || !h->has) { fprintf(stderr, "no render tables: %s\n", g_err.c_str()); return 1; }
  const int F = 2, W = 33, H = 17, nq = h->t.m.nq;
  std::vector<float> q((size_t)F * nq), qg((size_t)F * nq);
  for (int k = 0; k < F * nq; k++) { q[k] = h->t.m.qpos0[k % nq] + 0.01f * (k / nq); qg[k] = q[k] + ((k % nq) == 0 ? 0.05f : 0.02f * ((k % nq) > 6)); }
  tmjx_render_info_t info;
  if (remu_info(h, F, 1, &info)) return 1;
  std::vector<float> ws((size_t)info.workspace_floats + 4), depth((size_t)F * W * H);
  float *wsa = (float *)(((uintptr_t)ws.data() + 15) & ~(uintptr_t)15);
  std::vector<uint8_t> rgba((size_t)F * W * H * 4);
  std::vector<int32_t> gid((size_t)F * W * H);
  unsigned long long sum = 0;
  int hits = 0;
  for (const RNamedCamera &c : h->t.cams) {
    tmjx_camera_t cam;
    if (remu_camera(h, c.name.c_str(), &cam)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    if (remu_render(h, q.data(), qg.data(), F, F, &cam, W, H, wsa, rgba.data(), depth.data(), gid.data())) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    for (uint8_t v : rgba) sum += v;
    for (int32_t v : gid) hits += v >= 0;
    if (remu_prims(wsa + info.prims_offset, wsa, F, info.nprim, 1, 1, rgba.data(), depth.data(), gid.data())) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    sum += rgba[0];
  }
  printf("render_emu: %d cameras, %d primitives, checksum %llu, %d pixels hit\n", (int)h->t.cams.size(), info.nprim, sum, hits);
  remu_destroy(h);
  return hits > 0 ? 0 : 1;
}
#endif
