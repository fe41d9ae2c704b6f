// csrc/tmjx_render.hip — the roll-out renderer's translation unit (include/tmjx.h: tmjx_render_*): k_render_pose (Stage A: one thread per
// (frame, instance) walks the body tree and writes the frame's world-space primitive table and camera), k_render_rays (Stage B: one workgroup per
// pixel tile of one frame, the frame's table in LDS, one ray per thread).  The bodies are csrc/render_core.h; the tables a handle carries are
// built by csrc/render_host.h at tmjx_model_create and owned through the two tmjx_internal_render_* hooks below.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "render_host.h"

// pixel tile of one wave: TMJX_RENDER_TILE_X x (64 / TMJX_RENDER_TILE_X), 16 x 4 or 8 x 8.  16 x 4 by measurement (profiles/render_bench.txt: equal
// within the spread at 640 x 480, 4 % faster at 152 x 113, whose 32 x 8 workgroup tiles waste fewer lanes past the image edge than 16 x 16 ones)
#ifndef TMJX_RENDER_TILE_X
#define TMJX_RENDER_TILE_X 16
#endif


struct RenderHandle {
  tmjx_host::RenderTables t;
  RModel *d = nullptr;      // device copy of t.m
};

extern "C" const void *tmjx_internal_render(const tmjx_model *m);      // tmjx_hip.hip: the handle's RenderHandle, or null

// tmjx_model_create's hook: *out = the handle's render tables, null for a blob without them; a malformed table is an error
extern "C" int tmjx_internal_render_create(const void *blob, size_t nbytes, void **out) {
  *out = nullptr;
  RenderHandle *h = new RenderHandle();
  std::string err;
  if (!tmjx_host::build_rmodel(blob, nbytes, h->t, err)) {
    delete h;
    return err.empty() ? TMJX_OK : fail(TMJX_EINVAL, err);
  }
  hipError_t e = hipMalloc((void **)&h->d, sizeof(RModel));
  if (e != hipSuccess) { delete h; return fail(TMJX_ENOMEM, std::string("hipMalloc(RModel): ") + hipGetErrorString(e)); }
  e = hipMemcpy(h->d, &h->t.m, sizeof(RModel), hipMemcpyHostToDevice);
  if (e != hipSuccess) { hipFree(h->d); delete h; return fail(TMJX_EHIP, std::string("hipMemcpy(RModel): ") + hipGetErrorString(e)); }
  *out = h;
  return TMJX_OK;
}
extern "C" void tmjx_internal_render_destroy(void *p) {
  RenderHandle *h = (RenderHandle *)p;
  if (!h) return;
  if (h->d) hipFree(h->d);
  delete h;
}

// ----------------------------------------------------------------------------------------------- kernels
// Stage A.  Workspace: [F][TMR_CAM] cameras | [F][P][TMR_REC] primitive tables | [F][ninst][nbody][TMR_BODY] body frames (this stage's scratch:
// each thread writes its bodies' frames and reads its parents' back, so no per-thread array is indexed at run time).
__global__ __launch_bounds__(64) void k_render_pose(const RModel *__restrict__ mp, const float *__restrict__ qpos, const float *__restrict__ qghost, int F,
                                                    int ninst, int P, RCamera cam, float *ws) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= F * ninst) return;
  const int f = tid / ninst, inst = tid % ninst;
  const RModel &m = *mp;
  float *cams = ws, *prims = ws + (size_t)F * TMR_CAM, *bodies = prims + (size_t)F * P * TMR_REC;
  tmr_pose(m, (inst ? qghost : qpos) + (size_t)f * m.nq, inst, bodies + (size_t)tid * m.nbody * TMR_BODY, prims + (size_t)f * P * TMR_REC, cam,
           cams + (size_t)f * TMR_CAM);
}

// Stage B.  256 threads = four waves, each a WX x WY pixel tile (WX * WY = 64), the workgroup 2 x 2 of them.  Every lane walks the whole table:
// the record address is the same in every lane (an LDS broadcast), the type switch a scalar branch.
template <int WX, int WY>
__global__ __launch_bounds__(256) void k_render_rays(const float *__restrict__ prims, const float *__restrict__ cams, int P, int W, int H, int tiles_x,
                                                     int tiles, uint32_t *__restrict__ rgba, float *__restrict__ depth, int *__restrict__ geom_id) {
  static_assert(WX * WY == 64, "one wave per tile");
  __shared__ float4 s_prim[TMR_MAXP * TMR_REC / 4];
  __shared__ float s_cam[TMR_CAM];
  const int frame = blockIdx.x / tiles, tile = blockIdx.x % tiles, tid = threadIdx.x;
  const float4 *src = (const float4 *)(prims + (size_t)frame * P * TMR_REC);
  for (int k = tid; k < P * (TMR_REC / 4); k += 256) s_prim[k] = src[k];
  if (tid < TMR_CAM) s_cam[tid] = cams[(size_t)frame * TMR_CAM + tid];
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int px = (tile % tiles_x) * (2 * WX) + (wave & 1) * WX + lane % WX, py = (tile / tiles_x) * (2 * WY) + (wave >> 1) * WY + lane / WX;
  if (px >= W || py >= H) return;      // (after the only barrier)
  float o[3], d[3], dep;
  int gid;
  RHit h;
  tmr_ray(s_cam, px, py, W, H, o, d);
  tmr_trace((const float *)s_prim, P, o, d, h);
  const uint32_t c = tmr_shade((const float *)s_prim, h, o, d, dep, gid);
  const size_t at = ((size_t)frame * H + py) * W + px;
  rgba[at] = c;
  if (depth) depth[at] = dep;
  if (geom_id) geom_id[at] = gid;
}

// ----------------------------------------------------------------------------------------------- C-ABI
// (the argument checks are csrc/render_host.h's, shared with the host emulation)
using namespace tmjx_host;

static const RenderHandle *tables_of(const tmjx_model *m, int &rc) {
  rc = TMJX_OK;
  if (!m) { rc = fail(TMJX_EINVAL, "null argument"); return nullptr; }
  const RenderHandle *h = (const RenderHandle *)tmjx_internal_render(m);
  if (!h) rc = fail(TMJX_EINVAL, TMR_NO_TABLES);
  return h;
}

static int launch_pose(const RenderHandle *h, const float *qpos, const float *qpos_ghost, int F, const RCamera &cam, float *ws, hipStream_t s) {
  const int ninst = qpos_ghost ? 2 : 1, P = h->t.m.ngeom + (qpos_ghost ? h->t.m.nghost : 0), n = F * ninst;
  hipLaunchKernelGGL(k_render_pose, dim3((n + 63) / 64), dim3(64), 0, s, h->d, qpos, qpos_ghost, F, ninst, P, cam, ws);
  return check_launch("k_render_pose");
}

static int launch_rays(const float *prims, const float *cams, int F, int P, int W, int H, uint8_t *rgba, float *depth, int32_t *geom_id, hipStream_t s) {
  TM_TRY(render_check_rays(prims, cams, F, P, W, H, rgba, depth, geom_id));
  constexpr int WX = TMJX_RENDER_TILE_X, WY = 64 / TMJX_RENDER_TILE_X;
  const int tiles_x = (W + 2 * WX - 1) / (2 * WX), tiles_y = (H + 2 * WY - 1) / (2 * WY);
  const long long blocks = (long long)tiles_x * tiles_y * F;
  if (blocks > 0x7fffffffLL) return fail(TMJX_EINVAL, "F * tiles exceeds the grid size of one launch: render fewer frames per call");
  hipLaunchKernelGGL((k_render_rays<WX, WY>), dim3((unsigned)blocks), dim3(256), 0, s, prims, cams, P, W, H, tiles_x, tiles_x * tiles_y, (uint32_t *)rgba, depth,
                     geom_id);
  return check_launch("k_render_rays");
}

extern "C" {

int tmjx_render_info(const tmjx_model *m, int F, int ghost, tmjx_render_info_t *out) {
  int rc;
  const RenderHandle *h = tables_of(m, rc);
  if (!h) return rc;
  if (!out) return fail(TMJX_EINVAL, "null argument");
  if (F < 1) return fail(TMJX_EINVAL, "F must be >= 1 (got " + std::to_string(F) + ")");
  render_info(h->t, F, ghost, out);
  return TMJX_OK;
}

int tmjx_render_camera(const tmjx_model *m, const char *name, tmjx_camera_t *out) {
  int rc;
  const RenderHandle *h = tables_of(m, rc);
  if (!h) return rc;
  if (!name || !out) return fail(TMJX_EINVAL, "null argument");
  TM_TRY(render_find_camera(h->t, name, out));
  return TMJX_OK;
}

int tmjx_render_pose(const tmjx_model *m, const float *qpos, const float *qpos_ghost, int F, int F_ghost, const tmjx_camera_t *cam, float *workspace,
                     void *stream) {
  int rc;
  const RenderHandle *h = tables_of(m, rc);
  if (!h) return rc;
  RCamera rcam;
  TM_TRY(render_check_frames(F, F_ghost, qpos, qpos_ghost));
  TM_TRY(render_check_camera(h->t.m, cam, rcam));
  if (!workspace || !al16(workspace)) return fail(TMJX_EINVAL, "the workspace must be a 16-byte aligned device buffer of tmjx_render_info's size");
  return launch_pose(h, qpos, qpos_ghost, F, rcam, workspace, (hipStream_t)stream);
}

int tmjx_render_prims(const float *prims, const float *cams, int F, int P, int W, int H, uint8_t *rgba, float *depth, int32_t *geom_id, void *stream) {
  return launch_rays(prims, cams, F, P, W, H, rgba, depth, geom_id, (hipStream_t)stream);
}

int tmjx_render(const tmjx_model *m, const float *qpos, const float *qpos_ghost, int F, int F_ghost, const tmjx_camera_t *cam, int W, int H,
                float *workspace, uint8_t *rgba, float *depth, int32_t *geom_id, void *stream) {
  int rc;
  const RenderHandle *h = tables_of(m, rc);
  if (!h) return rc;
  RCamera rcam;
  TM_TRY(render_check_frames(F, F_ghost, qpos, qpos_ghost));
  TM_TRY(render_check_camera(h->t.m, cam, rcam));
  if (!workspace || !al16(workspace)) return fail(TMJX_EINVAL, "the workspace must be a 16-byte aligned device buffer of tmjx_render_info's size");
  const int P = h->t.m.ngeom + (qpos_ghost ? h->t.m.nghost : 0);
  TM_TRY(render_check_rays(workspace + (size_t)F * TMR_CAM, workspace, F, P, W, H, rgba, depth, geom_id));      // (before the first launch)
  if ((rc = launch_pose(h, qpos, qpos_ghost, F, rcam, workspace, (hipStream_t)stream))) return rc;
  return launch_rays(workspace + (size_t)F * TMR_CAM, workspace, F, P, W, H, rgba, depth, geom_id, (hipStream_t)stream);
}

}  // extern "C"
