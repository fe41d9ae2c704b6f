// csrc/tmjx_rollout.hip — sixth translation unit of libtmjx_hip.so: the checkpoint roll-out's recorder and deterministic-policy kernels
// (csrc/rollout_kernels.h) behind their C-ABI entry points (include/tmjx.h "Roll-out recorder").  Every argument error is refused before any
// device call.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "rollout_kernels.h"

static_assert(sizeof(tmjx_record_stream_t) == 176, "tmjx_record_stream_t: the layout hip.RecordStream declares");
static int grid_of(long long total) { long long g = (total + 255) / 256; return (int)(g < 4096 ? (g > 0 ? g : 1) : 4096); }

static std::string stream_why(const tmjx_record_stream_t &s, int n_env, int T) {
  if (!s.src || !s.dst) return "null src / dst";
  if (!al4(s.src) || !al4(s.dst)) return "misaligned src / dst (4-byte floats)";
  if (s.layout != TMJX_RECORD_SOA && s.layout != TMJX_RECORD_ROWMAJOR) return "layout must be TMJX_RECORD_SOA or TMJX_RECORD_ROWMAJOR";
  if (s.w < 1 || s.w > TMJX_RECORD_MAX_W) return "w must be in 1 .. TMJX_RECORD_MAX_W";
  if (s.n_idx != 0 && (s.n_idx != s.w || s.w > TMJX_RECORD_MAX_IDX)) return "n_idx must be 0 or w (<= TMJX_RECORD_MAX_IDX)";
  if (s.src_extent < 1) return "src_extent must be >= 1";
  if (s.n_idx) {
    for (int i = 0; i < s.n_idx; ++i)
      if (s.idx[i] < 0 || s.idx[i] >= s.src_extent) return "idx beyond src_extent";
  } else if (s.w > s.src_extent) {
    return "w > src_extent";
  }
  if (s.layout == TMJX_RECORD_SOA && s.ld < n_env) return "SoA source: ld must be >= n_env";
  if (s.layout == TMJX_RECORD_ROWMAJOR && s.ld < s.src_extent) return "row-major source: ld must be >= src_extent";
  if (s.T < 1 || s.t0 < 0 || (long long)s.t0 + T > s.T) return "t0 + T beyond the stream's T rows";
  return "";
}

extern "C" {
int tmjx_record_check(const tmjx_record_stream_t *table, int k, int n_env, int T) {
  if (!table) return fail(TMJX_EINVAL, "tmjx_record_check: null table");
  if (k < 1 || k > TMJX_RECORD_MAX_STREAMS || n_env < 1 || T < 1) return fail(TMJX_EINVAL, "tmjx_record_check: k in 1 .. TMJX_RECORD_MAX_STREAMS, n_env >= 1, T >= 1");
  for (int i = 0; i < k; ++i) {
    const std::string why = stream_why(table[i], n_env, T);
    if (!why.empty()) return fail(TMJX_EINVAL, "tmjx_record_check: stream " + std::to_string(i) + ": " + why);
  }
  return TMJX_OK;
}

int tmjx_record_step(const tmjx_record_stream_t *device_table, int k, int n_env, int t, int T, void *stream) {
  if (!device_table || ((uintptr_t)device_table & 15)) return fail(TMJX_EINVAL, "tmjx_record_step: null or misaligned (16 bytes) device table");
  if (k < 1 || k > TMJX_RECORD_MAX_STREAMS || n_env < 1) return fail(TMJX_EINVAL, "tmjx_record_step: k in 1 .. TMJX_RECORD_MAX_STREAMS, n_env >= 1");
  if (t < 0 || t >= T) return fail(TMJX_EINVAL, "tmjx_record_step: 0 <= t < T");
  hipLaunchKernelGGL(k_record_step, dim3((n_env + REC_ENVS - 1) / REC_ENVS, k), dim3(REC_NT), 0, (hipStream_t)stream, device_table, n_env, t);
  return check_launch("k_record_step");
}

int tmjx_latent_concat_det(const float *fc2, int ldf, const float *obs, int64_t obs_s0, int64_t obs_s1, const float *mean, const float *std,
                           float *x, int ldx, float *traj, int ldt, int n, int Z, int obs_w, int ref_w, void *stream) {
  if (!fc2 || !obs || !x) return fail(TMJX_EINVAL, "tmjx_latent_concat_det: null fc2 / obs / x");
  if (!mean != !std) return fail(TMJX_EINVAL, "tmjx_latent_concat_det: mean and std together");
  if (n < 1 || Z < 1 || ref_w < 0 || obs_w <= ref_w || ldf < 2 * Z || ldx < Z + obs_w - ref_w || (traj && ldt < ref_w) || obs_s0 < 0 || obs_s1 < 0)
    return fail(TMJX_EINVAL, "tmjx_latent_concat_det: bad sizes");
  for (const void *p : {(const void *)fc2, (const void *)obs, (const void *)mean, (const void *)std, (const void *)x, (const void *)traj})
    if (!al4(p)) return fail(TMJX_EINVAL, "tmjx_latent_concat_det: misaligned float pointer");
  const long long total = (long long)n * ldx + (traj ? (long long)n * ldt : 0);
  hipLaunchKernelGGL(k_latent_concat_det, dim3(grid_of(total)), dim3(256), 0, (hipStream_t)stream, fc2, ldf, obs, (long long)obs_s0, (long long)obs_s1, mean, std,
                     x, ldx, traj, ldt, n, Z, obs_w, ref_w);
  return check_launch("k_latent_concat_det");
}

int tmjx_decoder_input(const float *latents, int ldz, const float *obs, int64_t obs_s0, int64_t obs_s1, const float *mean, const float *std,
                       float *x, int ldx, int n, int Z, int obs_w, int ref_w, void *stream) {
  if (!latents || !obs || !x) return fail(TMJX_EINVAL, "tmjx_decoder_input: null latents / obs / x");
  if (!mean != !std) return fail(TMJX_EINVAL, "tmjx_decoder_input: mean and std together");
  if (n < 1 || Z < 1 || ref_w < 0 || obs_w <= ref_w || ldz < Z || ldx < Z + obs_w - ref_w || obs_s0 < 0 || obs_s1 < 0)
    return fail(TMJX_EINVAL, "tmjx_decoder_input: bad sizes (n >= 1, ldz >= Z >= 1, obs_w > ref_w >= 0, ldx >= Z + obs_w - ref_w)");
  for (const void *p : {(const void *)latents, (const void *)obs, (const void *)mean, (const void *)std, (const void *)x})
    if (!al4(p)) return fail(TMJX_EINVAL, "tmjx_decoder_input: misaligned float pointer");
  // k_latent_concat_det reads columns [0, Z) of its first operand only: the latents go where fc2 = [mean | logvar] goes in the policy step
  hipLaunchKernelGGL(k_latent_concat_det, dim3(grid_of((long long)n * ldx)), dim3(256), 0, (hipStream_t)stream, latents, ldz, obs, (long long)obs_s0,
                     (long long)obs_s1, mean, std, x, ldx, (float *)nullptr, 0, n, Z, obs_w, ref_w);
  return check_launch("k_latent_concat_det");
}

int tmjx_action_mode(const float *logits, int ldl, float *ctrl, float *action_t, int n, int A, void *stream) {
  if (!logits || !ctrl || !action_t) return fail(TMJX_EINVAL, "tmjx_action_mode: null logits / ctrl / action_t");
  if (n < 1 || A < 1 || ldl < 2 * A) return fail(TMJX_EINVAL, "tmjx_action_mode: n >= 1, A >= 1, ldl >= 2A");
  if (!al4(logits) || !al4(ctrl) || !al4(action_t)) return fail(TMJX_EINVAL, "tmjx_action_mode: misaligned float pointer");
  hipLaunchKernelGGL(k_action_mode, dim3(grid_of((long long)n * A)), dim3(256), 0, (hipStream_t)stream, logits, ldl, ctrl, action_t, n, A);
  return check_launch("k_action_mode");
}
}
