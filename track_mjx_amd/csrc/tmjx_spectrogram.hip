// csrc/tmjx_spectrogram.hip — Morlet wavelet spectrograms of recorded signals (include/tmjx.h: tmjx_wavelet_bank_size, tmjx_wavelet_bank,
// tmjx_spectrogram_workspace, tmjx_spectrogram; DESIGN.md "Spectrogram").  The bodies are csrc/spectrogram_core.h (they also compile on the host);
// the bank builder, the argument checks and the workspace layout csrc/spectrogram_host.h.
//   k_spec_prepare   the first tile of every sequence and the float64 prefix sums of the envelopes, one workgroup
//   k_spec_mean      the mean of every (sequence, channel), float64 in a fixed order
//   k_spec_tile      one tile of a sequence x one channel block, every frequency in turn: the sliding-window FIR
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "spectrogram_host.h"

using namespace tmjx_host;

__global__ __launch_bounds__(SPEC_THREADS) void k_spec_prepare(const int32_t *__restrict__ seq_start, int S, int tt, const float *__restrict__ bank,
                                                               const int32_t *__restrict__ offset, const int32_t *__restrict__ radius, int F,
                                                               int32_t *__restrict__ tile_start, double *__restrict__ prefix) {
  __shared__ int32_t s_cnt[SPEC_THREADS + 1];
  spec_prepare_wg(seq_start, S, tt, bank, offset, radius, F, tile_start, prefix, s_cnt);
}

// blockIdx.x: the sequence; blockIdx.y: its 64 channels
__global__ __launch_bounds__(SPEC_THREADS) void k_spec_mean(const float *__restrict__ x, int C, int64_t ldx, const int32_t *__restrict__ seq_start,
                                                            float *__restrict__ mean) {
  __shared__ double s_sum[SPEC_THREADS];
  spec_mean_wg(x, C, ldx, seq_start, blockIdx.x, blockIdx.y, mean, s_sum);
}

// blockIdx.x: the tile; blockIdx.y: the channel block.  Dynamic LDS: g.lds_floats floats (at most 40 KB).
__global__ __launch_bounds__(SPEC_THREADS) void k_spec_tile(const float *__restrict__ x, int C, int64_t ldx, const int32_t *__restrict__ seq_start,
                                                            const int32_t *__restrict__ tile_start, int S, const float *__restrict__ mean,
                                                            const float *__restrict__ bank, const int32_t *__restrict__ offset,
                                                            const int32_t *__restrict__ radius, const double *__restrict__ prefix, int F, int log_output,
                                                            float log_floor, float *__restrict__ out, int64_t ldo, float *__restrict__ coverage, SpecGeom g) {
  extern __shared__ float s_img[];
  __shared__ float s_G[2 * SPEC_MAX_TT];
  spec_tile_wg(x, C, ldx, seq_start, tile_start, S, mean, bank, offset, radius, prefix, F, log_output, log_floor, out, ldo, coverage, g, blockIdx.x, blockIdx.y,
               s_img, s_G);
}

extern "C" {

int tmjx_wavelet_bank_size(double rate, const double *freqs, int F, double omega0, double support, int64_t *floats) {
  TM_TRY(spec_check_bank(rate, freqs, F, omega0, support));
  if (!floats) return fail(TMJX_EINVAL, "null argument");
  *floats = spec_bank_floats(rate, freqs, F, omega0, support);
  return TMJX_OK;
}

int tmjx_wavelet_bank(double rate, const double *freqs, int F, double omega0, double support, float *bank, int32_t *offset, int32_t *radius) {
  TM_TRY(spec_check_bank(rate, freqs, F, omega0, support));
  if (!bank || !offset || !radius) return fail(TMJX_EINVAL, "null argument");
  spec_build_bank(rate, freqs, F, omega0, support, bank, offset, radius);
  return TMJX_OK;
}

int tmjx_spectrogram_workspace(int n, int C, int F, int S, int64_t *floats) {
  TM_TRY(spec_check_workspace(n, C, F, S, floats));
  *floats = spec_workspace(C, F, S).floats;
  return TMJX_OK;
}

int tmjx_spectrogram(const float *x, int n, int C, int64_t ldx, const int32_t *seq_start, int S, const float *bank, const int32_t *offset,
                     const int32_t *radius, int F, int detrend, int output_kind, float log_floor, float *out, int64_t ldo, float *coverage, float *workspace,
                     void *stream) {
  TM_TRY(spec_check(x, n, C, ldx, seq_start, S, bank, offset, radius, F, output_kind, log_floor, out, ldo, coverage, workspace));
  const SpecWorkspace w = spec_workspace(C, F, S);
  const SpecGeom g = spec_geom(C, spec_max_radius(radius, F));
  const int64_t tiles = spec_count_tiles(seq_start, S, g.tt);
  hipStream_t s = (hipStream_t)stream;
  int32_t *d_seq = (int32_t *)(workspace + w.seq), *d_tile = (int32_t *)(workspace + w.tile), *d_off = (int32_t *)(workspace + w.offset),
          *d_rad = (int32_t *)(workspace + w.radius);
  float *mean = workspace + w.mean;
  double *prefix = (double *)(workspace + w.prefix);
  TM_HIP("tmjx_spectrogram", hipMemcpyAsync(d_seq, seq_start, sizeof(int32_t) * (size_t)(S + 1), hipMemcpyHostToDevice, s));
  TM_HIP("tmjx_spectrogram", hipMemcpyAsync(d_off, offset, sizeof(int32_t) * (size_t)(F + 1), hipMemcpyHostToDevice, s));
  TM_HIP("tmjx_spectrogram", hipMemcpyAsync(d_rad, radius, sizeof(int32_t) * (size_t)F, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_spec_prepare, dim3(1), dim3(SPEC_THREADS), 0, s, d_seq, S, g.tt, bank, d_off, d_rad, F, d_tile, prefix);
  if (detrend) hipLaunchKernelGGL(k_spec_mean, dim3(S, kmeans_tiles(C, 64)), dim3(SPEC_THREADS), 0, s, x, C, ldx, d_seq, mean);
  hipLaunchKernelGGL(k_spec_tile, dim3((unsigned)tiles, g.cblocks), dim3(g.threads), sizeof(float) * (size_t)g.lds_floats, s, x, C, ldx, d_seq, d_tile, S,
                     detrend ? (const float *)mean : (const float *)nullptr, bank, d_off, d_rad, prefix, F, output_kind == TMJX_SPECTROGRAM_LOG ? 1 : 0,
                     log_floor, out, ldo, coverage, g);
  return check_launch("tmjx_spectrogram");
}

}  // extern "C"
