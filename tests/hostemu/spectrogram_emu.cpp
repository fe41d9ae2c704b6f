// tests/hostemu/spectrogram_emu.cpp — TEST-ONLY host emulation of the spectrogram C-ABI (include/tmjx.h: tmjx_wavelet_bank_size, tmjx_wavelet_bank,
// tmjx_spectrogram_workspace, tmjx_spectrogram): the bodies of csrc/spectrogram_core.h and the checks of csrc/spectrogram_host.h compiled with g++,
// one loop iteration where the GPU has one workgroup, in the order of the launches of csrc/tmjx_spectrogram.hip.  With -DSPECTROGRAM_EMU_MAIN it is
// a stand-alone program (for sanitizer builds):
//   spectrogram_emu [C F detrend log len...] — transforms one planted signal (3 channels, 5 frequencies, sequences of 1, 2, 5 and 70 rows by
//   default, strided input and output) with exactly sized buffers and prints a checksum.
#pragma once
#ifdef SPECTROGRAM_EMU_MAIN
#undef HMM_EMU_MAIN
#undef KMEANS_EMU_MAIN
#undef PCA_WIDE_EMU_MAIN
#undef PCA_EMU_MAIN
#endif
#include "hmm_emu.cpp"

#include "../../track_mjx_amd/csrc/spectrogram_host.h"

extern "C" {
int tmjx_wavelet_bank_size(double rate, const double *freqs, int F, double omega0, double support, int64_t *floats) {
  EMU_TRY(spec_check_bank(rate, freqs, F, omega0, support));
  if (!floats) return fail(TMJX_EINVAL, "null argument");
  *floats = spec_bank_floats(rate, freqs, F, omega0, support);
  return 0;
}

int tmjx_wavelet_bank(double rate, const double *freqs, int F, double omega0, double support, float *bank, int32_t *offset, int32_t *radius) {
  EMU_TRY(spec_check_bank(rate, freqs, F, omega0, support));
  if (!bank || !offset || !radius) return fail(TMJX_EINVAL, "null argument");
  spec_build_bank(rate, freqs, F, omega0, support, bank, offset, radius);
  return 0;
}

int tmjx_spectrogram_workspace(int n, int C, int F, int S, int64_t *floats) {
  EMU_TRY(spec_check_workspace(n, C, F, S, floats));
  *floats = spec_workspace(C, F, S).floats;
  return 0;
}

int tmjx_spectrogram(const float *x, int n, int C, int64_t ldx, const int32_t *seq_start, int S, const float *bank, const int32_t *offset, const int32_t *radius,
                     int F, int detrend, int output_kind, float log_floor, float *out, int64_t ldo, float *coverage, float *workspace, void *) {
  EMU_TRY(spec_check(x, n, C, ldx, seq_start, S, bank, offset, radius, F, output_kind, log_floor, out, ldo, coverage, workspace));
  const SpecWorkspace w = spec_workspace(C, F, S);
  const SpecGeom g = spec_geom(C, spec_max_radius(radius, F));
  const int64_t tiles = spec_count_tiles(seq_start, S, g.tt);
  int32_t *d_seq = (int32_t *)(workspace + w.seq), *d_tile = (int32_t *)(workspace + w.tile), *d_off = (int32_t *)(workspace + w.offset),
          *d_rad = (int32_t *)(workspace + w.radius);
  float *mean = workspace + w.mean;
  double *prefix = (double *)(workspace + w.prefix);
  memcpy(d_seq, seq_start, sizeof(int32_t) * (size_t)(S + 1));
  memcpy(d_off, offset, sizeof(int32_t) * (size_t)(F + 1));
  memcpy(d_rad, radius, sizeof(int32_t) * (size_t)F);
  std::vector<int32_t> s_cnt(SPEC_THREADS + 1);
  spec_prepare_wg(d_seq, S, g.tt, bank, d_off, d_rad, F, d_tile, prefix, s_cnt.data());
  if (detrend) {
    std::vector<double> s_sum(SPEC_THREADS);
    for (int s = 0; s < S; s++)
      for (int cb = 0; cb < kmeans_tiles(C, 64); cb++) spec_mean_wg(x, C, ldx, d_seq, s, cb, mean, s_sum.data());
  }
  std::vector<float> s_img(g.lds_floats), s_G(2 * SPEC_MAX_TT);      // exactly the LDS of the launch
  for (int64_t tile = 0; tile < tiles; tile++)
    for (int cb = 0; cb < g.cblocks; cb++)
      spec_tile_wg(x, C, ldx, d_seq, d_tile, S, detrend ? mean : nullptr, bank, d_off, d_rad, prefix, F, output_kind == TMJX_SPECTROGRAM_LOG ? 1 : 0, log_floor, out,
                   ldo, coverage, g, (int)tile, cb, s_img.data(), s_G.data());
  return 0;
}
}  // extern "C"

#ifdef SPECTROGRAM_EMU_MAIN
static float slcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }

int main(int argc, char **argv) {
  const int C = argc > 5 ? atoi(argv[1]) : 3, F = argc > 5 ? atoi(argv[2]) : 5, detrend = argc > 5 ? atoi(argv[3]) : 1, kind = argc > 5 ? atoi(argv[4]) : 0;
  std::vector<int32_t> seq(1, 0);
  if (argc > 5) for (int a = 5; a < argc; a++) seq.push_back(seq.back() + atoi(argv[a]));
  else for (int len : {1, 2, 5, 70}) seq.push_back(seq.back() + len);
  const int S = (int)seq.size() - 1, n = seq.back(), ldx = C + 5, ldo = F * C + 3;
  std::vector<double> freqs(F);
  for (int j = 0; j < F; j++) freqs[j] = F > 1 ? pow(25.0, (double)j / (F - 1)) : 5.0;      // 1 .. 25 Hz at rate 50
  int64_t bank_floats = 0, floats = 0;
  if (tmjx_wavelet_bank_size(50.0, freqs.data(), F, 5.0, 4.0, &bank_floats)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<float> bank((size_t)bank_floats);      // exactly the sizes asked for, so a sanitizer sees any overrun
  std::vector<int32_t> offset(F + 1), radius(F);
  if (tmjx_wavelet_bank(50.0, freqs.data(), F, 5.0, 4.0, bank.data(), offset.data(), radius.data())) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  uint32_t seed = 7;
  std::vector<float> x((size_t)(n - 1) * ldx + C), out((size_t)(n - 1) * ldo + (size_t)F * C, -7.25f), cov((size_t)n * F, -7.25f);
  for (int r = 0; r < n; r++)
    for (int c = 0; c < C; c++) x[(size_t)r * ldx + c] = 3.f + sinf(0.7f * r + c) + 0.1f * slcg(seed);
  if (tmjx_spectrogram_workspace(n, C, F, S, &floats)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<double> ws((size_t)floats / 2 + 2);
  if (tmjx_spectrogram(x.data(), n, C, ldx, seq.data(), S, bank.data(), offset.data(), radius.data(), F, detrend, kind, 1e-3f, out.data(), ldo, cov.data(),
                       (float *)ws.data(), nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  double sum = 0.0;
  int bad = 0;
  for (int r = 0; r < n; r++) {
    for (int e = 0; e < F * C; e++) { const float v = out[(size_t)r * ldo + e]; sum += v; bad += !(v == v) || v == -7.25f; }
    for (int e = F * C; e < ldo && r < n - 1; e++) bad += out[(size_t)r * ldo + e] != -7.25f;      // the padding columns are not written
    for (int j = 0; j < F; j++) { const float v = cov[(size_t)r * F + j]; sum += v; bad += !(v > 0.f && v <= 1.f); }
  }
  printf("spectrogram_emu: %d rows x %d channels in %d sequences, %d frequencies (radii %d .. %d), detrend %d, output %d: %d bad entries\n", n, C, S, F,
         radius[F - 1], radius[0], detrend, kind, bad);
  printf("spectrogram_emu: checksum %.6f\n", sum);
  return bad ? 1 : 0;
}
#endif
