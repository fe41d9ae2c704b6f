// tests/hostemu/intervene_emu.cpp — TEST-ONLY host emulation of the intervention C-ABI (include/tmjx.h: tmjx_intervene_ok, tmjx_intervene): the
// expressions of csrc/intervene_core.h and the checks of csrc/intervene_host.h compiled with g++, one loop iteration where the GPU has one wave, an
// array of 64 values where the wave has a register, in the order of csrc/tmjx_intervene.hip.  With -DINTERVENE_EMU_MAIN it is a stand-alone program
// (for sanitizer builds):
//   intervene_emu [n w K] — edits one seeded problem in both modes (130 x 1023, K = 16 by default, strided, a column offset) and prints a checksum.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../track_mjx_amd/csrc/intervene_host.h"

static std::string g_err;
using namespace tmjx_host;

static void emu_row(const tmjx_intervene_t &d, int t, int r) {
  const float dose = d.dose[r];
  const bool on = iv_on(t, d.t_on[r], d.t_off[r], dose);
  if (!on && (d.mode == TMJX_INTERVENE_UNITS || !d.proj)) return;
  float *row = d.h + (int64_t)r * d.ld;
  const int w = d.w;
  static thread_local float hr[IV_PER_LANE][IV_LANES], xc[IV_PER_LANE][IV_LANES], e[IV_PER_LANE][IV_LANES], vk[IV_PER_LANE][IV_LANES];
  for (int i = 0; i < IV_PER_LANE; i++)
    for (int lane = 0; lane < IV_LANES; lane++) {
      const int j = lane + IV_LANES * i;
      hr[i][lane] = j < w ? row[j] : 0.f;
      xc[i][lane] = j < w ? iv_centred(hr[i][lane], d.center, j) : 0.f;
      e[i][lane] = 0.f;
    }
  if (d.mode == TMJX_INTERVENE_UNITS) {
    for (int i = 0; i < IV_PER_LANE; i++)
      for (int lane = 0; lane < IV_LANES; lane++) {
        const int j = lane + IV_LANES * i;
        if (j < w) row[j] = iv_unit(hr[i][lane], xc[i][lane], d.gain[j], d.offset[j], dose);
      }
    return;
  }
  for (int k = 0; k < d.K; k++) {
    const float *v = d.dirs + (int64_t)k * d.ldv;
    float p[IV_LANES], q[IV_LANES];
    for (int lane = 0; lane < IV_LANES; lane++) {
      p[lane] = 0.f;
      for (int i = 0; i < IV_PER_LANE; i++) {
        const int j = lane + IV_LANES * i;
        vk[i][lane] = j < w ? v[j] : 0.f;
        if (j < w) p[lane] = iv_dot_term(xc[i][lane], vk[i][lane], p[lane]);
      }
    }
    for (int off = IV_LANES / 2; off >= 1; off >>= 1) {
      for (int lane = 0; lane < IV_LANES; lane++) q[lane] = iv_tree_step(p[lane], p[lane ^ off]);
      for (int lane = 0; lane < IV_LANES; lane++) p[lane] = q[lane];
    }
    if (d.proj) d.proj[(int64_t)r * d.ldp + k] = p[0];
    for (int lane = 0; lane < IV_LANES; lane++) {
      const float coef = iv_coef(d.gain[k], p[lane], d.offset[k]);
      for (int i = 0; i < IV_PER_LANE; i++) e[i][lane] = iv_edit_term(coef, vk[i][lane], e[i][lane]);
    }
  }
  if (!on) return;
  for (int i = 0; i < IV_PER_LANE; i++)
    for (int lane = 0; lane < IV_LANES; lane++) {
      const int j = lane + IV_LANES * i;
      if (j < w) row[j] = iv_apply(hr[i][lane], dose, e[i][lane]);
    }
}

extern "C" {
const char *ivemu_last_error() { return g_err.c_str(); }

int ivemu_intervene_ok(const tmjx_intervene_t *d) {
  const std::string e = intervene_check(d);
  if (e.empty()) return 1;
  g_err = "tmjx_intervene: " + e;
  return 0;
}

int ivemu_intervene(const tmjx_intervene_t *d, int t) {
  const std::string e = intervene_check(d);
  if (!e.empty()) {
    g_err = "tmjx_intervene: " + e;
    return TMJX_EINVAL;
  }
  for (int r = 0; r < d->n; r++) emu_row(*d, t, r);
  return 0;
}
}  // extern "C"

#ifdef INTERVENE_EMU_MAIN
static float rlcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }

int main(int argc, char **argv) {
  const int n = argc > 3 ? atoi(argv[1]) : 130, w = argc > 3 ? atoi(argv[2]) : 1023, K = argc > 3 ? atoi(argv[3]) : 16;
  const int c0 = 3, ld = w + 5, ldv = w + 1, ldp = K + 2;
  uint32_t seed = 29;
  std::vector<float> h((size_t)n * ld), dirs((size_t)K * ldv), center(w), gk(K), ok(K), gw(w), ow(w), dose(n), proj((size_t)n * ldp);
  std::vector<int32_t> t_on(n), t_off(n);
  for (float &v : h) v = 2.f * rlcg(seed);
  for (float &v : dirs) v = rlcg(seed) / 8.f;
  for (float &v : center) v = rlcg(seed);
  for (int k = 0; k < K; k++) gk[k] = k % 2 ? 0.5f : 0.f, ok[k] = rlcg(seed);
  for (int j = 0; j < w; j++) gw[j] = j % 3 ? 1.f : 0.f, ow[j] = j % 3 ? 0.f : rlcg(seed);
  for (int r = 0; r < n; r++) dose[r] = r % 4 == 3 ? 0.f : 0.25f * (1 + r % 4), t_on[r] = r % 5, t_off[r] = 3 + r % 7;
  tmjx_intervene_t d{};
  d.h = h.data() + c0; d.ld = ld; d.w = w; d.n = n; d.mode = TMJX_INTERVENE_SUBSPACE;
  d.dirs = dirs.data(); d.K = K; d.ldv = ldv; d.center = center.data(); d.gain = gk.data(); d.offset = ok.data();
  d.dose = dose.data(); d.t_on = t_on.data(); d.t_off = t_off.data(); d.proj = proj.data(); d.ldp = ldp;
  for (int t = 0; t < 8; t++)
    if (ivemu_intervene(&d, t)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  d.mode = TMJX_INTERVENE_UNITS; d.gain = gw.data(); d.offset = ow.data(); d.proj = nullptr;
  for (int t = 0; t < 8; t++)
    if (ivemu_intervene(&d, t)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  double sum = 0.0;
  for (float v : h) sum += fabs(v);
  for (float v : proj) sum += fabs(v);
  printf("intervene_emu: %d x %d (ld %d, column offset %d), K = %d, both modes, 8 steps\n", n, w, ld, c0, K);
  printf("intervene_emu: checksum %.6f\n", sum);
  return sum > 0.0 ? 0 : 1;
}
#endif
