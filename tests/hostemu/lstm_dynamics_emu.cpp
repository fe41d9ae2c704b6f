// tests/hostemu/lstm_dynamics_emu.cpp — TEST-ONLY host emulation of the LSTM-decoder-dynamics C-ABI (include/tmjx.h: tmjx_lstm_tangent_workspace,
// tmjx_lstm_tangent_step, tmjx_lstm_lyapunov): the bodies of csrc/lstm_tangent_core.h, csrc/lstm_jacobian_core.h and csrc/jacobian_core.h and the
// checks of csrc/lstm_tangent_host.h compiled with g++, one loop iteration where the GPU has one workgroup or thread, in the order of the launches
// of csrc/tmjx_lstm_tangent.hip.  A library of its own: it includes lstm_jacobian_emu.cpp (and through it the Jacobian, comparison and analysis
// emulations) for what the tool calls beside it.
// With -DLSTM_DYNAMICS_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   lstm_dynamics_emu d_in H L K ldx ld_carry len... — one seeded problem with every buffer of exactly the contract's size: the sequences of the
//   lengths given through tmjx_lstm_lyapunov with every output, then their rows through tmjx_lstm_tangent_step, and prints a checksum.
#pragma once
#include "lstm_jacobian_emu.cpp"

#include "../../track_mjx_amd/csrc/lstm_tangent_host.h"

namespace {
struct LstEmu {
  const tmjx_lstm_jacobian_desc_t d;
  const LstWorkspace w;
  float *workspace;
  std::vector<double> stage;      // (doubles: the alignment the kernel's LDS has)
  LstEmu(const tmjx_lstm_jacobian_desc_t *desc, int R, int K, float *ws) : d(*desc), w(lst_workspace(desc, R, K)), workspace(ws), stage((JAC_STAGE + 1) / 2) {}

  template <int RU>
  void gemm(const float *a, int64_t lda, const int32_t *gather, int n_src, const float *b, int64_t ldb, float *c, int64_t ldc, int M, int N, int K) {
    float *s_a = (float *)stage.data(), *s_b = s_a + JAC_TK * JAC_LD;
    for (int tm = 0; tm < jac_tiles(M, 16 * RU); tm++)
      for (int tn = 0; tn < jac_tiles(N, JAC_TN); tn++) jac_gemm_wg<true, RU>(a, lda, gather, n_src, b, ldb, c, ldc, M, N, K, tm, tn, s_a, s_b);
  }

  void forward(const float *x, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry, const int32_t *gather, int n_src, int R) {
    const int H = d.H, G4 = 4 * d.H;
    float *xg = workspace + w.xg, *hg = workspace + w.hg;
    for (int k = 0; k < d.L; k++) {
      const tmjx_lstm_jacobian_layer_t &y = d.layer[k];
      if (k == 0) gemm<2>(x, ldx, gather, n_src, y.W_ih, y.ldwi, xg, G4, R, G4, d.d_in);
      else gemm<2>(workspace + w.h[(k - 1) & 1], H, nullptr, 0, y.W_ih, y.ldwi, xg, G4, R, G4, H);
      gemm<2>(h_in + (int64_t)k * H, ld_carry, gather, n_src, y.W_hh, y.ldwh, hg, G4, R, G4, H);
      for (int blk = 0; blk < jac_tiles((int64_t)R * H, PCA_THREADS); blk++)
        lsj_cell_fwd_wg(xg, hg, y.b_hh, c_in + (int64_t)k * H, ld_carry, gather, n_src, R, H, blk, workspace + w.h[k & 1], workspace + w.keep[k]);
    }
  }

  void tangent(const float *in, float *out, int R, int K) {
    const int H = d.H, L = d.L, G4 = 4 * d.H, M = R * K;
    const int64_t W = w.W;
    float *dxp = workspace + w.dxp, *dhp = workspace + w.dhp;
    for (int k = 0; k < L; k++) {
      const tmjx_lstm_jacobian_layer_t &y = d.layer[k];
      gemm<8>(in + (int64_t)k * H, W, nullptr, 0, y.W_hh, y.ldwh, dhp, G4, M, G4, H);
      if (k > 0) gemm<8>(out + (int64_t)(k - 1) * H, W, nullptr, 0, y.W_ih, y.ldwi, dxp, G4, M, G4, H);
      for (int blk = 0; blk < jac_tiles((int64_t)M * H, PCA_THREADS); blk++)
        lst_cell_wg(k > 0 ? dxp : nullptr, dhp, workspace + w.keep[k], in + (int64_t)(L + k) * H, W, M, K, H, blk, out + (int64_t)k * H, out + (int64_t)(L + k) * H, W);
    }
  }
};
}  // namespace

extern "C" {
int tmjx_lstm_tangent_workspace(const tmjx_lstm_jacobian_desc_t *desc, int S, int K, int64_t *floats) {
  EMU_TRY(lst_check_workspace(desc, S, K, floats));
  *floats = lst_workspace(desc, S, K).floats;
  return 0;
}

int tmjx_lstm_tangent_step(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                           const float *v, int K, float *out, float *workspace, void *) {
  EMU_TRY(lst_check_step(desc, x, n, ldx, h_in, c_in, ld_carry, v, K, out, workspace));
  LstEmu e(desc, n < JAC_CHUNK ? n : JAC_CHUNK, K, workspace);
  for (int64_t pos0 = 0; pos0 < n; pos0 += JAC_CHUNK) {
    const int R = (int)(n - pos0 < JAC_CHUNK ? n - pos0 : JAC_CHUNK);
    e.forward(x + pos0 * ldx, ldx, h_in + pos0 * ld_carry, c_in + pos0 * ld_carry, ld_carry, nullptr, 0, R);
    e.tangent(v + pos0 * K * e.w.W, out + pos0 * K * e.w.W, R, K);
  }
  return 0;
}

int tmjx_lstm_lyapunov(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                       const int32_t *seq_start, int S, const float *q0, int q0_per_seq, int K, int warmup, float *local, float *energy, float *q_out,
                       int32_t *status, double *sums, float *workspace, void *) {
  EMU_TRY(lst_check_lyapunov(desc, x, n, ldx, h_in, c_in, ld_carry, seq_start, S, q0, q0_per_seq, K, warmup, local, energy, q_out, status, sums, workspace));
  LstEmu e(desc, S, K, workspace);
  const std::vector<int32_t> len = lst_lengths(seq_start, S);
  const int L = e.d.L, H = e.d.H;
  const int64_t KW = (int64_t)K * e.w.W;
  int32_t *ord = (int32_t *)(workspace + e.w.ord), *seq = (int32_t *)(workspace + e.w.seq);
  float *q = workspace + e.w.q;
  std::vector<float> s_red(LST_MAX_K * PCA_THREADS), s_r(2 * LST_MAX_K);
  memcpy(seq, seq_start, sizeof(int32_t) * (size_t)(S + 1));
  for (int blk = 0; blk < jac_tiles(S, PCA_THREADS); blk++) lst_order_wg(seq, S, blk, ord);
  for (int blk = 0; blk < jac_tiles(S * KW, PCA_THREADS); blk++) lst_init_wg(q0, q0_per_seq, ord, S, K, e.w.W, blk, q, sums, status);
  int active = S;
  for (int t = 0; t < len[0]; t++) {
    while (len[active - 1] <= t) active--;
    e.forward(x + (int64_t)t * ldx, ldx, h_in + (int64_t)t * ld_carry, c_in + (int64_t)t * ld_carry, ld_carry, ord, n - t, active);
    e.tangent(q, q, active, K);
    for (int slot = 0; slot < active; slot++) {
      const int sq = ord[S + slot];
      const int64_t row = (int64_t)ord[slot] + t;
      const bool last = t == ord[2 * S + slot] - 1;
      lst_qr_wg(q + slot * KW, K, L, H, local ? local + row * K : nullptr, t >= warmup ? sums + (int64_t)sq * K : nullptr, status ? status + sq : nullptr,
                energy ? energy + row * K * 2 * L : nullptr, last && q_out ? q_out + sq * KW : nullptr, s_red.data(), s_r.data());
    }
  }
  return 0;
}
}  // extern "C"

#ifdef LSTM_DYNAMICS_EMU_MAIN
static float lsd_lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }
#define LSD_MAIN_TRY(call) do { if (call) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; } } while (0)

int main(int argc, char **argv) {
  if (argc < 8) { fprintf(stderr, "usage: lstm_dynamics_emu d_in H L K ldx ld_carry len...\n"); return 2; }
  const int d_in = atoi(argv[1]), H = atoi(argv[2]), L = atoi(argv[3]), K = atoi(argv[4]), ldx = atoi(argv[5]), ldc = atoi(argv[6]), S = argc - 7;
  std::vector<int32_t> seq(S + 1, 0);
  for (int s = 0; s < S; s++) seq[s + 1] = seq[s] + atoi(argv[7 + s]);
  const int n = seq[S];
  uint32_t seed = 977;
  // every buffer of exactly the size its contract names, so that a sanitizer sees any overrun
  std::vector<std::vector<float>> keep;
  auto filled = [&](size_t count, float scale) { keep.emplace_back(count); for (float &t : keep.back()) t = scale * lsd_lcg(seed); return keep.back().data(); };
  tmjx_lstm_jacobian_desc_t d = {};
  d.L = L; d.H = H; d.d_in = d_in;
  int Kin = d_in;
  for (int k = 0; k < L && k < LSJ_MAX_LAYERS; k++) {
    d.layer[k].ldwi = Kin; d.layer[k].ldwh = H;
    d.layer[k].W_ih = filled((size_t)4 * H * Kin, 3.46f / sqrtf((float)Kin));
    d.layer[k].W_hh = filled((size_t)4 * H * H, 3.46f / sqrtf((float)H));
    d.layer[k].b_hh = filled((size_t)4 * H, 1.f);
    Kin = H;
  }
  const size_t W = (size_t)2 * L * H, carry = (size_t)(n - 1) * ldc + (size_t)L * H;
  // (std::vector<float> of the exact size for what the sanitizer guards; the 16-byte alignment the contract asks of the bases comes from operator new)
  std::vector<float> x((size_t)(n - 1) * ldx + d_in), h_in(carry), c_in(carry), q0((size_t)K * W), local((size_t)n * K), energy((size_t)n * K * 2 * L), q_out((size_t)S * K * W),
      v((size_t)n * K * W), out((size_t)n * K * W);
  for (float &t : x) t = 3.f * lsd_lcg(seed);
  for (float &t : h_in) t = lsd_lcg(seed);
  for (float &t : c_in) t = 2.f * lsd_lcg(seed);
  for (float &t : q0) t = lsd_lcg(seed);
  for (float &t : v) t = lsd_lcg(seed);
  std::vector<int32_t> status(S);
  std::vector<double> sums((size_t)S * K);
  int64_t floats = 0;
  const int pass = n < JAC_CHUNK ? n : JAC_CHUNK;
  double sum = 0.0;
  LSD_MAIN_TRY(tmjx_lstm_tangent_workspace(&d, S, K, &floats));
  std::vector<double> ws((size_t)floats / 2 + (floats & 1));      // (operator new aligns to 16 bytes, as it does the bases below)
  float *wsp = (float *)ws.data();
  LSD_MAIN_TRY(tmjx_lstm_lyapunov(&d, x.data(), n, ldx, h_in.data(), c_in.data(), ldc, seq.data(), S, q0.data(), 0, K, 1, local.data(), energy.data(), q_out.data(),
                                  status.data(), sums.data(), wsp, nullptr));
  for (float t : energy) sum += t;
  for (float t : q_out) sum += t;
  for (float t : local) sum += std::isfinite(t) ? t : 0.f;
  LSD_MAIN_TRY(tmjx_lstm_tangent_workspace(&d, pass, K, &floats));
  std::vector<double> ws2((size_t)floats / 2 + (floats & 1));
  LSD_MAIN_TRY(tmjx_lstm_tangent_step(&d, x.data(), n, ldx, h_in.data(), c_in.data(), ldc, v.data(), K, out.data(), (float *)ws2.data(), nullptr));
  for (float t : out) sum += t;
  printf("lstm_dynamics_emu: %d rows in %d sequences, d_in %d (ld %d), H %d, L %d (ld %d), K %d: checksum %.6f finite: %d\n", n, S, d_in, ldx, H, L, ldc, K, sum,
         (int)std::isfinite(sum));
  return std::isfinite(sum) ? 0 : 1;
}
#endif
