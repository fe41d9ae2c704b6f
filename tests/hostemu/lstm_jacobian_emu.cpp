// tests/hostemu/lstm_jacobian_emu.cpp — TEST-ONLY host emulation of the LSTM-decoder-Jacobian C-ABI (include/tmjx.h: tmjx_lstm_jacobian_workspace,
// tmjx_lstm_decoder_jacobian): the bodies of csrc/lstm_jacobian_core.h and csrc/jacobian_core.h and the checks of csrc/lstm_jacobian_host.h compiled
// with g++, one loop iteration where the GPU has one workgroup or thread, in the order of the launches of csrc/tmjx_lstm_jacobian.hip.  A library of
// its own: it includes jacobian_emu.cpp (and through it the comparison and analysis emulations) for what the tool calls beside it.
// With -DLSTM_JACOBIAN_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   lstm_jacobian_emu m d_in wrt_col0 wrt_cols H L A ldx ld_carry — both modes of one seeded problem with every buffer of exactly the contract's size,
//   a permuted row list with one index out of range, and prints a checksum.
#pragma once
#include "jacobian_emu.cpp"

#include "../../track_mjx_amd/csrc/lstm_jacobian_host.h"

extern "C" {
int tmjx_lstm_jacobian_workspace(const tmjx_lstm_jacobian_desc_t *desc, int m, int64_t *floats) {
  EMU_TRY(lsj_check_workspace(desc, m, floats));
  *floats = lsj_workspace(desc, m).floats;
  return 0;
}

int tmjx_lstm_decoder_jacobian(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                               const int32_t *row_index, int m, const float *scale, int64_t ld_scale, const float *carry_scale, int mode, float *ctrl_out,
                               float *jac, float *gain, float *col2, float *row2, float *action_var, float *carry_jac, float *carry_gain, double *sums,
                               float *workspace, void *) {
  EMU_TRY(lsj_check_call(desc, x, n, ldx, h_in, c_in, ld_carry, row_index, m, scale, ld_scale, carry_scale, mode, ctrl_out, jac, gain, col2, row2, action_var,
                         carry_jac, carry_gain, sums, workspace));
  const tmjx_lstm_jacobian_desc_t d = *desc;
  const LsjWorkspace w = lsj_workspace(&d, m);
  const int A = d.A, Z = d.wrt_cols, L = d.L, H = d.H, G4 = 4 * d.H;
  std::vector<double> stage((JAC_STAGE + 1) / 2);      // (doubles: the alignment the kernel's LDS has)
  float *s_a = (float *)stage.data(), *s_b = s_a + JAC_TK * JAC_LD;
  std::vector<float> s_red(PCA_THREADS), s_small(JAC_MAX_A), s_j(JAC_MAX_A * JAC_MAX_WRT);
  auto gemm = [&](bool fwd, const float *a, int64_t lda, const int32_t *gather, int n_src, const float *b, int64_t ldb, float *c, int64_t ldc, int M, int N, int K) {
    for (int tm = 0; tm < jac_tiles(M, fwd ? JAC_TM_FWD : JAC_TM); tm++)
      for (int tn = 0; tn < jac_tiles(N, JAC_TN); tn++) {
        if (fwd) jac_gemm_wg<true, 2>(a, lda, gather, n_src, b, ldb, c, ldc, M, N, K, tm, tn, s_a, s_b);
        else jac_gemm_wg<false, 8>(a, lda, gather, n_src, b, ldb, c, ldc, M, N, K, tm, tn, s_a, s_b);
      }
  };
  float *xg = workspace + w.xg, *hg = workspace + w.hg, *dpre = workspace + w.d, *cj = workspace + w.cj;
  for (int64_t pos0 = 0; pos0 < m; pos0 += JAC_CHUNK) {
    const int R = (int)(m - pos0 < JAC_CHUNK ? m - pos0 : JAC_CHUNK), M = R * A;
    const int32_t *gather = row_index ? row_index + pos0 : nullptr;
    const int64_t first = row_index ? 0 : pos0;
    for (int k = 0; k < L; k++) {
      const tmjx_lstm_jacobian_layer_t &y = d.layer[k];
      float *out = workspace + w.h[k & 1];
      if (k == 0) gemm(true, x + first * ldx, ldx, gather, n, y.W_ih, y.ldwi, xg, G4, R, G4, d.d_in);
      else gemm(true, workspace + w.h[(k - 1) & 1], H, nullptr, 0, y.W_ih, y.ldwi, xg, G4, R, G4, H);
      gemm(true, h_in + first * ld_carry + (int64_t)k * H, ld_carry, gather, n, y.W_hh, y.ldwh, hg, G4, R, G4, H);
      for (int blk = 0; blk < jac_tiles((int64_t)R * H, PCA_THREADS); blk++)
        lsj_cell_fwd_wg(xg, hg, y.b_hh, c_in + first * ld_carry + (int64_t)k * H, ld_carry, gather, n, R, H, blk, out, workspace + w.keep[k]);
    }
    const int top = (L - 1) & 1;
    float *zloc = workspace + w.h[top ^ 1];
    gemm(true, workspace + w.h[top], H, nullptr, 0, d.Wp, d.ldwp, zloc, A, R, A, H);
    int gc = 0;
    for (int row = 0; row < R; row++) jac_head_wg(zloc, d.Wp, d.ldwp, d.bp, A, H, mode, row, pos0 + row, ctrl_out, workspace + w.g[gc], s_small.data());
    for (int k = L - 1; k >= 0; k--) {
      const tmjx_lstm_jacobian_layer_t &y = d.layer[k];
      const int N = k == 0 ? Z : H;
      float *g = workspace + w.g[gc], *next = workspace + w.g[gc ^ 1];
      for (int blk = 0; blk < jac_tiles((int64_t)M * H, PCA_THREADS); blk++)
        lsj_cell_bwd_wg(g, workspace + w.keep[k], M, A, H, blk, dpre, cj + (int64_t)(L + k) * H, w.W);
      gemm(false, dpre, G4, nullptr, 0, y.W_hh, y.ldwh, cj + (int64_t)k * H, w.W, M, H, G4);
      gemm(false, dpre, G4, nullptr, 0, y.W_ih + (k == 0 ? d.wrt_col0 : 0), y.ldwi, next, N, M, N, G4);
      gc ^= 1;
    }
    const float *j_rows = workspace + w.g[gc];
    double *partial = (double *)(workspace + w.partial), *partial_carry = (double *)(workspace + w.partial_carry);
    const int chunks = jac_tiles(R, JAC_SUM_ROWS), EC = (int)w.EC;
    for (int row = 0; row < R; row++) {
      const int64_t pos = pos0 + row, src = row_index ? (int64_t)row_index[pos] : pos;
      const float *scale_row = scale && src >= 0 && src < n ? scale + src * ld_scale : nullptr;
      jac_outputs_wg(j_rows, A, Z, row, pos, scale_row, jac, gain, col2, row2, action_var, s_small.data());
      if (carry_jac || carry_gain) lsj_carry_outputs_wg(cj, A, L, H, row, pos, carry_scale, carry_jac, carry_gain, s_red.data());
    }
    for (int c = 0; c < chunks; c++) {
      const int i0 = c * JAC_SUM_ROWS, i1 = i0 + JAC_SUM_ROWS < R ? i0 + JAC_SUM_ROWS : R;
      for (int eb = 0; eb < jac_tiles(w.E, PCA_THREADS); eb++) jac_sum_rows_wg(j_rows, A, Z, i0, i1, eb, w.E, partial + (int64_t)c * w.E, s_j.data());
      for (int eb = 0; eb < jac_tiles(EC, PCA_THREADS); eb++) lsj_carry_sum_rows_wg(cj, EC, i0, i1, eb, partial_carry + (int64_t)c * EC);
    }
    for (int e = 0; e < w.E; e++) {
      if (pos0 == 0) sums[e] = 0.0;
      jac_sum_add(partial, chunks, w.E, e, sums);
    }
    for (int e = 0; e < EC; e++) {
      if (pos0 == 0) sums[w.E + e] = 0.0;
      jac_sum_add(partial_carry, chunks, EC, e, sums + w.E);
    }
  }
  return 0;
}
}  // extern "C"

#ifdef LSTM_JACOBIAN_EMU_MAIN
static float lsj_lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }
#define LSJ_MAIN_TRY(call) do { if (call) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; } } while (0)

int main(int argc, char **argv) {
  if (argc != 10) { fprintf(stderr, "usage: lstm_jacobian_emu m d_in wrt_col0 wrt_cols H L A ldx ld_carry\n"); return 2; }
  const int m = atoi(argv[1]), d_in = atoi(argv[2]), c0 = atoi(argv[3]), Z = atoi(argv[4]), H = atoi(argv[5]), L = atoi(argv[6]), A = atoi(argv[7]),
            ldx = atoi(argv[8]), ldc = atoi(argv[9]);
  uint32_t seed = 131;
  // every buffer of exactly the size its contract names, so that a sanitizer sees any overrun
  std::vector<std::vector<float>> keep;
  auto filled = [&](size_t count, float scale, float shift) { keep.emplace_back(count); for (float &v : keep.back()) v = shift + scale * lsj_lcg(seed); return keep.back().data(); };
  tmjx_lstm_jacobian_desc_t d = {};
  d.L = L; d.H = H; d.d_in = d_in; d.A = A; d.wrt_col0 = c0; d.wrt_cols = Z;
  int K = d_in;
  for (int k = 0; k < L && k < LSJ_MAX_LAYERS; k++) {
    d.layer[k].ldwi = K; d.layer[k].ldwh = H;
    d.layer[k].W_ih = filled((size_t)4 * H * K, 3.46f / sqrtf((float)K), 0.f);
    d.layer[k].W_hh = filled((size_t)4 * H * H, 3.46f / sqrtf((float)H), 0.f);
    d.layer[k].b_hh = filled((size_t)4 * H, 1.f, 0.f);
    K = H;
  }
  d.ldwp = H; d.Wp = filled((size_t)A * H, 3.46f / sqrtf((float)H), 0.f); d.bp = filled(A, 1.f, 0.f);      // (only the A loc rows are read)
  const size_t carry = (size_t)(m - 1) * ldc + (size_t)L * H;
  const float *x = filled((size_t)(m - 1) * ldx + d_in, 3.f, 0.f), *scale = filled((size_t)m * Z, 1.f, 1.f), *h_in = filled(carry, 1.f, 0.f), *c_in = filled(carry, 2.f, 0.f),
              *cs = filled((size_t)2 * L * H, 1.f, 1.f);
  std::vector<int32_t> index(m);
  for (int i = 0; i < m; i++) index[i] = (i * 7 + 3) % m;
  index[m / 2] = m;      // (one index out of range: a zero row with a zero carry)
  int64_t floats = 0;
  LSJ_MAIN_TRY(tmjx_lstm_jacobian_workspace(&d, m, &floats));
  std::vector<double> ws((size_t)floats / 2 + (floats & 1));
  double sum = 0.0;
  for (int mode = 0; mode < 2; mode++) {
    const size_t W = (size_t)2 * L * H;
    std::vector<float> ctrl((size_t)m * A), jac((size_t)m * A * Z), gain(m), col2((size_t)m * Z), row2((size_t)m * A), av((size_t)m * A), cjac((size_t)m * A * W),
        cgain((size_t)m * 2 * L);
    std::vector<double> sums((size_t)A * Z + Z * Z + A * A + A * W);
    LSJ_MAIN_TRY(tmjx_lstm_decoder_jacobian(&d, x, m, ldx, h_in, c_in, ldc, mode ? index.data() : nullptr, m, scale, Z, mode ? cs : nullptr, mode, ctrl.data(), jac.data(),
                                            gain.data(), col2.data(), row2.data(), av.data(), cjac.data(), cgain.data(), sums.data(), (float *)ws.data(), nullptr));
    for (float v : gain) sum += v;
    for (float v : av) sum += v;
    for (float v : cgain) sum += v;
    for (double v : sums) sum += v;
    for (float v : ctrl) sum += v;
  }
  printf("lstm_jacobian_emu: %d rows, d_in %d (ld %d), wrt %d:%d, H %d, L %d (ld %d), A %d: checksum %.6f finite: %d\n", m, d_in, ldx, c0, c0 + Z, H, L, ldc, A, sum,
         (int)std::isfinite(sum));
  return std::isfinite(sum) ? 0 : 1;
}
#endif
