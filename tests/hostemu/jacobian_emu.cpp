// tests/hostemu/jacobian_emu.cpp — TEST-ONLY host emulation of the decoder-Jacobian C-ABI (include/tmjx.h: tmjx_jacobian_workspace,
// tmjx_decoder_jacobian): the bodies of csrc/jacobian_core.h and the checks of csrc/jacobian_host.h compiled with g++, one loop iteration where
// the GPU has one workgroup or thread, in the order of the launches of csrc/tmjx_jacobian.hip.  A library of its own: it includes compare_emu.cpp
// (and through it the analysis emulation) for the decomposition and the PCA the tool calls beside the Jacobian, and adds the Jacobian's names.
// With -DJACOBIAN_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   jacobian_emu m d_in wrt_col0 wrt_cols A ldx width... — both modes of one seeded problem with every buffer of exactly the contract's size, a
//   permuted row list, and prints a checksum.
#pragma once
#include "compare_emu.cpp"

#include "../../track_mjx_amd/csrc/jacobian_host.h"

extern "C" {
int tmjx_jacobian_workspace(const tmjx_jacobian_desc_t *desc, int m, int64_t *floats) {
  EMU_TRY(jac_check_workspace(desc, m, floats));
  *floats = jac_workspace(desc, m).floats;
  return 0;
}

int tmjx_decoder_jacobian(const tmjx_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const int32_t *row_index, int m, const float *scale,
                          int64_t ld_scale, int mode, float *ctrl_out, float *jac, float *gain, float *col2, float *row2, float *action_var, double *sums,
                          float *workspace, void *) {
  EMU_TRY(jac_check_call(desc, x, n, ldx, row_index, m, scale, ld_scale, mode, ctrl_out, jac, gain, col2, row2, action_var, sums, workspace));
  const tmjx_jacobian_desc_t d = *desc;
  const JacWorkspace w = jac_workspace(&d, m);
  const int A = d.A, Z = d.wrt_cols, L = d.L;
  std::vector<double> stage((JAC_STAGE + 1) / 2);      // (doubles: the alignment the kernel's LDS has)
  float *s_a = (float *)stage.data(), *s_b = s_a + JAC_TK * JAC_LD;
  std::vector<float> s_red(2 * PCA_THREADS), s_small(JAC_MAX_A);
  auto gemm = [&](bool fwd, const float *a, int64_t lda, const int32_t *gather, int n_src, const float *b, int64_t ldb, float *c, int64_t ldc, int M, int N, int K) {
    for (int tm = 0; tm < jac_tiles(M, fwd ? JAC_TM_FWD : JAC_TM); tm++)
      for (int tn = 0; tn < jac_tiles(N, JAC_TN); tn++) {
        if (fwd) jac_gemm_wg<true, 2>(a, lda, gather, n_src, b, ldb, c, ldc, M, N, K, tm, tn, s_a, s_b);
        else jac_gemm_wg<false, 8>(a, lda, gather, n_src, b, ldb, c, ldc, M, N, K, tm, tn, s_a, s_b);
      }
  };
  std::vector<float> s_j(JAC_MAX_A * JAC_MAX_WRT);
  for (int64_t pos0 = 0; pos0 < m; pos0 += JAC_CHUNK) {
    const int R = (int)(m - pos0 < JAC_CHUNK ? m - pos0 : JAC_CHUNK), M = R * A;
    int cur = 0, K = d.d_in;
    for (int l = 0; l < L; l++) {
      const tmjx_jacobian_layer_t &y = d.layer[l];
      float *out = workspace + w.h[l & 1];
      if (l == 0) gemm(true, row_index ? x : x + pos0 * ldx, ldx, row_index ? row_index + pos0 : nullptr, n, y.W, y.ldw, out, y.width, R, y.width, K);
      else gemm(true, workspace + w.h[cur], K, nullptr, 0, y.W, y.ldw, out, y.width, R, y.width, K);
      for (int row = 0; row < R; row++) jac_block_fwd_wg(out, y.b, y.gamma, y.beta, d.eps, y.width, row, workspace + w.xhat[l], workspace + w.rs[l], s_red.data());
      cur = l & 1;
      K = y.width;
    }
    float *zloc = workspace + w.h[cur ^ 1];
    gemm(true, workspace + w.h[cur], K, nullptr, 0, d.Wh, d.ldwh, zloc, A, R, A, K);
    int gc = 0;
    for (int row = 0; row < R; row++) jac_head_wg(zloc, d.Wh, d.ldwh, d.bh, A, K, mode, row, pos0 + row, ctrl_out, workspace + w.g[gc], s_small.data());
    for (int l = L - 1; l >= 0; l--) {
      const tmjx_jacobian_layer_t &y = d.layer[l];
      const int H = y.width, N = l == 0 ? Z : d.layer[l - 1].width;
      float *g = workspace + w.g[gc], *next = workspace + w.g[gc ^ 1];
      for (int blk = 0; blk < jac_tiles(M, JAC_LN_ROWS); blk++) jac_ln_bwd_wg(g, M, A, H, y.gamma, workspace + w.xhat[l], workspace + w.rs[l], blk, s_red.data());
      gemm(false, g, H, nullptr, 0, y.W + (l == 0 ? d.wrt_col0 : 0), y.ldw, next, N, M, N, H);
      gc ^= 1;
    }
    const float *j_rows = workspace + w.g[gc];
    double *partial = (double *)(workspace + w.partial);
    const int chunks = jac_tiles(R, JAC_SUM_ROWS);
    for (int row = 0; row < R; row++) {
      const int64_t pos = pos0 + row, src = row_index ? (int64_t)row_index[pos] : pos;
      const float *scale_row = scale && src >= 0 && src < n ? scale + src * ld_scale : nullptr;
      jac_outputs_wg(j_rows, A, Z, row, pos, scale_row, jac, gain, col2, row2, action_var, s_small.data());
    }
    for (int c = 0; c < chunks; c++)
      for (int eb = 0; eb < jac_tiles(w.E, PCA_THREADS); eb++) {
        const int i0 = c * JAC_SUM_ROWS, i1 = i0 + JAC_SUM_ROWS < R ? i0 + JAC_SUM_ROWS : R;
        jac_sum_rows_wg(j_rows, A, Z, i0, i1, eb, w.E, partial + (int64_t)c * w.E, s_j.data());
      }
    for (int e = 0; e < w.E; e++) {
      if (pos0 == 0) sums[e] = 0.0;
      jac_sum_add(partial, chunks, w.E, e, sums);
    }
  }
  return 0;
}
}  // extern "C"

#ifdef JACOBIAN_EMU_MAIN
static float jlcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }
#define JACOBIAN_MAIN_TRY(call) do { if (call) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; } } while (0)

int main(int argc, char **argv) {
  if (argc < 8) { fprintf(stderr, "usage: jacobian_emu m d_in wrt_col0 wrt_cols A ldx width...\n"); return 2; }
  const int m = atoi(argv[1]), d_in = atoi(argv[2]), c0 = atoi(argv[3]), Z = atoi(argv[4]), A = atoi(argv[5]), ldx = atoi(argv[6]), L = argc - 7;
  uint32_t seed = 97;
  // every buffer of exactly the size its contract names, so that a sanitizer sees any overrun
  std::vector<std::vector<float>> keep;
  auto filled = [&](size_t count, float scale, float shift) { keep.emplace_back(count); for (float &v : keep.back()) v = shift + scale * jlcg(seed); return keep.back().data(); };
  tmjx_jacobian_desc_t d = {};
  d.L = L; d.d_in = d_in; d.eps = 1e-6f; d.A = A; d.wrt_col0 = c0; d.wrt_cols = Z;
  int K = d_in;
  for (int l = 0; l < L && l < JAC_MAX_LAYERS; l++) {
    const int H = atoi(argv[7 + l]);
    d.layer[l].width = H; d.layer[l].ldw = K;
    d.layer[l].W = filled((size_t)H * K, 3.46f / sqrtf((float)K), 0.f);
    d.layer[l].b = filled(H, 1.f, 0.f); d.layer[l].gamma = filled(H, 0.3f, 1.f); d.layer[l].beta = filled(H, 1.f, 0.f);
    K = H;
  }
  d.ldwh = K; d.Wh = filled((size_t)A * K, 3.46f / sqrtf((float)K), 0.f); d.bh = filled(A, 1.f, 0.f);      // (only the A loc rows are read)
  const float *x = filled((size_t)(m - 1) * ldx + d_in, 3.f, 0.f), *scale = filled((size_t)m * Z, 1.f, 1.f);
  std::vector<int32_t> index(m);
  for (int i = 0; i < m; i++) index[i] = (i * 7 + 3) % m;
  int64_t floats = 0;
  JACOBIAN_MAIN_TRY(tmjx_jacobian_workspace(&d, m, &floats));
  std::vector<double> ws((size_t)floats / 2 + (floats & 1));
  double sum = 0.0;
  for (int mode = 0; mode < 2; mode++) {
    std::vector<float> ctrl((size_t)m * A), jac((size_t)m * A * Z), gain(m), col2((size_t)m * Z), row2((size_t)m * A), av((size_t)m * A);
    std::vector<double> sums((size_t)A * Z + Z * Z + A * A);
    JACOBIAN_MAIN_TRY(tmjx_decoder_jacobian(&d, x, m, ldx, mode ? index.data() : nullptr, m, scale, Z, mode, ctrl.data(), jac.data(), gain.data(), col2.data(),
                                            row2.data(), av.data(), sums.data(), (float *)ws.data(), nullptr));
    for (float v : gain) sum += v;
    for (float v : av) sum += v;
    for (double v : sums) sum += v;
    for (float v : ctrl) sum += v;
  }
  printf("jacobian_emu: %d rows, d_in %d (ld %d), wrt %d:%d, %d blocks, A %d: checksum %.6f finite: %d\n", m, d_in, ldx, c0, c0 + Z, L, A, sum, (int)std::isfinite(sum));
  return std::isfinite(sum) ? 0 : 1;
}
#endif
