// csrc/tmjx_lstm_jacobian.hip — the LSTM decoder's Jacobian at recorded steps (include/tmjx.h: tmjx_lstm_jacobian_workspace,
// tmjx_lstm_decoder_jacobian; DESIGN.md "LSTM decoder Jacobian").  The bodies are csrc/lstm_jacobian_core.h and, for everything the MLP decoder's
// Jacobian already has, csrc/jacobian_core.h (they also compile on the host); the argument checks and the workspace layout
// csrc/lstm_jacobian_host.h.  The list of rows is worked through in passes of JAC_CHUNK rows; a pass is, on the caller's stream:
//   k_lsj_gemm<true, 2>    per layer the two products W_ih x_k and W_hh h_k for every row of the pass (x and the carry through the row list),
//                          then the projection's
//   k_lsj_cell_fwd         a layer's gates, c', h'; keeps the six coefficients of a unit its backward needs
//   k_lsj_head             loc, ctrl and the first gradient rows diag(1 - ctrl^2) Wp[:A]
//   k_lsj_cell_bwd         the gradient rows through a layer's cell: d out / d pre [rows A][4H], and d out / d c_k into the carry Jacobian
//   k_lsj_gemm<false, 8>   d out / d pre times W_hh (into the carry Jacobian) and times W_ih (the next gradient rows; layer 0: its wrt columns only)
//   k_lsj_outputs / k_lsj_carry_outputs    jac, gain, col2, row2, action_var / carry_jac, carry_gain of one row
//   k_lsj_sum_rows, k_lsj_carry_sum_rows / k_lsj_sum_add   the float64 sums over the rows: groups of JAC_SUM_ROWS rows, then the groups in order
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "lstm_jacobian_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
// blockIdx.x: the tile of 128 columns; blockIdx.y: the tile of 16 RU rows
template <bool TB, int RU>
__global__ __launch_bounds__(PCA_THREADS) void k_lsj_gemm(const float *__restrict__ a, int64_t lda, const int32_t *__restrict__ gather, int n_src,
                                                          const float *__restrict__ b, int64_t ldb, float *__restrict__ c, int64_t ldc, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) float s_stage[JAC_STAGE];
  jac_gemm_wg<TB, RU>(a, lda, gather, n_src, b, ldb, c, ldc, M, N, K, blockIdx.y, blockIdx.x, s_stage, s_stage + JAC_TK * JAC_LD);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lsj_cell_fwd(const float *__restrict__ xg, const float *__restrict__ hg, const float *__restrict__ b,
                                                              const float *__restrict__ c_src, int64_t ld_carry, const int32_t *__restrict__ gather, int n_src,
                                                              int R, int H, float *__restrict__ h_out, float *__restrict__ keep) {
  lsj_cell_fwd_wg(xg, hg, b, c_src, ld_carry, gather, n_src, R, H, blockIdx.x, h_out, keep);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lsj_head(const float *__restrict__ zloc, const float *__restrict__ wp, int64_t ldwp, const float *__restrict__ bp,
                                                          int A, int H, int mode, int64_t pos0, float *__restrict__ ctrl_out, float *__restrict__ g) {
  __shared__ float s_d[JAC_MAX_A];
  jac_head_wg(zloc, wp, ldwp, bp, A, H, mode, blockIdx.x, pos0 + blockIdx.x, ctrl_out, g, s_d);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lsj_cell_bwd(const float *__restrict__ gh, const float *__restrict__ keep, int M, int A, int H,
                                                              float *__restrict__ d, float *__restrict__ dc, int64_t ld_dc) {
  lsj_cell_bwd_wg(gh, keep, M, A, H, blockIdx.x, d, dc, ld_dc);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lsj_outputs(const float *__restrict__ j_rows, int A, int Z, int64_t pos0, const int32_t *__restrict__ row_index,
                                                             int n, const float *__restrict__ scale, int64_t ld_scale, float *__restrict__ jac,
                                                             float *__restrict__ gain, float *__restrict__ col2, float *__restrict__ row2,
                                                             float *__restrict__ action_var) {
  __shared__ float s_row[JAC_MAX_A];
  const int64_t pos = pos0 + blockIdx.x, src = row_index ? (int64_t)row_index[pos] : pos;
  const float *scale_row = scale && src >= 0 && src < n ? scale + src * ld_scale : nullptr;
  jac_outputs_wg(j_rows, A, Z, blockIdx.x, pos, scale_row, jac, gain, col2, row2, action_var, s_row);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lsj_carry_outputs(const float *__restrict__ cj, int A, int L, int H, int64_t pos0,
                                                                   const float *__restrict__ carry_scale, float *__restrict__ carry_jac,
                                                                   float *__restrict__ carry_gain) {
  __shared__ float s_red[PCA_THREADS];
  lsj_carry_outputs_wg(cj, A, L, H, blockIdx.x, pos0 + blockIdx.x, carry_scale, carry_jac, carry_gain, s_red);
}

// blockIdx.x: 256 elements of the sums; blockIdx.y: the group of JAC_SUM_ROWS rows of the pass
__global__ __launch_bounds__(PCA_THREADS) void k_lsj_sum_rows(const float *__restrict__ j_rows, int A, int Z, int rows, int E, double *__restrict__ partial) {
  __shared__ float s_j[JAC_MAX_A * JAC_MAX_WRT];
  const int i0 = blockIdx.y * JAC_SUM_ROWS, i1 = i0 + JAC_SUM_ROWS < rows ? i0 + JAC_SUM_ROWS : rows;
  jac_sum_rows_wg(j_rows, A, Z, i0, i1, blockIdx.x, E, partial + (int64_t)blockIdx.y * E, s_j);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lsj_carry_sum_rows(const float *__restrict__ cj, int64_t E, int rows, double *__restrict__ partial) {
  const int i0 = blockIdx.y * JAC_SUM_ROWS, i1 = i0 + JAC_SUM_ROWS < rows ? i0 + JAC_SUM_ROWS : rows;
  lsj_carry_sum_rows_wg(cj, E, i0, i1, blockIdx.x, partial + (int64_t)blockIdx.y * E);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lsj_sum_add(const double *__restrict__ partial, int chunks, int E, double *__restrict__ sums, int first) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < E) {
    if (first) sums[e] = 0.0;
    jac_sum_add(partial, chunks, E, e, sums);
  }
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_lstm_jacobian_workspace(const tmjx_lstm_jacobian_desc_t *desc, int m, int64_t *floats) {
  TM_TRY(lsj_check_workspace(desc, m, floats));
  *floats = lsj_workspace(desc, m).floats;
  return TMJX_OK;
}

int tmjx_lstm_decoder_jacobian(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                               const int32_t *row_index, int m, const float *scale, int64_t ld_scale, const float *carry_scale, int mode, float *ctrl_out,
                               float *jac, float *gain, float *col2, float *row2, float *action_var, float *carry_jac, float *carry_gain, double *sums,
                               float *workspace, void *stream) {
  TM_TRY(lsj_check_call(desc, x, n, ldx, h_in, c_in, ld_carry, row_index, m, scale, ld_scale, carry_scale, mode, ctrl_out, jac, gain, col2, row2, action_var,
                        carry_jac, carry_gain, sums, workspace));
  const tmjx_lstm_jacobian_desc_t d = *desc;
  const LsjWorkspace w = lsj_workspace(&d, m);
  hipStream_t s = (hipStream_t)stream;
  const int A = d.A, Z = d.wrt_cols, L = d.L, H = d.H, G4 = 4 * d.H;
  const dim3 wg(PCA_THREADS);
  float *xg = workspace + w.xg, *hg = workspace + w.hg, *dpre = workspace + w.d, *cj = workspace + w.cj;
  for (int64_t pos0 = 0; pos0 < m; pos0 += JAC_CHUNK) {
    const int R = (int)(m - pos0 < JAC_CHUNK ? m - pos0 : JAC_CHUNK), M = R * A;
    const int32_t *gather = row_index ? row_index + pos0 : nullptr;
    const int64_t first = row_index ? 0 : pos0;      // (without a list row r of the pass is row pos0 + r of x and of the carry)
    const dim3 fwd_grid(jac_tiles(G4, JAC_TN), jac_tiles(R, JAC_TM_FWD));
    // forward: the rows of the pass through every cell, then the projection's product
    for (int k = 0; k < L; k++) {
      const tmjx_lstm_jacobian_layer_t &y = d.layer[k];
      float *out = workspace + w.h[k & 1];
      if (k == 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lsj_gemm<true, 2>), fwd_grid, wg, 0, s, x + first * ldx, ldx, gather, n, y.W_ih, (int64_t)y.ldwi, xg, (int64_t)G4, R, G4, d.d_in);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lsj_gemm<true, 2>), fwd_grid, wg, 0, s, (const float *)(workspace + w.h[(k - 1) & 1]), (int64_t)H, (const int32_t *)nullptr, 0,
                           y.W_ih, (int64_t)y.ldwi, xg, (int64_t)G4, R, G4, H);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lsj_gemm<true, 2>), fwd_grid, wg, 0, s, h_in + first * ld_carry + (int64_t)k * H, ld_carry, gather, n, y.W_hh, (int64_t)y.ldwh, hg,
                         (int64_t)G4, R, G4, H);
      hipLaunchKernelGGL(k_lsj_cell_fwd, dim3(jac_tiles((int64_t)R * H, PCA_THREADS)), wg, 0, s, (const float *)xg, (const float *)hg, y.b_hh,
                         c_in + first * ld_carry + (int64_t)k * H, ld_carry, gather, n, R, H, out, workspace + w.keep[k]);
    }
    const int top = (L - 1) & 1;
    float *zloc = workspace + w.h[top ^ 1];
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lsj_gemm<true, 2>), dim3(jac_tiles(A, JAC_TN), jac_tiles(R, JAC_TM_FWD)), wg, 0, s, (const float *)(workspace + w.h[top]), (int64_t)H,
                       (const int32_t *)nullptr, 0, d.Wp, (int64_t)d.ldwp, zloc, (int64_t)A, R, A, H);
    // reverse: the A gradient rows of every row of the pass, from the projection back to the differentiated columns and to every layer's carry
    int gc = 0;
    hipLaunchKernelGGL(k_lsj_head, dim3(R), wg, 0, s, (const float *)zloc, d.Wp, (int64_t)d.ldwp, d.bp, A, H, mode, pos0, ctrl_out, workspace + w.g[gc]);
    for (int k = L - 1; k >= 0; k--) {
      const tmjx_lstm_jacobian_layer_t &y = d.layer[k];
      const int N = k == 0 ? Z : H;
      float *g = workspace + w.g[gc], *next = workspace + w.g[gc ^ 1];
      hipLaunchKernelGGL(k_lsj_cell_bwd, dim3(jac_tiles((int64_t)M * H, PCA_THREADS)), wg, 0, s, (const float *)g, (const float *)(workspace + w.keep[k]), M, A, H, dpre,
                         cj + (int64_t)(L + k) * H, (int64_t)w.W);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lsj_gemm<false, 8>), dim3(jac_tiles(H, JAC_TN), jac_tiles(M, JAC_TM)), wg, 0, s, (const float *)dpre, (int64_t)G4,
                         (const int32_t *)nullptr, 0, y.W_hh, (int64_t)y.ldwh, cj + (int64_t)k * H, (int64_t)w.W, M, H, G4);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lsj_gemm<false, 8>), dim3(jac_tiles(N, JAC_TN), jac_tiles(M, JAC_TM)), wg, 0, s, (const float *)dpre, (int64_t)G4,
                         (const int32_t *)nullptr, 0, y.W_ih + (k == 0 ? d.wrt_col0 : 0), (int64_t)y.ldwi, next, (int64_t)N, M, N, G4);
      gc ^= 1;
    }
    const float *j_rows = workspace + w.g[gc];
    double *partial = (double *)(workspace + w.partial), *partial_carry = (double *)(workspace + w.partial_carry);
    const int chunks = jac_tiles(R, JAC_SUM_ROWS), EC = (int)w.EC;
    hipLaunchKernelGGL(k_lsj_outputs, dim3(R), wg, 0, s, j_rows, A, Z, pos0, row_index, n, scale, ld_scale, jac, gain, col2, row2, action_var);
    if (carry_jac || carry_gain)
      hipLaunchKernelGGL(k_lsj_carry_outputs, dim3(R), wg, 0, s, (const float *)cj, A, L, H, pos0, carry_scale, carry_jac, carry_gain);
    hipLaunchKernelGGL(k_lsj_sum_rows, dim3(jac_tiles(w.E, PCA_THREADS), chunks), wg, 0, s, j_rows, A, Z, R, w.E, partial);
    hipLaunchKernelGGL(k_lsj_sum_add, dim3(jac_tiles(w.E, PCA_THREADS)), wg, 0, s, (const double *)partial, chunks, w.E, sums, pos0 == 0 ? 1 : 0);
    hipLaunchKernelGGL(k_lsj_carry_sum_rows, dim3(jac_tiles(EC, PCA_THREADS), chunks), wg, 0, s, (const float *)cj, (int64_t)EC, R, partial_carry);
    hipLaunchKernelGGL(k_lsj_sum_add, dim3(jac_tiles(EC, PCA_THREADS)), wg, 0, s, (const double *)partial_carry, chunks, EC, sums + w.E, pos0 == 0 ? 1 : 0);
    const int rc = check_launch("tmjx_lstm_decoder_jacobian");
    if (rc) return rc;
  }
  return TMJX_OK;
}

}  // extern "C"
