// csrc/tmjx_jacobian.hip — the decoder's Jacobian at recorded steps (include/tmjx.h: tmjx_jacobian_workspace, tmjx_decoder_jacobian; DESIGN.md
// "Decoder Jacobian").  The bodies are csrc/jacobian_core.h (they also compile on the host); the argument checks and the workspace layout
// csrc/jacobian_host.h.  The list of rows is worked through in passes of JAC_CHUNK rows; a pass is, on the caller's stream:
//   k_jac_gemm<true, 2>   a layer's product W h for every row of the pass (the first layer reads x through the row list), then the head's
//   k_jac_block_fwd    bias, SiLU, LayerNorm of one row; keeps xhat and r silu'(u)
//   k_jac_head         loc, ctrl and the first gradient rows diag(1 - ctrl^2) Wh[:A]
//   k_jac_ln_bwd       the gradient rows through a block's LayerNorm and SiLU, in place: the left operand of
//   k_jac_gemm<false, 8>  the product with the block's weight, [rows A][H_l] x [H_l][H_l-1] (the first layer: its wrt columns only)
//   k_jac_outputs      jac, gain, col2, row2, action_var of one row
//   k_jac_sum_rows / k_jac_sum_add   the float64 sums over the rows: groups of JAC_SUM_ROWS rows, then the groups in order
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "jacobian_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
// blockIdx.x: the tile of 128 columns; blockIdx.y: the tile of 16 RU rows
template <bool TB, int RU>
__global__ __launch_bounds__(PCA_THREADS) void k_jac_gemm(const float *__restrict__ a, int64_t lda, const int32_t *__restrict__ gather, int n_src,
                                                          const float *__restrict__ b, int64_t ldb, float *__restrict__ c, int64_t ldc, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) float s_stage[JAC_STAGE];
  jac_gemm_wg<TB, RU>(a, lda, gather, n_src, b, ldb, c, ldc, M, N, K, blockIdx.y, blockIdx.x, s_stage, s_stage + JAC_TK * JAC_LD);
}

__global__ __launch_bounds__(PCA_THREADS) void k_jac_block_fwd(float *__restrict__ z, const float *__restrict__ bias, const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, float eps, int H, float *__restrict__ xhat, float *__restrict__ rs) {
  __shared__ float s_red[PCA_THREADS];
  jac_block_fwd_wg(z, bias, gamma, beta, eps, H, blockIdx.x, xhat, rs, s_red);
}

__global__ __launch_bounds__(PCA_THREADS) void k_jac_head(const float *__restrict__ zloc, const float *__restrict__ wh, int64_t ldwh, const float *__restrict__ bh,
                                                          int A, int H, int mode, int64_t pos0, float *__restrict__ ctrl_out, float *__restrict__ g) {
  __shared__ float s_d[JAC_MAX_A];
  jac_head_wg(zloc, wh, ldwh, bh, A, H, mode, blockIdx.x, pos0 + blockIdx.x, ctrl_out, g, s_d);
}

__global__ __launch_bounds__(PCA_THREADS) void k_jac_ln_bwd(float *__restrict__ g, int M, int A, int H, const float *__restrict__ gamma,
                                                            const float *__restrict__ xhat, const float *__restrict__ rs) {
  __shared__ float s_red[2 * PCA_THREADS];
  jac_ln_bwd_wg(g, M, A, H, gamma, xhat, rs, blockIdx.x, s_red);
}

__global__ __launch_bounds__(PCA_THREADS) void k_jac_outputs(const float *__restrict__ j_rows, int A, int Z, int64_t pos0, const int32_t *__restrict__ row_index,
                                                             int n, const float *__restrict__ scale, int64_t ld_scale, float *__restrict__ jac,
                                                             float *__restrict__ gain, float *__restrict__ col2, float *__restrict__ row2,
                                                             float *__restrict__ action_var) {
  __shared__ float s_row[JAC_MAX_A];
  const int64_t pos = pos0 + blockIdx.x, src = row_index ? (int64_t)row_index[pos] : pos;
  const float *scale_row = scale && src >= 0 && src < n ? scale + src * ld_scale : nullptr;
  jac_outputs_wg(j_rows, A, Z, blockIdx.x, pos, scale_row, jac, gain, col2, row2, action_var, s_row);
}

// blockIdx.x: 256 elements of the sums; blockIdx.y: the group of JAC_SUM_ROWS rows of the pass
__global__ __launch_bounds__(PCA_THREADS) void k_jac_sum_rows(const float *__restrict__ j_rows, int A, int Z, int rows, int E, double *__restrict__ partial) {
  __shared__ float s_j[JAC_MAX_A * JAC_MAX_WRT];
  const int i0 = blockIdx.y * JAC_SUM_ROWS, i1 = i0 + JAC_SUM_ROWS < rows ? i0 + JAC_SUM_ROWS : rows;
  jac_sum_rows_wg(j_rows, A, Z, i0, i1, blockIdx.x, E, partial + (int64_t)blockIdx.y * E, s_j);
}

__global__ __launch_bounds__(PCA_THREADS) void k_jac_sum_add(const double *__restrict__ partial, int chunks, int E, double *__restrict__ sums, int first) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < E) {
    if (first) sums[e] = 0.0;
    jac_sum_add(partial, chunks, E, e, sums);
  }
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_jacobian_workspace(const tmjx_jacobian_desc_t *desc, int m, int64_t *floats) {
  TM_TRY(jac_check_workspace(desc, m, floats));
  *floats = jac_workspace(desc, m).floats;
  return TMJX_OK;
}

int tmjx_decoder_jacobian(const tmjx_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const int32_t *row_index, int m, const float *scale,
                          int64_t ld_scale, int mode, float *ctrl_out, float *jac, float *gain, float *col2, float *row2, float *action_var, double *sums,
                          float *workspace, void *stream) {
  TM_TRY(jac_check_call(desc, x, n, ldx, row_index, m, scale, ld_scale, mode, ctrl_out, jac, gain, col2, row2, action_var, sums, workspace));
  const tmjx_jacobian_desc_t d = *desc;
  const JacWorkspace w = jac_workspace(&d, m);
  hipStream_t s = (hipStream_t)stream;
  const int A = d.A, Z = d.wrt_cols, L = d.L;
  const dim3 wg(PCA_THREADS);
  for (int64_t pos0 = 0; pos0 < m; pos0 += JAC_CHUNK) {
    const int R = (int)(m - pos0 < JAC_CHUNK ? m - pos0 : JAC_CHUNK), M = R * A;
    // forward: the rows of the pass through every block, then the head's product
    int cur = 0, K = d.d_in;
    for (int l = 0; l < L; l++) {
      const tmjx_jacobian_layer_t &y = d.layer[l];
      float *out = workspace + w.h[l & 1];
      if (l == 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_jac_gemm<true, 2>), dim3(jac_tiles(y.width, JAC_TN), jac_tiles(R, JAC_TM_FWD)), wg, 0, s, row_index ? x : x + pos0 * ldx, ldx,
                           row_index ? row_index + pos0 : nullptr, n, y.W, (int64_t)y.ldw, out, (int64_t)y.width, R, y.width, K);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_jac_gemm<true, 2>), dim3(jac_tiles(y.width, JAC_TN), jac_tiles(R, JAC_TM_FWD)), wg, 0, s, (const float *)(workspace + w.h[cur]), (int64_t)K,
                           (const int32_t *)nullptr, 0, y.W, (int64_t)y.ldw, out, (int64_t)y.width, R, y.width, K);
      hipLaunchKernelGGL(k_jac_block_fwd, dim3(R), wg, 0, s, out, y.b, y.gamma, y.beta, d.eps, y.width, workspace + w.xhat[l], workspace + w.rs[l]);
      cur = l & 1;
      K = y.width;
    }
    float *zloc = workspace + w.h[cur ^ 1];
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_jac_gemm<true, 2>), dim3(jac_tiles(A, JAC_TN), jac_tiles(R, JAC_TM_FWD)), wg, 0, s, (const float *)(workspace + w.h[cur]), (int64_t)K,
                       (const int32_t *)nullptr, 0, d.Wh, (int64_t)d.ldwh, zloc, (int64_t)A, R, A, K);
    // reverse: the A gradient rows of every row of the pass, from the head back to the differentiated columns
    int gc = 0;
    hipLaunchKernelGGL(k_jac_head, dim3(R), wg, 0, s, (const float *)zloc, d.Wh, (int64_t)d.ldwh, d.bh, A, K, mode, pos0, ctrl_out, workspace + w.g[gc]);
    for (int l = L - 1; l >= 0; l--) {
      const tmjx_jacobian_layer_t &y = d.layer[l];
      const int H = y.width, N = l == 0 ? Z : d.layer[l - 1].width;
      float *g = workspace + w.g[gc], *next = workspace + w.g[gc ^ 1];
      hipLaunchKernelGGL(k_jac_ln_bwd, dim3(jac_tiles(M, JAC_LN_ROWS)), wg, 0, s, g, M, A, H, y.gamma, (const float *)(workspace + w.xhat[l]),
                         (const float *)(workspace + w.rs[l]));
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_jac_gemm<false, 8>), dim3(jac_tiles(N, JAC_TN), jac_tiles(M, JAC_TM)), wg, 0, s, (const float *)g, (int64_t)H, (const int32_t *)nullptr, 0,
                         y.W + (l == 0 ? d.wrt_col0 : 0), (int64_t)y.ldw, next, (int64_t)N, M, N, H);
      gc ^= 1;
    }
    const float *j_rows = workspace + w.g[gc];
    double *partial = (double *)(workspace + w.partial);
    const int chunks = jac_tiles(R, JAC_SUM_ROWS);
    hipLaunchKernelGGL(k_jac_outputs, dim3(R), wg, 0, s, j_rows, A, Z, pos0, row_index, n, scale, ld_scale, jac, gain, col2, row2, action_var);
    hipLaunchKernelGGL(k_jac_sum_rows, dim3(jac_tiles(w.E, PCA_THREADS), chunks), wg, 0, s, j_rows, A, Z, R, w.E, partial);
    hipLaunchKernelGGL(k_jac_sum_add, dim3(jac_tiles(w.E, PCA_THREADS)), wg, 0, s, (const double *)partial, chunks, w.E, sums, pos0 == 0 ? 1 : 0);
    const int rc = check_launch("tmjx_decoder_jacobian");
    if (rc) return rc;
  }
  return TMJX_OK;
}

}  // extern "C"
