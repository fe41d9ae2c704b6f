// csrc/tmjx_lstm_tangent.hip — the LSTM decoder's recurrent dynamics at recorded steps (include/tmjx.h: tmjx_lstm_tangent_workspace,
// tmjx_lstm_tangent_step, tmjx_lstm_lyapunov; DESIGN.md "LSTM decoder dynamics").  The bodies are csrc/lstm_tangent_core.h and, for the forward and
// the products, csrc/lstm_jacobian_core.h and csrc/jacobian_core.h (they also compile on the host); the argument checks, the workspace layout and
// the schedule csrc/lstm_tangent_host.h.  One step over R rows and their R K tangent rows is, on the caller's stream:
//   k_lst_gemm<2>      per layer the forward products W_ih x_k and W_hh h_k of the R rows (x and the carry through the list of first rows)
//   k_lst_cell_fwd     a layer's gates, c', h'; keeps the six coefficients of a unit (lsj_cell_fwd_wg)
//   k_lst_gemm<8>      per layer the tangent products W_hh dh_k and, above layer 0, W_ih dh'_(k-1) of the R K tangent rows
//   k_lst_cell         the tangent cell of a layer: dc'_k and dh'_k into their blocks of the tangent rows
// tmjx_lstm_tangent_step runs it once per pass of JAC_CHUNK rows, from v into out.  tmjx_lstm_lyapunov orders the sequences by descending length
// (k_lst_order), copies the first bases (k_lst_init) and then runs it once per time step t over the sequences longer than t, which are the first
// slots, in place on their bases, followed by k_lst_qr: one workgroup per active sequence.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "lstm_tangent_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
// blockIdx.x: the tile of 128 columns; blockIdx.y: the tile of 16 RU rows
template <int RU>
__global__ __launch_bounds__(PCA_THREADS) void k_lst_gemm(const float *__restrict__ a, int64_t lda, const int32_t *__restrict__ gather, int n_src,
                                                          const float *__restrict__ b, int64_t ldb, float *__restrict__ c, int64_t ldc, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) float s_stage[JAC_STAGE];
  jac_gemm_wg<true, RU>(a, lda, gather, n_src, b, ldb, c, ldc, M, N, K, blockIdx.y, blockIdx.x, s_stage, s_stage + JAC_TK * JAC_LD);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lst_cell_fwd(const float *__restrict__ xg, const float *__restrict__ hg, const float *__restrict__ b,
                                                              const float *__restrict__ c_src, int64_t ld_carry, const int32_t *__restrict__ gather, int n_src,
                                                              int R, int H, float *__restrict__ h_out, float *__restrict__ keep) {
  lsj_cell_fwd_wg(xg, hg, b, c_src, ld_carry, gather, n_src, R, H, blockIdx.x, h_out, keep);
}

// (dc_src and out_c may be the same block: no __restrict__ on them)
__global__ __launch_bounds__(PCA_THREADS) void k_lst_cell(const float *__restrict__ dxp, const float *__restrict__ dhp, const float *__restrict__ keep,
                                                          const float *dc_src, int64_t ld_src, int64_t M, int K, int H, float *out_h, float *out_c, int64_t ld_out) {
  lst_cell_wg(dxp, dhp, keep, dc_src, ld_src, M, K, H, blockIdx.x, out_h, out_c, ld_out);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lst_order(const int32_t *__restrict__ seq_start, int S, int32_t *__restrict__ ord) {
  lst_order_wg(seq_start, S, blockIdx.x, ord);
}

__global__ __launch_bounds__(PCA_THREADS) void k_lst_init(const float *__restrict__ q0, int q0_per_seq, const int32_t *__restrict__ ord, int S, int K, int W,
                                                          float *__restrict__ q, double *__restrict__ sums, int32_t *__restrict__ status) {
  lst_init_wg(q0, q0_per_seq, ord, S, K, W, blockIdx.x, q, sums, status);
}

// blockIdx.x: the slot of an active sequence at step t
__global__ __launch_bounds__(PCA_THREADS) void k_lst_qr(float *q, const int32_t *__restrict__ ord, int S, int t, int K, int L, int H, int warmup, float *local,
                                                        float *energy, float *q_out, int32_t *status, double *sums) {
  __shared__ float s_red[LST_MAX_K * PCA_THREADS];
  __shared__ float s_r[2 * LST_MAX_K];
  const int slot = blockIdx.x, seq = ord[S + slot];
  const int64_t row = (int64_t)ord[slot] + t, KW = (int64_t)K * 2 * L * H;
  const bool last = t == ord[2 * S + slot] - 1;
  lst_qr_wg(q + slot * KW, K, L, H, local ? local + row * K : nullptr, t >= warmup ? sums + (int64_t)seq * K : nullptr, status ? status + seq : nullptr,
            energy ? energy + row * K * 2 * L : nullptr, last && q_out ? q_out + seq * KW : nullptr, s_red, s_r);
}

// ----------------------------------------------------------------------------------------------- one step
// the forward of R rows: row r is row (gather ? gather[r] : r) of x, h_in, c_in as given (already moved to the pass or the time step)
static void lst_forward(const tmjx_lstm_jacobian_desc_t &d, const LstWorkspace &w, float *workspace, const float *x, int64_t ldx, const float *h_in, const float *c_in,
                        int64_t ld_carry, const int32_t *gather, int n_src, int R, hipStream_t s) {
  const int H = d.H, G4 = 4 * d.H;
  const dim3 wg(PCA_THREADS), grid(jac_tiles(G4, JAC_TN), jac_tiles(R, JAC_TM_FWD));
  float *xg = workspace + w.xg, *hg = workspace + w.hg;
  for (int k = 0; k < d.L; k++) {
    const tmjx_lstm_jacobian_layer_t &y = d.layer[k];
    if (k == 0)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lst_gemm<2>), grid, wg, 0, s, x, ldx, gather, n_src, y.W_ih, (int64_t)y.ldwi, xg, (int64_t)G4, R, G4, d.d_in);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lst_gemm<2>), grid, wg, 0, s, (const float *)(workspace + w.h[(k - 1) & 1]), (int64_t)H, (const int32_t *)nullptr, 0, y.W_ih,
                         (int64_t)y.ldwi, xg, (int64_t)G4, R, G4, H);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lst_gemm<2>), grid, wg, 0, s, h_in + (int64_t)k * H, ld_carry, gather, n_src, y.W_hh, (int64_t)y.ldwh, hg, (int64_t)G4, R, G4, H);
    hipLaunchKernelGGL(k_lst_cell_fwd, dim3(jac_tiles((int64_t)R * H, PCA_THREADS)), wg, 0, s, (const float *)xg, (const float *)hg, y.b_hh, c_in + (int64_t)k * H, ld_carry,
                       gather, n_src, R, H, workspace + w.h[k & 1], workspace + w.keep[k]);
  }
}

// the tangent map of the R K tangent rows `in` [R K][W] into `out` (which may be `in`)
static void lst_tangent(const tmjx_lstm_jacobian_desc_t &d, const LstWorkspace &w, float *workspace, const float *in, float *out, int R, int K, hipStream_t s) {
  const int H = d.H, L = d.L, G4 = 4 * d.H, M = R * K;
  const int64_t W = w.W;
  const dim3 wg(PCA_THREADS), grid(jac_tiles(G4, JAC_TN), jac_tiles(M, LST_TM));
  float *dxp = workspace + w.dxp, *dhp = workspace + w.dhp;
  for (int k = 0; k < L; k++) {
    const tmjx_lstm_jacobian_layer_t &y = d.layer[k];
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lst_gemm<8>), grid, wg, 0, s, in + (int64_t)k * H, W, (const int32_t *)nullptr, 0, y.W_hh, (int64_t)y.ldwh, dhp, (int64_t)G4, M, G4, H);
    if (k > 0)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lst_gemm<8>), grid, wg, 0, s, (const float *)out + (int64_t)(k - 1) * H, W, (const int32_t *)nullptr, 0, y.W_ih, (int64_t)y.ldwi,
                         dxp, (int64_t)G4, M, G4, H);
    hipLaunchKernelGGL(k_lst_cell, dim3(jac_tiles((int64_t)M * H, PCA_THREADS)), wg, 0, s, (const float *)(k > 0 ? dxp : nullptr), (const float *)dhp,
                       (const float *)(workspace + w.keep[k]), in + (int64_t)(L + k) * H, W, (int64_t)M, K, H, out + (int64_t)k * H, out + (int64_t)(L + k) * H, W);
  }
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_lstm_tangent_workspace(const tmjx_lstm_jacobian_desc_t *desc, int S, int K, int64_t *floats) {
  TM_TRY(lst_check_workspace(desc, S, K, floats));
  *floats = lst_workspace(desc, S, K).floats;
  return TMJX_OK;
}

int tmjx_lstm_tangent_step(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                           const float *v, int K, float *out, float *workspace, void *stream) {
  TM_TRY(lst_check_step(desc, x, n, ldx, h_in, c_in, ld_carry, v, K, out, workspace));
  const tmjx_lstm_jacobian_desc_t d = *desc;
  const LstWorkspace w = lst_workspace(&d, n < JAC_CHUNK ? n : JAC_CHUNK, K);
  hipStream_t s = (hipStream_t)stream;
  for (int64_t pos0 = 0; pos0 < n; pos0 += JAC_CHUNK) {
    const int R = (int)(n - pos0 < JAC_CHUNK ? n - pos0 : JAC_CHUNK);
    lst_forward(d, w, workspace, x + pos0 * ldx, ldx, h_in + pos0 * ld_carry, c_in + pos0 * ld_carry, ld_carry, nullptr, 0, R, s);
    lst_tangent(d, w, workspace, v + pos0 * K * w.W, out + pos0 * K * w.W, R, K, s);
    const int rc = check_launch("tmjx_lstm_tangent_step");
    if (rc) return rc;
  }
  return TMJX_OK;
}

int tmjx_lstm_lyapunov(const tmjx_lstm_jacobian_desc_t *desc, const float *x, int n, int64_t ldx, const float *h_in, const float *c_in, int64_t ld_carry,
                       const int32_t *seq_start, int S, const float *q0, int q0_per_seq, int K, int warmup, float *local, float *energy, float *q_out,
                       int32_t *status, double *sums, float *workspace, void *stream) {
  TM_TRY(lst_check_lyapunov(desc, x, n, ldx, h_in, c_in, ld_carry, seq_start, S, q0, q0_per_seq, K, warmup, local, energy, q_out, status, sums, workspace));
  const tmjx_lstm_jacobian_desc_t d = *desc;
  const LstWorkspace w = lst_workspace(&d, S, K);
  const std::vector<int32_t> len = lst_lengths(seq_start, S);
  hipStream_t s = (hipStream_t)stream;
  const dim3 wg(PCA_THREADS);
  int32_t *ord = (int32_t *)(workspace + w.ord), *seq = (int32_t *)(workspace + w.seq);
  float *q = workspace + w.q;
  TM_HIP("tmjx_lstm_lyapunov", hipMemcpyAsync(seq, seq_start, sizeof(int32_t) * (size_t)(S + 1), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_lst_order, dim3(jac_tiles(S, PCA_THREADS)), wg, 0, s, (const int32_t *)seq, S, ord);
  hipLaunchKernelGGL(k_lst_init, dim3(jac_tiles((int64_t)S * K * w.W, PCA_THREADS)), wg, 0, s, q0, q0_per_seq, (const int32_t *)ord, S, K, w.W, q, sums, status);
  int active = S;
  for (int t = 0; t < len[0]; t++) {
    while (len[active - 1] <= t) active--;      // (len[0] > t: at least one stays)
    // row r of the step is row ord[r] + t: the arrays moved by t rows, read through the list of first rows
    lst_forward(d, w, workspace, x + (int64_t)t * ldx, ldx, h_in + (int64_t)t * ld_carry, c_in + (int64_t)t * ld_carry, ld_carry, ord, n - t, active, s);
    lst_tangent(d, w, workspace, q, q, active, K, s);
    hipLaunchKernelGGL(k_lst_qr, dim3(active), wg, 0, s, q, (const int32_t *)ord, S, t, K, d.L, d.H, warmup, local, energy, q_out, status, sums);
    const int rc = check_launch("tmjx_lstm_lyapunov");
    if (rc) return rc;
  }
  return TMJX_OK;
}

}  // extern "C"
