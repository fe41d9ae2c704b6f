// csrc/tmjx_hmm.hip — a hidden Markov model with diagonal Gaussian emissions over recorded activations (include/tmjx.h: tmjx_hmm_workspace,
// tmjx_hmm_emission, tmjx_hmm_forward_backward, tmjx_hmm_mstep, tmjx_hmm_transitions, tmjx_hmm_viterbi, tmjx_hmm_fit; DESIGN.md "Sequence model").
// The bodies are csrc/hmm_core.h (they also compile on the host); the argument checks and the workspace layout csrc/hmm_host.h.
//   k_hmm_const    c_j, one thread per state                                k_hmm_emission  logb: 128 rows per workgroup walk the state tiles
//   k_hmm_fb       the scaled recursion, one workgroup per sequence          k_hmm_start     start and the total loglik, in sequence order
//   k_hmm_outer    float64 outer-product sums per (row part, 64 x 64 tile)   k_hmm_xi        the parts in order, times A
//   k_moments_colsum / _mean    the column mean of x, as the k-means forms it   k_hmm_mreduce   the M-step from the parts
//   k_hmm_trans    transmat and startprob from the counts                    k_hmm_viterbi   one workgroup per sequence
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "hmm_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(PCA_THREADS) void k_hmm_const(const float *__restrict__ vars, int d, int k, float *__restrict__ cj) {
  const int j = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (j < k) cj[j] = hmm_logconst(vars, d, j);
}

__global__ __launch_bounds__(PCA_THREADS, 4) void k_hmm_emission(const float *__restrict__ x, int n, int d, int64_t ldx, const float *__restrict__ means,
                                                                 const float *__restrict__ vars, int k, const float *__restrict__ cj,
                                                                 float *__restrict__ logb) {
  __shared__ __attribute__((aligned(16))) float s_x[HMM_TK * HMM_LDX], s_m[HMM_TK * HMM_LDC], s_iv[HMM_TK * HMM_LDC];
  hmm_emission_wg(x, n, d, ldx, means, vars, k, cj, logb, blockIdx.x, s_x, s_m, s_iv);
}

// one workgroup per sequence.  Dynamic LDS: hmm_fb_lds_floats(k) floats.
__global__ __launch_bounds__(HMM_THREADS) void k_hmm_fb(const float *__restrict__ logb, int k, const int32_t *__restrict__ seq_start,
                                                        const float *__restrict__ transmat, const float *__restrict__ startprob, float *mrow, float *cs,
                                                        float *alphahat, float *__restrict__ vnext, float *__restrict__ gamma,
                                                        double *__restrict__ loglik) {
  extern __shared__ double s_dyn[];
  const int s = blockIdx.x;
  hmm_fb_wg(logb, k, seq_start[s], seq_start[s + 1], transmat, startprob, mrow, cs, alphahat, vnext, gamma, loglik, s, (float *)s_dyn);
}

__global__ __launch_bounds__(HMM_THREADS) void k_hmm_start(const float *__restrict__ gamma, int k, const int32_t *__restrict__ seq_start, int S,
                                                           const double *__restrict__ loglik, double *__restrict__ start, double *__restrict__ total) {
  hmm_start_total_wg(gamma, k, seq_start, S, loglik, start, total);
}

// blockIdx.x: the 64 columns of the output; blockIdx.y: its 64 rows; blockIdx.z: the row part
__global__ __launch_bounds__(PCA_THREADS) void k_hmm_outer(const float *__restrict__ a, int64_t lda, int ka, const float *__restrict__ b, int64_t ldb, int kb,
                                                           const float *__restrict__ bmean, int n, KmeansSplit sp, double *__restrict__ out1,
                                                           double *__restrict__ out2, double *__restrict__ outw) {
  __shared__ __attribute__((aligned(16))) float s_a[HMM_OR * HMM_OT], s_b[HMM_OR * HMM_OT];
  hmm_outer_wg(a, lda, ka, b, ldb, kb, bmean, n, sp, blockIdx.z, blockIdx.y, blockIdx.x, out1, out2, outw, s_a, s_b);
}

__global__ __launch_bounds__(PCA_THREADS) void k_hmm_xi(const double *__restrict__ part, int P, int k, const float *__restrict__ transmat,
                                                        double *__restrict__ xi) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < k * k) hmm_xi_reduce(part, P, k, transmat, xi, e);
}

__global__ __launch_bounds__(PCA_THREADS) void k_hmm_mreduce(const double *__restrict__ part1, const double *__restrict__ part2,
                                                             const double *__restrict__ partw, int P, int k, int d, const float *__restrict__ mean,
                                                             double min_var, double min_weight, float *__restrict__ means, float *__restrict__ vars,
                                                             double *__restrict__ weight) {
  const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < k * d) hmm_mstep_reduce(part1, part2, partw, P, k, d, mean, min_var, min_weight, means, vars, weight, e);
}

__global__ __launch_bounds__(HMM_THREADS) void k_hmm_trans(const double *__restrict__ xi, const double *__restrict__ start, int k, double prior, double kappa,
                                                           float *__restrict__ transmat, float *__restrict__ startprob) {
  hmm_transitions_wg(xi, start, k, prior, kappa, transmat, startprob);
}

// one workgroup per sequence.  Dynamic LDS: k hmm_lda(k) + 2 x 128 floats.
__global__ __launch_bounds__(HMM_THREADS) void k_hmm_viterbi(const float *__restrict__ logb, int k, const int32_t *__restrict__ seq_start,
                                                             const float *__restrict__ transmat, const float *__restrict__ startprob, int logspace,
                                                             uint8_t *bp, int32_t *__restrict__ labels, double *__restrict__ path_logprob) {
  extern __shared__ double s_dyn[];
  const int s = blockIdx.x;
  hmm_viterbi_wg(logb, k, seq_start[s], seq_start[s + 1], transmat, startprob, logspace, bp, labels, path_logprob, s, (float *)s_dyn);
}

// ----------------------------------------------------------------------------------------------- launches
static int upload_seq(const int32_t *seq_start, int S, float *workspace, const HmmWorkspace &w, hipStream_t s, const char *what) {
  TM_HIP(what, hipMemcpyAsync(workspace + w.seq, seq_start, sizeof(int32_t) * (size_t)(S + 1), hipMemcpyHostToDevice, s));
  return TMJX_OK;
}

static int launch_emission(const float *x, int n, int d, int64_t ldx, const float *means, const float *vars, int k, float *logb, float *cj, hipStream_t s) {
  hipLaunchKernelGGL(k_hmm_const, dim3(kmeans_tiles(k, PCA_THREADS)), dim3(PCA_THREADS), 0, s, vars, d, k, cj);
  hipLaunchKernelGGL(k_hmm_emission, dim3(kmeans_tiles(n, HMM_ROWS)), dim3(PCA_THREADS), 0, s, x, n, d, ldx, means, vars, k, cj, logb);
  return check_launch("tmjx_hmm_emission");
}

// (the sequence offsets are in the workspace already)
static int launch_fb(const float *logb, int n, int k, int S, const float *transmat, const float *startprob, float *gamma, double *xi, double *start,
                     double *loglik, double *total, float *workspace, const HmmWorkspace &w, hipStream_t s) {
  const int32_t *seq = (const int32_t *)(workspace + w.seq);
  float *alphahat = workspace + w.alphahat, *vnext = workspace + w.vnext;
  double *xipart = (double *)(workspace + w.xipart);
  const int rc = launch_lds<k_hmm_fb>("tmjx_hmm_forward_backward", dim3(S), dim3(HMM_THREADS), sizeof(float) * hmm_fb_lds_floats(HMM_MAX_K), sizeof(float) * hmm_fb_lds_floats(k), s,
                                      logb, k, seq, transmat, startprob, workspace + w.mrow, workspace + w.cs, alphahat, vnext, gamma, loglik);
  if (rc) return rc;
  hipLaunchKernelGGL(k_hmm_start, dim3(1), dim3(HMM_THREADS), 0, s, gamma, k, seq, S, loglik, start, total);
  const int tiles = kmeans_tiles(k, HMM_OT);
  hipLaunchKernelGGL(k_hmm_outer, dim3(tiles, tiles, w.xsplit.P), dim3(PCA_THREADS), 0, s, alphahat, (int64_t)k, k, vnext, (int64_t)k, k, (const float *)nullptr, n,
                     w.xsplit, xipart, (double *)nullptr, (double *)nullptr);
  hipLaunchKernelGGL(k_hmm_xi, dim3(kmeans_tiles(k * k, PCA_THREADS)), dim3(PCA_THREADS), 0, s, xipart, w.xsplit.P, k, transmat, xi);
  return check_launch("tmjx_hmm_forward_backward");
}

static int launch_mstep(const float *x, int n, int d, int64_t ldx, const float *gamma, int k, double min_var, double min_weight, float *means, float *vars,
                        double *weight, float *workspace, const HmmWorkspace &w, hipStream_t s, bool have_mean) {
  double *colsum = (double *)(workspace + w.colsum), *p1 = (double *)(workspace + w.part1), *p2 = (double *)(workspace + w.part2),
         *pw = (double *)(workspace + w.partw);
  float *mean = workspace + w.mean;
  if (!have_mean) moments_launch_mean<true>(x, ldx, n, d, colsum, mean, s);      // (a fit forms the column mean of x once)
  hipLaunchKernelGGL(k_hmm_outer, dim3(kmeans_tiles(d, HMM_OT), kmeans_tiles(k, HMM_OT), w.msplit.P), dim3(PCA_THREADS), 0, s, gamma, (int64_t)k, k, x, ldx, d,
                     (const float *)mean, n, w.msplit, p1, p2, pw);
  hipLaunchKernelGGL(k_hmm_mreduce, dim3(kmeans_tiles(k * d, PCA_THREADS)), dim3(PCA_THREADS), 0, s, p1, p2, pw, w.msplit.P, k, d, mean, min_var, min_weight, means,
                     vars, weight);
  return check_launch("tmjx_hmm_mstep");
}

static int launch_viterbi(const float *logb, int k, int S, const float *transmat, const float *startprob, int logspace, int32_t *labels, double *path_logprob,
                          float *workspace, const HmmWorkspace &w, hipStream_t s) {
  return launch_lds<k_hmm_viterbi>("tmjx_hmm_viterbi", dim3(S), dim3(HMM_THREADS), sizeof(float) * (HMM_MAX_K * hmm_lda(HMM_MAX_K) + 2 * HMM_THREADS),
                                   sizeof(float) * (k * hmm_lda(k) + 2 * HMM_THREADS), s, logb, k, (const int32_t *)(workspace + w.seq), transmat, startprob, logspace, (uint8_t *)(workspace + w.bp), labels, path_logprob);
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_hmm_workspace(int n, int d, int k, int S, int64_t *floats) {
  TM_TRY(hmm_check_workspace(n, d, k, S, floats));
  *floats = hmm_workspace(n, d, k).floats;
  return TMJX_OK;
}

int tmjx_hmm_emission(const float *x, int n, int d, int64_t ldx, const float *means, const float *vars, int k, float *logb, float *workspace, void *stream) {
  TM_TRY(hmm_check_emission(x, n, d, ldx, means, vars, k, logb, workspace));
  return launch_emission(x, n, d, ldx, means, vars, k, logb, workspace + hmm_workspace(n, d, k).cj, (hipStream_t)stream);
}

int tmjx_hmm_forward_backward(const float *logb, int n, int k, const int32_t *seq_start, int S, const float *transmat, const float *startprob, float *gamma,
                              double *xi, double *start, double *loglik, double *total, float *workspace, void *stream) {
  TM_TRY(hmm_check_fb(logb, n, k, seq_start, S, transmat, startprob, gamma, xi, start, loglik, total, workspace));
  const HmmWorkspace w = hmm_workspace(n, 1, k);
  const int rc = upload_seq(seq_start, S, workspace, w, (hipStream_t)stream, "tmjx_hmm_forward_backward");
  if (rc) return rc;
  return launch_fb(logb, n, k, S, transmat, startprob, gamma, xi, start, loglik, total, workspace, w, (hipStream_t)stream);
}

int tmjx_hmm_mstep(const float *x, int n, int d, int64_t ldx, const float *gamma, int k, double min_var, double min_weight, float *means, float *vars,
                   double *weight, float *workspace, void *stream) {
  TM_TRY(hmm_check_mstep(x, n, d, ldx, gamma, k, min_var, min_weight, means, vars, weight, workspace));
  return launch_mstep(x, n, d, ldx, gamma, k, min_var, min_weight, means, vars, weight, workspace, hmm_workspace(n, d, k), (hipStream_t)stream, false);
}

int tmjx_hmm_transitions(const double *xi, const double *start, int k, double prior, double kappa, float *transmat, float *startprob, void *stream) {
  TM_TRY(hmm_check_transitions(xi, start, k, prior, kappa, transmat, startprob));
  hipLaunchKernelGGL(k_hmm_trans, dim3(1), dim3(HMM_THREADS), 0, (hipStream_t)stream, xi, start, k, prior, kappa, transmat, startprob);
  return check_launch("tmjx_hmm_transitions");
}

int tmjx_hmm_viterbi(const float *logb, int n, int k, const int32_t *seq_start, int S, const float *transmat, const float *startprob, int logspace,
                     int32_t *labels, double *path_logprob, float *workspace, void *stream) {
  TM_TRY(hmm_check_viterbi(logb, n, k, seq_start, S, transmat, startprob, labels, path_logprob, workspace));
  const HmmWorkspace w = hmm_workspace(n, 1, k);
  const int rc = upload_seq(seq_start, S, workspace, w, (hipStream_t)stream, "tmjx_hmm_viterbi");
  if (rc) return rc;
  return launch_viterbi(logb, k, S, transmat, startprob, logspace, labels, path_logprob, workspace, w, (hipStream_t)stream);
}

int tmjx_hmm_fit(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int k, float *means, float *vars, float *transmat,
                 float *startprob, float *gamma, int32_t *labels, int max_iter, double tol, double prior, double kappa, double min_var, double min_weight,
                 tmjx_hmm_info_t *info, float *workspace, void *stream) {
  TM_TRY(hmm_check_fit(x, n, d, ldx, seq_start, S, k, means, vars, transmat, startprob, labels, max_iter, tol, prior, kappa, min_var, min_weight, info,
                        workspace));
  const HmmWorkspace w = hmm_workspace(n, d, k);
  hipStream_t s = (hipStream_t)stream;
  float *logb = workspace + w.logb, *cj = workspace + w.cj, *g = gamma ? gamma : workspace + w.gamma;
  double *xi = (double *)(workspace + w.xi), *start = (double *)(workspace + w.start), *weight = (double *)(workspace + w.weight),
         *loglik = (double *)(workspace + w.loglik), *path = (double *)(workspace + w.path), *total = (double *)(workspace + w.total);
  hipEvent_t ev[8];
  for (int i = 0; i < 8; i++) TM_HIP("hipEventCreate", hipEventCreate(&ev[i]));
  auto finish = [&](int code) { for (int i = 0; i < 8; i++) (void)hipEventDestroy(ev[i]); return code; };
  int rc = upload_seq(seq_start, S, workspace, w, s, "tmjx_hmm_fit");
  if (rc) return finish(rc);
  info->n_iter = 0; info->converged = 0; info->loglik = 0.0;
  info->emission_ms = info->fb_ms = info->mstep_ms = info->viterbi_ms = 0.f;
  double host = 0.0, previous = 0.0;
  float ms = 0.f;
  bool mstep_pending = false, have_mean = false;
  // one E-step and the read-back of its total loglik: the only synchronisation of an iteration
  auto estep = [&]() -> int {
    (void)hipEventRecord(ev[0], s);
    int r = launch_emission(x, n, d, ldx, means, vars, k, logb, cj, s);
    if (r) return r;
    (void)hipEventRecord(ev[1], s);
    if ((r = launch_fb(logb, n, k, S, transmat, startprob, g, xi, start, loglik, total, workspace, w, s))) return r;
    (void)hipEventRecord(ev[2], s);
    hipError_t e = hipMemcpyAsync(&host, total, sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(TMJX_EHIP, std::string("tmjx_hmm_fit: ") + hipGetErrorString(e));
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) info->emission_ms += ms;
    if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) info->fb_ms += ms;
    if (mstep_pending && hipEventElapsedTime(&ms, ev[3], ev[4]) == hipSuccess) info->mstep_ms += ms;
    mstep_pending = false;
    return TMJX_OK;
  };
  for (int it = 0; it < max_iter; it++) {
    if ((rc = estep())) return finish(rc);
    info->n_iter = it + 1;
    if (hmm_converged(it, host, previous, tol)) { info->converged = 1; break; }
    previous = host;
    (void)hipEventRecord(ev[3], s);
    if ((rc = launch_mstep(x, n, d, ldx, g, k, min_var, min_weight, means, vars, weight, workspace, w, s, have_mean))) return finish(rc);
    have_mean = true;
    hipLaunchKernelGGL(k_hmm_trans, dim3(1), dim3(HMM_THREADS), 0, s, xi, start, k, prior, kappa, transmat, startprob);
    if ((rc = check_launch("tmjx_hmm_fit"))) return finish(rc);
    (void)hipEventRecord(ev[4], s);
    mstep_pending = true;
  }
  // after a break the parameters are those of the last E-step, whose outputs stand; after max_iter M-steps one more E-step against the final ones
  if (!info->converged && (rc = estep())) return finish(rc);
  info->loglik = host;
  (void)hipEventRecord(ev[5], s);
  if ((rc = launch_viterbi(logb, k, S, transmat, startprob, 0, labels, path, workspace, w, s))) return finish(rc);
  (void)hipEventRecord(ev[6], s);
  hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) return finish(fail(TMJX_EHIP, std::string("tmjx_hmm_fit: ") + hipGetErrorString(e)));
  if (hipEventElapsedTime(&ms, ev[5], ev[6]) == hipSuccess) info->viterbi_ms = ms;
  return finish(TMJX_OK);
}

}  // extern "C"
