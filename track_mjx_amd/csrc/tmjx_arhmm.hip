// csrc/tmjx_arhmm.hip — a hidden Markov model with autoregressive emissions over recorded signals (include/tmjx.h: tmjx_arhmm_workspace,
// tmjx_arhmm_emission, tmjx_arhmm_moments, tmjx_arhmm_solve, tmjx_arhmm_fit; DESIGN.md "Autoregressive sequence model").  The bodies are
// csrc/arhmm_core.h (they also compile on the host); the argument checks and the workspace layout csrc/arhmm_host.h.  What does not look at x is
// the Gaussian HMM's: the fit calls tmjx_hmm_forward_backward, tmjx_hmm_transitions and tmjx_hmm_viterbi on the HMM part of its workspace.
//   k_arhmm_pos       the position of every row in its sequence          k_arhmm_const     c_j, one thread per state
//   k_arhmm_emission  logb: 128 rows and their halo per workgroup         k_arhmm_moments   float64 Gram sums per (row part, state, 64 x 64 tile)
//   k_arhmm_mreduce   the parts in order, and the weights                 k_arhmm_solve     Cholesky and the solves, one workgroup per state
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/tmjx.h"
#include "host_launch.h"
#include "arhmm_host.h"

using namespace tmjx_host;

// ----------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(PCA_THREADS) void k_arhmm_pos(const int32_t *__restrict__ seq_start, int S, int n, int32_t *__restrict__ pos) {
  const int64_t t = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (t < n) pos[t] = arhmm_pos(seq_start, S, (int)t);
}

__global__ __launch_bounds__(PCA_THREADS) void k_arhmm_const(const float *__restrict__ vars, int d, int k, float *__restrict__ cj) {
  const int j = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (j < k) cj[j] = hmm_logconst(vars, d, j);
}

__global__ __launch_bounds__(PCA_THREADS, 2) void k_arhmm_emission(const float *__restrict__ x, int n, int d, int64_t ldx, const int32_t *__restrict__ pos,
                                                                   int lags, int warmup, const float *__restrict__ center,
                                                                   const float *__restrict__ weights, const float *__restrict__ vars, int k,
                                                                   const float *__restrict__ cj, float *__restrict__ logb) {
  __shared__ __attribute__((aligned(16))) float s_x[ARHMM_MAX_D * ARHMM_LDX], s_w[ARHMM_TK * ARHMM_LDW];
  arhmm_emission_wg(x, n, d, ldx, pos, lags, warmup, center, weights, vars, k, cj, logb, blockIdx.x, s_x, s_w);
}

// blockIdx.x: the row part (the dimension that grows with n); blockIdx.y: the state; blockIdx.z: the tile pair (ib <= jb) of the output
__global__ __launch_bounds__(PCA_THREADS) void k_arhmm_moments(const float *__restrict__ x, int n, int d, int64_t ldx, const int32_t *__restrict__ pos, int lags,
                                                               int warmup, const float *__restrict__ center, const float *__restrict__ gamma, int k,
                                                               KmeansSplit sp, double *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_a[ARHMM_OR * ARHMM_OT], s_b[ARHMM_OR * ARHMM_OT], s_g[ARHMM_OR];
  int ib = 0, jb = blockIdx.z;
  for (int t = kmeans_tiles(arhmm_q(d, lags), ARHMM_OT); jb >= t - ib; jb -= t - ib, ib++) {}
  jb += ib;
  arhmm_moments_wg(x, n, d, ldx, pos, lags, warmup, center, gamma, k, sp, blockIdx.x, blockIdx.y, ib, jb, out, s_a, s_b, s_g);
}

__global__ __launch_bounds__(PCA_THREADS) void k_arhmm_mreduce(const double *__restrict__ part, int P, int k, int p, int q, double *__restrict__ moments,
                                                               double *__restrict__ weight) {
  const int64_t e = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (e < (int64_t)k * q * q) arhmm_moments_reduce(part, P, k, p, q, moments, weight, e);
}

// (fac, rhs and dg are read and written by the whole workgroup between barriers: no __restrict__)
__global__ __launch_bounds__(PCA_THREADS) void k_arhmm_solve(const double *__restrict__ moments, const double *__restrict__ weight, int d, int lags,
                                                             const float *__restrict__ center, double ridge, double min_var, double min_weight,
                                                             float *__restrict__ weights, float *__restrict__ vars, float *__restrict__ means,
                                                             int32_t *__restrict__ status, double *fac, double *rhs, double *dg) {
  arhmm_solve_wg(moments, weight, d, lags, center, ridge, min_var, min_weight, weights, vars, means, status, fac, rhs, dg, blockIdx.x);
}

// ----------------------------------------------------------------------------------------------- launches
// the sequence offsets to the workspace and every row's position from them
static int launch_pos(const int32_t *seq_start, int S, int n, float *workspace, const ArhmmWorkspace &w, hipStream_t s, const char *what) {
  TM_HIP(what, hipMemcpyAsync(workspace + w.seq, seq_start, sizeof(int32_t) * (size_t)(S + 1), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_arhmm_pos, dim3(kmeans_tiles(n, PCA_THREADS)), dim3(PCA_THREADS), 0, s, (const int32_t *)(workspace + w.seq), S, n,
                     (int32_t *)(workspace + w.pos));
  return check_launch(what);
}

// (the positions are in the workspace already)
static int launch_emission(const float *x, int n, int d, int64_t ldx, int lags, int warmup, const float *center, const float *weights, const float *vars, int k,
                           float *logb, float *workspace, const ArhmmWorkspace &w, hipStream_t s) {
  float *cj = workspace + w.cj;
  hipLaunchKernelGGL(k_arhmm_const, dim3(kmeans_tiles(k, PCA_THREADS)), dim3(PCA_THREADS), 0, s, vars, d, k, cj);
  hipLaunchKernelGGL(k_arhmm_emission, dim3(kmeans_tiles(n, ARHMM_ROWS)), dim3(PCA_THREADS), 0, s, x, n, d, ldx, (const int32_t *)(workspace + w.pos), lags, warmup,
                     center, weights, vars, k, (const float *)cj, logb);
  return check_launch("tmjx_arhmm_emission");
}

static int launch_moments(const float *x, int n, int d, int64_t ldx, int lags, int warmup, const float *center, const float *gamma, int k, double *moments,
                          double *weight, float *workspace, const ArhmmWorkspace &w, hipStream_t s) {
  double *parts = (double *)(workspace + w.parts);
  hipLaunchKernelGGL(k_arhmm_moments, dim3(w.split.P, k, arhmm_pairs(w.q)), dim3(PCA_THREADS), 0, s, x, n, d, ldx, (const int32_t *)(workspace + w.pos), lags, warmup,
                     center, gamma, k, w.split, parts);
  hipLaunchKernelGGL(k_arhmm_mreduce, dim3((unsigned)(((int64_t)k * w.q * w.q + PCA_THREADS - 1) / PCA_THREADS)), dim3(PCA_THREADS), 0, s, (const double *)parts,
                     w.split.P, k, w.p, w.q, moments, weight);
  return check_launch("tmjx_arhmm_moments");
}

static int launch_solve(const double *moments, const double *weight, int k, int d, int lags, const float *center, double ridge, double min_var, double min_weight,
                        float *weights, float *vars, float *means, int32_t *status, float *workspace, const ArhmmWorkspace &w, hipStream_t s) {
  hipLaunchKernelGGL(k_arhmm_solve, dim3(k), dim3(PCA_THREADS), 0, s, moments, weight, d, lags, center, ridge, min_var, min_weight, weights, vars, means, status,
                     (double *)(workspace + w.fac), (double *)(workspace + w.rhs), (double *)(workspace + w.dg));
  return check_launch("tmjx_arhmm_solve");
}

// ----------------------------------------------------------------------------------------------- entry points
extern "C" {

int tmjx_arhmm_workspace(int n, int d, int lags, int k, int S, int64_t *floats) {
  TM_TRY(arhmm_check_workspace(n, d, lags, k, S, floats));
  *floats = arhmm_workspace(n, d, lags, k, S).floats;
  return TMJX_OK;
}

int tmjx_arhmm_emission(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center,
                        const float *weights, const float *vars, int k, float *logb, float *workspace, void *stream) {
  TM_TRY(arhmm_check_emission(x, n, d, ldx, seq_start, S, lags, warmup, weights, vars, k, logb, workspace));
  const ArhmmWorkspace w = arhmm_workspace(n, d, lags, k, S);
  const int rc = launch_pos(seq_start, S, n, workspace, w, (hipStream_t)stream, "tmjx_arhmm_emission");
  if (rc) return rc;
  return launch_emission(x, n, d, ldx, lags, warmup, center, weights, vars, k, logb, workspace, w, (hipStream_t)stream);
}

int tmjx_arhmm_moments(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center,
                       const float *gamma, int k, double *moments, double *weight, float *workspace, void *stream) {
  TM_TRY(arhmm_check_moments(x, n, d, ldx, seq_start, S, lags, warmup, gamma, k, moments, weight, workspace));
  const ArhmmWorkspace w = arhmm_workspace(n, d, lags, k, S);
  const int rc = launch_pos(seq_start, S, n, workspace, w, (hipStream_t)stream, "tmjx_arhmm_moments");
  if (rc) return rc;
  return launch_moments(x, n, d, ldx, lags, warmup, center, gamma, k, moments, weight, workspace, w, (hipStream_t)stream);
}

int tmjx_arhmm_solve(const double *moments, const double *weight, int k, int d, int lags, const float *center, double ridge, double min_var, double min_weight,
                     float *weights, float *vars, float *means, int32_t *status, float *workspace, void *stream) {
  TM_TRY(arhmm_check_solve(moments, weight, k, d, lags, ridge, min_var, min_weight, weights, vars, status, workspace));
  return launch_solve(moments, weight, k, d, lags, center, ridge, min_var, min_weight, weights, vars, means, status, workspace, arhmm_workspace(1, d, lags, k, 1),
                      (hipStream_t)stream);
}

int tmjx_arhmm_fit(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center, int k, float *weights,
                   float *vars, float *transmat, float *startprob, float *gamma, int32_t *labels, int32_t *status, int max_iter, double tol, double prior,
                   double kappa, double ridge, double min_var, double min_weight, tmjx_arhmm_info_t *info, float *workspace, void *stream) {
  TM_TRY(arhmm_check_fit(x, n, d, ldx, seq_start, S, lags, warmup, k, weights, vars, transmat, startprob, labels, max_iter, tol, prior, kappa, ridge, min_var,
                            min_weight, info, workspace));
  const ArhmmWorkspace w = arhmm_workspace(n, d, lags, k, S);
  const HmmWorkspace hw = hmm_workspace(n, 1, k);
  hipStream_t s = (hipStream_t)stream;
  float *hws = workspace + w.hmm;      // the reused HMM steps' workspace; the fit's own arrays sit where tmjx_hmm_fit keeps them
  float *logb = hws + hw.logb, *g = gamma ? gamma : hws + hw.gamma;
  double *xi = (double *)(hws + hw.xi), *start = (double *)(hws + hw.start), *loglik = (double *)(hws + hw.loglik), *path = (double *)(hws + hw.path),
         *total = (double *)(hws + hw.total), *moments = (double *)(workspace + w.moments), *weight = (double *)(workspace + w.weight);
  int32_t *st = status ? status : (int32_t *)(workspace + w.status);
  hipEvent_t ev[8];
  for (int i = 0; i < 8; i++) TM_HIP("hipEventCreate", hipEventCreate(&ev[i]));
  auto finish = [&](int code) { for (int i = 0; i < 8; i++) (void)hipEventDestroy(ev[i]); return code; };
  int rc = launch_pos(seq_start, S, n, workspace, w, s, "tmjx_arhmm_fit");
  if (rc) return finish(rc);
  info->n_iter = 0; info->converged = 0; info->loglik = 0.0; info->n_singular = 0; info->pad_ = 0;
  info->emission_ms = info->fb_ms = info->mstep_ms = info->viterbi_ms = 0.f;
  double host = 0.0, previous = 0.0;
  float ms = 0.f;
  bool mstep_pending = false;
  // one E-step and the read-back of its total loglik: the only synchronisation of an iteration
  auto estep = [&]() -> int {
    (void)hipEventRecord(ev[0], s);
    int r = launch_emission(x, n, d, ldx, lags, warmup, center, weights, vars, k, logb, workspace, w, s);
    if (r) return r;
    (void)hipEventRecord(ev[1], s);
    if ((r = tmjx_hmm_forward_backward(logb, n, k, seq_start, S, transmat, startprob, g, xi, start, loglik, total, hws, stream))) return r;
    (void)hipEventRecord(ev[2], s);
    hipError_t e = hipMemcpyAsync(&host, total, sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(TMJX_EHIP, std::string("tmjx_arhmm_fit: ") + hipGetErrorString(e));
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
    if ((rc = launch_moments(x, n, d, ldx, lags, warmup, center, g, k, moments, weight, workspace, w, s))) return finish(rc);
    if ((rc = launch_solve(moments, weight, k, d, lags, center, ridge, min_var, min_weight, weights, vars, nullptr, st, workspace, w, s))) return finish(rc);
    if ((rc = tmjx_hmm_transitions(xi, start, k, prior, kappa, transmat, startprob, stream))) return finish(rc);
    (void)hipEventRecord(ev[4], s);
    mstep_pending = true;
  }
  // after a break the parameters are those of the last E-step, whose outputs stand; after max_iter M-steps one more E-step against the final ones
  if (!info->converged && (rc = estep())) return finish(rc);
  info->loglik = host;
  (void)hipEventRecord(ev[5], s);
  if ((rc = tmjx_hmm_viterbi(logb, n, k, seq_start, S, transmat, startprob, 0, labels, path, hws, stream))) return finish(rc);
  (void)hipEventRecord(ev[6], s);
  // the states the last M-step found singular (the only other read-back, after the loop)
  int32_t codes[HMM_MAX_K];
  hipError_t e = hipMemcpyAsync(codes, st, sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return finish(fail(TMJX_EHIP, std::string("tmjx_arhmm_fit: ") + hipGetErrorString(e)));
  for (int j = 0; j < k; j++) info->n_singular += codes[j] == 2;
  if (hipEventElapsedTime(&ms, ev[5], ev[6]) == hipSuccess) info->viterbi_ms = ms;
  return finish(TMJX_OK);
}

}  // extern "C"
