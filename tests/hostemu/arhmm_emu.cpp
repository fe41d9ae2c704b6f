// tests/hostemu/arhmm_emu.cpp — TEST-ONLY host emulation of the autoregressive-HMM C-ABI (include/tmjx.h: tmjx_arhmm_workspace, tmjx_arhmm_emission,
// tmjx_arhmm_moments, tmjx_arhmm_solve, tmjx_arhmm_fit): the bodies of csrc/arhmm_core.h and the checks of csrc/arhmm_host.h compiled with g++, one
// loop iteration where the GPU has one workgroup, in the order of the launches of csrc/tmjx_arhmm.hip.  A library of its own: it includes
// analysis_emu.cpp for the tmjx_hmm_* steps the fit reuses, and adds the tmjx_arhmm_* names.  With -DARHMM_EMU_MAIN it is a stand-alone program
// (for sanitizer builds):
//   arhmm_emu [d lags k len...] — fits one planted problem (3 features, 2 lags, 2 states, sequences of 1, 2, 3 and 140 rows by default, strided)
//   and prints a checksum.
#pragma once
#ifdef ARHMM_EMU_MAIN
#undef HMM_EMU_MAIN
#undef KMEANS_EMU_MAIN
#undef PCA_WIDE_EMU_MAIN
#undef PCA_EMU_MAIN
#undef READOUT_EMU_MAIN
#undef SPECTROGRAM_EMU_MAIN
#endif
#include "analysis_emu.cpp"

#include "../../track_mjx_amd/csrc/arhmm_host.h"

static void aemu_pos_run(const int32_t *seq_start, int S, int n, float *workspace, const ArhmmWorkspace &w) {
  int32_t *seq = (int32_t *)(workspace + w.seq), *pos = (int32_t *)(workspace + w.pos);
  memcpy(seq, seq_start, sizeof(int32_t) * (size_t)(S + 1));
  for (int t = 0; t < n; t++) pos[t] = arhmm_pos(seq, S, t);
}

static void aemu_emission_run(const float *x, int n, int d, int64_t ldx, int lags, int warmup, const float *center, const float *weights, const float *vars,
                              int k, float *logb, float *workspace, const ArhmmWorkspace &w) {
  std::vector<float> s_x(ARHMM_MAX_D * ARHMM_LDX), s_w(ARHMM_TK * ARHMM_LDW);
  float *cj = workspace + w.cj;
  for (int j = 0; j < k; j++) cj[j] = hmm_logconst(vars, d, j);
  for (int wg = 0; wg < kmeans_tiles(n, ARHMM_ROWS); wg++)
    arhmm_emission_wg(x, n, d, ldx, (const int32_t *)(workspace + w.pos), lags, warmup, center, weights, vars, k, cj, logb, wg, s_x.data(), s_w.data());
}

static void aemu_moments_run(const float *x, int n, int d, int64_t ldx, int lags, int warmup, const float *center, const float *gamma, int k, double *moments,
                             double *weight, float *workspace, const ArhmmWorkspace &w) {
  double *parts = (double *)(workspace + w.parts);
  std::vector<float> s_a(ARHMM_OR * ARHMM_OT), s_b(ARHMM_OR * ARHMM_OT), s_g(ARHMM_OR);
  const int tiles = kmeans_tiles(w.q, ARHMM_OT);
  for (int part = 0; part < w.split.P; part++)
    for (int j = 0; j < k; j++)
      for (int ib = 0; ib < tiles; ib++)
        for (int jb = ib; jb < tiles; jb++)
          arhmm_moments_wg(x, n, d, ldx, (const int32_t *)(workspace + w.pos), lags, warmup, center, gamma, k, w.split, part, j, ib, jb, parts, s_a.data(),
                           s_b.data(), s_g.data());
  for (int64_t e = 0; e < (int64_t)k * w.q * w.q; e++) arhmm_moments_reduce(parts, w.split.P, k, w.p, w.q, moments, weight, e);
}

static void aemu_solve_run(const double *moments, const double *weight, int k, int d, int lags, const float *center, double ridge, double min_var,
                           double min_weight, float *weights, float *vars, float *means, int32_t *status, float *workspace, const ArhmmWorkspace &w) {
  for (int j = 0; j < k; j++)
    arhmm_solve_wg(moments, weight, d, lags, center, ridge, min_var, min_weight, weights, vars, means, status, (double *)(workspace + w.fac),
                   (double *)(workspace + w.rhs), (double *)(workspace + w.dg), j);
}

extern "C" {
int tmjx_arhmm_workspace(int n, int d, int lags, int k, int S, int64_t *floats) {
  EMU_TRY(arhmm_check_workspace(n, d, lags, k, S, floats));
  *floats = arhmm_workspace(n, d, lags, k, S).floats;
  return 0;
}

int tmjx_arhmm_emission(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center,
                        const float *weights, const float *vars, int k, float *logb, float *workspace, void *) {
  EMU_TRY(arhmm_check_emission(x, n, d, ldx, seq_start, S, lags, warmup, weights, vars, k, logb, workspace));
  const ArhmmWorkspace w = arhmm_workspace(n, d, lags, k, S);
  aemu_pos_run(seq_start, S, n, workspace, w);
  aemu_emission_run(x, n, d, ldx, lags, warmup, center, weights, vars, k, logb, workspace, w);
  return 0;
}

int tmjx_arhmm_moments(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center,
                       const float *gamma, int k, double *moments, double *weight, float *workspace, void *) {
  EMU_TRY(arhmm_check_moments(x, n, d, ldx, seq_start, S, lags, warmup, gamma, k, moments, weight, workspace));
  const ArhmmWorkspace w = arhmm_workspace(n, d, lags, k, S);
  aemu_pos_run(seq_start, S, n, workspace, w);
  aemu_moments_run(x, n, d, ldx, lags, warmup, center, gamma, k, moments, weight, workspace, w);
  return 0;
}

int tmjx_arhmm_solve(const double *moments, const double *weight, int k, int d, int lags, const float *center, double ridge, double min_var, double min_weight,
                     float *weights, float *vars, float *means, int32_t *status, float *workspace, void *) {
  EMU_TRY(arhmm_check_solve(moments, weight, k, d, lags, ridge, min_var, min_weight, weights, vars, status, workspace));
  aemu_solve_run(moments, weight, k, d, lags, center, ridge, min_var, min_weight, weights, vars, means, status, workspace, arhmm_workspace(1, d, lags, k, 1));
  return 0;
}

int tmjx_arhmm_fit(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int lags, int warmup, const float *center, int k, float *weights,
                   float *vars, float *transmat, float *startprob, float *gamma, int32_t *labels, int32_t *status, int max_iter, double tol, double prior,
                   double kappa, double ridge, double min_var, double min_weight, tmjx_arhmm_info_t *info, float *workspace, void *) {
  EMU_TRY(arhmm_check_fit(x, n, d, ldx, seq_start, S, lags, warmup, k, weights, vars, transmat, startprob, labels, max_iter, tol, prior, kappa, ridge, min_var,
                          min_weight, info, workspace));
  const ArhmmWorkspace w = arhmm_workspace(n, d, lags, k, S);
  const HmmWorkspace hw = hmm_workspace(n, 1, k);
  float *hws = workspace + w.hmm;
  float *logb = hws + hw.logb, *g = gamma ? gamma : hws + hw.gamma;
  double *xi = (double *)(hws + hw.xi), *start = (double *)(hws + hw.start), *loglik = (double *)(hws + hw.loglik), *path = (double *)(hws + hw.path),
         *total = (double *)(hws + hw.total), *moments = (double *)(workspace + w.moments), *weight = (double *)(workspace + w.weight);
  int32_t *st = status ? status : (int32_t *)(workspace + w.status);
  aemu_pos_run(seq_start, S, n, workspace, w);
  info->n_iter = 0; info->converged = 0; info->loglik = 0.0; info->n_singular = 0; info->pad_ = 0;
  info->emission_ms = info->fb_ms = info->mstep_ms = info->viterbi_ms = 0.f;
  double previous = 0.0;
  auto estep = [&]() -> int {
    aemu_emission_run(x, n, d, ldx, lags, warmup, center, weights, vars, k, logb, workspace, w);
    return tmjx_hmm_forward_backward(logb, n, k, seq_start, S, transmat, startprob, g, xi, start, loglik, total, hws, nullptr);
  };
  int rc = 0;
  for (int it = 0; it < max_iter; it++) {
    if ((rc = estep())) return rc;
    info->n_iter = it + 1;
    if (hmm_converged(it, *total, previous, tol)) { info->converged = 1; break; }
    previous = *total;
    aemu_moments_run(x, n, d, ldx, lags, warmup, center, g, k, moments, weight, workspace, w);
    aemu_solve_run(moments, weight, k, d, lags, center, ridge, min_var, min_weight, weights, vars, nullptr, st, workspace, w);
    if ((rc = tmjx_hmm_transitions(xi, start, k, prior, kappa, transmat, startprob, nullptr))) return rc;
  }
  if (!info->converged && (rc = estep())) return rc;
  info->loglik = *total;
  if ((rc = tmjx_hmm_viterbi(logb, n, k, seq_start, S, transmat, startprob, 0, labels, path, hws, nullptr))) return rc;
  for (int j = 0; j < k; j++) info->n_singular += st[j] == 2;
  return 0;
}
}  // extern "C"

#ifdef ARHMM_EMU_MAIN
static float alcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }

int main(int argc, char **argv) {
  const int d = argc > 4 ? atoi(argv[1]) : 3, lags = argc > 4 ? atoi(argv[2]) : 2, k = argc > 4 ? atoi(argv[3]) : 2;
  std::vector<int32_t> seq(1, 0);
  if (argc > 4) for (int a = 4; a < argc; a++) seq.push_back(seq.back() + atoi(argv[a]));
  else for (int len : {1, 2, 3, 140}) seq.push_back(seq.back() + len);
  const int S = (int)seq.size() - 1, n = seq.back(), ldx = d + 5, p = arhmm_p(d, lags), q = p + d;
  uint32_t seed = 31;
  // state (r / 25) % k contracts every feature by its own factor: x_t = a_j x_(t-1) + noise
  std::vector<float> x((size_t)n * ldx, 1e6f), center(d, 0.25f), W((size_t)k * d * p, 0.f), var((size_t)k * d, 1.f), A((size_t)k * k, 1.f / k), pi(k, 1.f / k);
  for (int r = 0; r < n; r++)
    for (int c = 0; c < d; c++) {
      const float a = 0.9f - 1.6f * (float)((r / 25) % k) / (float)(k > 1 ? k - 1 : 1);
      x[(size_t)r * ldx + c] = 0.25f + (r ? a * (x[(size_t)(r - 1) * ldx + c] - 0.25f) : 0.f) + alcg(seed);
    }
  for (int j = 0; j < k; j++)
    for (int c = 0; c < d && lags > 0; c++) W[((size_t)j * d + c) * p + c] = 0.8f - 1.4f * (float)j / (float)(k > 1 ? k - 1 : 1);
  std::vector<float> gamma((size_t)n * k), logb((size_t)n * k), means((size_t)k * d);
  std::vector<int32_t> labels(n), status(k), again(n);
  std::vector<double> M((size_t)k * q * q), wt(k), xi((size_t)k * k), start(k), ll(S), path(S);
  int64_t floats = 0;
  if (tmjx_arhmm_workspace(n, d, lags, k, S, &floats)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<double> ws((size_t)floats / 2 + 2);      // exactly the size asked for (rounded up to a double), so a sanitizer sees any overrun
  float *wsa = (float *)ws.data();
  tmjx_arhmm_info_t info;
  if (tmjx_arhmm_fit(x.data(), n, d, ldx, seq.data(), S, lags, lags + 1, center.data(), k, W.data(), var.data(), A.data(), pi.data(), gamma.data(), labels.data(),
                     status.data(), 12, 1e-6, 0.1, 0.0, 0.5, 1e-3, 1e-3, &info, wsa, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  double total = 0.0;
  const HmmWorkspace hw = hmm_workspace(n, 1, k);
  float *hws = wsa + arhmm_workspace(n, d, lags, k, S).hmm;
  (void)hw;
  if (tmjx_arhmm_emission(x.data(), n, d, ldx, seq.data(), S, lags, lags + 1, center.data(), W.data(), var.data(), k, logb.data(), wsa, nullptr) ||
      tmjx_hmm_forward_backward(logb.data(), n, k, seq.data(), S, A.data(), pi.data(), gamma.data(), xi.data(), start.data(), ll.data(), &total, hws, nullptr) ||
      tmjx_hmm_viterbi(logb.data(), n, k, seq.data(), S, A.data(), pi.data(), 0, again.data(), path.data(), hws, nullptr) ||
      tmjx_arhmm_moments(x.data(), n, d, ldx, seq.data(), S, lags, lags + 1, center.data(), gamma.data(), k, M.data(), wt.data(), wsa, nullptr) ||
      tmjx_arhmm_solve(M.data(), wt.data(), k, d, lags, center.data(), 0.5, 1e-3, 1e-3, W.data(), var.data(), means.data(), status.data(), wsa, nullptr)) {
    fprintf(stderr, "%s\n", g_err.c_str());
    return 1;
  }
  double sum = total;
  for (float v : W) sum += fabs(v);
  for (float v : A) sum += v;
  printf("arhmm_emu: %d rows x %d in %d sequences, %d lags, %d states (ld %d): %d iterations, loglik %.6f, %d singular, the same path again: %d\n", n, d, S, lags,
         k, ldx, info.n_iter, info.loglik, info.n_singular, (int)(again == labels));
  printf("arhmm_emu: checksum %.6f\n", sum);
  return again == labels && total == info.loglik ? 0 : 1;
}
#endif
