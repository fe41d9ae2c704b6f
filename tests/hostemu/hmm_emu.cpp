// tests/hostemu/hmm_emu.cpp — TEST-ONLY host emulation of the hidden-Markov-model C-ABI (include/tmjx.h: tmjx_hmm_workspace, tmjx_hmm_emission,
// tmjx_hmm_forward_backward, tmjx_hmm_mstep, tmjx_hmm_transitions, tmjx_hmm_viterbi, tmjx_hmm_fit): the bodies of csrc/hmm_core.h and the checks of
// csrc/hmm_host.h compiled with g++, one loop iteration where the GPU has one workgroup, in the order of the launches of csrc/tmjx_hmm.hip.  It
// includes kmeans_emu.cpp for the column sums it shares with the k-means.  With -DHMM_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   hmm_emu [d k len...] — fits one planted problem (3 features, 2 states, sequences of 1, 2 and 40 rows by default, strided) and prints a checksum.
#pragma once
#ifdef HMM_EMU_MAIN
#undef KMEANS_EMU_MAIN
#undef PCA_WIDE_EMU_MAIN
#undef PCA_EMU_MAIN
#endif
#include "kmeans_emu.cpp"

#include "../../track_mjx_amd/csrc/hmm_host.h"

static void hemu_emission_run(const float *x, int n, int d, int64_t ldx, const float *means, const float *vars, int k, float *logb, float *cj) {
  std::vector<float> s_x(HMM_TK * HMM_LDX), s_m(HMM_TK * HMM_LDC), s_iv(HMM_TK * HMM_LDC);
  for (int j = 0; j < k; j++) cj[j] = hmm_logconst(vars, d, j);
  for (int wg = 0; wg < kmeans_tiles(n, HMM_ROWS); wg++) hmm_emission_wg(x, n, d, ldx, means, vars, k, cj, logb, wg, s_x.data(), s_m.data(), s_iv.data());
}

static void hemu_fb_run(const float *logb, int n, int k, const int32_t *seq, int S, const float *transmat, const float *startprob, float *gamma, double *xi,
                        double *start, double *loglik, double *total, float *workspace, const HmmWorkspace &w) {
  float *alphahat = workspace + w.alphahat, *vnext = workspace + w.vnext;
  double *xipart = (double *)(workspace + w.xipart);
  std::vector<double> lds((hmm_fb_lds_floats(k) + 1) / 2);      // exactly the dynamic LDS of the launch
  for (int s = 0; s < S; s++)
    hmm_fb_wg(logb, k, seq[s], seq[s + 1], transmat, startprob, workspace + w.mrow, workspace + w.cs, alphahat, vnext, gamma, loglik, s, (float *)lds.data());
  hmm_start_total_wg(gamma, k, seq, S, loglik, start, total);
  std::vector<float> s_a(HMM_OR * HMM_OT), s_b(HMM_OR * HMM_OT);
  const int tiles = kmeans_tiles(k, HMM_OT);
  for (int p = 0; p < w.xsplit.P; p++)
    for (int ib = 0; ib < tiles; ib++)
      for (int jb = 0; jb < tiles; jb++)
        hmm_outer_wg(alphahat, k, k, vnext, k, k, nullptr, n, w.xsplit, p, ib, jb, xipart, nullptr, nullptr, s_a.data(), s_b.data());
  for (int e = 0; e < k * k; e++) hmm_xi_reduce(xipart, w.xsplit.P, k, transmat, xi, e);
}

static void hemu_mstep_run(const float *x, int n, int d, int64_t ldx, const float *gamma, int k, double min_var, double min_weight, float *means, float *vars,
                           double *weight, float *workspace, const HmmWorkspace &w) {
  double *colsum = (double *)(workspace + w.colsum), *p1 = (double *)(workspace + w.part1), *p2 = (double *)(workspace + w.part2),
         *pw = (double *)(workspace + w.partw);
  float *mean = workspace + w.mean;
  std::vector<double> s_sum(2 * PCA_WIDE_TILE);
  for (int ch = 0; ch < w.nchunks; ch++)
    for (int cb = 0; cb < pca_wide_tiles(d); cb++) kmeans_colsum_wg(x, ldx, n, d, ch, cb, colsum, s_sum.data());
  for (int c = 0; c < d; c++) mean[c] = kmeans_mean_col(colsum, w.nchunks, d, n, c);
  std::vector<float> s_a(HMM_OR * HMM_OT), s_b(HMM_OR * HMM_OT);
  for (int p = 0; p < w.msplit.P; p++)
    for (int ib = 0; ib < kmeans_tiles(k, HMM_OT); ib++)
      for (int jb = 0; jb < kmeans_tiles(d, HMM_OT); jb++) hmm_outer_wg(gamma, k, k, x, ldx, d, mean, n, w.msplit, p, ib, jb, p1, p2, pw, s_a.data(), s_b.data());
  for (int e = 0; e < k * d; e++) hmm_mstep_reduce(p1, p2, pw, w.msplit.P, k, d, mean, min_var, min_weight, means, vars, weight, e);
}

static void hemu_viterbi_run(const float *logb, int k, const int32_t *seq, int S, const float *transmat, const float *startprob, int logspace, int32_t *labels,
                             double *path_logprob, float *workspace, const HmmWorkspace &w) {
  std::vector<float> lds(k * hmm_lda(k) + 2 * HMM_THREADS);
  for (int s = 0; s < S; s++)
    hmm_viterbi_wg(logb, k, seq[s], seq[s + 1], transmat, startprob, logspace, (uint8_t *)(workspace + w.bp), labels, path_logprob, s, lds.data());
}

static const int32_t *hemu_seq(const int32_t *seq_start, int S, float *workspace, const HmmWorkspace &w) {
  memcpy(workspace + w.seq, seq_start, sizeof(int32_t) * (size_t)(S + 1));
  return (const int32_t *)(workspace + w.seq);
}

extern "C" {
int tmjx_hmm_workspace(int n, int d, int k, int S, int64_t *floats) {
  EMU_TRY(hmm_check_workspace(n, d, k, S, floats));
  *floats = hmm_workspace(n, d, k).floats;
  return 0;
}

int tmjx_hmm_emission(const float *x, int n, int d, int64_t ldx, const float *means, const float *vars, int k, float *logb, float *workspace, void *) {
  EMU_TRY(hmm_check_emission(x, n, d, ldx, means, vars, k, logb, workspace));
  hemu_emission_run(x, n, d, ldx, means, vars, k, logb, workspace + hmm_workspace(n, d, k).cj);
  return 0;
}

int tmjx_hmm_forward_backward(const float *logb, int n, int k, const int32_t *seq_start, int S, const float *transmat, const float *startprob, float *gamma,
                              double *xi, double *start, double *loglik, double *total, float *workspace, void *) {
  EMU_TRY(hmm_check_fb(logb, n, k, seq_start, S, transmat, startprob, gamma, xi, start, loglik, total, workspace));
  const HmmWorkspace w = hmm_workspace(n, 1, k);
  hemu_fb_run(logb, n, k, hemu_seq(seq_start, S, workspace, w), S, transmat, startprob, gamma, xi, start, loglik, total, workspace, w);
  return 0;
}

int tmjx_hmm_mstep(const float *x, int n, int d, int64_t ldx, const float *gamma, int k, double min_var, double min_weight, float *means, float *vars,
                   double *weight, float *workspace, void *) {
  EMU_TRY(hmm_check_mstep(x, n, d, ldx, gamma, k, min_var, min_weight, means, vars, weight, workspace));
  hemu_mstep_run(x, n, d, ldx, gamma, k, min_var, min_weight, means, vars, weight, workspace, hmm_workspace(n, d, k));
  return 0;
}

int tmjx_hmm_transitions(const double *xi, const double *start, int k, double prior, double kappa, float *transmat, float *startprob, void *) {
  EMU_TRY(hmm_check_transitions(xi, start, k, prior, kappa, transmat, startprob));
  hmm_transitions_wg(xi, start, k, prior, kappa, transmat, startprob);
  return 0;
}

int tmjx_hmm_viterbi(const float *logb, int n, int k, const int32_t *seq_start, int S, const float *transmat, const float *startprob, int logspace,
                     int32_t *labels, double *path_logprob, float *workspace, void *) {
  EMU_TRY(hmm_check_viterbi(logb, n, k, seq_start, S, transmat, startprob, labels, path_logprob, workspace));
  const HmmWorkspace w = hmm_workspace(n, 1, k);
  hemu_viterbi_run(logb, k, hemu_seq(seq_start, S, workspace, w), S, transmat, startprob, logspace, labels, path_logprob, workspace, w);
  return 0;
}

int tmjx_hmm_fit(const float *x, int n, int d, int64_t ldx, const int32_t *seq_start, int S, int k, float *means, float *vars, float *transmat,
                 float *startprob, float *gamma, int32_t *labels, int max_iter, double tol, double prior, double kappa, double min_var, double min_weight,
                 tmjx_hmm_info_t *info, float *workspace, void *) {
  EMU_TRY(hmm_check_fit(x, n, d, ldx, seq_start, S, k, means, vars, transmat, startprob, labels, max_iter, tol, prior, kappa, min_var, min_weight, info,
                        workspace));
  const HmmWorkspace w = hmm_workspace(n, d, k);
  const int32_t *seq = hemu_seq(seq_start, S, workspace, w);
  float *logb = workspace + w.logb, *cj = workspace + w.cj, *g = gamma ? gamma : workspace + w.gamma;
  double *xi = (double *)(workspace + w.xi), *start = (double *)(workspace + w.start), *weight = (double *)(workspace + w.weight),
         *loglik = (double *)(workspace + w.loglik), *path = (double *)(workspace + w.path), *total = (double *)(workspace + w.total);
  info->n_iter = 0; info->converged = 0; info->loglik = 0.0;
  info->emission_ms = info->fb_ms = info->mstep_ms = info->viterbi_ms = 0.f;
  double previous = 0.0;
  auto estep = [&]() {
    hemu_emission_run(x, n, d, ldx, means, vars, k, logb, cj);
    hemu_fb_run(logb, n, k, seq, S, transmat, startprob, g, xi, start, loglik, total, workspace, w);
  };
  for (int it = 0; it < max_iter; it++) {
    estep();
    info->n_iter = it + 1;
    if (hmm_converged(it, *total, previous, tol)) { info->converged = 1; break; }
    previous = *total;
    hemu_mstep_run(x, n, d, ldx, g, k, min_var, min_weight, means, vars, weight, workspace, w);
    hmm_transitions_wg(xi, start, k, prior, kappa, transmat, startprob);
  }
  if (!info->converged) estep();
  info->loglik = *total;
  hemu_viterbi_run(logb, k, seq, S, transmat, startprob, 0, labels, path, workspace, w);
  return 0;
}
}  // extern "C"

#ifdef HMM_EMU_MAIN
static float hlcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }

int main(int argc, char **argv) {
  const int d = argc > 3 ? atoi(argv[1]) : 3, k = argc > 3 ? atoi(argv[2]) : 2;
  std::vector<int32_t> seq(1, 0);
  if (argc > 3) for (int a = 3; a < argc; a++) seq.push_back(seq.back() + atoi(argv[a]));
  else for (int len : {1, 2, 40}) seq.push_back(seq.back() + len);
  const int S = (int)seq.size() - 1, n = seq.back(), ldx = d + 5;
  uint32_t seed = 31;
  std::vector<float> centre((size_t)k * d), x((size_t)n * ldx, 1e6f), mu((size_t)k * d), var((size_t)k * d, 1.f), A((size_t)k * k, 1.f / k), pi(k, 1.f / k);
  for (float &v : centre) v = 6.f * hlcg(seed) + 3.f;
  for (int r = 0; r < n; r++)
    for (int c = 0; c < d; c++) x[(size_t)r * ldx + c] = centre[(size_t)((r / 5) % k) * d + c] + hlcg(seed);
  for (size_t e = 0; e < mu.size(); e++) mu[e] = centre[e] + 0.5f * hlcg(seed);
  std::vector<float> gamma((size_t)n * k);
  std::vector<int32_t> labels(n);
  int64_t floats = 0;
  if (tmjx_hmm_workspace(n, d, k, S, &floats)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<double> ws((size_t)floats / 2 + 2);      // exactly the size asked for (rounded up to a double), so a sanitizer sees any overrun
  float *wsa = (float *)ws.data();
  tmjx_hmm_info_t info;
  if (tmjx_hmm_fit(x.data(), n, d, ldx, seq.data(), S, k, mu.data(), var.data(), A.data(), pi.data(), gamma.data(), labels.data(), 20, 1e-6, 0.1, 0.0, 1e-3, 1e-3, &info,
                   wsa, nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  std::vector<float> logb((size_t)n * k);
  std::vector<double> xi((size_t)k * k), start(k), ll(S), path(S), weight(k);
  double total = 0.0;
  std::vector<int32_t> again(n);
  if (tmjx_hmm_emission(x.data(), n, d, ldx, mu.data(), var.data(), k, logb.data(), wsa, nullptr) ||
      tmjx_hmm_forward_backward(logb.data(), n, k, seq.data(), S, A.data(), pi.data(), gamma.data(), xi.data(), start.data(), ll.data(), &total, wsa, nullptr) ||
      tmjx_hmm_viterbi(logb.data(), n, k, seq.data(), S, A.data(), pi.data(), 0, again.data(), path.data(), wsa, nullptr) ||
      tmjx_hmm_mstep(x.data(), n, d, ldx, gamma.data(), k, 1e-3, 1e-3, mu.data(), var.data(), weight.data(), wsa, nullptr) ||
      tmjx_hmm_transitions(xi.data(), start.data(), k, 0.1, 0.0, A.data(), pi.data(), nullptr)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
  double sum = total;
  for (float v : mu) sum += fabs(v);
  for (float v : A) sum += v;
  printf("hmm_emu: %d rows x %d in %d sequences, %d states (ld %d): %d iterations, loglik %.6f, the same path again: %d\n", n, d, S, k, ldx, info.n_iter,
         info.loglik, (int)(again == labels));
  printf("hmm_emu: checksum %.6f\n", sum);
  return again == labels && total == info.loglik ? 0 : 1;
}
#endif
