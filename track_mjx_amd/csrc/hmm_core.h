// csrc/hmm_core.h — the bodies of the hidden-Markov-model kernels (DESIGN.md "Sequence model"; include/tmjx.h: tmjx_hmm_*): K states with
// diagonal-covariance Gaussian emissions over recorded activations x [n][d], the rows split into S sequences.  Written with the PCA_WG / PCA_PAR /
// PCA_SYNC discipline of csrc/wg_core.h, so that they also compile on the host (tests/hostemu/hmm_emu.cpp; the column mean and the row split are
// csrc/moments_core.h, km_f4 and kmeans_inf the k-means'): whatever a thread carries from one
// PCA_PAR region to the next lives in LDS.  Every product is a chain of float32 FMAs in a fixed order, every sum across rows or workgroups is
// float64 in a fixed order: no floating-point atomics, the same bits on every run.
#pragma once
#include "kmeans_core.h"
#include "moments_core.h"

#define HMM_MAX_D 1024
#define HMM_MAX_K 128
#define HMM_THREADS 128          // threads of a forward-backward or Viterbi workgroup: thread j owns state j
#define HMM_GROUP 16             // the K-term sums of a step: groups of 16 consecutive states added in order, then the groups in order
#define HMM_ROWS 128             // rows of x an emission workgroup owns
#define HMM_TILE 64              // states of one tile of its walk
#define HMM_TK 32                // features staged per barrier pair
#define HMM_LDX 132              // row stride of the staged rows  s_x[feature][row]
#define HMM_LDC 68               // row stride of the staged means and inverse variances  s_m, s_iv [feature][state]
#define HMM_OT 64                // side of an output tile of the outer-product sums (M-step, expected transitions)
#define HMM_OR 16                // rows staged per barrier pair there
#define HMM_MIN_PART 16          // row parts of those sums: at most max(16, 2^22 / (rows x columns of the output)) parts, whatever n is
#define HMM_PART_DOUBLES (1 << 22)

PCA_HD int hmm_lda(int k) { return k | 1; }      // row stride of the transition matrix in LDS: odd, so a column walk (thread j reads A[i][j]) and a row walk
                                                 // (thread i reads A[i][j]) both touch k different banks
PCA_HD int hmm_fb_lds_floats(int k) { return k * hmm_lda(k) + 4 * HMM_THREADS + HMM_GROUP + 4; }
PCA_HD int hmm_groups(int k) { return (k + HMM_GROUP - 1) / HMM_GROUP; }

// the fixed row split of the outer-product sums with an output of ka x kb: chunks of 256 rows, `per` consecutive chunks to a part.  It depends on
// n, ka and kb only.
PCA_HD KmeansSplit hmm_split(int n, int ka, int kb) {
  KmeansSplit s;
  int cap = HMM_PART_DOUBLES / (ka * kb);
  if (cap < HMM_MIN_PART) cap = HMM_MIN_PART;
  s.nchunks = pca_nwg(n);
  s.per = (s.nchunks + cap - 1) / cap;
  s.P = (s.nchunks + s.per - 1) / s.per;
  return s;
}

// ----------------------------------------------------------------------------------------------- emission
// c_j = -1/2 sum_c log(2 pi var_jc), in float64, rounded once
TM_DEV float hmm_logconst(const float *vars, int d, int j) {
  double s = 0.0;
  for (int c = 0; c < d; c++) s += log(6.283185307179586476925 * (double)vars[(int64_t)j * d + c]);
  return (float)(-0.5 * s);
}

// logb of the rows [128 wg, 128 wg + 128): the workgroup walks the state tiles in order; thread (ty, tx) owns the rows 8 ty + u and, in a tile, the
// states 4 tx + v.  q = sum_c (x - mu)^2 / var written directly: v = x - mu, q = fma(v, v * (1 / var), q), one chain per (row, state) in ascending
// feature order, no expansion into moments: every term is non-negative.  logb = fma(-1/2, q, c_j).  The padding of a stage is x = mu = 0,
// 1 / var = 0: it adds +0.  s_x: [HMM_TK][HMM_LDX], s_m and s_iv: [HMM_TK][HMM_LDC] floats of LDS.
PCA_WG void hmm_emission_wg(const float *x, int n, int d, int64_t ldx, const float *means, const float *vars, int k, const float *cj, float *logb, int wg,
                            float *s_x, float *s_m, float *s_iv) {
  const int64_t r0 = (int64_t)wg * HMM_ROWS;
  PCA_PRIVATE(float, acc, 32);
  for (int c0 = 0; c0 < k; c0 += HMM_TILE) {
    PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
      for (int e = 0; e < 32; e++) PCA_MINE(acc, tid)[e] = 0.f;
    }
    for (int k0 = 0; k0 < d; k0 += HMM_TK) {
      PCA_PAR(tid, PCA_THREADS) {
        for (int e = tid; e < HMM_ROWS * HMM_TK; e += PCA_THREADS) {
          const int row = e / HMM_TK, f = e % HMM_TK;
          s_x[f * HMM_LDX + row] = (r0 + row < n && k0 + f < d) ? x[(r0 + row) * ldx + k0 + f] : 0.f;
        }
        for (int e = tid; e < HMM_TILE * HMM_TK; e += PCA_THREADS) {
          const int j = e / HMM_TK, f = e % HMM_TK;
          const bool in = c0 + j < k && k0 + f < d;
          s_m[f * HMM_LDC + j] = in ? means[(int64_t)(c0 + j) * d + k0 + f] : 0.f;
          s_iv[f * HMM_LDC + j] = in ? 1.f / vars[(int64_t)(c0 + j) * d + k0 + f] : 0.f;
        }
      }
      PCA_SYNC();
      PCA_PAR(tid, PCA_THREADS) {
        const int ty = tid >> 4, tx = tid & 15;
        float *mine = PCA_MINE(acc, tid);
#pragma unroll 4
        for (int f = 0; f < HMM_TK; f++) {
          const km_f4 a0 = *(const km_f4 *)(s_x + f * HMM_LDX + 8 * ty), a1 = *(const km_f4 *)(s_x + f * HMM_LDX + 8 * ty + 4);
          const km_f4 mu = *(const km_f4 *)(s_m + f * HMM_LDC + 4 * tx), iv = *(const km_f4 *)(s_iv + f * HMM_LDC + 4 * tx);
#pragma unroll
          for (int u = 0; u < 8; u++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
              const float df = (u < 4 ? a0[u] : a1[u - 4]) - mu[v];
              mine[u * 4 + v] = fmaf(df, df * iv[v], mine[u * 4 + v]);
            }
        }
      }
      PCA_SYNC();
    }
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int j = c0 + 4 * tx + v;
        if (j < k) {
          const float c = cj[j];
#pragma unroll
          for (int u = 0; u < 8; u++)
            if (r0 + 8 * ty + u < n) logb[(r0 + 8 * ty + u) * k + j] = fmaf(-0.5f, PCA_MINE(acc, tid)[u * 4 + v], c);
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- forward-backward
// the sum of s_v[0 .. k) as every thread forms it: the groups' sums s_part (each 16 consecutive entries added in order) added in order
TM_DEV float hmm_sum_groups(const float *s_part, int k) {
  float c = 0.f;
  for (int g = 0; g < hmm_groups(k); g++) c += s_part[g];
  return c;
}
TM_DEV void hmm_group_sum(const float *s_v, float *s_part, int k, int g) {
  float s = 0.f;
  for (int q = g * HMM_GROUP; q < (g + 1) * HMM_GROUP && q < k; q++) s += s_v[q];
  s_part[g] = s;
}
TM_DEV float hmm_btilde(float lb, float m) { return m == -kmeans_inf() ? 0.f : expf(lb - m); }

// The scaled recursion of the sequence [t0, t1), one workgroup of HMM_THREADS, thread j owning state j.  With m_t = max_j logb_t(j) and
// bt_t(j) = exp(logb_t(j) - m_t):
//   forward   a_t(j) = bt_t(j) sum_i ah_(t-1)(i) A_ij  (pi_j bt_t(j) at t0), c_t = sum_j a_t(j), ah_t = a_t / c_t; loglik = sum_t (log c_t + m_t), float64
//   backward  bh_(T-1) = 1, w_t(j) = bt_t(j) bh_t(j) / c_t, bh_(t-1)(i) = sum_j A_ij w_t(j); gamma_t = ah_t bh_t / sum_j ah_t(j) bh_t(j)
// The K-term sums are fmaf chains in ascending index order; c_t and the normaliser of gamma go by hmm_group_sum.  alphahat [n][k] and
// vnext [n][k] (row t holds w_(t+1), zeros in the last row of the sequence) are left for the expected transitions; mrow [n] and cs [n] are scratch.
// A sequence the model gives probability zero (some c_t == 0) gets loglik = -inf and gamma rows of zeros: every a from that step on is 0, and
// every w before it, so no NaN is formed.
// s: hmm_fb_lds_floats(k) floats of LDS: A [k][hmm_lda(k)], ah [128], bh [128], tmp [128], w [128], part [16], then one float64 for the loglik.
PCA_WG void hmm_fb_wg(const float *logb, int k, int t0, int t1, const float *transmat, const float *startprob, float *mrow, float *cs, float *alphahat,
                      float *vnext, float *gamma, double *loglik, int seq, float *s) {
  const int ld = hmm_lda(k);
  float *s_A = s, *s_ah = s + k * ld, *s_bh = s_ah + HMM_THREADS, *s_tmp = s_bh + HMM_THREADS, *s_w = s_tmp + HMM_THREADS, *s_part = s_w + HMM_THREADS;
  double *s_ll = (double *)(s + ((k * ld + 4 * HMM_THREADS + HMM_GROUP + 1) & ~1));
  PCA_PAR(tid, HMM_THREADS) {
    for (int e = tid; e < k * k; e += HMM_THREADS) s_A[(e / k) * ld + e % k] = transmat[e];
    for (int t = t0 + tid; t < t1; t += HMM_THREADS) {
      float m = -kmeans_inf();
      for (int j = 0; j < k; j++) m = fmaxf(m, logb[(int64_t)t * k + j]);
      mrow[t] = m;
    }
    if (tid == 0) s_ll[0] = 0.0;
  }
  PCA_SYNC();
  for (int t = t0; t < t1; t++) {
    PCA_PAR(tid, HMM_THREADS) {
      if (tid < k) {
        const float bt = hmm_btilde(logb[(int64_t)t * k + tid], mrow[t]);
        float a;
        if (t == t0) a = startprob[tid] * bt;
        else {
          float sum = 0.f;
          for (int i = 0; i < k; i++) sum = fmaf(s_ah[i], s_A[i * ld + tid], sum);
          a = bt * sum;
        }
        s_tmp[tid] = a;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, HMM_THREADS) {
      if (tid < hmm_groups(k)) hmm_group_sum(s_tmp, s_part, k, tid);
    }
    PCA_SYNC();
    PCA_PAR(tid, HMM_THREADS) {
      const float c = hmm_sum_groups(s_part, k);
      if (tid < k) {
        const float ah = c > 0.f ? s_tmp[tid] / c : 0.f;
        s_ah[tid] = ah;
        alphahat[(int64_t)t * k + tid] = ah;
      }
      if (tid == 0) {
        cs[t] = c;
        s_ll[0] += (double)logf(c) + (double)mrow[t];
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, HMM_THREADS) {
    s_bh[tid] = 1.f;
    if (tid == 0) loglik[seq] = s_ll[0];
  }
  PCA_SYNC();
  for (int t = t1 - 1; t >= t0; t--) {
    PCA_PAR(tid, HMM_THREADS) {
      if (tid < k) s_tmp[tid] = alphahat[(int64_t)t * k + tid] * s_bh[tid];
    }
    PCA_SYNC();
    PCA_PAR(tid, HMM_THREADS) {
      if (tid < hmm_groups(k)) hmm_group_sum(s_tmp, s_part, k, tid);
    }
    PCA_SYNC();
    PCA_PAR(tid, HMM_THREADS) {
      const float G = hmm_sum_groups(s_part, k);
      if (tid < k) {
        gamma[(int64_t)t * k + tid] = G > 0.f ? s_tmp[tid] / G : 0.f;
        const float c = cs[t];
        const float w = c > 0.f ? hmm_btilde(logb[(int64_t)t * k + tid], mrow[t]) * s_bh[tid] / c : 0.f;
        s_w[tid] = w;
        if (t > t0) vnext[(int64_t)(t - 1) * k + tid] = w;
        if (t == t1 - 1) vnext[(int64_t)t * k + tid] = 0.f;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, HMM_THREADS) {
      if (tid < k && t > t0) {
        float sum = 0.f;
        for (int j = 0; j < k; j++) sum = fmaf(s_A[tid * ld + j], s_w[j], sum);
        s_bh[tid] = sum;
      }
    }
    PCA_SYNC();
  }
}

// start [k] = the sum of gamma at each sequence's first row, in sequence order; total = the sum of loglik [S] in sequence order.  One workgroup.
PCA_WG void hmm_start_total_wg(const float *gamma, int k, const int32_t *seq_start, int S, const double *loglik, double *start, double *total) {
  PCA_PAR(tid, HMM_THREADS) {
    if (tid < k) {
      double s = 0.0;
      for (int q = 0; q < S; q++) s += (double)gamma[(int64_t)seq_start[q] * k + tid];
      start[tid] = s;
    }
    if (tid == 0) {
      double s = 0.0;
      for (int q = 0; q < S; q++) s += loglik[q];
      *total = s;
    }
  }
}

// ----------------------------------------------------------------------------------------------- outer-product sums
// Part p of `sp`, the output tile (ib, jb) of 64 x 64: out1[i][j] = sum_r a[r][i] (b[r][j] - bmean[j]), and where out2 is given
// out2[i][j] = sum_r a[r][i] (b[r][j] - bmean[j])^2, over the part's rows in row order, float64 from the first product (the centring is float32;
// bmean null: none).  Thread (ty, tx) owns i = 64 ib + 4 ty + u and j = 64 jb + 4 tx + v.  The parts go to out1 / out2 [P][ka][kb]; where outw is
// given the workgroups of jb = 0 also write outw [P][ka] = sum_r a[r][i].  The M-step is a = gamma, b = x; the expected transitions a = alphahat,
// b = vnext.  s_a, s_b: [HMM_OR][64] floats of LDS.
PCA_WG void hmm_outer_wg(const float *a, int64_t lda, int ka, const float *b, int64_t ldb, int kb, const float *bmean, int n, KmeansSplit sp, int p, int ib,
                         int jb, double *out1, double *out2, double *outw, float *s_a, float *s_b) {
  const int64_t row0 = (int64_t)p * sp.per * PCA_ROWS_PER_WG;
  const int64_t left = (int64_t)n - row0, span = (int64_t)sp.per * PCA_ROWS_PER_WG;
  const int rows = (int)(left < span ? left : span);
  PCA_PRIVATE(double, s1, 16);
  PCA_PRIVATE(double, s2, 16);
  PCA_PRIVATE(double, sw, 4);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < 16; e++) { PCA_MINE(s1, tid)[e] = 0.0; PCA_MINE(s2, tid)[e] = 0.0; }
#pragma unroll
    for (int e = 0; e < 4; e++) PCA_MINE(sw, tid)[e] = 0.0;
  }
  for (int r0 = 0; r0 < rows; r0 += HMM_OR) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < HMM_OR * HMM_OT; e += PCA_THREADS) {
        const int r = e / HMM_OT, c = e % HMM_OT, i = ib * HMM_OT + c, j = jb * HMM_OT + c;
        const bool in = r0 + r < rows;
        s_a[e] = in && i < ka ? a[(row0 + r0 + r) * lda + i] : 0.f;
        s_b[e] = in && j < kb ? b[(row0 + r0 + r) * ldb + j] - (bmean ? bmean[j] : 0.f) : 0.f;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
      double *m1 = PCA_MINE(s1, tid), *m2 = PCA_MINE(s2, tid), *mw = PCA_MINE(sw, tid);
#pragma unroll 4
      for (int r = 0; r < HMM_OR; r++) {
        const km_f4 av = *(const km_f4 *)(s_a + r * HMM_OT + 4 * ty), bv = *(const km_f4 *)(s_b + r * HMM_OT + 4 * tx);
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const double g = (double)av[u];
          if (outw) mw[u] += g;
#pragma unroll
          for (int v = 0; v < 4; v++) {
            const double xv = (double)bv[v], t = g * xv;
            m1[u * 4 + v] += t;
            if (out2) m2[u * 4 + v] = fma(t, xv, m2[u * 4 + v]);
          }
        }
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = ib * HMM_OT + 4 * ty + u;
      if (i >= ka) continue;
      if (outw && jb == 0 && tx == 0) outw[(int64_t)p * ka + i] = PCA_MINE(sw, tid)[u];
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int j = jb * HMM_OT + 4 * tx + v;
        if (j >= kb) continue;
        out1[((int64_t)p * ka + i) * kb + j] = PCA_MINE(s1, tid)[u * 4 + v];
        if (out2) out2[((int64_t)p * ka + i) * kb + j] = PCA_MINE(s2, tid)[u * 4 + v];
      }
    }
  }
}

// element e = i k + j of the expected transition counts: the parts' sums added in part order, times A_ij once
TM_DEV void hmm_xi_reduce(const double *part, int P, int k, const float *transmat, double *xi, int e) {
  double s = 0.0;
  for (int p = 0; p < P; p++) s += part[(int64_t)p * k * k + e];
  xi[e] = (double)transmat[e] * s;
}

// element e = j d + c of the M-step: w = sum_t gamma_tj, S1 and S2 the parts' sums in part order; mu = m + S1 / w, var = max(S2 / w - (S1 / w)^2,
// min_var), float64 rounded once.  A state with w < min_weight keeps the bits of its mu and var.
TM_DEV void hmm_mstep_reduce(const double *part1, const double *part2, const double *partw, int P, int k, int d, const float *mean, double min_var,
                             double min_weight, float *means, float *vars, double *weight, int e) {
  const int j = e / d, c = e % d;
  double a = 0.0, b = 0.0, w = 0.0;
  for (int p = 0; p < P; p++) {
    a += part1[((int64_t)p * k + j) * d + c];
    b += part2[((int64_t)p * k + j) * d + c];
    w += partw[(int64_t)p * k + j];
  }
  if (c == 0) weight[j] = w;
  if (!(w >= min_weight) || !(w > 0.0)) return;
  const double m1 = a / w, var = b / w - m1 * m1;
  means[e] = (float)((double)mean[c] + m1);
  vars[e] = (float)(var > min_var ? var : min_var);
}

// ----------------------------------------------------------------------------------------------- transitions
// transmat_ij = (xi_ij + prior + kappa [i == j]) / sum_j (...), startprob_j = (start_j + prior) / sum_j (...): float64 sums in ascending j,
// rounded once; a row whose denominator is 0 keeps its bits.  One workgroup, thread i owns row i of the matrix and entry i of startprob.
PCA_WG void hmm_transitions_wg(const double *xi, const double *start, int k, double prior, double kappa, float *transmat, float *startprob) {
  PCA_PAR(tid, HMM_THREADS) {
    if (tid < k) {
      double den = 0.0, sden = 0.0;
      for (int j = 0; j < k; j++) {
        den += xi[tid * k + j] + prior + (j == tid ? kappa : 0.0);
        sden += start[j] + prior;
      }
      if (den > 0.0)
        for (int j = 0; j < k; j++) transmat[tid * k + j] = (float)((xi[tid * k + j] + prior + (j == tid ? kappa : 0.0)) / den);
      if (sden > 0.0) startprob[tid] = (float)((start[tid] + prior) / sden);
    }
  }
}

// ----------------------------------------------------------------------------------------------- Viterbi
// The best path of the sequence [t0, t1), one workgroup: delta_t0(j) = log pi_j + logb_t0(j), delta_t(j) = logb_t(j) + max_i (delta_(t-1)(i) +
// log A_ij) in float32, a strictly larger candidate wins in ascending i: the lowest i keeps a tie.  log 0 = -inf: such a step is chosen only
// where every candidate is -inf.  With `logspace` transmat and startprob already hold logarithms.  Back-pointers bp [n][k] uint8; thread 0 takes
// the lowest best final state and walks back.  s: A' [k][hmm_lda(k)] logs, delta [2][128] floats of LDS.
PCA_WG void hmm_viterbi_wg(const float *logb, int k, int t0, int t1, const float *transmat, const float *startprob, int logspace, uint8_t *bp,
                           int32_t *labels, double *path_logprob, int seq, float *s) {
  const int ld = hmm_lda(k);
  float *s_A = s, *s_d = s + k * ld;
  PCA_PAR(tid, HMM_THREADS) {
    for (int e = tid; e < k * k; e += HMM_THREADS) s_A[(e / k) * ld + e % k] = logspace ? transmat[e] : logf(transmat[e]);
    if (tid < k) s_d[tid] = (logspace ? startprob[tid] : logf(startprob[tid])) + logb[(int64_t)t0 * k + tid];
  }
  PCA_SYNC();
  for (int t = t0 + 1; t < t1; t++) {
    PCA_PAR(tid, HMM_THREADS) {
      if (tid < k) {
        const float *prev = s_d + ((t - t0 - 1) & 1) * HMM_THREADS;
        float best = prev[0] + s_A[tid];
        int arg = 0;
        for (int i = 1; i < k; i++) {
          const float v = prev[i] + s_A[i * ld + tid];
          if (v > best) { best = v; arg = i; }
        }
        s_d[((t - t0) & 1) * HMM_THREADS + tid] = logb[(int64_t)t * k + tid] + best;
        bp[(int64_t)t * k + tid] = (uint8_t)arg;
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, HMM_THREADS) {
    if (tid == 0) {
      const float *last = s_d + ((t1 - 1 - t0) & 1) * HMM_THREADS;
      int arg = 0;
      for (int j = 1; j < k; j++)
        if (last[j] > last[arg]) arg = j;
      path_logprob[seq] = (double)last[arg];
      for (int t = t1 - 1; t >= t0; t--) {
        labels[t] = arg;
        if (t > t0) arg = bp[(int64_t)t * k + arg];
      }
    }
  }
}
