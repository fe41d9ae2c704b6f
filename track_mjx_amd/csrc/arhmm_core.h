// csrc/arhmm_core.h — the bodies of the autoregressive hidden-Markov-model kernels (DESIGN.md "Autoregressive sequence model"; include/tmjx.h:
// tmjx_arhmm_*): K states, each its own linear law x_t ~ W_j phi_t with diagonal noise, phi_t = [xc_(t-1); ...; xc_(t-L); 1] the centred rows
// before t inside its sequence.  Written with the PCA_WG / PCA_PAR / PCA_SYNC discipline of csrc/wg_core.h, so that they also compile on the host
// (tests/hostemu/arhmm_emu.cpp).  Every product of the emission is a chain of float32 FMAs in a fixed order, every moment sum float64 in a fixed
// order: no floating-point atomics, the same bits on every run.  What does not look at x (forward-backward, transitions, Viterbi) is
// csrc/hmm_core.h, called as it stands.
#pragma once
#include "hmm_core.h"
#include "moments_core.h"

#define ARHMM_MAX_D 32
#define ARHMM_MAX_LAGS 4
#define ARHMM_MAX_LD 128         // lags x d: p = lags d + 1 <= 129 regressor columns, q = p + d <= 161 columns of the moments
#define ARHMM_ROWS 128           // rows of x an emission workgroup owns
#define ARHMM_TILE 64            // states of one tile of its walk
#define ARHMM_TK 32              // regressor columns staged per barrier pair
#define ARHMM_LDX 136            // row stride of the staged rows  s_x[feature][halo + row]
#define ARHMM_LDW 68             // row stride of the staged weights  s_w[column][state]
#define ARHMM_OT 64              // side of an output tile of the moments
#define ARHMM_OR 16              // rows staged per barrier pair there (64 measured slower: 10.5 against 8.3 ms at 210 000 x 10, 3 lags, 128 states)
#define ARHMM_MIN_PART 8         // row parts of the moments: at most max(8, 2^22 / (k q q)) parts, whatever n is

PCA_HD int arhmm_p(int d, int lags) { return lags * d + 1; }
PCA_HD int arhmm_q(int d, int lags) { return lags * d + 1 + d; }
PCA_HD int arhmm_pairs(int q) { const int t = kmeans_tiles(q, ARHMM_OT); return t * (t + 1) / 2; }

// the fixed row split of the moment sums: chunks of 256 rows, `per` consecutive chunks to a part.  It depends on n, k and q only.
PCA_HD KmeansSplit arhmm_split(int n, int k, int q) {
  KmeansSplit s;
  int64_t cap = (int64_t)HMM_PART_DOUBLES / ((int64_t)k * q * q);
  if (cap < ARHMM_MIN_PART) cap = ARHMM_MIN_PART;
  s.nchunks = pca_nwg(n);
  s.per = (int)((s.nchunks + cap - 1) / cap);
  s.P = (s.nchunks + s.per - 1) / s.per;
  return s;
}

// ----------------------------------------------------------------------------------------------- positions
// the position of row t in its sequence: t - seq_start[s] for the last s with seq_start[s] <= t
TM_DEV int arhmm_pos(const int32_t *seq_start, int S, int t) {
  int lo = 0, hi = S;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seq_start[mid] <= t) lo = mid; else hi = mid;
  }
  return t - seq_start[lo];
}

// ----------------------------------------------------------------------------------------------- emission
// logb of the rows [128 wg, 128 wg + 128): the rows and the `lags` rows before them are staged once, centred (xc = x - center, rounded once).  The
// workgroup walks the state tiles in order; thread (ty, tx) owns the rows 8 ty + u and, in a tile, the states 4 tx + v.  Per (row, state), the
// features in ascending order: pred starts at the intercept W[j][c][p - 1], one fmaf per regressor column in ascending column order (column
// l d + c' multiplies xc_(t-1-l)[c']), r = xc - pred, q = fmaf(r, r (1 / var), q); logb = fmaf(-1/2, q, c_j).  With lags = 0 this is the chain of
// hmm_emission_wg.  A row whose position in its sequence is below `warmup` is unscored: logb = 0 for every state (whatever its chain read).
// s_x: [ARHMM_MAX_D][ARHMM_LDX], s_w: [ARHMM_TK][ARHMM_LDW] floats of LDS.
PCA_WG void arhmm_emission_wg(const float *x, int n, int d, int64_t ldx, const int32_t *pos, int lags, int warmup, const float *center, const float *weights,
                              const float *vars, int k, const float *cj, float *logb, int wg, float *s_x, float *s_w) {
  const int64_t r0 = (int64_t)wg * ARHMM_ROWS;
  const int ld = lags * d, p = ld + 1;
  PCA_PRIVATE(float, acc, 32);
  PCA_PRIVATE(float, pred, 32);
  PCA_PAR(tid, PCA_THREADS) {
    for (int e = tid; e < (ARHMM_ROWS + lags) * d; e += PCA_THREADS) {
      const int i = e / d, c = e % d;
      const int64_t g = r0 - lags + i;
      float v = 0.f;
      if (g >= 0 && g < n) v = center ? x[g * ldx + c] - center[c] : x[g * ldx + c];
      s_x[c * ARHMM_LDX + i] = v;
    }
  }
  PCA_SYNC();
  for (int c0 = 0; c0 < k; c0 += ARHMM_TILE) {
    PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
      for (int e = 0; e < 32; e++) PCA_MINE(acc, tid)[e] = 0.f;
    }
    for (int c = 0; c < d; c++) {
      PCA_PAR(tid, PCA_THREADS) {
        const int tx = tid & 15;
#pragma unroll
        for (int v = 0; v < 4; v++) {
          const int j = c0 + 4 * tx + v;
          const float b = j < k ? weights[((int64_t)j * d + c) * p + ld] : 0.f;
#pragma unroll
          for (int u = 0; u < 8; u++) PCA_MINE(pred, tid)[u * 4 + v] = b;
        }
      }
      for (int k0 = 0; k0 < ld; k0 += ARHMM_TK) {
        const int cols = ld - k0 < ARHMM_TK ? ld - k0 : ARHMM_TK;
        PCA_PAR(tid, PCA_THREADS) {
          for (int e = tid; e < ARHMM_TILE * ARHMM_TK; e += PCA_THREADS) {
            const int j = e / ARHMM_TK, f = e % ARHMM_TK;
            s_w[f * ARHMM_LDW + j] = (c0 + j < k && f < cols) ? weights[((int64_t)(c0 + j) * d + c) * p + k0 + f] : 0.f;
          }
        }
        PCA_SYNC();
        PCA_PAR(tid, PCA_THREADS) {
          const int ty = tid >> 4, tx = tid & 15;
          float *mine = PCA_MINE(pred, tid);
          int l = k0 / d, cc = k0 % d;
          for (int f = 0; f < cols; f++) {
            const float *xr = s_x + cc * ARHMM_LDX + 8 * ty + lags - 1 - l;      // row 8 ty + u, lag l + 1
            const km_f4 w = *(const km_f4 *)(s_w + f * ARHMM_LDW + 4 * tx);
#pragma unroll
            for (int u = 0; u < 8; u++) {
              const float xv = xr[u];
#pragma unroll
              for (int v = 0; v < 4; v++) mine[u * 4 + v] = fmaf(w[v], xv, mine[u * 4 + v]);
            }
            if (++cc == d) { cc = 0; l++; }
          }
        }
        PCA_SYNC();
      }
      PCA_PAR(tid, PCA_THREADS) {
        const int ty = tid >> 4, tx = tid & 15;
        const float *xr = s_x + c * ARHMM_LDX + 8 * ty + lags;
#pragma unroll
        for (int v = 0; v < 4; v++) {
          const int j = c0 + 4 * tx + v;
          const float iv = j < k ? 1.f / vars[(int64_t)j * d + c] : 0.f;
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const float r = xr[u] - PCA_MINE(pred, tid)[u * 4 + v];
            PCA_MINE(acc, tid)[u * 4 + v] = fmaf(r, r * iv, PCA_MINE(acc, tid)[u * 4 + v]);
          }
        }
      }
    }
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int j = c0 + 4 * tx + v;
        if (j < k) {
          const float c = cj[j];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int64_t row = r0 + 8 * ty + u;
            if (row < n) logb[row * k + j] = pos[row] >= warmup ? fmaf(-0.5f, PCA_MINE(acc, tid)[u * 4 + v], c) : 0.f;
          }
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- moments
// column a of psi_t = [phi_t; xc_t] as (lag, feature): a < p - 1 is feature a % d at lag a / d + 1, a >= p feature a - p of the row itself (lag 0);
// lag -1: the intercept's 1 (a = p - 1), lag -2: beyond the q columns (0)
TM_DEV void arhmm_psi_column(int d, int p, int a, int *lag, int *feature) {
  *lag = a >= p + d ? -2 : a == p - 1 ? -1 : a < p ? a / d + 1 : 0;
  *feature = a >= p + d || a == p - 1 ? 0 : a < p ? a % d : a - p;
}
TM_DEV float arhmm_psi(const float *x, int64_t ldx, const float *center, int64_t t, int lag, int feature) {
  if (lag < 0) return lag == -1 ? 1.f : 0.f;
  const float v = x[(t - lag) * ldx + feature];
  return center ? v - center[feature] : v;
}

// Part `part` of `sp`, state j, the output tile (ib, jb), ib <= jb, of 64 x 64: out[a][b] = sum_t gamma_tj psi_t[a] psi_t[b] over the part's scored
// rows in row order, float64 from the first product: gamma psi_a in double, then one fma with psi_b.  hmm_outer_wg's tile pattern with the left
// operand formed on the fly: a thread owns a 4 x 4 block (bi, bj) of the tile, a = 64 ib + 4 bi + u and b = 64 jb + 4 bj + v.  Only the blocks that
// hold an entry with a <= b < q are given a thread (a diagonal tile: the pairs bi <= bj in row-major order; another tile: the blocks inside q), so
// the waves beyond them do nothing; only the entries with a <= b are kept, and each is written to [a][b] and to [b][a]: both triangles hold the
// same bits.  out: [P][k][q][q].  An unscored row is staged as gamma = 0 and psi = 0; a stage of 16 rows whose gamma is 0 throughout is not
// multiplied out (posteriors are sparse once a fit has settled).  A staging thread keeps its column tid % 64 of both operands
// for the whole walk.  s_a, s_b: [ARHMM_OR][64], s_g: [ARHMM_OR] floats of LDS.
PCA_WG void arhmm_moments_wg(const float *x, int n, int d, int64_t ldx, const int32_t *pos, int lags, int warmup, const float *center, const float *gamma, int k,
                             KmeansSplit sp, int part, int j, int ib, int jb, double *out, float *s_a, float *s_b, float *s_g) {
  const int p = arhmm_p(d, lags), q = p + d;
  const int64_t row0 = (int64_t)part * sp.per * PCA_ROWS_PER_WG;
  const int64_t left = (int64_t)n - row0, span = (int64_t)sp.per * PCA_ROWS_PER_WG;
  const int rows = (int)(left < span ? left : span);
  const int wa = q - ib * ARHMM_OT < ARHMM_OT ? q - ib * ARHMM_OT : ARHMM_OT, wb = q - jb * ARHMM_OT < ARHMM_OT ? q - jb * ARHMM_OT : ARHMM_OT;
  const int nba = (wa + 3) / 4, nbb = (wb + 3) / 4, blocks = ib == jb ? nba * (nba + 1) / 2 : nba * nbb;
  PCA_PRIVATE(double, s1, 16);
  PCA_PRIVATE(int, col, 4);      // the staged columns' (lag, feature) of the a and the b operand
  PCA_PRIVATE(int, blk, 2);      // the thread's block (bi, bj)
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < 16; e++) PCA_MINE(s1, tid)[e] = 0.0;
    int *c = PCA_MINE(col, tid), *b = PCA_MINE(blk, tid);
    arhmm_psi_column(d, p, ib * ARHMM_OT + (tid & (ARHMM_OT - 1)), &c[0], &c[1]);
    arhmm_psi_column(d, p, jb * ARHMM_OT + (tid & (ARHMM_OT - 1)), &c[2], &c[3]);
    if (ib == jb) {
      int bi = 0, rem = tid;
      while (bi < nba && rem >= nba - bi) { rem -= nba - bi; bi++; }
      b[0] = bi; b[1] = bi + rem;
    } else {
      b[0] = tid / nbb; b[1] = tid % nbb;
    }
  }
  for (int r0 = 0; r0 < rows; r0 += ARHMM_OR) {
    PCA_PAR(tid, PCA_THREADS) {
      const int *c = PCA_MINE(col, tid);
      for (int e = tid; e < ARHMM_OR * ARHMM_OT; e += PCA_THREADS) {
        const int r = e / ARHMM_OT;
        const int64_t t = row0 + r0 + r;
        const bool in = r0 + r < rows && pos[t] >= warmup;
        s_a[e] = in ? arhmm_psi(x, ldx, center, t, c[0], c[1]) : 0.f;
        s_b[e] = in ? arhmm_psi(x, ldx, center, t, c[2], c[3]) : 0.f;
        if ((e & (ARHMM_OT - 1)) == 0) s_g[r] = in ? gamma[t * k + j] : 0.f;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      bool any = false;      // a stage in which the state's gamma is 0 throughout adds +-0 to every sum: skipped, no bit changes (finite data)
      for (int r = 0; r < ARHMM_OR; r++) any = any || s_g[r] != 0.f;
      if (tid < blocks && any) {
        const int bi = PCA_MINE(blk, tid)[0], bj = PCA_MINE(blk, tid)[1];
        double *m1 = PCA_MINE(s1, tid);
#pragma unroll 4
        for (int r = 0; r < ARHMM_OR; r++) {
          const km_f4 av = *(const km_f4 *)(s_a + r * ARHMM_OT + 4 * bi), bv = *(const km_f4 *)(s_b + r * ARHMM_OT + 4 * bj);
          const double g = (double)s_g[r];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const double ga = g * (double)av[u];
#pragma unroll
            for (int v = 0; v < 4; v++) m1[u * 4 + v] = fma(ga, (double)bv[v], m1[u * 4 + v]);
          }
        }
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < blocks) {
      const int bi = PCA_MINE(blk, tid)[0], bj = PCA_MINE(blk, tid)[1];
      double *o = out + ((int64_t)part * k + j) * q * q;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int a = ib * ARHMM_OT + 4 * bi + u;
#pragma unroll
        for (int v = 0; v < 4; v++) {
          const int b = jb * ARHMM_OT + 4 * bj + v;
          if (a < q && b < q && a <= b) {
            o[(int64_t)a * q + b] = PCA_MINE(s1, tid)[u * 4 + v];
            o[(int64_t)b * q + a] = PCA_MINE(s1, tid)[u * 4 + v];
          }
        }
      }
    }
  }
}

// element e of moments [k][q][q]: the parts' sums added in part order; the intercept's diagonal entry is the state's weight sum_t gamma_tj
TM_DEV void arhmm_moments_reduce(const double *part, int P, int k, int p, int q, double *moments, double *weight, int64_t e) {
  const int64_t kqq = (int64_t)k * q * q;
  double s = 0.0;
  for (int i = 0; i < P; i++) s += part[(int64_t)i * kqq + e];
  moments[e] = s;
  if (e % ((int64_t)q * q) == (int64_t)(p - 1) * q + (p - 1)) weight[e / ((int64_t)q * q)] = s;
}

// ----------------------------------------------------------------------------------------------- solve
// State j, one workgroup, float64: G = M[:p,:p] + ridge diag(1, .., 1, 0), C = M[p:, :p]; G = L L^T column by column (column c: every row's
// s = G_ic - sum_(m<c) L_im L_cm as one fma chain in ascending m, the pivot's root, the division), then thread c solves L L^T w = C_c by forward
// and back substitution (fma chains in ascending and descending index order), var_c = max((M_xx[c][c] - w . C_c) / weight, min_var),
// means_c = center_c + C[c][p - 1] / weight; everything rounded once.  status: 0 updated, 1 light (weight < min_weight or <= 0), 2 a pivot <= 0
// (or NaN); with 1 or 2 nothing of the state is written.  The factor lives in the workspace, not in LDS: fac [k][p][p], rhs [k][d][p], dg [k][p].
PCA_WG void arhmm_solve_wg(const double *moments, const double *weight, int d, int lags, const float *center, double ridge, double min_var, double min_weight,
                           float *weights, float *vars, float *means, int32_t *status, double *fac, double *rhs, double *dg, int j) {
  const int p = arhmm_p(d, lags), q = p + d;
  const double *M = moments + (int64_t)j * q * q;
  double *Lf = fac + (int64_t)j * p * p, *y = rhs + (int64_t)j * d * p, *dj = dg + (int64_t)j * p;
  const double w = weight[j];
  int code = (!(w >= min_weight) || !(w > 0.0)) ? 1 : 0;
  for (int jc = 0; jc < p && code == 0; jc++) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int i = jc + tid; i < p; i += PCA_THREADS) {
        double s = M[(int64_t)i * q + jc] + (i == jc && jc < p - 1 ? ridge : 0.0);
        for (int m = 0; m < jc; m++) s = fma(-Lf[i * p + m], Lf[jc * p + m], s);
        if (i == jc) dj[jc] = s; else Lf[i * p + jc] = s;
      }
    }
    PCA_SYNC();
    if (!(dj[jc] > 0.0)) { code = 2; break; }
    PCA_PAR(tid, PCA_THREADS) {
      const double rt = sqrt(dj[jc]);
      for (int i = jc + tid; i < p; i += PCA_THREADS) {
        if (i == jc) Lf[i * p + jc] = rt; else Lf[i * p + jc] /= rt;
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    if (tid == 0) status[j] = code;
    if (code == 0 && tid < d) {
      const int c = tid;
      const double *Cc = M + (int64_t)(p + c) * q;
      double *yc = y + c * p;
      for (int i = 0; i < p; i++) {
        double s = Cc[i];
        for (int m = 0; m < i; m++) s = fma(-Lf[i * p + m], yc[m], s);
        yc[i] = s / Lf[i * p + i];
      }
      for (int i = p - 1; i >= 0; i--) {
        double s = yc[i];
        for (int m = p - 1; m > i; m--) s = fma(-Lf[m * p + i], yc[m], s);
        yc[i] = s / Lf[i * p + i];
      }
      double s = Cc[p + c];
      for (int i = 0; i < p; i++) s = fma(-yc[i], Cc[i], s);
      const double var = s / w;
      for (int i = 0; i < p; i++) weights[((int64_t)j * d + c) * p + i] = (float)yc[i];
      vars[(int64_t)j * d + c] = (float)(var > min_var ? var : min_var);
      if (means) means[(int64_t)j * d + c] = (float)((center ? (double)center[c] : 0.0) + Cc[p - 1] / w);
    }
  }
}
