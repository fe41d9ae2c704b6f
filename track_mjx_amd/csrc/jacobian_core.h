// csrc/jacobian_core.h — the bodies of the decoder-Jacobian kernels (DESIGN.md "Decoder Jacobian"; include/tmjx.h: tmjx_decoder_jacobian): the
// shared-weight product every matrix of the computation goes through, the Dense -> SiLU -> LayerNorm block forward that keeps what its backward
// needs, the head (loc, ctrl, the first gradient rows), the LayerNorm / SiLU backward that turns a gradient with respect to a block's output
// into the left operand of the next product, the per-row outputs and the float64 sums over the rows.  Written with the PCA_WG / PCA_PAR /
// PCA_SYNC / PCA_PRIVATE discipline of csrc/wg_core.h, so that they also compile on the host (tests/hostemu/jacobian_emu.cpp).  Every number
// is one chain of float32 operations in a stated order (a product: acc = fmaf(a_k, b_k, acc) from 0 in ascending k); a sum across a row of a
// layer is a fixed tree; the sums across the rows of the call are float64 in row order: no atomics, the same bits on every run, and the bits of
// a row depend neither on how many rows the call has nor on where the row stands in the list.
#pragma once
#include "wg_core.h"

#define JAC_MAX_LAYERS 8
#define JAC_MAX_WIDTH 1024
#define JAC_MAX_A 64
#define JAC_MAX_WRT 128
#define JAC_CHUNK 1024          // rows of the list one pass of the launches covers (the workspace holds one pass)
#define JAC_TM 128              // rows of a reverse product's tile (8 a thread)
#define JAC_TM_FWD 32           // rows of a forward product's tile (2 a thread): a pass has 1024 rows, 8 tiles of 128 would leave the chip idle
#define JAC_TN 128              // columns of a product tile
#define JAC_TK 16               // terms staged per barrier pair
#define JAC_LD 132              // row stride of a staged operand  s[k][row or column]: a thread reads its 8 as two 16-byte words
#define JAC_STAGE (2 * JAC_TK * JAC_LD)      // floats of the stage (16.5 KB)
#define JAC_PER_THREAD (JAC_MAX_WIDTH / PCA_THREADS)      // values of a layer's row a thread keeps
#define JAC_LN_ROWS 4           // gradient rows a workgroup of the LayerNorm backward owns: 64 threads a row
#define JAC_SUM_ROWS 32         // rows of the list one float64 partial sum covers

static_assert(JAC_TM == 8 * 16 && JAC_TM_FWD == 2 * 16 && JAC_TN == 8 * 16 && PCA_THREADS == 256, "a thread of the 16 x 16 grid owns 8 (or 2) x 8 outputs");
static_assert(JAC_CHUNK % JAC_SUM_ROWS == 0, "a partial sum never straddles two passes");
static_assert(JAC_MAX_A + JAC_MAX_WRT <= PCA_THREADS, "one thread per actuator and per input column in the output kernel");

typedef float jac_f4 __attribute__((vector_size(16)));

// the logistic function as the Jacobian has it (csrc/silu_math.h is device-only): differs from the recording kernels' fast form at 1e-6
TM_DEV float jac_sigmoid(float u) { return 1.f / (1.f + expf(-u)); }

// ----------------------------------------------------------------------------------------------- the product
// Tile (tm, tn) of C [M][N] (row stride ldc) = A [M][K] . B: every element is the chain acc = fmaf(A[m][k], B(k, n), acc) from 0 in ascending k.
// Row m of A is a + m lda, or with `gather` a + gather[m] lda (an index outside 0 .. n_src - 1 reads as a row of zeros).  B(k, n) = b[k ldb + n],
// or b[n ldb + k] with TB (a weight matrix [N][K] applied to rows).  A tile is 16 RU rows by 128 columns: thread (ty, tx) of the 16 x 16 grid owns
// the rows RU ty + u and the columns 4 tx + v and 64 + 4 tx + v of it (RU = 8: the reverse products, whose M is rows x A; RU = 2: the forward
// ones, whose M is the rows of a pass, so that they still fill the chip).  What lies outside M, N or K is staged as zeros and never stored.  The
// next JAC_TK terms are read from memory into registers before the staged ones are multiplied, and written to LDS behind them.  s_a, s_b:
// [JAC_TK][JAC_LD] floats of LDS each, 16-byte aligned.
template <bool TB, int RU>
PCA_WG void jac_gemm_wg(const float *a, int64_t lda, const int32_t *gather, int n_src, const float *b, int64_t ldb, float *c, int64_t ldc, int M, int N, int K,
                        int tm, int tn, float *s_a, float *s_b) {
  constexpr int TM = 16 * RU, NA = TM * JAC_TK / PCA_THREADS, NB = JAC_TN * JAC_TK / PCA_THREADS;
  const int m0 = tm * TM, n0 = tn * JAC_TN;
  PCA_PRIVATE(float, acc, RU * 8);
  PCA_PRIVATE(float, pa, NA);
  PCA_PRIVATE(float, pb, NB);
#define JAC_FETCH(k0_)                                                                                                                    \
  {                                                                                                                                       \
    _Pragma("unroll") for (int i = 0; i < NA; i++) {                                                                                      \
      const int e = tid + i * PCA_THREADS, row = e / JAC_TK, f = e % JAC_TK, m = m0 + row;                                                \
      float v = 0.f;                                                                                                                      \
      if (m < M && (k0_) + f < K) {                                                                                                       \
        const int64_t src = gather ? (int64_t)gather[m] : (int64_t)m;                                                                     \
        if (!gather || (src >= 0 && src < n_src)) v = a[src * lda + (k0_) + f];                                                           \
      }                                                                                                                                   \
      PCA_MINE(pa, tid)[i] = v;                                                                                                           \
    }                                                                                                                                     \
    _Pragma("unroll") for (int i = 0; i < NB; i++) {                                                                                      \
      const int e = tid + i * PCA_THREADS, col = TB ? e / JAC_TK : e % JAC_TN, f = TB ? e % JAC_TK : e / JAC_TN;                           \
      float v = 0.f;                                                                                                                      \
      if (n0 + col < N && (k0_) + f < K) v = TB ? b[(int64_t)(n0 + col) * ldb + (k0_) + f] : b[(int64_t)((k0_) + f) * ldb + n0 + col];    \
      PCA_MINE(pb, tid)[i] = v;                                                                                                           \
    }                                                                                                                                     \
  }
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < RU * 8; e++) PCA_MINE(acc, tid)[e] = 0.f;
    JAC_FETCH(0)
  }
  for (int k0 = 0; k0 < K; k0 += JAC_TK) {
    PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
      for (int i = 0; i < NA; i++) {
        const int e = tid + i * PCA_THREADS;
        s_a[(e % JAC_TK) * JAC_LD + e / JAC_TK] = PCA_MINE(pa, tid)[i];
      }
#pragma unroll
      for (int i = 0; i < NB; i++) {
        const int e = tid + i * PCA_THREADS;
        s_b[(TB ? e % JAC_TK : e / JAC_TN) * JAC_LD + (TB ? e / JAC_TK : e % JAC_TN)] = PCA_MINE(pb, tid)[i];
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      const int ty = tid >> 4, tx = tid & 15;
      float *mine = PCA_MINE(acc, tid);
      if (k0 + JAC_TK < K) JAC_FETCH(k0 + JAC_TK)
      if (m0 + RU * ty < M && n0 + 4 * tx < N) {      // (a thread whose outputs all lie outside C has nothing to add)
#pragma unroll 4
        for (int f = 0; f < JAC_TK; f++) {
          float av[RU];
#pragma unroll
          for (int u = 0; u < RU; u++) av[u] = s_a[f * JAC_LD + RU * ty + u];
          const jac_f4 b0 = *(const jac_f4 *)(s_b + f * JAC_LD + 4 * tx), b1 = *(const jac_f4 *)(s_b + f * JAC_LD + 64 + 4 * tx);
#pragma unroll
          for (int u = 0; u < RU; u++)
#pragma unroll
            for (int v = 0; v < 8; v++) mine[u * 8 + v] = fmaf(av[u], v < 4 ? b0[v] : b1[v - 4], mine[u * 8 + v]);
        }
      }
    }
    PCA_SYNC();
  }
#undef JAC_FETCH
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
    for (int u = 0; u < RU; u++)
#pragma unroll
      for (int v = 0; v < 8; v++) {
        const int m = m0 + RU * ty + u, n = n0 + (v < 4 ? 4 * tx + v : 64 + 4 * tx + v - 4);
        if (m < M && n < N) c[(int64_t)m * ldc + n] = PCA_MINE(acc, tid)[u * 8 + v];
      }
  }
}

// ----------------------------------------------------------------------------------------------- a block forward
// Row `row` of a Dense -> SiLU -> LayerNorm block behind the product: z [rows][H] holds W h and leaves as the block's output.  Thread t owns the
// columns t, t + 256, ...:  u = z + bias,  sig = 1 / (1 + expf(-u)),  s = u sig;  mean = (wg_tree over the threads' sums, each in column order) / H;
// var = (the same tree over (s - mean)^2, one fmaf a term) / H;  r = 1 / sqrtf(var + eps);  xhat = (s - mean) r;  h = fmaf(gamma, xhat, beta).
// Kept for the backward: xhat, and rs = r silu'(u) with silu'(u) = sig (1 + u (1 - sig)).  s_red: [PCA_THREADS] floats of LDS.
PCA_WG void jac_block_fwd_wg(float *z, const float *bias, const float *gamma, const float *beta, float eps, int H, int row, float *xhat, float *rs, float *s_red) {
  float *zr = z + (int64_t)row * H, *xr = xhat + (int64_t)row * H, *rr = rs + (int64_t)row * H;
  PCA_PRIVATE(float, sv, JAC_PER_THREAD);
  PCA_PRIVATE(float, dv, JAC_PER_THREAD);
  PCA_PAR(tid, PCA_THREADS) {
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < JAC_PER_THREAD; e++) {
      const int j = tid + e * PCA_THREADS;
      float s = 0.f, d = 0.f;
      if (j < H) {
        const float u = zr[j] + bias[j], sig = jac_sigmoid(u);
        s = u * sig;
        d = sig * (1.f + u * (1.f - sig));
        sum += s;
      }
      PCA_MINE(sv, tid)[e] = s;
      PCA_MINE(dv, tid)[e] = d;
    }
    s_red[tid] = sum;
  }
  PCA_SYNC();
  wg_tree<1>(s_red);
  const float mean = s_red[0] / (float)H;
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < JAC_PER_THREAD; e++)
      if (tid + e * PCA_THREADS < H) {
        const float c = PCA_MINE(sv, tid)[e] - mean;
        sum = fmaf(c, c, sum);
      }
    s_red[tid] = sum;
  }
  PCA_SYNC();
  wg_tree<1>(s_red);
  const float r = 1.f / sqrtf(s_red[0] / (float)H + eps);
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < JAC_PER_THREAD; e++) {
      const int j = tid + e * PCA_THREADS;
      if (j < H) {
        const float xh = (PCA_MINE(sv, tid)[e] - mean) * r;
        xr[j] = xh;
        rr[j] = r * PCA_MINE(dv, tid)[e];
        zr[j] = fmaf(gamma[j], xh, beta[j]);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- the head
// Row `row` of the pass (position `pos` of the list): zloc [rows][A] holds W_h[:A] h;  loc = zloc + b_h,  ctrl = tanhf(loc) (written to ctrl_out
// where there is one), and the first gradient rows  g [(row A + a)][H] = d_a W_h[a][:]  with d_a = fmaf(-ctrl, ctrl, 1) (mode 0: through the tanh)
// or 1 (mode 1).  s_d: [JAC_MAX_A] floats of LDS.
PCA_WG void jac_head_wg(const float *zloc, const float *wh, int64_t ldwh, const float *bh, int A, int H, int mode, int row, int64_t pos, float *ctrl_out, float *g,
                        float *s_d) {
  PCA_PAR(tid, PCA_THREADS) {
    if (tid < A) {
      const float ctrl = tanhf(zloc[(int64_t)row * A + tid] + bh[tid]);
      if (ctrl_out) ctrl_out[pos * A + tid] = ctrl;
      s_d[tid] = mode == 0 ? fmaf(-ctrl, ctrl, 1.f) : 1.f;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    for (int e = tid; e < A * H; e += PCA_THREADS) {
      const int a = e / H, j = e % H;
      g[((int64_t)row * A + a) * H + j] = s_d[a] * wh[(int64_t)a * ldwh + j];
    }
  }
}

// ----------------------------------------------------------------------------------------------- the LayerNorm / SiLU backward
// Gradient rows JAC_LN_ROWS blk .. of g [M][H] (row m belongs to row m / A of the pass), in place: with q_j = g_j gamma_j,
//   mq = (sum_j q_j) / H,  mqx = (sum_j q_j xhat_j) / H  (64 threads a row: thread `lane` adds the columns lane, lane + 64, ... in order, the second
//   sum one fmaf a term; the 64 sums meet in a fixed tree),  du_j = fmaf(-xhat_j, mqx, q_j - mq) rs_j,
// which is r (q - mean(q) - xhat mean(q xhat)) silu'(u): the left operand of the product with the block's weight.  s_red: [2][PCA_THREADS] floats.
PCA_WG void jac_ln_bwd_wg(float *g, int M, int A, int H, const float *gamma, const float *xhat, const float *rs, int blk, float *s_red) {
  PCA_PAR(tid, PCA_THREADS) {
    const int m = blk * JAC_LN_ROWS + tid / 64, lane = tid % 64;
    float sq = 0.f, sqx = 0.f;
    if (m < M) {
      const float *gr = g + (int64_t)m * H, *xr = xhat + (int64_t)(m / A) * H;
      for (int j = lane; j < H; j += 64) {
        const float q = gr[j] * gamma[j];
        sq += q;
        sqx = fmaf(q, xr[j], sqx);
      }
    }
    s_red[tid] = sq;
    s_red[PCA_THREADS + tid] = sqx;
  }
  PCA_SYNC();
  for (int half = 32; half >= 1; half >>= 1) {
    PCA_PAR(tid, PCA_THREADS) {
      if (tid % 64 < half) {
        s_red[tid] += s_red[tid + half];
        s_red[PCA_THREADS + tid] += s_red[PCA_THREADS + tid + half];
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int m = blk * JAC_LN_ROWS + tid / 64, lane = tid % 64;
    if (m < M) {
      const float mq = s_red[tid - lane] / (float)H, mqx = s_red[PCA_THREADS + tid - lane] / (float)H;
      float *gr = g + (int64_t)m * H;
      const float *xr = xhat + (int64_t)(m / A) * H, *rr = rs + (int64_t)(m / A) * H;
      for (int j = lane; j < H; j += 64) {
        const float q = gr[j] * gamma[j];
        gr[j] = fmaf(-xr[j], mqx, q - mq) * rr[j];
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- the outputs of a row
// Row `row` of the pass (position `pos` of the list, row `src` of x; src < 0: no scale for it, zeros): J = j_rows + row A Z, [A][Z].  jac gets J;
// thread a < A:  row2_a = the chain fmaf(J_aj, J_aj, .) over j,  action_var_a = the chain fmaf(t, t, .) with t = J_aj scale_j;  thread 64 + j:
// col2_j = the chain fmaf(J_aj, J_aj, .) over a;  gain = the row2 added in actuator order.  Every output is optional.  s_row: [JAC_MAX_A] floats.
PCA_WG void jac_outputs_wg(const float *j_rows, int A, int Z, int row, int64_t pos, const float *scale_row, float *jac, float *gain, float *col2, float *row2,
                           float *action_var, float *s_row) {
  const float *J = j_rows + (int64_t)row * A * Z;
  PCA_PAR(tid, PCA_THREADS) {
    if (jac)
      for (int e = tid; e < A * Z; e += PCA_THREADS) jac[pos * A * Z + e] = J[e];
    if (tid < A) {
      float r2 = 0.f, av = 0.f;
      for (int j = 0; j < Z; j++) {
        const float v = J[tid * Z + j];
        r2 = fmaf(v, v, r2);
        if (action_var) {
          const float t = v * (scale_row ? scale_row[j] : 0.f);
          av = fmaf(t, t, av);
        }
      }
      s_row[tid] = r2;
      if (row2) row2[pos * A + tid] = r2;
      if (action_var) action_var[pos * A + tid] = av;
    }
    if (col2 && tid >= JAC_MAX_A && tid - JAC_MAX_A < Z) {
      const int j = tid - JAC_MAX_A;
      float c2 = 0.f;
      for (int a = 0; a < A; a++) c2 = fmaf(J[a * Z + j], J[a * Z + j], c2);
      col2[pos * Z + j] = c2;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, PCA_THREADS) {
    if (gain && tid == 0) {
      float s = 0.f;
      for (int a = 0; a < A; a++) s += s_row[a];
      gain[pos] = s;
    }
  }
}

// ----------------------------------------------------------------------------------------------- the sums over the rows
// elements of `sums`: J [A][Z] | J^T J [Z][Z] | J J^T [A][A]
PCA_HD int jac_sum_elements(int A, int Z) { return A * Z + Z * Z + A * A; }

// Elements 256 eb .. of the rows [i0, i1) of the pass: per row the element itself, or the float32 chain over the actuators (J^T J) or over the
// input columns (J J^T), one fmaf a term in ascending order, read from the row's J staged in LDS; the rows added in float64 in row order.
// out: [E] float64 of this group of rows.  s_j: [JAC_MAX_A * JAC_MAX_WRT] floats of LDS.
PCA_WG void jac_sum_rows_wg(const float *j_rows, int A, int Z, int i0, int i1, int eb, int E, double *out, float *s_j) {
  PCA_PRIVATE(double, acc, 1);
  PCA_PAR(tid, PCA_THREADS) { PCA_MINE(acc, tid)[0] = 0.0; }
  for (int i = i0; i < i1; i++) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < A * Z; e += PCA_THREADS) s_j[e] = j_rows[(int64_t)i * A * Z + e];
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) {
      const int e = eb * PCA_THREADS + tid;
      if (e < E) {
        float v = 0.f;
        if (e < A * Z) {
          v = s_j[e];
        } else if (e < A * Z + Z * Z) {
          const int j = (e - A * Z) / Z, k = (e - A * Z) % Z;
          for (int a = 0; a < A; a++) v = fmaf(s_j[a * Z + j], s_j[a * Z + k], v);
        } else {
          const int a = (e - A * Z - Z * Z) / A, b = (e - A * Z - Z * Z) % A;
          for (int j = 0; j < Z; j++) v = fmaf(s_j[a * Z + j], s_j[b * Z + j], v);
        }
        PCA_MINE(acc, tid)[0] += (double)v;
      }
    }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int e = eb * PCA_THREADS + tid;
    if (e < E) out[e] = PCA_MINE(acc, tid)[0];
  }
}

// sums[e] += the partial sums of `chunks` groups of JAC_SUM_ROWS rows, in group order
TM_DEV void jac_sum_add(const double *partial, int chunks, int E, int e, double *sums) {
  double s = sums[e];
  for (int c = 0; c < chunks; c++) s += partial[(int64_t)c * E + e];
  sums[e] = s;
}
