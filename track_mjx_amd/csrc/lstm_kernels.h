// csrc/lstm_kernels.h — the recurrence of the LSTM decoder (flax nn.LSTMCell as track_mjx/agent/lstm_ppo/intention_network.py stacks it), one layer,
// T steps, forward and backward (include/tmjx.h "LSTM decoder recurrence").  The input projections x W_i^T do not depend on the recurrence: they are
// one GEMM over all T x rows rows each (tmjx_gemm_nt) outside these kernels.  What is left is a chain of T small products h W_h^T, latency-bound.
//
// Layout: the rows are independent sequences, so a workgroup of 256 threads owns LSTM_RB = 8 rows for all T steps (no grid-wide sync); h stays in LDS
// between steps, c in registers.  Thread (rg, j) owns hidden unit j of rows rg, rg + 256 / H, ... : all four gates of its units, so the cell update
// needs no exchange.  Forward: the recurrent product streams W_h from L2 in K chunks of LSTM_KC columns, transposed into LDS ([k][4H]: the four
// gate columns of unit j are consecutive across the wave).  Backward: d h_prev = dgates W_h reads W_h rows straight from global memory (unit j's
// column: consecutive across the wave), dgates of the step through LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

#define LSTM_RB 8
#define LSTM_NT 256

struct LstmFwd {
  const float *xg; int ldx;
  const float *Wh; int ldw;
  const float *bh;
  const float *h0, *c0; int ld0;
  const float *reset; int ldr;
  float *h, *c; int ldo;
  float *gates, *h_prev;
  int T, rows;
};

struct LstmBwd {
  const float *dh; int ldd;
  const float *Wh; int ldw;
  const float *gates;
  const float *c; int ldo;
  const float *c0; int ld0;
  const float *reset; int ldr;
  float *dgates, *dh0, *dc0;
  int T, rows;
};

__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

template <int H>
__global__ __launch_bounds__(LSTM_NT) void k_lstm_fwd(const LstmFwd P) {
  constexpr int G4 = 4 * H, NRG = LSTM_NT / H, RPT = LSTM_RB / NRG, KC = H >= 256 ? 8 : 16;
  static_assert(LSTM_NT % H == 0 && LSTM_RB % NRG == 0 && H % KC == 0, "unsupported H");
  __shared__ float hs[2][LSTM_RB][H];
  __shared__ float ws[KC][G4 + 1];
  const int tid = threadIdx.x, j = tid % H, rg = tid / H;
  const int row0 = blockIdx.x * LSTM_RB;
  for (int e = tid; e < LSTM_RB * H; e += LSTM_NT) {
    const int r = e / H, k = e % H, row = row0 + r;
    hs[0][r][k] = row < P.rows ? P.h0[(size_t)row * P.ld0 + k] : 0.f;
  }
  float c[RPT];
#pragma unroll
  for (int i = 0; i < RPT; i++) {
    const int row = row0 + rg + i * NRG;
    c[i] = row < P.rows ? P.c0[(size_t)row * P.ld0 + j] : 0.f;
  }
  int cur = 0;
  for (int t = 0; t < P.T; t++) {
    float acc[RPT][4];
#pragma unroll
    for (int i = 0; i < RPT; i++)
#pragma unroll
      for (int g = 0; g < 4; g++) acc[i][g] = 0.f;
    for (int k0 = 0; k0 < H; k0 += KC) {
      __syncthreads();            // the previous chunk's readers of ws are done (and, at t = 0, the initial h is in LDS)
      for (int e = tid; e < G4 * (KC / 4); e += LSTM_NT) {
        const int n = e / (KC / 4), q = e % (KC / 4);
        const float4 w = *reinterpret_cast<const float4 *>(P.Wh + (size_t)n * P.ldw + k0 + 4 * q);
        ws[4 * q + 0][n] = w.x; ws[4 * q + 1][n] = w.y; ws[4 * q + 2][n] = w.z; ws[4 * q + 3][n] = w.w;
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < KC; kk++) {
        const float w0 = ws[kk][j], w1 = ws[kk][H + j], w2 = ws[kk][2 * H + j], w3 = ws[kk][3 * H + j];
#pragma unroll
        for (int i = 0; i < RPT; i++) {
          const float hv = hs[cur][rg + i * NRG][k0 + kk];
          acc[i][0] = fmaf(hv, w0, acc[i][0]); acc[i][1] = fmaf(hv, w1, acc[i][1]);
          acc[i][2] = fmaf(hv, w2, acc[i][2]); acc[i][3] = fmaf(hv, w3, acc[i][3]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < RPT; i++) {
      const int r = rg + i * NRG, row = row0 + r;
      float hn = 0.f;
      if (row < P.rows) {
        const bool keep = !(P.reset && P.reset[(size_t)t * P.ldr + row] != 0.f);
        const size_t xo = ((size_t)t * P.rows + row) * P.ldx;
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; g++) pre[g] = P.xg[xo + g * H + j] + P.bh[g * H + j] + (keep ? acc[i][g] : 0.f);
        const float gi = lstm_sigmoid(pre[0]), gf = lstm_sigmoid(pre[1]), gg = tanhf(pre[2]), go = lstm_sigmoid(pre[3]);
        const float cp = keep ? c[i] : 0.f;
        const float cn = gf * cp + gi * gg;
        hn = go * tanhf(cn);
        c[i] = cn;
        const size_t oo = ((size_t)t * P.rows + row) * P.ldo + j;
        P.h[oo] = hn;
        P.c[oo] = cn;
        if (P.h_prev) P.h_prev[oo] = keep ? hs[cur][r][j] : 0.f;
        if (P.gates) {
          float *gp = P.gates + ((size_t)t * P.rows + row) * G4 + j;
          gp[0] = gi; gp[H] = gf; gp[2 * H] = gg; gp[3 * H] = go;
        }
      }
      hs[cur ^ 1][r][j] = hn;     // read by the next step behind its first barrier
    }
    cur ^= 1;
  }
}

template <int H>
__global__ __launch_bounds__(LSTM_NT) void k_lstm_bwd(const LstmBwd P) {
  constexpr int G4 = 4 * H, NRG = LSTM_NT / H, RPT = LSTM_RB / NRG;
  static_assert(LSTM_NT % H == 0 && LSTM_RB % NRG == 0, "unsupported H");
  __shared__ float dgs[LSTM_RB][G4];
  const int tid = threadIdx.x, j = tid % H, rg = tid / H;
  const int row0 = blockIdx.x * LSTM_RB;
  float dhc[RPT], dcc[RPT];        // d loss / d (h, c) of the carry that leaves step t (flows into step t + 1)
  bool rs[RPT];
#pragma unroll
  for (int i = 0; i < RPT; i++) dhc[i] = dcc[i] = 0.f;
  for (int t = P.T - 1; t >= 0; t--) {
    __syncthreads();              // the previous step's readers of dgs are done
#pragma unroll
    for (int i = 0; i < RPT; i++) {
      const int r = rg + i * NRG, row = row0 + r;
      float d[4] = {0.f, 0.f, 0.f, 0.f};
      rs[i] = false;
      if (row < P.rows) {
        rs[i] = P.reset && P.reset[(size_t)t * P.ldr + row] != 0.f;
        const size_t go_ = ((size_t)t * P.rows + row) * G4 + j;
        const float gi = P.gates[go_], gf = P.gates[go_ + H], gg = P.gates[go_ + 2 * H], go = P.gates[go_ + 3 * H];
        const float ct = P.c[((size_t)t * P.rows + row) * P.ldo + j];
        const float cp = rs[i] ? 0.f : (t > 0 ? P.c[((size_t)(t - 1) * P.rows + row) * P.ldo + j] : P.c0[(size_t)row * P.ld0 + j]);
        const float dh = P.dh[((size_t)t * P.rows + row) * P.ldd + j] + dhc[i];
        const float tc = tanhf(ct);
        const float dc = dcc[i] + dh * go * (1.f - tc * tc);
        d[0] = dc * gg * gi * (1.f - gi);
        d[1] = dc * cp * gf * (1.f - gf);
        d[2] = dc * gi * (1.f - gg * gg);
        d[3] = dh * tc * go * (1.f - go);
        dcc[i] = rs[i] ? 0.f : dc * gf;
        float *dp = P.dgates + go_;
        dp[0] = d[0]; dp[H] = d[1]; dp[2 * H] = d[2]; dp[3 * H] = d[3];
      }
#pragma unroll
      for (int g = 0; g < 4; g++) dgs[r][g * H + j] = d[g];
    }
    __syncthreads();
    float acc[RPT];
#pragma unroll
    for (int i = 0; i < RPT; i++) acc[i] = 0.f;
#pragma unroll 8
    for (int n = 0; n < G4; n++) {
      const float w = P.Wh[(size_t)n * P.ldw + j];
#pragma unroll
      for (int i = 0; i < RPT; i++) acc[i] = fmaf(dgs[rg + i * NRG][n], w, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < RPT; i++) dhc[i] = rs[i] ? 0.f : acc[i];
  }
#pragma unroll
  for (int i = 0; i < RPT; i++) {
    const int row = row0 + rg + i * NRG;
    if (row < P.rows) {
      if (P.dh0) P.dh0[(size_t)row * P.ld0 + j] = dhc[i];
      if (P.dc0) P.dc0[(size_t)row * P.ld0 + j] = dcc[i];
    }
  }
}
