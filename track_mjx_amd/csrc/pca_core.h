// csrc/pca_core.h — the bodies of the PCA kernels and of the progression panel (DESIGN.md "PCA"; include/tmjx.h: tmjx_pca_*, tmjx_plot_strips).
// Like render_core.h they also compile on the host (tests/hostemu/pca_emu.cpp): the discipline is csrc/wg_core.h, the column sums, the mean and
// the inner step of the Gram tile csrc/moments_core.h.
#pragma once
#include "moments_core.h"

#define PCA_MAX_D 128          // two [128][129] float images (A and V) are 132 KB of the CU's 160 KB of LDS
#define PCA_TILE_LD 128        // row stride of the Gram kernel's stage (every lane of a wave reads the same row: the stride does not matter to the banks)
#define PCA_TROWS 64           // rows of x per workgroup of the transform kernel
#define PCA_MAX_K 8            // curves of a panel
#define PCA_SWEEP_LIMIT 30
#define PCA_TOL 5.9604645e-8f  // 2^-24: sweeps stop at off(A) <= PCA_TOL * ||A||_F

static_assert(PCA_MAX_D == PCA_WIDE_TILE, "the narrow fit's column sums are one tile of moments_colsum_wg");

// what the Jacobi kernel reports (device side of tmjx_pca_info_t)
struct PcaInfo { int sweeps, converged; float off_rel; int pad_; };

// ----------------------------------------------------------------------------------------------- moments
// Pass 1: the column sums of the workgroup's PCA_ROWS_PER_WG rows are one chunk and one tile (cb = 0) of csrc/moments_core.h; partial: [nwg][d].
PCA_WG void pca_colsum_wg(const float *x, int64_t ldx, int n, int d, int wg, double *partial, double *s_sum) { kmeans_colsum_wg(x, ldx, n, d, wg, 0, partial, s_sum); }
TM_DEV float pca_mean_col(const double *partial, int nwg, int d, int n, int c) { return moments_mean_col(partial, nwg, d, n, c); }

// Pass 2: the workgroup's partial of (x - mean)^T (x - mean), plain float32 FMAs.  256 threads as a 16 x 16 grid; thread (ty, tx) owns the NT x NT
// elements (ty + 16 a, tx + 16 b), so the 16 lanes of a row read 16 consecutive floats of the staged row and the four ty of a wave broadcast.
// partial[wg]: [d][d].  s_tile: [PCA_KB][PCA_TILE_LD] floats of LDS.  (i, j) and (j, i) see the same products in the same order: the partial is
// symmetric to the bit.
template <int NT>
PCA_WG void pca_gram_wg(const float *x, int64_t ldx, int n, int d, const float *mean, int wg, float *partial, float *s_tile) {
  const int row0 = wg * PCA_ROWS_PER_WG, rows = n - row0 < PCA_ROWS_PER_WG ? n - row0 : PCA_ROWS_PER_WG, cols = 16 * NT;
  PCA_PRIVATE(float, acc, NT * NT);
  PCA_PAR(tid, PCA_THREADS) {
#pragma unroll
    for (int e = 0; e < NT * NT; e++) PCA_MINE(acc, tid)[e] = 0.f;
  }
  for (int kb = 0; kb < rows; kb += PCA_KB) {
    PCA_PAR(tid, PCA_THREADS) {
      for (int e = tid; e < PCA_KB * cols; e += PCA_THREADS) {
        const int r = e / cols, c = e % cols;
        s_tile[r * PCA_TILE_LD + c] = (kb + r < rows && c < d) ? x[(int64_t)(row0 + kb + r) * ldx + c] - mean[c] : 0.f;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, PCA_THREADS) { moments_fma_rows<NT, NT>(s_tile, PCA_TILE_LD, s_tile, PCA_TILE_LD, tid >> 4, tid & 15, PCA_MINE(acc, tid)); }
    PCA_SYNC();
  }
  PCA_PAR(tid, PCA_THREADS) {
    const int ty = tid >> 4, tx = tid & 15;
    float *out = partial + (int64_t)wg * d * d;
#pragma unroll
    for (int u = 0; u < NT; u++)
#pragma unroll
      for (int v = 0; v < NT; v++) {
        const int i = ty + 16 * u, j = tx + 16 * v;
        if (i < d && j < d) out[i * d + j] = PCA_MINE(acc, tid)[u * NT + v];
      }
  }
}

// element e of the covariance: the partials added in workgroup order, in float64, over n - 1
TM_DEV float pca_gram_reduce(const float *partial, int nwg, int d, int n, int e) { return (float)(wg_sum(partial + e, nwg, (int64_t)d * d) / (double)(n - 1)); }

// ----------------------------------------------------------------------------------------------- Jacobi
// pair k of step r of the round-robin tournament on m (even) players: player m - 1 stays, the others turn; p < q
TM_DEV void pca_pair(int m, int r, int k, int &p, int &q) {
  int a, b;
  if (k == 0) { a = m - 1; b = r; }
  else { a = (r + k) % (m - 1); b = (r - k + (m - 1)) % (m - 1); }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// LDS floats of pca_jacobi_wg for a d x d problem
PCA_HD int pca_jacobi_lds_floats(int d) {
  const int m = (d + 1) & ~1, ld = m + 1;
  return 2 * m * ld + 4 * (PCA_MAX_D / 2) + 2 * PCA_MAX_D + 4 + PCA_MAX_D + PCA_MAX_D;
}

// One workgroup of nt threads: the eigen-decomposition of the symmetric cov [d][d] by parallel-ordered cyclic Jacobi.  A and V^T (rows: the
// eigenvectors) are float32 images in LDS with the odd row stride m + 1, so that the column walk of A J touches m different banks.  An odd d is
// padded with a zero row and column, which no rotation ever touches (its off-diagonal stays exactly 0).
PCA_WG void pca_jacobi_wg(const float *cov, int d, float *components, float *variance, PcaInfo *info, float *lds, int nt) {
  const int m = (d + 1) & ~1, ld = m + 1, half = m / 2;
  float *A = lds, *Vt = A + m * ld, *rot = Vt + m * ld;      // rot[k]: c, s, a_pp', a_qq' of pair k
  double *rs = (double *)(rot + 4 * (PCA_MAX_D / 2));        // (2 m ld is even: 8-byte aligned) per-row sums
  double *sc = rs + PCA_MAX_D;                               // sc[0] = ||A||_F^2, sc[1] = off(A)^2
  int *rank = (int *)(sc + 2);
  float *lam = (float *)(rank + PCA_MAX_D);
  PCA_PAR(tid, nt) {
    for (int e = tid; e < m * m; e += nt) {
      const int i = e / m, j = e % m;
      A[i * ld + j] = (i < d && j < d) ? cov[i * d + j] : 0.f;
      Vt[i * ld + j] = i == j ? 1.f : 0.f;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, nt) {
    for (int i = tid; i < m; i += nt) {
      double s = 0.0;
      for (int j = 0; j < m; j++) s += (double)A[i * ld + j] * (double)A[i * ld + j];
      rs[i] = s;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, nt) {
    if (tid == 0) {
      double s = 0.0;
      for (int i = 0; i < m; i++) s += rs[i];
      sc[0] = s;
    }
  }
  PCA_SYNC();
  int sweeps = 0, converged = 0;
  double off2 = 0.0;
  const double norm2 = sc[0];
  const float thresh = PCA_TOL * (float)sqrt(norm2) / (float)m;      // every |a_pq| <= thresh means off(A) <= PCA_TOL ||A||_F
  for (;;) {
    PCA_PAR(tid, nt) {
      for (int i = tid; i < m; i += nt) {
        double s = 0.0;
        for (int j = 0; j < m; j++) s += j == i ? 0.0 : (double)A[i * ld + j] * (double)A[i * ld + j];
        rs[i] = s;
      }
    }
    PCA_SYNC();
    PCA_PAR(tid, nt) {
      if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < m; i++) s += rs[i];
        sc[1] = s;
      }
    }
    PCA_SYNC();
    off2 = sc[1];
    if (off2 <= (double)PCA_TOL * (double)PCA_TOL * norm2) { converged = 1; break; }      // (a NaN compares false: never "converged")
    if (sweeps == PCA_SWEEP_LIMIT) break;
    for (int r = 0; r < m - 1; r++) {
      PCA_PAR(tid, nt) {
        for (int k = tid; k < half; k += nt) {
          int p, q;
          pca_pair(m, r, k, p, q);
          const float app = A[p * ld + p], aqq = A[q * ld + q], apq = A[p * ld + q];
          float c = 1.f, s = 0.f, t = 0.f;
          if (fabsf(apq) > thresh) {
            const float tau = (aqq - app) / (2.f * apq);
            t = (tau >= 0.f ? 1.f : -1.f) / (fabsf(tau) + sqrtf(1.f + tau * tau));
            c = 1.f / sqrtf(1.f + t * t);
            s = t * c;
          }
          rot[4 * k + 0] = c; rot[4 * k + 1] = s; rot[4 * k + 2] = app - t * apq; rot[4 * k + 3] = aqq + t * apq;
        }
      }
      PCA_SYNC();
      PCA_PAR(tid, nt) {      // J^T A and J^T V^T: rows p and q
        for (int e = tid; e < half * m; e += nt) {
          const int k = e / m, j = e % m;
          const float c = rot[4 * k + 0], s = rot[4 * k + 1];
          if (s != 0.f) {
            int p, q;
            pca_pair(m, r, k, p, q);
            const float ap = A[p * ld + j], aq = A[q * ld + j], vp = Vt[p * ld + j], vq = Vt[q * ld + j];
            A[p * ld + j] = c * ap - s * aq; A[q * ld + j] = s * ap + c * aq;
            Vt[p * ld + j] = c * vp - s * vq; Vt[q * ld + j] = s * vp + c * vq;
          }
        }
      }
      PCA_SYNC();
      PCA_PAR(tid, nt) {      // (J^T A) J: columns p and q
        for (int e = tid; e < half * m; e += nt) {
          const int k = e / m, i = e % m;
          const float c = rot[4 * k + 0], s = rot[4 * k + 1];
          if (s != 0.f) {
            int p, q;
            pca_pair(m, r, k, p, q);
            const float ap = A[i * ld + p], aq = A[i * ld + q];
            A[i * ld + p] = c * ap - s * aq; A[i * ld + q] = s * ap + c * aq;
          }
        }
      }
      PCA_SYNC();
      PCA_PAR(tid, nt) {      // the rotated 2 x 2 block in closed form: the annihilated element is exactly 0
        for (int k = tid; k < half; k += nt) {
          if (rot[4 * k + 1] != 0.f) {
            int p, q;
            pca_pair(m, r, k, p, q);
            A[p * ld + p] = rot[4 * k + 2]; A[q * ld + q] = rot[4 * k + 3];
            A[p * ld + q] = 0.f; A[q * ld + p] = 0.f;
          }
        }
      }
      PCA_SYNC();
    }
    sweeps++;
  }
  // eigenvalues clamped at 0, ranked by descending value (the lower index first among equals)
  PCA_PAR(tid, nt) {
    for (int i = tid; i < d; i += nt) { const float v = A[i * ld + i]; lam[i] = v > 0.f ? v : 0.f; }      // (NaN -> 0 here; the fit is refused as not converged)
  }
  PCA_SYNC();
  PCA_PAR(tid, nt) {
    for (int i = tid; i < d; i += nt) {
      int rk = 0;
      for (int j = 0; j < d; j++) rk += (lam[j] > lam[i]) || (lam[j] == lam[i] && j < i);
      rank[i] = rk;
    }
  }
  PCA_SYNC();
  PCA_PAR(tid, nt) {
    for (int i = tid; i < d; i += nt) {
      // unit norm, and the largest-magnitude coefficient positive (the lowest index among equals)
      double n2 = 0.0;
      float big = 0.f, sgn = 1.f;
      for (int j = 0; j < d; j++) {
        const float v = Vt[i * ld + j];
        n2 += (double)v * (double)v;
        if (fabsf(v) > big) { big = fabsf(v); sgn = v < 0.f ? -1.f : 1.f; }
      }
      const float scale = n2 > 0.0 ? sgn / (float)sqrt(n2) : sgn;
      for (int j = 0; j < d; j++) components[rank[i] * d + j] = Vt[i * ld + j] * scale;
      variance[rank[i]] = lam[i];
    }
  }
  PCA_PAR(tid, nt) {
    if (tid == 0) {
      info->sweeps = sweeps; info->converged = converged; info->pad_ = 0;
      info->off_rel = norm2 > 0.0 ? (float)sqrt(off2 / norm2) : 0.f;
    }
  }
}

// ----------------------------------------------------------------------------------------------- transform
// one output: (x_row - mean) . component, x_row and mean already centred into `xc` [d]
TM_DEV float pca_project(const float *xc, const float *comp, int d) {
  float s = 0.f;
  for (int j = 0; j < d; j++) s = fmaf(xc[j], comp[j], s);
  return s;
}

// ----------------------------------------------------------------------------------------------- the progression panel
// the panel of one call (DESIGN.md "PCA", panel geometry): the plot rectangle is the pixel columns [x0, x1) and rows [y0, y1)
struct PcaStrip {
  int W, H, T, k, window;
  int64_t ldp;
  float ymin, ymax;
  int x0, x1, y0, y1;
  float hw, radius;
  uint32_t colour[PCA_MAX_K], background, axes, terminated;      // r | g << 8 | b << 16 | 255 << 24
};

TM_DEV bool pca_finite(float v) { return fabsf(v) <= 3.4028234e38f; }      // false for NaN and +-inf

// squared distance of (px, py) to the segment a-b (a != b)
TM_DEV float pca_seg_d2(float px, float py, float ax, float ay, float bx, float by) {
  const float ex = bx - ax, ey = by - ay, wx = px - ax, wy = py - ay;
  const float l2 = ex * ex + ey * ey, u = wx * ex + wy * ey;
  if (u <= 0.f) return wx * wx + wy * wy;
  if (u >= l2) { const float vx = px - bx, vy = py - by; return vx * vx + vy * vy; }
  const float cr = wx * ey - wy * ex;
  return cr * cr / l2;
}

// the colour of pixel (px, py) of the frame that shows timesteps [0, i)
TM_DEV uint32_t pca_strip_pixel(const PcaStrip &s, const float *proj, int i, int flag, int px, int py) {
  if (px < s.x0 || px >= s.x1 || py < s.y0 || py >= s.y1) return s.background;
  const uint32_t under = (px == s.x0 || px == s.x1 - 1 || py == s.y0 || py == s.y1 - 1) ? s.axes : s.background;      // the 1-px frame lies under the curves
  i = i < 0 ? 0 : (i > s.T ? s.T : i);
  const float cx = (float)px + 0.5f, cy = (float)py + 0.5f;
  const float xa = i <= s.window ? 0.f : (float)(i - s.window);
  const float sx = (float)(s.x1 - s.x0) / (float)s.window, sy = (float)(s.y1 - s.y0) / (s.ymax - s.ymin);
  const float fx0 = (float)s.x0, fy1 = (float)s.y1;
  if ((flag & 1) && fabsf(cx - (fx0 + ((float)i - xa) * sx)) <= s.hw) return s.terminated;
  if (i < 1) return under;
  const float mx = fx0 + ((float)(i - 1) - xa) * sx, r2 = s.radius * s.radius;
  if (fabsf(cx - mx) <= s.radius)
    for (int c = s.k - 1; c >= 0; c--) {
      const float v = proj[(int64_t)(i - 1) * s.ldp + c];
      if (!pca_finite(v)) continue;
      const float dx = cx - mx, dy = cy - (fy1 - (v - s.ymin) * sy);
      if (dx * dx + dy * dy <= r2) return s.colour[c];
    }
  // segment t joins the points t and t + 1: only those with X(t) - hw <= cx <= X(t + 1) + hw can reach this pixel (one more on each side
  // against rounding; a superset changes nothing)
  const float tc = xa + (cx - fx0) / sx, dt = s.hw / sx;
  int tlo = (int)floorf(tc - dt) - 2, thi = (int)floorf(tc + dt) + 1;
  tlo = tlo < 0 ? 0 : tlo;
  thi = thi > i - 2 ? i - 2 : thi;
  const float h2 = s.hw * s.hw;
  for (int c = s.k - 1; c >= 0; c--)
    for (int t = tlo; t <= thi; t++) {
      const float v0 = proj[(int64_t)t * s.ldp + c], v1 = proj[(int64_t)(t + 1) * s.ldp + c];
      if (!pca_finite(v0) || !pca_finite(v1)) continue;
      const float ax = fx0 + ((float)t - xa) * sx, bx = fx0 + ((float)(t + 1) - xa) * sx;
      if (pca_seg_d2(cx, cy, ax, fy1 - (v0 - s.ymin) * sy, bx, fy1 - (v1 - s.ymin) * sy) <= h2) return s.colour[c];
    }
  return under;
}
