// csrc/compare_host.h — the host side the representation-comparison entry points share with the host emulation (tests/hostemu/compare_emu.cpp):
// the argument checks (an empty string: accepted), the workspace layout and the rule that picks the components a side of the CCA keeps.
#pragma once
#include "compare_core.h"
#include "readout_host.h"

namespace tmjx_host {

static inline std::string compare_misaligned() { return "the workspace must be a 16-byte aligned device buffer of tmjx_compare_workspace's size"; }
static inline std::string compare_check_d(const char *name, int d) {
  if (d < 1) return std::string(name) + " must be >= 1 (got " + std::to_string(d) + ")";
  if (d > COMPARE_MAX_D) return std::string(name) + " = " + std::to_string(d) + " exceeds the comparison limit of " + std::to_string(COMPARE_MAX_D) + " features";
  return "";
}
static inline std::string compare_check_shape(int n, int d1, int d2) {
  if (n < 3) return "a comparison needs n >= 3 rows (got " + std::to_string(n) + ")";
  std::string e = compare_check_d("d1", d1);
  if (e.empty()) e = compare_check_d("d2", d2);
  return e;
}
static inline std::string compare_check_rows(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy) {
  std::string e = compare_check_shape(n, d1, d2);
  if (e.empty()) e = readout_check_ld("ldx", ldx, "d1", d1);
  if (e.empty()) e = readout_check_ld("ldy", ldy, "d2", d2);
  if (!e.empty()) return e;
  if (!x || !y) return "null argument";
  if (((uintptr_t)x | (uintptr_t)y) & 3) return "x and y must be 4-byte aligned";
  return "";
}
static inline std::string compare_check_metric(const char *name, int metric, const char *dname, int d) {
  if (metric < 0 || metric > 3) return std::string(name) + " = " + std::to_string(metric) + " is no metric (0 squared Euclidean, 1 Euclidean, 2 correlation, 3 labels)";
  if (metric == COMPARE_LABEL && d != 1) return std::string(name) + " = 3 (labels) takes one column (" + dname + " = " + std::to_string(d) + ")";
  if (metric == COMPARE_CORRELATION && d < 2) return std::string(name) + " = 2 (correlation) needs " + dname + " >= 2 (got " + std::to_string(d) + ")";
  return "";
}

// one workspace for every call, in floats (every part starts at a multiple of 4 floats):
//   [16][d1], [16][d2] float64 column sums | mean_x [d1] | mean_y [d2] | [16][dmax][dmax] float64 partial moments | [dmax] float64 row sums |
//   per side shift, scale, ok [rows] of the all-pairs pass (rows = min(n, 32768)) | its [tiles of 128][tiles of 64][5] float64 tile sums |
//   the PCA's workspace (the larger of tmjx_pca_wide_workspace of d1 and of d2: `pca_floats`) | components and variance of both sides |
//   C [dmax][dmax], E [256 + 128][dmax] (the components up to the end of the window, and the window's Ritz vectors), Wx [128][d1], Wy [128][d2], T [128][dmax], M [128][128], sigma [128], U, V, W [128][128] float64 |
//   the five decompositions' reports
// The moment partials have PCA_WIDE_MAX_SUPER slots of which S are used: the size grows with n only through the all-pairs part.
struct CompareWorkspace {
  PcaWideSplit split;
  int nib, ntj;
  int64_t xsum, ysum, mean_x, mean_y, cross, rowsum, stat_x, stat_y, parts, pca, comp_x, var_x, comp_y, var_y, c, e, wx, wy, t, m, sigma, u, v, w, info, floats;
};
static inline int compare_tiles(int n, int per) { return (n + per - 1) / per; }
static inline CompareWorkspace compare_workspace(int n, int d1, int d2, int64_t pca_floats) {
  CompareWorkspace w;
  auto up4 = [](int64_t v) { return (v + 3) & ~(int64_t)3; };
  const int64_t dmax = d1 > d2 ? d1 : d2, rows = n < COMPARE_MAX_N ? n : COMPARE_MAX_N, R = COMPARE_MAX_RANK;
  w.split = pca_wide_split(n);
  w.nib = compare_tiles((int)rows, COMPARE_ROWS);
  w.ntj = compare_tiles((int)rows, COMPARE_TILE);
  w.xsum = 0;
  w.ysum = w.xsum + up4(2 * (int64_t)PCA_WIDE_MAX_SUPER * d1);
  w.mean_x = w.ysum + up4(2 * (int64_t)PCA_WIDE_MAX_SUPER * d2);
  w.mean_y = w.mean_x + up4(d1);
  w.cross = w.mean_y + up4(d2);
  w.rowsum = w.cross + up4(2 * (int64_t)PCA_WIDE_MAX_SUPER * dmax * dmax);
  w.stat_x = w.rowsum + up4(2 * dmax);
  w.stat_y = w.stat_x + 3 * up4(rows);
  w.parts = w.stat_y + 3 * up4(rows);
  w.pca = w.parts + up4(2 * 5 * (int64_t)w.nib * w.ntj);
  w.comp_x = w.pca + up4(pca_floats);
  w.var_x = w.comp_x + up4((int64_t)d1 * d1);
  w.comp_y = w.var_x + up4(d1);
  w.var_y = w.comp_y + up4((int64_t)d2 * d2);
  w.c = w.var_y + up4(d2);
  w.e = w.c + up4(2 * dmax * dmax);
  w.wx = w.e + up4(2 * 3 * R * dmax);
  w.wy = w.wx + up4(2 * R * d1);
  w.t = w.wy + up4(2 * R * d2);
  w.m = w.t + up4(2 * R * dmax);
  w.sigma = w.m + 2 * R * R;
  w.u = w.sigma + 2 * R;
  w.v = w.u + 2 * R * R;
  w.w = w.v + 2 * R * R;
  w.info = w.w + 2 * R * R;
  w.floats = w.info + 12;
  return w;
}

static inline std::string compare_check_workspace(int n, int d1, int d2, const int64_t *floats) {
  std::string e = compare_check_shape(n, d1, d2);
  if (e.empty() && !floats) e = "null argument";
  return e;
}

static inline std::string compare_check_cka(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, const double *out,
                                            const float *workspace) {
  std::string e = compare_check_rows(x, n, d1, ldx, y, d2, ldy);
  if (!e.empty()) return e;
  if (!out || !workspace) return "null argument";
  if (!pca_al16(workspace)) return compare_misaligned();
  if ((uintptr_t)out & 7) return "out must be 8-byte aligned";
  return "";
}

static inline std::string compare_check_rdm(const float *x, int n, int d1, int64_t ldx, int metric_x, const float *y, int d2, int64_t ldy, int metric_y,
                                            const double *sums, const float *workspace) {
  if (n > COMPARE_MAX_N) return "n = " + std::to_string(n) + " exceeds the all-pairs limit of " + std::to_string(COMPARE_MAX_N) + " rows";
  std::string e = compare_check_rows(x, n, d1, ldx, y, d2, ldy);
  if (e.empty()) e = compare_check_metric("metric_x", metric_x, "d1", d1);
  if (e.empty()) e = compare_check_metric("metric_y", metric_y, "d2", d2);
  if (!e.empty()) return e;
  if (!sums || !workspace) return "null argument";
  if (!pca_al16(workspace)) return compare_misaligned();
  if ((uintptr_t)sums & 7) return "sums must be 8-byte aligned";
  return "";
}

static inline std::string compare_check_cca(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, double var_keep, int max_rank,
                                            const float *rho, const float *a, const float *b, const tmjx_cca_info_t *info, const float *workspace) {
  std::string e = compare_check_rows(x, n, d1, ldx, y, d2, ldy);
  if (!e.empty()) return e;
  if (!(var_keep > 0.0) || !(var_keep <= 1.0)) return "var_keep must be in (0, 1] (got " + std::to_string(var_keep) + ")";
  if (max_rank < 1 || max_rank > COMPARE_MAX_RANK)
    return "max_rank = " + std::to_string(max_rank) + " is outside 1 .. " + std::to_string(COMPARE_MAX_RANK) + " components a side";
  if (!rho || !a || !b || !info || !workspace) return "null argument";
  if (!pca_al16(workspace)) return compare_misaligned();
  if (((uintptr_t)rho | (uintptr_t)a | (uintptr_t)b) & 3) return "rho, a and b must be 4-byte aligned";
  return "";
}

static inline std::string compare_check_svd(const double *a, int rows, int cols, int64_t lda, const double *sigma, const double *u, const double *v,
                                            const int32_t *sweeps, const float *workspace) {
  if (rows < 1 || cols < 1) return "the decomposition needs rows, cols >= 1 (got " + std::to_string(rows) + " x " + std::to_string(cols) + ")";
  if (rows > COMPARE_MAX_RANK || cols > COMPARE_MAX_RANK)
    return std::to_string(rows) + " x " + std::to_string(cols) + " exceeds the decomposition's limit of " + std::to_string(COMPARE_MAX_RANK) + " a side";
  if (lda < cols) return "lda = " + std::to_string((long long)lda) + " is smaller than cols = " + std::to_string(cols);
  if (!a || !sigma || !u || !v || !sweeps || !workspace) return "null argument";
  if (!pca_al16(workspace)) return "the workspace must be a 16-byte aligned device buffer of 2 min(rows, cols)^2 + 4 floats";
  if (((uintptr_t)a | (uintptr_t)sigma | (uintptr_t)u | (uintptr_t)v) & 7) return "a, sigma, u and v must be 8-byte aligned";
  return "";
}

// The components a side keeps: the leading ones whose cumulative variance (float64, in order) first reaches var_keep of the total, at least 1, at
// most max_rank, and never one whose eigenvalue is <= 2^-20 of the largest.  variance [d]: descending, >= 0.  0: the side has no variance.
static inline int compare_keep(const float *variance, int d, double var_keep, int max_rank) {
  if (!(variance[0] > 0.f)) return 0;
  double total = 0.0;
  for (int i = 0; i < d; i++) total += (double)variance[i];
  int k = 0;
  double cum = 0.0;
  while (k < d && k < max_rank) {
    if (k > 0 && (double)variance[k] <= COMPARE_EIG_FLOOR * (double)variance[0]) break;
    cum += (double)variance[k++];
    if (cum >= var_keep * total) break;
  }
  return k;
}
// The window of components around the cut behind the first k of d that the Ritz step sharpens: [lo, hi), at most 128 wide, 64 to each side of the
// cut where there is room; nothing (lo = hi = 0) when every component is kept.
struct CompareWindow { int lo, hi; };
static inline CompareWindow compare_window(int d, int k) {
  CompareWindow w = {0, 0};
  if (k >= d) return w;
  w.lo = k - COMPARE_MAX_RANK / 2 > 0 ? k - COMPARE_MAX_RANK / 2 : 0;
  w.hi = w.lo + COMPARE_MAX_RANK < d ? w.lo + COMPARE_MAX_RANK : d;
  w.lo = w.hi - COMPARE_MAX_RANK > 0 ? w.hi - COMPARE_MAX_RANK : 0;
  return w;
}
static inline std::string compare_flat_message(const char *side) {
  return std::string("tmjx_cca: ") + side + " has no variance: there is nothing to correlate";
}
static inline std::string compare_svd_noconv_message(int sweeps) {
  return "the one-sided Jacobi decomposition still rotated a column pair in sweep " + std::to_string(sweeps) + " (is every value finite?)";
}

}  // namespace tmjx_host
