// tests/hostemu/compare_emu.cpp — TEST-ONLY host emulation of the representation-comparison C-ABI (include/tmjx.h: tmjx_compare_workspace,
// tmjx_cka_linear, tmjx_rdm_corr, tmjx_cca, tmjx_compare_svd): the bodies of csrc/compare_core.h and the checks of csrc/compare_host.h compiled
// with g++, one loop iteration where the GPU has one workgroup or thread, in the order of the launches of csrc/tmjx_compare.hip.  A library of its
// own: it includes analysis_emu.cpp for the moments it shares with the readout and for the wide PCA a CCA starts from, and adds the comparison's
// names.  With -DCOMPARE_EMU_MAIN it is a stand-alone program (for sanitizer builds):
//   compare_emu [n d1 d2] — CKA, the RDM correlation under every metric and the CCA of one planted problem (300 x 7 x 5 by default, strided),
//   then the decomposition of four small matrices, and prints a checksum.
#pragma once
#ifdef COMPARE_EMU_MAIN
#undef HMM_EMU_MAIN
#undef KMEANS_EMU_MAIN
#undef PCA_WIDE_EMU_MAIN
#undef PCA_EMU_MAIN
#undef READOUT_EMU_MAIN
#undef SPECTROGRAM_EMU_MAIN
#endif
#include "analysis_emu.cpp"

#include "../../track_mjx_amd/csrc/compare_host.h"

static int cemu_pca_floats(int n, int d1, int d2, int64_t *floats) {
  int64_t p1 = 0, p2 = 0;
  int rc = pwemu_workspace(n, d1, &p1);
  if (!rc) rc = pwemu_workspace(n, d2, &p2);
  *floats = p1 > p2 ? p1 : p2;
  return rc;
}

static void cemu_means(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, float *workspace, const CompareWorkspace &w) {
  double *xsum = (double *)(workspace + w.xsum), *ysum = (double *)(workspace + w.ysum);
  std::vector<double> s_sum(2 * PCA_WIDE_TILE);
  const int S = w.split.S;
  for (int s = 0; s < S; s++)
    for (int cb = 0; cb < pca_wide_tiles(d1); cb++) pca_wide_colsum_wg(x, ldx, n, d1, s, cb, xsum, s_sum.data());
  for (int c = 0; c < d1; c++) (workspace + w.mean_x)[c] = pca_wide_mean_col(xsum, S, d1, n, c);
  for (int s = 0; s < S; s++)
    for (int cb = 0; cb < pca_wide_tiles(d2); cb++) pca_wide_colsum_wg(y, ldy, n, d2, s, cb, ysum, s_sum.data());
  for (int c = 0; c < d2; c++) (workspace + w.mean_y)[c] = pca_wide_mean_col(ysum, S, d2, n, c);
}

static void cemu_cross(const float *x, int64_t ldx, int d, const float *mean_x, const float *y, int64_t ldy, int m, const float *mean_y, int n, float *workspace,
                       const CompareWorkspace &w) {
  std::vector<float> s_x(PCA_KB * PCA_WIDE_TILE), s_y(PCA_KB * READOUT_TILE_M);
  for (int s = 0; s < w.split.S; s++)
    for (int tj = 0; tj < readout_tiles(m, READOUT_TILE_M); tj++)
      for (int ti = 0; ti < pca_wide_tiles(d); ti++)
        readout_cross_wg(x, ldx, y, ldy, n, d, m, mean_x, mean_y, ti, tj, s, (double *)(workspace + w.cross), s_x.data(), s_y.data());
}

static void cemu_svd(const double *a, int ra, int ca, int64_t lda, double *sigma, double *u, double *v, int32_t *info, double *work) {
  std::vector<double> lds(compare_svd_lds_doubles(ra, ca));      // (of exactly the size the launch asks for)
  compare_svd_wg(a, ra, ca, lda, sigma, u, v, info, work, lds.data());
}

template <bool TB>
static void cemu_gemm(const double *a, int64_t lda, const double *b, int64_t ldb, int K, int rows, int cols, double *out) {
  for (int e = 0; e < rows * cols; e++) out[e] = compare_dot<TB>(a, lda, b, ldb, K, e / cols, e % cols);
}

// (launch_whitener of csrc/tmjx_compare.hip)
static void cemu_whitener(const float *x, int64_t ldx, int d, const float *mean, const float *comp, int k, int n, float *workspace, const CompareWorkspace &w,
                          double *W, int32_t *dinfo) {
  double *cross = (double *)(workspace + w.cross), *c = (double *)(workspace + w.c), *e = (double *)(workspace + w.e), *t = (double *)(workspace + w.t),
         *m = (double *)(workspace + w.m), *sigma = (double *)(workspace + w.sigma), *u = (double *)(workspace + w.u), *v = (double *)(workspace + w.v),
         *work = (double *)(workspace + w.w);
  const CompareWindow win = compare_window(d, k);
  const int top = win.hi > k ? win.hi : k, nw = win.hi - win.lo;
  cemu_cross(x, ldx, d, mean, x, ldx, d, mean, n, workspace, w);
  for (int64_t i = 0; i < (int64_t)d * d; i++) c[i] = compare_cross_reduce(cross, w.split.S, d, d, n, i);
  for (int i = 0; i < top * d; i++) e[i] = (double)comp[i];
  if (nw > 0) {
    double *ew = e + (int64_t)win.lo * d, *ritz = e + 2 * (int64_t)COMPARE_MAX_RANK * d;
    cemu_gemm<false>(ew, d, c, d, d, nw, d, t);
    cemu_gemm<true>(t, d, ew, d, d, nw, nw, m);
    cemu_svd(m, nw, nw, nw, sigma, u, v, dinfo + 2, work);
    cemu_gemm<false>(v, nw, ew, d, nw, k - win.lo, d, ritz);
    memcpy(ew, ritz, sizeof(double) * (size_t)(k - win.lo) * d);
  } else {
    dinfo[2] = 0; dinfo[3] = 1;
  }
  cemu_gemm<false>(e, d, c, d, d, k, d, t);
  cemu_gemm<true>(t, d, e, d, d, k, k, m);
  cemu_svd(m, k, k, k, sigma, u, v, dinfo, work);
  for (int i = 0; i < k * k; i++) v[i] = compare_inv_sqrt_row(v, sigma, k, i);
  cemu_gemm<false>(v, k, e, d, k, k, d, W);
}

extern "C" {
int tmjx_compare_workspace(int n, int d1, int d2, int64_t *floats) {
  EMU_TRY(compare_check_workspace(n, d1, d2, floats));
  int64_t pca = 0;
  const int rc = cemu_pca_floats(n, d1, d2, &pca);
  if (rc) return rc;
  *floats = compare_workspace(n, d1, d2, pca).floats;
  return 0;
}

int tmjx_cka_linear(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, double *out, float *workspace, void *) {
  EMU_TRY(compare_check_cka(x, n, d1, ldx, y, d2, ldy, out, workspace));
  const CompareWorkspace w = compare_workspace(n, d1, d2, 0);
  const float *mean_x = workspace + w.mean_x, *mean_y = workspace + w.mean_y;
  double *cross = (double *)(workspace + w.cross), *rowsum = (double *)(workspace + w.rowsum);
  cemu_means(x, n, d1, ldx, y, d2, ldy, workspace, w);
  const struct { const float *a; int64_t lda; int da; const float *ma; const float *b; int64_t ldb; int db; const float *mb; } pass[3] = {
      {x, ldx, d1, mean_x, y, ldy, d2, mean_y}, {x, ldx, d1, mean_x, x, ldx, d1, mean_x}, {y, ldy, d2, mean_y, y, ldy, d2, mean_y}};
  std::vector<double> s_red(PCA_THREADS);
  for (int k = 0; k < 3; k++) {
    cemu_cross(pass[k].a, pass[k].lda, pass[k].da, pass[k].ma, pass[k].b, pass[k].ldb, pass[k].db, pass[k].mb, n, workspace, w);
    for (int row = 0; row < pass[k].da; row++) compare_frob_row_wg(cross, w.split.S, pass[k].da, pass[k].db, n, row, rowsum, s_red.data());
    out[k] = compare_total(rowsum, pass[k].da);
  }
  return 0;
}

int tmjx_rdm_corr(const float *x, int n, int d1, int64_t ldx, int metric_x, const float *y, int d2, int64_t ldy, int metric_y, double *sums, float *workspace,
                  void *) {
  EMU_TRY(compare_check_rdm(x, n, d1, ldx, metric_x, y, d2, ldy, metric_y, sums, workspace));
  const CompareWorkspace w = compare_workspace(n, d1, d2, 0);
  const int64_t up = (n + 3) & ~3;
  float *stat_x = workspace + w.stat_x, *stat_y = workspace + w.stat_y;
  const CompareSide sx = {x, ldx, d1, metric_x, workspace + w.mean_x, stat_x, stat_x + up, (const int32_t *)(stat_x + 2 * up)};
  const CompareSide sy = {y, ldy, d2, metric_y, workspace + w.mean_y, stat_y, stat_y + up, (const int32_t *)(stat_y + 2 * up)};
  double *parts = (double *)(workspace + w.parts);
  cemu_means(x, n, d1, ldx, y, d2, ldy, workspace, w);
  for (int64_t r = 0; r < n; r++) compare_rowstat(x, ldx, sx.mean, d1, metric_x, r, stat_x, stat_x + up, (int32_t *)(stat_x + 2 * up));
  for (int64_t r = 0; r < n; r++) compare_rowstat(y, ldy, sy.mean, d2, metric_y, r, stat_y, stat_y + up, (int32_t *)(stat_y + 2 * up));
  std::vector<double> stage((COMPARE_STAGE + 1) / 2), s_red(5 * PCA_THREADS);      // (doubles: the alignment the kernel's LDS has)
  for (int ib = 0; ib < w.nib; ib++)
    for (int jt = 0; jt < w.ntj; jt++) compare_pairs_wg(sx, sy, n, ib, jt, w.ntj, parts, (float *)stage.data());
  compare_pairs_total_wg(parts, (int64_t)w.nib * w.ntj, sums, s_red.data());
  return 0;
}

int tmjx_compare_svd(const double *a, int rows, int cols, int64_t lda, double *sigma, double *u, double *v, int32_t *sweeps, float *workspace, void *) {
  EMU_TRY(compare_check_svd(a, rows, cols, lda, sigma, u, v, sweeps, workspace));
  const int nn = rows < cols ? rows : cols;
  int32_t *info = (int32_t *)(workspace + 2 * (int64_t)nn * nn);
  cemu_svd(a, rows, cols, lda, sigma, u, v, info, (double *)workspace);
  *sweeps = info[0];
  if (!info[1]) return fail(TMJX_ENOCONV, "tmjx_compare_svd: " + compare_svd_noconv_message(info[0]));
  return 0;
}

int tmjx_cca(const float *x, int n, int d1, int64_t ldx, const float *y, int d2, int64_t ldy, double var_keep, int max_rank, float *rho, float *a, float *b,
             tmjx_cca_info_t *info, float *workspace, void *) {
  EMU_TRY(compare_check_cca(x, n, d1, ldx, y, d2, ldy, var_keep, max_rank, rho, a, b, info, workspace));
  int64_t pca = 0;
  int rc = cemu_pca_floats(n, d1, d2, &pca);
  if (rc) return rc;
  const CompareWorkspace w = compare_workspace(n, d1, d2, pca);
  float *mean_x = workspace + w.mean_x, *mean_y = workspace + w.mean_y, *comp_x = workspace + w.comp_x, *var_x = workspace + w.var_x,
        *comp_y = workspace + w.comp_y, *var_y = workspace + w.var_y;
  double *cross = (double *)(workspace + w.cross), *c = (double *)(workspace + w.c), *wx = (double *)(workspace + w.wx), *wy = (double *)(workspace + w.wy),
         *t = (double *)(workspace + w.t), *m = (double *)(workspace + w.m), *sigma = (double *)(workspace + w.sigma), *u = (double *)(workspace + w.u),
         *v = (double *)(workspace + w.v), *work = (double *)(workspace + w.w);
  int32_t *dinfo = (int32_t *)(workspace + w.info);
  *info = tmjx_cca_info_t{};
  tmjx_pca_info_t px, py;
  if ((rc = pwemu_fit(x, n, d1, ldx, mean_x, comp_x, var_x, workspace + w.pca, &px))) return rc;
  if ((rc = pwemu_fit(y, n, d2, ldy, mean_y, comp_y, var_y, workspace + w.pca, &py))) return rc;
  const int kx = compare_keep(var_x, d1, var_keep, max_rank), ky = compare_keep(var_y, d2, var_keep, max_rank);
  if (kx == 0) return fail(TMJX_EINVAL, compare_flat_message("x"));
  if (ky == 0) return fail(TMJX_EINVAL, compare_flat_message("y"));
  const int r = kx < ky ? kx : ky;
  info->kx = kx; info->ky = ky;
  cemu_whitener(x, ldx, d1, mean_x, comp_x, kx, n, workspace, w, wx, dinfo + 2);
  cemu_whitener(y, ldy, d2, mean_y, comp_y, ky, n, workspace, w, wy, dinfo + 6);
  cemu_cross(x, ldx, d1, mean_x, y, ldy, d2, mean_y, n, workspace, w);
  for (int64_t e = 0; e < (int64_t)d1 * d2; e++) c[e] = compare_cross_reduce(cross, w.split.S, d1, d2, n, e);
  cemu_gemm<false>(wx, d1, c, d2, d1, kx, d2, t);
  cemu_gemm<true>(t, d2, wy, d2, d2, kx, ky, m);
  cemu_svd(m, kx, ky, ky, sigma, u, v, dinfo, work);
  double *dir = cross;
  cemu_gemm<false>(v, ky, wy, d2, ky, r, d2, dir);
  for (int e = 0; e < r * d2; e++) b[e] = (float)dir[e];
  cemu_gemm<false>(u, kx, wx, d1, kx, r, d1, dir);
  for (int e = 0; e < r * d1; e++) a[e] = (float)dir[e];
  for (int e = 0; e < r; e++) rho[e] = (float)sigma[e];
  info->sweeps = dinfo[0];
  info->converged = 1;
  for (int i = 0; i < 5; i++)
    if (!dinfo[2 * i + 1]) {
      info->converged = 0;
      return fail(TMJX_ENOCONV, "tmjx_cca: " + compare_svd_noconv_message(dinfo[2 * i]));
    }
  return 0;
}
}  // extern "C"

#ifdef COMPARE_EMU_MAIN
static float clcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.f - 0.5f; }
#define COMPARE_MAIN_TRY(call) do { if (call) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; } } while (0)

int main(int argc, char **argv) {
  const int n = argc > 3 ? atoi(argv[1]) : 300, d1 = argc > 3 ? atoi(argv[2]) : 7, d2 = argc > 3 ? atoi(argv[3]) : 5;
  const int ldx = d1 + 3, ldy = d2 + 2;
  uint32_t seed = 41;
  // every buffer of exactly the size its contract names, so that a sanitizer sees any overrun
  std::vector<float> x((size_t)(n - 1) * ldx + d1), y((size_t)(n - 1) * ldy + d2), lab(n);
  for (int r = 0; r < n; r++) {
    const float shared = 3.f * clcg(seed);
    for (int c = 0; c < d1; c++) x[(size_t)r * ldx + c] = 100.f + (c == 0 ? shared : 0.f) + clcg(seed);
    for (int c = 0; c < d2; c++) y[(size_t)r * ldy + c] = (c == d2 - 1 ? shared : 0.f) + clcg(seed);
    lab[r] = (float)(r % 4);
  }
  int64_t floats = 0;
  COMPARE_MAIN_TRY(tmjx_compare_workspace(n, d1, d2, &floats));
  std::vector<double> ws((size_t)floats / 2 + (floats & 1));
  float *wsa = (float *)ws.data();
  double out[3], sums[5], sum = 0.0;
  COMPARE_MAIN_TRY(tmjx_cka_linear(x.data(), n, d1, ldx, y.data(), d2, ldy, out, wsa, nullptr));
  const double cka = out[0] / sqrt(out[1] * out[2]);
  sum += cka;
  for (int mx = 0; mx < 3; mx++)
    for (int my = 0; my < 3; my++) {
      if ((mx == 2 && d1 < 2) || (my == 2 && d2 < 2)) continue;
      COMPARE_MAIN_TRY(tmjx_rdm_corr(x.data(), n, d1, ldx, mx, y.data(), d2, ldy, my, sums, wsa, nullptr));
      sum += sums[4] / sqrt(sums[2] * sums[3]);
    }
  COMPARE_MAIN_TRY(tmjx_rdm_corr(lab.data(), n, 1, 1, 3, y.data(), d2, ldy, 0, sums, wsa, nullptr));
  sum += sums[0];
  const int cap = d1 < d2 ? d1 : d2;
  std::vector<float> rho(cap), a((size_t)cap * d1), b((size_t)cap * d2);
  tmjx_cca_info_t info;
  COMPARE_MAIN_TRY(tmjx_cca(x.data(), n, d1, ldx, y.data(), d2, ldy, 1.0, 128, rho.data(), a.data(), b.data(), &info, wsa, nullptr));
  const int r = info.kx < info.ky ? info.kx : info.ky;
  for (int i = 0; i < r; i++) sum += rho[i];
  // the decomposition alone: one value, a row, a tall matrix, the largest
  const int shapes[4][2] = {{1, 1}, {1, 128}, {37, 5}, {128, 128}};
  bool ok = true;
  for (const auto &sh : shapes) {
    const int ra = sh[0], ca = sh[1], nn = ra < ca ? ra : ca;
    std::vector<double> m((size_t)ra * ca), sg(nn), uu((size_t)nn * ra), vv((size_t)nn * ca);
    for (double &e : m) e = clcg(seed);
    std::vector<double> wk((size_t)nn * nn + 2);
    int32_t sweeps = 0;
    COMPARE_MAIN_TRY(tmjx_compare_svd(m.data(), ra, ca, ca, sg.data(), uu.data(), vv.data(), &sweeps, (float *)wk.data(), nullptr));
    double worst = 0.0;      // || m - U^T diag(sigma) V ||_max
    for (int i = 0; i < ra; i++)
      for (int j = 0; j < ca; j++) {
        double s = 0.0;
        for (int k = 0; k < nn; k++) s += uu[(size_t)k * ra + i] * sg[k] * vv[(size_t)k * ca + j];
        worst = fmax(worst, fabs(s - m[(size_t)i * ca + j]));
      }
    ok = ok && worst < 1e-12;
    sum += sg[0];
  }
  printf("compare_emu: %d x %d x %d (ld %d, %d): cka %.6f, CCA kept %d x %d, rho[0] %.6f in %d sweeps, the decompositions rebuild their matrices: %d\n", n, d1,
         d2, ldx, ldy, cka, info.kx, info.ky, rho[0], info.sweeps, (int)ok);
  printf("compare_emu: checksum %.6f\n", sum);
  return ok ? 0 : 1;
}
#endif
