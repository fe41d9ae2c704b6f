#!/usr/bin/env python3
"""Times of the GPU representation comparison (track_mjx_amd/analysis/compare.py; tmjx_cka_linear, tmjx_rdm_corr, tmjx_cca, tmjx_compare_svd).

  cka   tmjx_cka_linear (column means, the three moments with their Frobenius norms) between two device events: 210 000 rows of 128, 512 and
        1024 features against 1024.  Yardstick: tmjx_readout_fit at the same rows and features against 512 targets (its limit): the PCA and ONE
        cross moment of the same split
  rdm   tmjx_rdm_corr at n = 5 000 / 20 000 / 32 768 with d = 60 / 512 / 1024 on both sides, correlation distance.  Yardstick: tmjx_knn of the same
        rows against themselves at the same d (k = 96): the same all-pairs access for ONE feature set.  Counted per pair and feature and side:
        one subtraction and one FMA, against the float32 vector peak
  cca   tmjx_cca at 210 000 x 1024 x 512 (var_keep 0.99, 128 components a side at most), split by its own report into PCA / cross / SVD
  svd   tmjx_compare_svd of a random 128 x 128 matrix

usage: python tools/compare_bench.py [--out profiles/compare_bench.txt]
The shapes run in one child process under its own time limit; the timings are recorded, not asserted.
"""
import argparse
import ctypes as C
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

REPEATS, LIMIT = 3, 400
N_BIG, CKA_D1, CKA_D2 = 210_000, (128, 512, 1024), 1024
RDM_NS, RDM_DS, K_KNN = (5_000, 20_000, 32_768), (60, 512, 1024), 96
CCA_D1, CCA_D2 = 1024, 512
PEAK_TF = 157.3      # float32 vector = matrix peak (TFLOP/s) of the MI355X, an FMA counted as two operations
PAIR_OPS = 3         # counted per pair, feature and side (csrc/compare_core.h compare_side_wg): one subtraction and one FMA (two)


def med(v):
    return f"{statistics.median(v):10.3f} ms  ({min(v):.3f} .. {max(v):.3f})"


def timed(f, repeats=REPEATS):
    import torch
    out = []
    f()
    torch.cuda.synchronize()
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def step():
    import torch
    from track_mjx_amd import hip
    Lb = hip.lib()
    print(f"# representation comparison: median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    dev = dict(device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)

    def rows(n, d, shared=None):
        x = torch.randn((n, d), generator=g, **dev)
        if shared is not None:
            x[:, :shared.shape[1]] += 2.0 * shared
        return (x + 3.0).contiguous()

    def workspace(entry, *dims):
        floats = C.c_int64(0)
        hip.check(getattr(Lb, entry)(*dims, C.byref(floats)), entry)
        return torch.empty(int(floats.value), dtype=torch.float32, **dev), int(floats.value)

    # ------------------------------------------------------------------ CKA next to the readout's fit
    z = torch.randn((N_BIG, 16), generator=g, **dev)
    y = rows(N_BIG, CKA_D2, z)
    for d in CKA_D1:
        x = rows(N_BIG, d, z)
        ws, floats = workspace("tmjx_compare_workspace", N_BIG, d, CKA_D2)
        out = torch.zeros(3, dtype=torch.float64, **dev)
        t = timed(lambda: hip.check(Lb.tmjx_cka_linear(x.data_ptr(), N_BIG, d, d, y.data_ptr(), CKA_D2, CKA_D2, out.data_ptr(), ws.data_ptr(), None), "tmjx_cka_linear"))
        o = out.cpu().numpy()
        del ws
        m = hip.READOUT_MAX_M
        rws, _ = workspace("tmjx_readout_workspace", N_BIG, d, m, 1)
        bufs = [torch.empty(s, dtype=torch.float32, **dev) for s in ((d,), (d, d), (d,), (m,), (d, m))]
        info = hip.PcaInfo()
        tr = timed(lambda: hip.check(Lb.tmjx_readout_fit(x.data_ptr(), N_BIG, d, d, y.data_ptr(), m, CKA_D2, *[b.data_ptr() for b in bufs], rws.data_ptr(),
                                                         C.byref(info), None), "tmjx_readout_fit"), 1)
        fmas = float(N_BIG) * (d * CKA_D2 + d * d + CKA_D2 * CKA_D2)
        s = statistics.median(t) * 1e-3
        tag = f"cka {N_BIG} x {d:<4d} x {CKA_D2}"
        print(f"{tag} tmjx_cka_linear  {med(t)}   cka {o[0] / (o[1] * o[2]) ** 0.5:.4f}")
        print(f"{tag} tmjx_readout_fit (x {m} targets) {med(tr)}   of it moments {info.moments_ms:.3f} ms, Jacobi {info.jacobi_ms:.3f} ms")
        print(f"{tag} three moments: {2 * fmas / s / 1e12:.2f} TFLOP/s of float32 FMAs ({100 * 2 * fmas / s / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF); "
              f"workspace {floats * 4 / 1e6:.1f} MB", flush=True)
        del x, rws, bufs
        torch.cuda.empty_cache()
    del y, z
    torch.cuda.empty_cache()

    # ------------------------------------------------------------------ the all-pairs pass next to the kNN search
    for n in RDM_NS:
        z = torch.randn((n, 16), generator=g, **dev)
        for d in RDM_DS:
            x, y = rows(n, d, z), rows(n, d, z)
            ws, floats = workspace("tmjx_compare_workspace", n, d, d)
            sums = torch.zeros(5, dtype=torch.float64, **dev)
            t = timed(lambda: hip.check(Lb.tmjx_rdm_corr(x.data_ptr(), n, d, d, hip.COMPARE_CORRELATION, y.data_ptr(), d, d, hip.COMPARE_CORRELATION,
                                                         sums.data_ptr(), ws.data_ptr(), None), "tmjx_rdm_corr"))
            kws, _ = workspace("tmjx_tsne_workspace", n, n, d, K_KNN)
            idx, dist2 = torch.empty((n, K_KNN), dtype=torch.int32, **dev), torch.empty((n, K_KNN), dtype=torch.float32, **dev)
            tk = timed(lambda: hip.check(Lb.tmjx_knn(x.data_ptr(), n, d, d, x.data_ptr(), n, d, 1, K_KNN, idx.data_ptr(), dist2.data_ptr(), kws.data_ptr(), None),
                                         "tmjx_knn"))
            pairs = n * (n - 1) / 2.0
            s, k = statistics.median(t) * 1e-3, statistics.median(tk) * 1e-3
            ops = PAIR_OPS * 2 * pairs * d
            tag = f"rdm n {n:>6d} d {d:<4d}"
            print(f"{tag} tmjx_rdm_corr (two sides, the pairs i < j) {med(t)}")
            print(f"{tag} tmjx_knn k {K_KNN} (one side, every ordered pair) {med(tk)}")
            print(f"{tag} rdm / knn {s / k:.3f}; {pairs / s / 1e9:.1f} G pairs/s; {ops / s / 1e12:.2f} T float32 op/s counted ({100 * ops / s / 1e12 / PEAK_TF:.1f} % of "
                  f"{PEAK_TF} TF); workspace {floats * 4 / 1e6:.1f} MB", flush=True)
            del x, y, ws, kws, idx, dist2
            torch.cuda.empty_cache()

    # ------------------------------------------------------------------ CCA and the decomposition alone
    z = torch.randn((N_BIG, 16), generator=g, **dev)
    x, y = rows(N_BIG, CCA_D1, z), rows(N_BIG, CCA_D2, z)
    ws, floats = workspace("tmjx_compare_workspace", N_BIG, CCA_D1, CCA_D2)
    rho, a, b = (torch.empty(s, dtype=torch.float32, **dev) for s in ((128,), (128, CCA_D1), (128, CCA_D2)))
    info = hip.CcaInfo()
    t = timed(lambda: hip.check(Lb.tmjx_cca(x.data_ptr(), N_BIG, CCA_D1, CCA_D1, y.data_ptr(), CCA_D2, CCA_D2, 0.99, 128, rho.data_ptr(), a.data_ptr(), b.data_ptr(),
                                            C.byref(info), ws.data_ptr(), None), "tmjx_cca"), 1)
    print(f"cca {N_BIG} x {CCA_D1} x {CCA_D2} tmjx_cca {med(t)}   kept {info.kx} x {info.ky}; PCA {info.pca_ms:.3f} ms, whitening and cross {info.cross_ms:.3f} ms, "
          f"SVD {info.svd_ms:.3f} ms ({info.sweeps} sweeps); rho[0:3] {rho[:3].cpu().numpy()}; workspace {floats * 4 / 1e6:.1f} MB", flush=True)
    del x, y, ws
    m = torch.randn((128, 128), dtype=torch.float64, generator=g, **dev)
    sg, u, v = (torch.empty(s, dtype=torch.float64, **dev) for s in ((128,), (128, 128), (128, 128)))
    sws, sweeps = torch.empty(2 * 128 * 128 + 4, dtype=torch.float32, **dev), C.c_int32(0)
    t = timed(lambda: hip.check(Lb.tmjx_compare_svd(m.data_ptr(), 128, 128, 128, sg.data_ptr(), u.data_ptr(), v.data_ptr(), C.byref(sweeps), sws.data_ptr(), None),
                                "tmjx_compare_svd"))
    print(f"svd 128 x 128 tmjx_compare_svd {med(t)}   {sweeps.value} sweeps", flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "compare_bench.txt"))
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("compare_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step()
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"compare_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"compare_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/compare_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
