#!/usr/bin/env python3
"""Times of the GPU behaviour map (track_mjx_amd/analysis/embed.py; tmjx_knn, tmjx_tsne_*).

  knn        tmjx_knn (column mean, norms, the fused search) between two device events: 20 000 rows of 60, 375 and 1024 features against
             themselves at k = 96, and 210 000 queries against 20 000 rows.  Yardstick: tmjx_kmeans_assign of the same queries at the same d
             against 256 centroids, scaled by the reference count (n / 256); and the 2 m n d FMA flops against the float32 vector peak
  affinities tmjx_tsne_affinities of those lists at perplexity 30
  gradient   one tmjx_tsne_gradient at n = 5 000 / 20 000 / 65 536 on the P of blob data (k = 90, perplexity 30), with the pair rate
  fit        tmjx_tsne_fit of 750 iterations (250 exaggerated) at the same sizes, with its own gradient / update times
  place      tmjx_tsne_place of 210 000 rows at k = 96

usage: python tools/embed_bench.py [--out profiles/embed_bench.txt]
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

REPEATS, LIMIT = 3, 900
N_KNN, M_BIG, K_KNN, DS = 20_000, 210_000, 96, (60, 375, 1024)
FIT_NS, FIT_ITERS, FIT_EARLY, FIT_K, FIT_D, PERPLEXITY = (5_000, 20_000, 65_536), 750, 250, 90, 60, 30.0
PEAK_TF = 157.3      # float32 vector = matrix peak (TFLOP/s) of the MI355X
# counted per pair of the repulsion kernel (csrc/tsne_core.h tsne_rep_wg): 2 subtractions, 2 FMAs, 1 division, 3 products in float32; 3 conversions
# and 3 additions in float64
PAIR_F32, PAIR_DIV, PAIR_F64 = 7, 1, 3


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


def blobs(n, d, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    ctr = 2.0 * torch.randn((32, d), generator=g, device="cuda")
    return (ctr[torch.randint(0, 32, (n,), generator=g, device="cuda")] + torch.randn((n, d), generator=g, device="cuda") + 3.0).contiguous()


def step():
    import numpy as np
    import torch
    from track_mjx_amd import hip
    from track_mjx_amd.analysis import embed as EM
    from track_mjx_amd.analysis.pca import HipBackend
    Lb = hip.lib()
    print(f"# behaviour map: median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    dev = dict(device="cuda")

    def workspace(n, m, d, k):
        floats = C.c_int64(0)
        hip.check(Lb.tmjx_tsne_workspace(n, m, d, k, C.byref(floats)), "tmjx_tsne_workspace")
        return torch.empty(int(floats.value), dtype=torch.float32, **dev), int(floats.value)

    # ------------------------------------------------------------------ kNN, affinities, placement
    for d, m in [(d, N_KNN) for d in DS] + [(60, M_BIG)]:
        x = blobs(N_KNN, d, 100 + d)
        q = x if m == N_KNN else blobs(m, d, 200 + d)
        ws, floats = workspace(N_KNN, m, d, K_KNN)
        idx, dist2 = torch.empty((m, K_KNN), dtype=torch.int32, **dev), torch.empty((m, K_KNN), dtype=torch.float32, **dev)
        p, beta = torch.empty((m, K_KNN), dtype=torch.float32, **dev), torch.empty(m, dtype=torch.float32, **dev)
        t = timed(lambda: hip.check(Lb.tmjx_knn(x.data_ptr(), N_KNN, d, d, q.data_ptr(), m, d, int(m == N_KNN), K_KNN, idx.data_ptr(), dist2.data_ptr(),
                                                ws.data_ptr(), None), "tmjx_knn"))
        # the yardstick: the k-means assign of the same queries against 256 centroids
        kfl = C.c_int64(0)
        hip.check(Lb.tmjx_kmeans_workspace(m, d, 256, C.byref(kfl)), "tmjx_kmeans_workspace")
        kws = torch.empty(int(kfl.value), dtype=torch.float32, **dev)
        cen, labels = x[:256].contiguous(), torch.empty(m, dtype=torch.int32, **dev)
        inertia = torch.zeros(1, dtype=torch.float64, **dev)
        ta = timed(lambda: hip.check(Lb.tmjx_kmeans_assign(q.data_ptr(), m, d, d, cen.data_ptr(), 256, None, labels.data_ptr(), None, inertia.data_ptr(), None,
                                                           kws.data_ptr(), None), "tmjx_kmeans_assign"))
        tf = timed(lambda: hip.check(Lb.tmjx_tsne_affinities(dist2.data_ptr(), m, K_KNN, PERPLEXITY, p.data_ptr(), beta.data_ptr(), None), "affinities"))
        tag = f"knn {m:>6d} x {N_KNN} x {d:<4d} k {K_KNN}"
        s, a = statistics.median(t) * 1e-3, statistics.median(ta) * 1e-3
        flops = 2.0 * m * N_KNN * d
        print(f"{tag} search     {med(t)}")
        print(f"{tag} assign-256 {med(ta)}")
        print(f"{tag} affinities {med(tf)}")
        print(f"{tag} search / (assign x {N_KNN} / 256) {s / (a * N_KNN / 256):.3f}; {flops / s / 1e12:.2f} TFLOP/s of float32 FMAs "
              f"({100 * flops / s / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF); workspace {floats * 4 / 1e6:.2f} MB", flush=True)
        if m == M_BIG:
            y, out = torch.randn((N_KNN, 2), **dev), torch.empty((m, 2), dtype=torch.float32, **dev)
            tp = timed(lambda: hip.check(Lb.tmjx_tsne_place(idx.data_ptr(), p.data_ptr(), m, K_KNN, y.data_ptr(), N_KNN, out.data_ptr(), None), "place"))
            print(f"place {m} rows at k {K_KNN}  {med(tp)}  ({(m * K_KNN * 8 + m * 8) / (statistics.median(tp) * 1e-3) / 1e12:.3f} TB/s of idx, p and y_out)", flush=True)
        del x, q, ws, idx, dist2, p, kws
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ gradient and fit
    b = HipBackend("cuda")
    for n in FIT_NS:
        x = blobs(n, FIT_D, 300 + n)
        idx, dist2 = b.knn(x, None, FIT_K, exclude_self=True)
        p, _ = b.tsne_affinities(dist2, PERPLEXITY)
        row_ptr, col, val = EM.symmetric_csr(idx, p)
        nnz = int(col.shape[0])
        rp = row_ptr.ctypes.data_as(C.POINTER(C.c_int32))
        cold, vald = torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda()
        ws, floats = workspace(n, 1, 1, 1)
        y0 = (1e-4 * torch.randn((n, 2), generator=torch.Generator(device="cuda").manual_seed(n), **dev)).contiguous()
        y, grad = y0.clone(), torch.empty((n, 2), dtype=torch.float32, **dev)
        vel, gains = torch.zeros((n, 2), **dev), torch.ones((n, 2), **dev)
        z, kl, info = torch.zeros(1, dtype=torch.float64, **dev), torch.zeros(1, dtype=torch.float64, **dev), hip.TsneInfo()
        eta = max(n / 12.0 / 4.0, 50.0)
        tg = timed(lambda: hip.check(Lb.tmjx_tsne_gradient(y.data_ptr(), n, rp, cold.data_ptr(), vald.data_ptr(), nnz, 12.0, grad.data_ptr(), z.data_ptr(),
                                                           kl.data_ptr(), ws.data_ptr(), None), "gradient"))
        tu = timed(lambda: hip.check(Lb.tmjx_tsne_update(y.data_ptr(), grad.data_ptr(), vel.data_ptr(), gains.data_ptr(), n, 0.5, eta, 0.01, ws.data_ptr(), None),
                                     "update"))

        def fit():
            y.copy_(y0); vel.zero_(); gains.fill_(1.0)
            hip.check(Lb.tmjx_tsne_fit(y.data_ptr(), n, rp, cold.data_ptr(), vald.data_ptr(), nnz, FIT_ITERS, 12.0, FIT_EARLY, 0.5, 0.8, eta, 0.01, vel.data_ptr(),
                                       gains.data_ptr(), C.byref(info), ws.data_ptr(), None), "fit")
        tfit, g_in, u_in = [], [], []
        for _ in range(REPEATS if n < 65_536 else 1):
            tfit += timed(fit, 1) if not tfit else []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fit(); e1.record(); e1.synchronize()
            tfit.append(e0.elapsed_time(e1)); g_in.append(info.gradient_ms); u_in.append(info.update_ms)
        tag = f"tsne n {n:>6d} ({nnz} entries of P)"
        g = statistics.median(tg) * 1e-3
        pairs = float(n) * n
        print(f"{tag} gradient      {med(tg)}")
        print(f"{tag} update        {med(tu)}")
        print(f"{tag} fit of {FIT_ITERS}    {med(tfit)}")
        print(f"{tag} fit: gradients {med(g_in)}; updates {med(u_in)}")
        print(f"{tag} gradient: {pairs / g / 1e9:.1f} G pairs/s; per pair {PAIR_F32} float32 operations + {PAIR_DIV} division + {PAIR_F64} float64 adds: "
              f"{PAIR_F32 * pairs / g / 1e12:.2f} T float32 op/s without the division; kl {info.kl:.4f}, Z {info.z:.6g}; workspace {floats * 4 / 1e6:.2f} MB", flush=True)
        del x, ws, cold, vald
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "embed_bench.txt"))
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("embed_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step()
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"embed_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"embed_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/embed_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
