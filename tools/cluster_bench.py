#!/usr/bin/env python3
"""Times of the GPU k-means (track_mjx_amd/analysis/cluster.py; tmjx_kmeans_*): 210 000 rows of 60, 512 and 1024 features into 16, 64 and 256 clusters.

  seed      tmjx_kmeans_seed (k-means++: one pass over x per centre), between two device events, with the call's wait
  assign    tmjx_kmeans_assign (column mean, centroid norms, the fused pass, totals) between two device events over LOOPS calls
  predict   the yardstick: tmjx_readout_predict at the same (n, d, m = k), which forms the same product and writes n k floats more
  update    tmjx_kmeans_update, likewise
  fit       tmjx_kmeans_fit, 20 iterations (tol = 0 from the k-means++ seeds; fewer if it converges), with its own assign / update times

usage: python tools/cluster_bench.py [--out profiles/cluster_bench.txt]
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

N, DS, KS, REPEATS, LOOPS, FIT_ITERS, LIMIT = 210_000, (60, 512, 1024), (16, 64, 256), 3, 3, 20, 500
PEAK_TF, PEAK_HBM = 157.3, 8.0      # float32 vector = matrix peak (TFLOP/s) and HBM3E peak (TB/s) of the MI355X


def med(v):
    return f"{statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})"


def step():
    import numpy as np
    import torch
    from track_mjx_amd import hip
    Lb = hip.lib()
    print(f"# k-means: {N} rows, median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    for d in DS:
        for k in KS:
            g = torch.Generator(device="cuda").manual_seed(1000 * d + k)
            ctr = 2.0 * torch.randn((k, d), generator=g, device="cuda")
            x = (ctr[torch.randint(0, k, (N,), generator=g, device="cuda")] + torch.randn((N, d), generator=g, device="cuda") + 3.0).contiguous()
            floats, info = C.c_int64(0), hip.KMeansInfo()
            hip.check(Lb.tmjx_kmeans_workspace(N, d, k, C.byref(floats)), "tmjx_kmeans_workspace")
            ws = torch.empty(int(floats.value), dtype=torch.float32, device="cuda")
            cen, seeds, zero = (torch.zeros((k, d), dtype=torch.float32, device="cuda") for _ in range(3))
            labels, prev, counts = (torch.zeros(s, dtype=torch.int32, device="cuda") for s in (N, N, k))
            dist2, out = torch.empty(N, dtype=torch.float32, device="cuda"), torch.empty((N, k), dtype=torch.float32, device="cuda")
            inertia, changed = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            wt = torch.randn((d, k), generator=g, device="cuda")      # the yardstick's weights: any [d][k] matrix times alike
            u = np.random.default_rng(7).random(k)
            index = np.zeros(k, np.int32)
            X = (x.data_ptr(), N, d, d)
            calls = {
                "seed": (1, lambda: hip.check(Lb.tmjx_kmeans_seed(*X, k, u.ctypes.data_as(C.POINTER(C.c_double)), seeds.data_ptr(),
                                                                  index.ctypes.data_as(C.POINTER(C.c_int32)), ws.data_ptr(), None), "seed")),
                "assign": (LOOPS, lambda: hip.check(Lb.tmjx_kmeans_assign(*X, seeds.data_ptr(), k, prev.data_ptr(), labels.data_ptr(), dist2.data_ptr(),
                                                                          inertia.data_ptr(), changed.data_ptr(), ws.data_ptr(), None), "assign")),
                "predict": (LOOPS, lambda: hip.check(Lb.tmjx_readout_predict(*X, zero.data_ptr(), wt.data_ptr(), zero.data_ptr(), k,
                                                                            out.data_ptr(), k, None), "predict")),
                "update": (LOOPS, lambda: hip.check(Lb.tmjx_kmeans_update(*X, labels.data_ptr(), k, cen.data_ptr(), counts.data_ptr(), ws.data_ptr(), None),
                                                    "update")),
            }

            def fit():
                cen.copy_(seeds)
                hip.check(Lb.tmjx_kmeans_fit(*X, k, cen.data_ptr(), labels.data_ptr(), dist2.data_ptr(), FIT_ITERS, 0.0, C.byref(info), ws.data_ptr(), None), "fit")

            for _, f in calls.values():      # warm-up (and the seeds the other calls use)
                f()
            fit()
            torch.cuda.synchronize()
            t = {name: [] for name in (*calls, "fit", "fit: assigns", "fit: updates")}
            for _ in range(REPEATS):
                for name, (loops, f) in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(loops):
                        f()
                    e1.record()
                    e1.synchronize()
                    t[name].append(e0.elapsed_time(e1) / loops)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fit()
                e1.record()
                e1.synchronize()
                t["fit"].append(e0.elapsed_time(e1)); t["fit: assigns"].append(info.assign_ms); t["fit: updates"].append(info.update_ms)
            tag = f"{N} x {d:<4d} k {k:<3d}"
            for name, v in t.items():
                print(f"{tag} {name:14s} {med(v)}")
            a, p, up = (statistics.median(t[name]) * 1e-3 for name in ("assign", "predict", "update"))
            print(f"{tag} assign / predict {a / p:.3f}; assign {2.0 * N * d * k / a / 1e12:.2f} TFLOP/s of float32 FMAs ({100 * 2.0 * N * d * k / a / 1e12 / PEAK_TF:.1f} % "
                  f"of {PEAK_TF} TF); update {4.0 * N * d / up / 1e12:.3f} TB/s of x ({100 * 4.0 * N * d / up / 1e12 / PEAK_HBM:.1f} % of {PEAK_HBM} TB/s); fit "
                  f"{info.n_iter} iterations, inertia {info.inertia:.6g}", flush=True)
            del x, ws, out
            torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cluster_bench.txt"))
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("cluster_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step()
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"cluster_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"cluster_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/cluster_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
