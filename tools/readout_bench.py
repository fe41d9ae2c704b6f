#!/usr/bin/env python3
"""Times of the GPU linear readout (track_mjx_amd/analysis/readout.py; tmjx_readout_*): 210 000 rows of 128, 512 and 1024 features -> 74 targets
under L = 8 penalties.

  fit       tmjx_readout_fit between two device events (with the call's waits): the PCA part from the events it records itself (moments, eigen-solver),
            the rest — column means of y, the cross moment, Z — by difference
  weights   tmjx_readout_weights for the 8 penalties, between two device events over LOOPS calls
  score     tmjx_readout_score (the fused product, sse and sst) over the same rows, likewise
  predict   tmjx_readout_predict for one penalty, likewise

usage: python tools/readout_bench.py [--out profiles/readout_bench.txt]
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

N, DS, M, L, REPEATS, LOOPS, LIMIT = 210_000, (128, 512, 1024), 74, 8, 3, 5, 400


def med(v):
    return f"{statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})"


def step():
    import numpy as np
    import torch
    from track_mjx_amd import hip
    from track_mjx_amd.analysis import pca as P
    Lb, b = hip.lib(), P.HipBackend("cuda")
    print(f"# readout: {N} rows -> {M} targets, {L} penalties, median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    for d in DS:
        g = torch.Generator(device="cuda").manual_seed(d)
        z = torch.randn((N, d), generator=g, device="cuda") * (0.7 ** torch.arange(d, device="cuda")).sqrt()
        q, _ = torch.linalg.qr(torch.randn((d, d), generator=g, device="cuda"))
        x = (z @ q.T + 3.0).contiguous()
        w0 = torch.randn((d, M), generator=g, device="cuda") / torch.arange(1, d + 1, device="cuda").sqrt()[:, None]
        sig = (x - x.mean(0)) @ w0
        y = (sig + 0.5 * sig.std(0) * torch.randn((N, M), generator=g, device="cuda") + 10.0).contiguous()
        del z, sig
        floats, info = C.c_int64(0), hip.PcaInfo()
        hip.check(Lb.tmjx_readout_workspace(N, d, M, L, C.byref(floats)), "tmjx_readout_workspace")
        ws = torch.empty(int(floats.value), dtype=torch.float32, device="cuda")
        mean_x, comp, var, mean_y, zz, w = (torch.empty(s, dtype=torch.float32, device="cuda") for s in ((d,), (d, d), (d,), (M,), (d, M), (L, d, M)))
        sse, sst = torch.empty((L, M), dtype=torch.float64, device="cuda"), torch.empty((M,), dtype=torch.float64, device="cuda")
        out = torch.empty((N, M), dtype=torch.float32, device="cuda")

        def fit():
            hip.check(Lb.tmjx_readout_fit(x.data_ptr(), N, d, d, y.data_ptr(), M, M, mean_x.data_ptr(), comp.data_ptr(), var.data_ptr(), mean_y.data_ptr(),
                                          zz.data_ptr(), ws.data_ptr(), C.byref(info), None), "tmjx_readout_fit")

        fit()                                              # warm-up, and the variances the penalties are relative to
        lam = np.ascontiguousarray(2.0 ** np.arange(L) * 1e-2 * float(var.double().sum()) / d, np.float64)
        lam_p = lam.ctypes.data_as(C.POINTER(C.c_double))
        calls = {"weights": lambda: hip.check(Lb.tmjx_readout_weights(comp.data_ptr(), var.data_ptr(), zz.data_ptr(), d, M, lam_p, L, w.data_ptr(), None), "weights"),
                 "score": lambda: hip.check(Lb.tmjx_readout_score(x.data_ptr(), N, d, d, y.data_ptr(), M, M, mean_x.data_ptr(), w.data_ptr(), mean_y.data_ptr(), L,
                                                                  sse.data_ptr(), sst.data_ptr(), ws.data_ptr(), None), "score"),
                 "predict": lambda: hip.check(Lb.tmjx_readout_predict(x.data_ptr(), N, d, d, mean_x.data_ptr(), w.data_ptr(), mean_y.data_ptr(), M, out.data_ptr(), M,
                                                                      None), "predict")}
        for f in calls.values():
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in ("fit", "fit: PCA moments", "fit: PCA eigen-solver", "fit: y means, cross moment, Z", *calls)}
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fit()
            e1.record()
            e1.synchronize()
            total = e0.elapsed_time(e1)
            t["fit"].append(total); t["fit: PCA moments"].append(info.moments_ms); t["fit: PCA eigen-solver"].append(info.jacobi_ms)
            t["fit: y means, cross moment, Z"].append(total - info.moments_ms - info.jacobi_ms)
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LOOPS):
                    f()
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1) / LOOPS)
        r2 = (1.0 - sse / sst).mean(1).cpu().numpy()
        tag = f"{N} x {d:<4d} -> {M}"
        for k, v in t.items():
            print(f"{tag} {k:30s} {med(v)}")
        s = statistics.median(t["score"]) * 1e-3
        print(f"{tag} score: {2.0 * N * d * L * M / s / 1e12:.2f} TFLOP/s of float32 FMAs; {info.sweeps} sweeps; R2 on the training rows by penalty " +
              " ".join(f"{v:.4f}" for v in r2), flush=True)
        del x, y, ws, out
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "readout_bench.txt"))
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("readout_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step()
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"readout_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"readout_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/readout_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
