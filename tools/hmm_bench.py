#!/usr/bin/env python3
"""Times of the GPU hidden Markov model (track_mjx_amd/analysis/hmm.py; tmjx_hmm_*): 210 000 rows as 840 sequences of 250, 60, 512 and 1024 features,
16, 64 and 128 states, and one line of 8 sequences of 26 250 rows (whole-clip roll-outs: one workgroup per sequence serialises there).

  emission  tmjx_hmm_emission (c_j, then the fused pass) between two device events over LOOPS calls
  assign    the emission's yardstick: tmjx_kmeans_assign at the same (n, d, k): the same data movement, 2/3 of the arithmetic
  fb        tmjx_hmm_forward_backward (the recursion, start and total, the expected transitions), likewise
  mstep     tmjx_hmm_mstep (column mean, the float64 outer-product sums, the reduction), likewise
  update    the M-step's yardstick: tmjx_kmeans_update at the same (n, d, k)
  viterbi   tmjx_hmm_viterbi, likewise
  fit       tmjx_hmm_fit, 10 iterations (tol = 0), with its own emission / fb / mstep / viterbi times

The blocks alternate inside each repeat, so a drift of the clocks falls on all of them alike.
usage: python tools/hmm_bench.py [--out profiles/hmm_bench.txt]
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

N, T, DS, KS, REPEATS, LOOPS, FIT_ITERS, LIMIT = 210_000, 250, (60, 512, 1024), (16, 64, 128), 3, 2, 10, 540
LONG = (8, 26_250, 60, 64)      # sequences, rows of each, d, k
PEAK_TF = 157.3      # float32 vector peak (TFLOP/s) of the MI355X


def med(v):
    return f"{statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})"


def shape(S, T, d, k, fit_too=True):
    import numpy as np
    import torch
    from track_mjx_amd import hip
    Lb = hip.lib()
    n = S * T
    g = torch.Generator(device="cuda").manual_seed(1000 * d + k)
    ctr = 2.0 * torch.randn((k, d), generator=g, device="cuda")
    z = torch.randint(0, k, (n // 25 + 1,), generator=g, device="cuda").repeat_interleave(25)[:n]      # states that dwell 25 rows
    x = (ctr[z] + torch.randn((n, d), generator=g, device="cuda") + 3.0).contiguous()
    seq = (np.arange(S + 1, dtype=np.int32) * T)
    seq_p = seq.ctypes.data_as(C.POINTER(C.c_int32))
    floats, kfloats, info = C.c_int64(0), C.c_int64(0), hip.HmmInfo()
    hip.check(Lb.tmjx_hmm_workspace(n, d, k, S, C.byref(floats)), "tmjx_hmm_workspace")
    hip.check(Lb.tmjx_kmeans_workspace(n, d, k, C.byref(kfloats)), "tmjx_kmeans_workspace")
    ws = torch.empty(int(floats.value), dtype=torch.float32, device="cuda")
    kws = torch.empty(int(kfloats.value), dtype=torch.float32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")      # noqa: E731
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")      # noqa: E731
    mu0 = (ctr + 3.0 + 0.25 * torch.randn((k, d), generator=g, device="cuda")).contiguous()
    var0, A0, pi0 = torch.ones((k, d), device="cuda"), torch.full((k, k), 1.0 / k, device="cuda"), torch.full((k,), 1.0 / k, device="cuda")
    mu, var, A, pi, cen = mu0.clone(), var0.clone(), A0.clone(), pi0.clone(), mu0.clone()
    logb, gamma = f32(n, k), f32(n, k)
    xi, start, ll, total, weight, path = f64(k, k), f64(k), f64(S), f64(1), f64(k), f64(S)
    labels, klabels, counts = (torch.zeros(s, dtype=torch.int32, device="cuda") for s in (n, n, k))
    inertia = torch.zeros(1, dtype=torch.float64, device="cuda")
    X = (x.data_ptr(), n, d, d)
    calls = {
        "emission": lambda: hip.check(Lb.tmjx_hmm_emission(*X, mu0.data_ptr(), var0.data_ptr(), k, logb.data_ptr(), ws.data_ptr(), None), "emission"),
        "assign": lambda: hip.check(Lb.tmjx_kmeans_assign(*X, mu0.data_ptr(), k, None, klabels.data_ptr(), None, inertia.data_ptr(), None, kws.data_ptr(), None),
                                    "assign"),
        "fb": lambda: hip.check(Lb.tmjx_hmm_forward_backward(logb.data_ptr(), n, k, seq_p, S, A0.data_ptr(), pi0.data_ptr(), gamma.data_ptr(), xi.data_ptr(),
                                                             start.data_ptr(), ll.data_ptr(), total.data_ptr(), ws.data_ptr(), None), "fb"),
        "mstep": lambda: hip.check(Lb.tmjx_hmm_mstep(*X, gamma.data_ptr(), k, 1e-3, 1e-3, mu.data_ptr(), var.data_ptr(), weight.data_ptr(), ws.data_ptr(), None),
                                   "mstep"),
        "update": lambda: hip.check(Lb.tmjx_kmeans_update(*X, klabels.data_ptr(), k, cen.data_ptr(), counts.data_ptr(), kws.data_ptr(), None), "update"),
        "viterbi": lambda: hip.check(Lb.tmjx_hmm_viterbi(logb.data_ptr(), n, k, seq_p, S, A0.data_ptr(), pi0.data_ptr(), 0, labels.data_ptr(), path.data_ptr(),
                                                         ws.data_ptr(), None), "viterbi"),
    }

    def fit():
        for dst, src in ((mu, mu0), (var, var0), (A, A0), (pi, pi0)):
            dst.copy_(src)
        hip.check(Lb.tmjx_hmm_fit(*X, seq_p, S, k, mu.data_ptr(), var.data_ptr(), A.data_ptr(), pi.data_ptr(), gamma.data_ptr(), labels.data_ptr(), FIT_ITERS, 0.0,
                                  0.1, 0.0, 1e-3, 1e-3, C.byref(info), ws.data_ptr(), None), "fit")

    for f in calls.values():      # warm-up (and the logb and gamma the later calls read)
        f()
    if fit_too:
        fit()
    torch.cuda.synchronize()
    t = {name: [] for name in (*calls, *(("fit", "fit: emissions", "fit: fb", "fit: msteps", "fit: viterbi") if fit_too else ()))}
    for _ in range(REPEATS):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LOOPS):
                f()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1) / LOOPS)
        if fit_too:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fit()
            e1.record()
            e1.synchronize()
            for name, v in (("fit", e0.elapsed_time(e1)), ("fit: emissions", info.emission_ms), ("fit: fb", info.fb_ms), ("fit: msteps", info.mstep_ms),
                            ("fit: viterbi", info.viterbi_ms)):
                t[name].append(v)
    tag = f"{S} x {T} x {d:<4d} k {k:<3d}"
    for name, v in t.items():
        print(f"{tag} {name:14s} {med(v)}")
    e, a, m, up = (statistics.median(t[name]) * 1e-3 for name in ("emission", "assign", "mstep", "update"))
    print(f"{tag} emission / assign {e / a:.3f}; mstep / update {m / up:.3f}; emission {3.0 * n * d * k / e / 1e12:.2f} TFLOP/s of float32 operations "
          f"({100 * 3.0 * n * d * k / e / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF); mstep {4.0 * n * d * k / m / 1e12:.2f} TFLOP/s of float64 operations" +
          (f"; fit {info.n_iter} iterations, loglik per row {info.loglik / n:.4f}" if fit_too else ""), flush=True)
    del x, ws, kws, logb, gamma
    torch.cuda.empty_cache()


def step():
    import torch
    from track_mjx_amd import hip
    print(f"# HMM: median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    for d in DS:
        for k in KS:
            shape(N // T, T, d, k)
    print("# whole-clip roll-outs: one workgroup per sequence, 8 workgroups on the device")
    shape(*LONG, fit_too=False)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hmm_bench.txt"))
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("hmm_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step()
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"hmm_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"hmm_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/hmm_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
