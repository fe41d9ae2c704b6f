#!/usr/bin/env python3
"""Times of the GPU autoregressive HMM (track_mjx_amd/analysis/arhmm.py; tmjx_arhmm_*): 210 000 rows as 840 sequences of 250, d = 10 features with
L = 3 lags (MoSeq's shape) into 16, 64 and 128 states, and every limit at once: d = 32, L = 4, 128 states.

  emission      tmjx_arhmm_emission (positions, c_j, then the fused pass) between two device events over LOOPS calls
  hmm emission  its yardstick: tmjx_hmm_emission at the same rows, d and k (1 / (p + 1) of the FMAs)
  moments       tmjx_arhmm_moments (positions, the float64 Gram sums, the reduction), likewise
  hmm mstep     its yardstick: tmjx_hmm_mstep at the same rows, d and k
  solve         tmjx_arhmm_solve (one Cholesky and d solves per state), likewise
  fit           tmjx_arhmm_fit, 20 iterations (tol = 0), with its own emission / fb / mstep / viterbi times

and the FMA counts against the vector peaks: n k d (p + 1) float32 FMAs of the emission over 157.3 TFLOP/s, n k q (q + 1) / 2 float64 FMAs of the
moments over 78.6 TFLOP/s (the MI355X's public float64 vector peak).  The moment kernel computes whole 64 x 64 tiles on and above the diagonal,
so it executes more than the count.  The blocks alternate inside each repeat, so a drift of the clocks falls on all of them alike.
usage: python tools/arhmm_bench.py [--out profiles/arhmm_bench.txt]
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

N, T, SHAPES, REPEATS, LOOPS, FIT_ITERS, LIMIT = 210_000, 250, ((10, 3, 16), (10, 3, 64), (10, 3, 128), (32, 4, 128)), 3, 2, 20, 540
PEAK32_TF, PEAK64_TF = 157.3, 78.6      # float32 and float64 vector peaks (TFLOP/s) of the MI355X


def med(v):
    return f"{statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})"


def shape(S, T, d, L, k):
    import numpy as np
    import torch
    from track_mjx_amd import hip
    Lb = hip.lib()
    n, p = S * T, L * d + 1
    q = p + d
    g = torch.Generator(device="cuda").manual_seed(1000 * d + k)
    # a contracting walk: x_t = 0.8 x_(t-1) + noise, every sequence from its own start
    noise = torch.randn((T, S, d), generator=g, device="cuda")
    walk = torch.empty_like(noise)
    v = torch.randn((S, d), generator=g, device="cuda")
    for t in range(T):
        v = 0.8 * v + 0.6 * noise[t]
        walk[t] = v
    x = (walk.permute(1, 0, 2).reshape(n, d) + 1.5).contiguous()
    seq = (np.arange(S + 1, dtype=np.int32) * T)
    seq_p = seq.ctypes.data_as(C.POINTER(C.c_int32))
    floats, hfloats, info = C.c_int64(0), C.c_int64(0), hip.ArhmmInfo()
    hip.check(Lb.tmjx_arhmm_workspace(n, d, L, k, S, C.byref(floats)), "tmjx_arhmm_workspace")
    hip.check(Lb.tmjx_hmm_workspace(n, d, k, S, C.byref(hfloats)), "tmjx_hmm_workspace")
    ws = torch.empty(int(floats.value), dtype=torch.float32, device="cuda")
    hws = torch.empty(int(hfloats.value), dtype=torch.float32, device="cuda")
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")      # noqa: E731
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")      # noqa: E731
    center = x.mean(0).contiguous()
    W0 = (0.3 * torch.randn((k, d, p), generator=g, device="cuda") / max(L * d, 1) ** 0.5).contiguous()
    var0, A0, pi0 = torch.ones((k, d), device="cuda"), torch.full((k, k), 1.0 / k, device="cuda"), torch.full((k,), 1.0 / k, device="cuda")
    W, var, A, pi, Ws, vs = W0.clone(), var0.clone(), A0.clone(), pi0.clone(), W0.clone(), var0.clone()
    mu0 = (1.5 + torch.randn((k, d), generator=g, device="cuda")).contiguous()
    mu, hvar = mu0.clone(), var0.clone()
    logb = f32(n, k)
    gamma = torch.softmax(2.0 * torch.randn((n // 25 + 1, k), generator=g, device="cuda"), 1).repeat_interleave(25, 0)[:n].contiguous()      # posteriors that dwell
    M, weight, hweight, means = f64(k, q, q), f64(k), f64(k), f32(k, d)
    labels, status = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(k, dtype=torch.int32, device="cuda")
    ridge = float(x.var(0).mean())
    X = (x.data_ptr(), n, d, d)
    calls = {
        "emission": lambda: hip.check(Lb.tmjx_arhmm_emission(*X, seq_p, S, L, L, center.data_ptr(), W0.data_ptr(), var0.data_ptr(), k, logb.data_ptr(), ws.data_ptr(),
                                                             None), "emission"),
        "hmm emission": lambda: hip.check(Lb.tmjx_hmm_emission(*X, mu0.data_ptr(), var0.data_ptr(), k, logb.data_ptr(), hws.data_ptr(), None), "hmm emission"),
        "moments": lambda: hip.check(Lb.tmjx_arhmm_moments(*X, seq_p, S, L, L, center.data_ptr(), gamma.data_ptr(), k, M.data_ptr(), weight.data_ptr(), ws.data_ptr(),
                                                           None), "moments"),
        "hmm mstep": lambda: hip.check(Lb.tmjx_hmm_mstep(*X, gamma.data_ptr(), k, 1e-3, 1e-3, mu.data_ptr(), hvar.data_ptr(), hweight.data_ptr(), hws.data_ptr(), None),
                                       "hmm mstep"),
        "solve": lambda: hip.check(Lb.tmjx_arhmm_solve(M.data_ptr(), weight.data_ptr(), k, d, L, center.data_ptr(), ridge, 1e-3, 1e-3, Ws.data_ptr(), vs.data_ptr(),
                                                       means.data_ptr(), status.data_ptr(), ws.data_ptr(), None), "solve"),
    }

    def fit():
        for dst, src in ((W, W0), (var, var0), (A, A0), (pi, pi0)):
            dst.copy_(src)
        hip.check(Lb.tmjx_arhmm_fit(*X, seq_p, S, L, L, center.data_ptr(), k, W.data_ptr(), var.data_ptr(), A.data_ptr(), pi.data_ptr(), None, labels.data_ptr(),
                                    status.data_ptr(), FIT_ITERS, 0.0, 0.1, 0.0, ridge, 1e-3, 1e-3, C.byref(info), ws.data_ptr(), None), "fit")

    for f in calls.values():      # warm-up (and the moments the solve reads)
        f()
    fit()
    torch.cuda.synchronize()
    t = {name: [] for name in (*calls, "fit", "fit: emissions", "fit: fb", "fit: msteps", "fit: viterbi")}
    for _ in range(REPEATS):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LOOPS):
                f()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1) / LOOPS)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fit()
        e1.record()
        e1.synchronize()
        for name, v in (("fit", e0.elapsed_time(e1)), ("fit: emissions", info.emission_ms), ("fit: fb", info.fb_ms), ("fit: msteps", info.mstep_ms),
                        ("fit: viterbi", info.viterbi_ms)):
            t[name].append(v)
    tag = f"{S} x {T} x {d:<2d} L {L} k {k:<3d}"
    for name, v in t.items():
        print(f"{tag} {name:14s} {med(v)}")
    e, he, m, hm = (statistics.median(t[name]) * 1e-3 for name in ("emission", "hmm emission", "moments", "hmm mstep"))
    fma32, fma64 = float(n) * k * d * (p + 1), float(n) * k * q * (q + 1) / 2
    print(f"{tag} emission / hmm emission {e / he:.2f} (p + 1 = {p + 1}); moments / hmm mstep {m / hm:.2f}; emission {fma32:.3g} float32 FMAs: "
          f"{2 * fma32 / e / 1e12:.2f} TFLOP/s, {100 * 2 * fma32 / e / 1e12 / PEAK32_TF:.1f} % of {PEAK32_TF} TF; moments {fma64:.3g} float64 FMAs: "
          f"{2 * fma64 / m / 1e12:.2f} TFLOP/s, {100 * 2 * fma64 / m / 1e12 / PEAK64_TF:.1f} % of {PEAK64_TF} TF; fit {info.n_iter} iterations, "
          f"{info.n_singular} singular, loglik per row {info.loglik / n:.4f}; workspace {int(floats.value) * 4 / 2 ** 20:.0f} MiB", flush=True)
    del x, ws, hws, logb, gamma, noise, walk
    torch.cuda.empty_cache()


def step():
    import torch
    from track_mjx_amd import hip
    print(f"# AR-HMM: median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    floats = C.c_int64(0)
    hip.check(hip.lib().tmjx_arhmm_workspace(N, 32, 4, 128, N // T, C.byref(floats)), "tmjx_arhmm_workspace")
    print(f"# tmjx_arhmm_workspace at the limits ({N} rows, d = 32, L = 4, k = 128, {N // T} sequences): {int(floats.value)} floats = "
          f"{int(floats.value) * 4 / 2 ** 20:.0f} MiB")
    for d, L, k in SHAPES:
        shape(N // T, T, d, L, k)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "arhmm_bench.txt"))
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("arhmm_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step()
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"arhmm_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"arhmm_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/arhmm_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
