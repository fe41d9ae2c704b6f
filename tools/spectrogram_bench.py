#!/usr/bin/env python3
"""Times of the GPU wavelet spectrogram (track_mjx_amd/analysis/spectrogram.py; tmjx_spectrogram): 210 000 rows as 840 sequences of 250 at rate 50,
C = 4, 16, 67 and 512 channels with the default bank of 25 frequencies (1 .. 25 Hz, 2 501 taps per channel-row), and C = 67 with the 15-frequency
bank whose 1 005 columns the motif tools take.  Three floors stand next to each time:

  fill      a plain device fill of the same output bytes: the write bound
  fma       the tap count of the bank, two FMAs a tap (re and im), at the float32 vector peak of the MI355X (157.3 TFLOP/s).  `taps in range` counts
            only the taps that fall inside a 250-row sequence, which is what the kernel executes; `all taps` is the bank's nominal count
  assign    tmjx_kmeans_assign at 210 000 x 1024 into 64 centroids: the project's usual yardstick

The blocks alternate inside each repeat, so a drift of the clocks falls on all of them alike.
usage: python tools/spectrogram_bench.py [--out profiles/spectrogram_bench.txt]
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

N, T, RATE, REPEATS, LOOPS, WARMUP, LIMIT = 210_000, 250, 50.0, 5, 3, 2, 540
SHAPES = ((4, 25), (16, 25), (67, 25), (67, 15), (512, 25))      # (channels, frequencies)
PEAK_TF = 157.3      # float32 vector peak (TFLOP/s) of the MI355X


def med(v):
    return f"{statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})"


def timed(f, loops=LOOPS):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(loops):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / loops


def shape(Cn, F, assign):
    import numpy as np
    import torch
    from track_mjx_amd import hip
    from track_mjx_amd.analysis.pca import HipBackend
    from track_mjx_amd.analysis.spectrogram import dyadic_frequencies
    Lb, S = hip.lib(), N // T
    freqs = dyadic_frequencies(1.0, 25.0, F)
    bank, offset, radius = HipBackend("cuda").wavelet_bank(RATE, freqs)
    g = torch.Generator(device="cuda").manual_seed(100 * Cn + F)
    x = torch.randn((N, Cn), generator=g, device="cuda") + 3.0
    bk = torch.from_numpy(bank).cuda()
    out, cov = torch.empty((N, F * Cn), dtype=torch.float32, device="cuda"), torch.empty((N, F), dtype=torch.float32, device="cuda")
    floats = C.c_int64(0)
    hip.check(Lb.tmjx_spectrogram_workspace(N, Cn, F, S, C.byref(floats)), "tmjx_spectrogram_workspace")
    ws = torch.empty(int(floats.value), dtype=torch.float32, device="cuda")
    seq = np.arange(S + 1, dtype=np.int32) * T
    i32p = C.POINTER(C.c_int32)
    seq_p, off_p, rad_p = seq.ctypes.data_as(i32p), offset.ctypes.data_as(i32p), radius.ctypes.data_as(i32p)
    calls = {"spectrogram": lambda: hip.check(Lb.tmjx_spectrogram(x.data_ptr(), N, Cn, Cn, seq_p, S, bk.data_ptr(), off_p, rad_p, F, 1, 0, 1e-3, out.data_ptr(),
                                                                  F * Cn, cov.data_ptr(), ws.data_ptr(), None), "tmjx_spectrogram"),
             "fill": lambda: out.fill_(1.0), "assign": assign}
    for _ in range(WARMUP):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    t = {name: [] for name in calls}
    for _ in range(REPEATS):
        for name, f in calls.items():
            t[name].append(timed(f))
    tt = np.arange(T)[:, None]
    inside = sum(int((np.minimum(int(R), T - 1 - tt) - np.maximum(-int(R), -tt) + 1).sum()) for R in radius) / T      # taps in range per channel-row, averaged
    nominal = int((2 * radius.astype(np.int64) + 1).sum())
    tag = f"C {Cn:<4d} F {F:<3d}"
    for name, v in t.items():
        print(f"{tag} {name:12s} {med(v)}")
    sp, fl, asg = (statistics.median(t[name]) * 1e-3 for name in ("spectrogram", "fill", "assign"))
    byt = 4.0 * N * F * Cn
    fma_in, fma_all = (4.0 * N * Cn * taps / (PEAK_TF * 1e12) for taps in (inside, nominal))
    print(f"{tag} output {byt / 1e9:.3f} GB: fill {byt / fl / 1e12:.2f} TB/s, spectrogram {byt / sp / 1e12:.3f} TB/s of output; {nominal} taps per channel-row "
          f"({inside:.0f} in range): the FMA floor at {PEAK_TF} TF is {1e3 * fma_in:.3f} ms in range ({1e3 * fma_all:.3f} ms all taps), the kernel runs "
          f"{4.0 * N * Cn * inside / sp / 1e12:.1f} TFLOP/s = {100 * fma_in / sp:.1f} % of it; spectrogram / fill {sp / fl:.2f}, / FMA floor {sp / fma_in:.2f}, "
          f"/ assign {sp / asg:.2f}", flush=True)
    del x, out, ws
    torch.cuda.empty_cache()


def step():
    import torch
    from track_mjx_amd import hip
    Lb = hip.lib()
    print(f"# spectrogram: {N} rows as {N // T} sequences of {T} at rate {RATE:g}; median of {REPEATS} repeats of {LOOPS} calls (min .. max) after {WARMUP} warm-up "
          f"rounds; build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    d, k = 1024, 64
    g = torch.Generator(device="cuda").manual_seed(7)
    xa, cen = torch.randn((N, d), generator=g, device="cuda"), torch.randn((k, d), generator=g, device="cuda")
    kfloats = C.c_int64(0)
    hip.check(Lb.tmjx_kmeans_workspace(N, d, k, C.byref(kfloats)), "tmjx_kmeans_workspace")
    kws = torch.empty(int(kfloats.value), dtype=torch.float32, device="cuda")
    labels, inertia = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")

    def assign():
        hip.check(Lb.tmjx_kmeans_assign(xa.data_ptr(), N, d, d, cen.data_ptr(), k, None, labels.data_ptr(), None, inertia.data_ptr(), None, kws.data_ptr(), None),
                  "tmjx_kmeans_assign")
    for Cn, F in SHAPES:
        shape(Cn, F, assign)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spectrogram_bench.txt"))
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("spectrogram_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step()
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step"], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"spectrogram_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"spectrogram_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/spectrogram_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
