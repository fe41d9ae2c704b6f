#!/usr/bin/env python3
"""Times of the GPU decoder Jacobian (track_mjx_amd/analysis/jacobian.py; tmjx_decoder_jacobian).

  jac   tmjx_decoder_jacobian between two device events: 210 000 rows of a 286-wide decoder input, A = 38 actuators, the 60 intention columns
        differentiated, through three decoders: (256, 256), (512, 512, 512) and (1024, 1024).  Outputs: ctrl, gain, col2, row2 and the sums (the
        Jacobians themselves, 1.9 GB, are not stored).  Counted beside each: the float32 FMAs of the reverse products (rows A sum_l H_l N_l, N_l
        the width before layer l, 60 at the first) and of the forward ones, against the float32 vector peak.
  gemm  the yardstick: the learner's tmjx_gemm_nn (dx = dy W) at the same N and K per layer, summed over the layers.  It is timed at
        M = 8192 x 38 rows (a 1.3 GB left operand at K = 1024) and scaled to M = 210 000 x 38: the whole left operand would be 33 GB.

usage: python tools/jacobian_bench.py [--out profiles/jacobian_bench.txt] [--decoders 256,256/512,512,512/1024,1024]
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

REPEATS, LIMIT = 3, 500
ROWS, D_IN, A, Z = 210_000, 286, 38, 60
GEMM_ROWS = 8192
DECODERS = "256,256/512,512,512/1024,1024"
PEAK_TF = 157.3      # float32 vector = matrix peak (TFLOP/s) of the MI355X, an FMA counted as two operations


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


def step(decoders):
    import torch
    from track_mjx_amd import hip
    Lb = hip.lib()
    print(f"# decoder Jacobian: median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    dev = dict(device="cuda", dtype=torch.float32)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((ROWS, D_IN), generator=g, **dev)
    for widths in decoders:
        keep, desc, K = [], hip.JacobianDesc(), D_IN
        desc.L, desc.d_in, desc.eps, desc.A, desc.wrt_col0, desc.wrt_cols = len(widths), D_IN, 1e-6, A, 0, Z
        for slot, H in zip(desc.layer, widths):
            W, b = torch.randn((H, K), generator=g, **dev) / K ** 0.5, torch.randn(H, generator=g, **dev)
            gamma, beta = 1.0 + 0.1 * torch.randn(H, generator=g, **dev), torch.randn(H, generator=g, **dev)
            keep += [W, b, gamma, beta]
            slot.W, slot.b, slot.gamma, slot.beta, slot.width, slot.ldw = W.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), H, K
            K = H
        wh, bh = torch.randn((2 * A, K), generator=g, **dev) / K ** 0.5, 0.1 * torch.randn(2 * A, generator=g, **dev)
        desc.Wh, desc.bh, desc.ldwh = wh.data_ptr(), bh.data_ptr(), K
        floats = C.c_int64(0)
        hip.check(Lb.tmjx_jacobian_workspace(C.byref(desc), ROWS, C.byref(floats)), "tmjx_jacobian_workspace")
        ws = torch.empty(int(floats.value), **dev)
        ctrl, gain, col2, row2 = (torch.empty(s, **dev) for s in ((ROWS, A), (ROWS,), (ROWS, Z), (ROWS, A)))
        sums = torch.zeros(A * Z + Z * Z + A * A, dtype=torch.float64, device="cuda")
        t = timed(lambda: hip.check(Lb.tmjx_decoder_jacobian(C.byref(desc), x.data_ptr(), ROWS, D_IN, None, ROWS, None, 0, 0, ctrl.data_ptr(), None, gain.data_ptr(),
                                                             col2.data_ptr(), row2.data_ptr(), None, sums.data_ptr(), ws.data_ptr(), None), "tmjx_decoder_jacobian"))
        ins = [Z, *widths[:-1]]
        reverse = float(ROWS) * A * sum(h * n for h, n in zip(widths, ins))
        forward = float(ROWS) * (sum(h * k for h, k in zip(widths, [D_IN, *widths[:-1]])) + A * widths[-1])
        s = statistics.median(t) * 1e-3
        tag = f"jac {ROWS} x {A} x {Z} decoder {'-'.join(str(h) for h in widths):<13s}"
        print(f"{tag} tmjx_decoder_jacobian {med(t)}   mean gain {float(gain.double().mean()):.4g}, trace of the sums / rows {float(sums[A * Z:A * Z + Z * Z].view(Z, Z).trace()) / ROWS:.4g}")
        del ws
        torch.cuda.empty_cache()
        # the yardstick: dx = dy W per layer at M = GEMM_ROWS x A, scaled to ROWS x A
        M, total = GEMM_ROWS * A, 0.0
        parts = []
        for l, (H, N) in enumerate(zip(widths, ins)):
            dy, dx = torch.randn((M, H), generator=g, **dev), torch.empty((M, N), **dev)
            W = keep[4 * l]
            tg = timed(lambda: hip.check(Lb.tmjx_gemm_nn(dy.data_ptr(), H, W.data_ptr(), W.shape[1], dx.data_ptr(), N, M, N, H, None), "tmjx_gemm_nn"))
            total += statistics.median(tg) * ROWS / GEMM_ROWS
            parts.append(f"[{M} x {H}] x [{H} x {N}] {statistics.median(tg):.3f} ms")
            del dy, dx
        print(f"{tag} tmjx_gemm_nn per layer at M = {GEMM_ROWS} x {A}: {'; '.join(parts)}; scaled to {ROWS} x {A} rows and summed {total:10.3f} ms")
        print(f"{tag} jacobian / gemm_nn {s * 1e3 / total:.2f}; counted {reverse:.3g} reverse + {forward:.3g} forward float32 FMAs: {2 * (reverse + forward) / s / 1e12:.2f} TFLOP/s "
              f"({100 * 2 * (reverse + forward) / s / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF); workspace {int(floats.value) * 4 / 1e6:.1f} MB", flush=True)
        del keep, wh, bh
        torch.cuda.empty_cache()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "jacobian_bench.txt"))
    ap.add_argument("--decoders", default=DECODERS)
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    decoders = [tuple(int(h) for h in d.split(",")) for d in args.decoders.split("/")]
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("jacobian_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step(decoders)
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step", "--decoders", args.decoders], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"jacobian_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"jacobian_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/jacobian_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
