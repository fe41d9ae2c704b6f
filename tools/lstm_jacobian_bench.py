#!/usr/bin/env python3
"""Times of the GPU LSTM-decoder Jacobian (track_mjx_amd/analysis/jacobian.py; tmjx_lstm_decoder_jacobian).

  lstm  tmjx_lstm_decoder_jacobian between two device events: 210 000 rows of a 286-wide decoder input with their carry, A = 38 actuators, the 60
        intention columns differentiated, through the shipped decoder (H = 128, L = 2) and through the limits (H = 256, L = 4).  Outputs: ctrl, gain,
        col2, row2, carry_gain and the sums (the Jacobians themselves are not stored).  Counted beside each: the float32 FMAs of the reverse
        products (rows A sum_k 4H (H + N_k), N_k the width below layer k, 60 at the first) and of the forward ones, against the float32 vector peak.
  mlp   next to them: tmjx_decoder_jacobian through the (256, 256) MLP decoder at the same rows, with its own count.

usage: python tools/lstm_jacobian_bench.py [--out profiles/lstm_jacobian_bench.txt] [--shapes 128,2/256,4]
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

from tools.jacobian_bench import PEAK_TF, REPEATS, med, timed  # noqa: E402

LIMIT = 500
ROWS, D_IN, A, Z = 210_000, 286, 38, 60
SHAPES = "128,2/256,4"
MLP = (256, 256)


def step(shapes):
    import torch
    from track_mjx_amd import hip
    Lb = hip.lib()
    print(f"# LSTM decoder Jacobian: median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    dev = dict(device="cuda", dtype=torch.float32)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((ROWS, D_IN), generator=g, **dev)
    for H, L in shapes:
        keep, desc, K = [], hip.LstmJacobianDesc(), D_IN
        desc.L, desc.H, desc.d_in, desc.A, desc.wrt_col0, desc.wrt_cols = L, H, D_IN, A, 0, Z
        for slot in list(desc.layer)[:L]:
            wi, wh, b = torch.randn((4 * H, K), generator=g, **dev) / K ** 0.5, torch.randn((4 * H, H), generator=g, **dev) / H ** 0.5, 0.5 * torch.randn(4 * H, generator=g, **dev)
            keep += [wi, wh, b]
            slot.W_ih, slot.W_hh, slot.b_hh, slot.ldwi, slot.ldwh = wi.data_ptr(), wh.data_ptr(), b.data_ptr(), K, H
            K = H
        wp, bp = torch.randn((2 * A, H), generator=g, **dev) / H ** 0.5, 0.1 * torch.randn(2 * A, generator=g, **dev)
        desc.Wp, desc.bp, desc.ldwp = wp.data_ptr(), bp.data_ptr(), H
        h_in, c_in = (0.5 * torch.randn((ROWS, L * H), generator=g, **dev)).clamp_(-0.99, 0.99), torch.randn((ROWS, L * H), generator=g, **dev)
        floats = C.c_int64(0)
        hip.check(Lb.tmjx_lstm_jacobian_workspace(C.byref(desc), ROWS, C.byref(floats)), "tmjx_lstm_jacobian_workspace")
        ws = torch.empty(int(floats.value), **dev)
        ctrl, gain, col2, row2, cgain = (torch.empty(s, **dev) for s in ((ROWS, A), (ROWS,), (ROWS, Z), (ROWS, A), (ROWS, 2 * L)))
        E = A * Z + Z * Z + A * A
        sums = torch.zeros(E + A * 2 * L * H, dtype=torch.float64, device="cuda")
        t = timed(lambda: hip.check(Lb.tmjx_lstm_decoder_jacobian(C.byref(desc), x.data_ptr(), ROWS, D_IN, h_in.data_ptr(), c_in.data_ptr(), L * H, None, ROWS, None, 0, None, 0,
                                                                  ctrl.data_ptr(), None, gain.data_ptr(), col2.data_ptr(), row2.data_ptr(), None, None, cgain.data_ptr(),
                                                                  sums.data_ptr(), ws.data_ptr(), None), "tmjx_lstm_decoder_jacobian"))
        reverse = float(ROWS) * A * sum(4 * H * (H + (Z if k == 0 else H)) for k in range(L))
        forward = float(ROWS) * (sum(4 * H * ((D_IN if k == 0 else H) + H) for k in range(L)) + A * H)
        s = statistics.median(t) * 1e-3
        tag = f"lstm {ROWS} x {A} x {Z} H {H} L {L}"
        print(f"{tag:<36s} tmjx_lstm_decoder_jacobian {med(t)}   mean gain {float(gain.double().mean()):.4g}, mean carry gain (h, then c, per layer) "
              f"{[round(v, 4) for v in cgain.double().mean(0).tolist()]}")
        print(f"{tag:<36s} counted {reverse:.3g} reverse + {forward:.3g} forward float32 FMAs: {2 * (reverse + forward) / s / 1e12:.2f} TFLOP/s "
              f"({100 * 2 * (reverse + forward) / s / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF); workspace {int(floats.value) * 4 / 1e6:.1f} MB", flush=True)
        del ws, keep, wp, bp, h_in, c_in, sums, cgain
        torch.cuda.empty_cache()
    # next to them: the MLP decoder's Jacobian through (256, 256) at the same rows
    keep, desc, K = [], hip.JacobianDesc(), D_IN
    desc.L, desc.d_in, desc.eps, desc.A, desc.wrt_col0, desc.wrt_cols = len(MLP), D_IN, 1e-6, A, 0, Z
    for slot, H in zip(desc.layer, MLP):
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
    reverse = float(ROWS) * A * sum(h * n for h, n in zip(MLP, [Z, *MLP[:-1]]))
    forward = float(ROWS) * (sum(h * k for h, k in zip(MLP, [D_IN, *MLP[:-1]])) + A * MLP[-1])
    s = statistics.median(t) * 1e-3
    tag = f"mlp  {ROWS} x {A} x {Z} decoder {'-'.join(str(h) for h in MLP)}"
    print(f"{tag:<36s} tmjx_decoder_jacobian      {med(t)}   mean gain {float(gain.double().mean()):.4g}")
    print(f"{tag:<36s} counted {reverse:.3g} reverse + {forward:.3g} forward float32 FMAs: {2 * (reverse + forward) / s / 1e12:.2f} TFLOP/s "
          f"({100 * 2 * (reverse + forward) / s / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF); workspace {int(floats.value) * 4 / 1e6:.1f} MB", flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lstm_jacobian_bench.txt"))
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in d.split(",")) for d in args.shapes.split("/")]
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("lstm_jacobian_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step(shapes)
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step", "--shapes", args.shapes], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"lstm_jacobian_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"lstm_jacobian_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/lstm_jacobian_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
