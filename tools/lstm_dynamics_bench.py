#!/usr/bin/env python3
"""Times of the GPU LSTM-decoder dynamics (track_mjx_amd/analysis/dynamics.py; tmjx_lstm_lyapunov, tmjx_lstm_tangent_step).

  lyapunov  tmjx_lstm_lyapunov between two device events: 210 000 rows of a 286-wide decoder input with their carry as S sequences of T rows, K
            tangents, with the outputs local, energy, q_out, status and sums: 840 x 250 through the shipped decoder (H = 128, L = 2, K = 16) and
            through the limits (H = 256, L = 4, K = 32), and 8 x 26 250, where the serial length dominates.
  step      next to each: tmjx_lstm_tangent_step over the same n x K tangent rows in one call: the same products without the serial dependence
            (and without the QR).
  jacobian  next to each: tmjx_lstm_decoder_jacobian at the same rows (A = 38, 60 differentiated columns), the one-step linearisation.
  counted   the float32 FMAs of the tangent products (n K sum_k 4H (H + [k > 0] H)), of the forward ones and of the QR (2 sweeps, K (K + 1) / 2 dots
            or norms and as many updates of W elements: n 2 K (K + 1) W), against the float32 vector peak.
  share     in a run of its own under `rocprofv3 --kernel-trace --stats` (one call of the first shape): the QR kernel's share of the kernels' time.

usage: python tools/lstm_dynamics_bench.py [--out profiles/lstm_dynamics_bench.txt] [--shapes 128,2,16,840,250/256,4,32,840,250/128,2,16,8,26250]
The shapes run in one child process under its own time limit; the timings are recorded, not asserted.
"""
import argparse
import csv
import ctypes as C
import shutil
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tools.jacobian_bench import PEAK_TF, REPEATS, med, timed  # noqa: E402

LIMIT = 900
D_IN, A, Z = 286, 38, 60
SHAPES = "128,2,16,840,250/256,4,32,840,250/128,2,16,8,26250"
WARMUP = 25
STEP_BYTES = 8 << 30      # the tangents tmjx_lstm_tangent_step is timed on, at the most (as many again for its output)


def step(shapes, once=False):
    import numpy as np
    import torch
    from track_mjx_amd import hip
    from track_mjx_amd.analysis.dynamics import first_basis
    Lb = hip.lib()
    print(f"# LSTM decoder dynamics: median of {REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    dev = dict(device="cuda", dtype=torch.float32)
    g = torch.Generator(device="cuda").manual_seed(7)
    for H, L, K, S, T in shapes:
        n, W = S * T, 2 * L * H
        x = torch.randn((n, D_IN), generator=g, **dev)
        keep, desc, Kin = [], hip.LstmJacobianDesc(), D_IN
        desc.L, desc.H, desc.d_in, desc.A, desc.wrt_col0, desc.wrt_cols = L, H, D_IN, A, 0, Z
        for slot in list(desc.layer)[:L]:
            wi, wh, b = torch.randn((4 * H, Kin), generator=g, **dev) / Kin ** 0.5, torch.randn((4 * H, H), generator=g, **dev) / H ** 0.5, 0.5 * torch.randn(4 * H, generator=g, **dev)
            b[H:2 * H] += 1.0
            keep += [wi, wh, b]
            slot.W_ih, slot.W_hh, slot.b_hh, slot.ldwi, slot.ldwh = wi.data_ptr(), wh.data_ptr(), b.data_ptr(), Kin, H
            Kin = H
        wp, bp = torch.randn((2 * A, H), generator=g, **dev) / H ** 0.5, 0.1 * torch.randn(2 * A, generator=g, **dev)
        desc.Wp, desc.bp, desc.ldwp = wp.data_ptr(), bp.data_ptr(), H
        h_in, c_in = (0.5 * torch.randn((n, L * H), generator=g, **dev)).clamp_(-0.99, 0.99), torch.randn((n, L * H), generator=g, **dev)
        tag = f"{S} x {T} rows, H {H} L {L} K {K}"
        # the spectrum
        floats = C.c_int64(0)
        hip.check(Lb.tmjx_lstm_tangent_workspace(C.byref(desc), S, K, C.byref(floats)), "tmjx_lstm_tangent_workspace")
        ws = torch.empty(int(floats.value), **dev)
        seq = np.arange(0, n + 1, T, dtype=np.int32)
        q0 = torch.from_numpy(first_basis(W, K, 0)).cuda()
        local, energy, q_out = (torch.empty(s, **dev) for s in ((n, K), (n, K, 2 * L), (S, K, W)))
        status, sums = torch.empty(S, dtype=torch.int32, device="cuda"), torch.empty((S, K), dtype=torch.float64, device="cuda")

        def lyapunov():
            hip.check(Lb.tmjx_lstm_lyapunov(C.byref(desc), x.data_ptr(), n, D_IN, h_in.data_ptr(), c_in.data_ptr(), L * H, seq.ctypes.data_as(C.POINTER(C.c_int32)), S,
                                            q0.data_ptr(), 0, K, WARMUP, local.data_ptr(), energy.data_ptr(), q_out.data_ptr(), status.data_ptr(), sums.data_ptr(),
                                            ws.data_ptr(), None), "tmjx_lstm_lyapunov")
        if once:
            lyapunov()
            torch.cuda.synchronize()
            return
        t = timed(lyapunov)
        tangent = float(n) * K * sum(4 * H * (H + (H if k else 0)) for k in range(L))
        forward = float(n) * sum(4 * H * ((D_IN if k == 0 else H) + H) for k in range(L))
        qr = float(n) * 2 * K * (K + 1) * W
        s = statistics.median(t) * 1e-3
        lam = (sums.sum(0) / (S * max(T - WARMUP, 0))).tolist()
        print(f"{tag:<34s} tmjx_lstm_lyapunov         {med(t)}   {1e3 * statistics.median(t) / T:.1f} us a step; leading exponents {[round(v, 4) for v in lam[:3]]}, "
              f"dead columns in {int(status.sum())} sequences")
        print(f"{tag:<34s} counted {tangent:.3g} tangent + {forward:.3g} forward + {qr:.3g} QR float32 FMAs: {2 * (tangent + forward + qr) / s / 1e12:.2f} TFLOP/s "
              f"({100 * 2 * (tangent + forward + qr) / s / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF); workspace {int(floats.value) * 4 / 1e6:.1f} MB", flush=True)
        del ws, local, energy, q_out
        torch.cuda.empty_cache()
        # the same tangent rows without the serial dependence
        hip.check(Lb.tmjx_lstm_tangent_workspace(C.byref(desc), min(n, hip.JACOBIAN_CHUNK), K, C.byref(floats)), "tmjx_lstm_tangent_workspace")
        ws = torch.empty(int(floats.value), **dev)
        # (the tangents of all n rows are n K W floats, 55 GB at the limits: the call is timed on the first ns rows, whole passes, and its rows are
        # independent, so the time of n rows is that times n / ns; both are printed and named)
        ns = min(n, max(hip.JACOBIAN_CHUNK, STEP_BYTES // (K * W * 4) // hip.JACOBIAN_CHUNK * hip.JACOBIAN_CHUNK))
        v, out = torch.randn((ns, K, W), generator=g, **dev), torch.empty((ns, K, W), **dev)
        t = timed(lambda: hip.check(Lb.tmjx_lstm_tangent_step(C.byref(desc), x.data_ptr(), ns, D_IN, h_in.data_ptr(), c_in.data_ptr(), L * H, v.data_ptr(), K, out.data_ptr(),
                                                              ws.data_ptr(), None), "tmjx_lstm_tangent_step"))
        s = statistics.median(t) * 1e-3 * n / ns
        print(f"{tag:<34s} tmjx_lstm_tangent_step     {med(t)}   measured on {ns} rows; times n / ns = {1e3 * s:.3f} ms for the {n} rows: "
              f"{2 * (tangent + forward) / s / 1e12:.2f} TFLOP/s ({100 * 2 * (tangent + forward) / s / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF); workspace "
              f"{int(floats.value) * 4 / 1e6:.1f} MB", flush=True)
        del ws, v, out
        torch.cuda.empty_cache()
        # the one-step linearisation at the same rows
        hip.check(Lb.tmjx_lstm_jacobian_workspace(C.byref(desc), n, C.byref(floats)), "tmjx_lstm_jacobian_workspace")
        ws = torch.empty(int(floats.value), **dev)
        ctrl, gain, col2, row2, cgain = (torch.empty(s_, **dev) for s_ in ((n, A), (n,), (n, Z), (n, A), (n, 2 * L)))
        jsums = torch.zeros(A * Z + Z * Z + A * A + A * W, dtype=torch.float64, device="cuda")
        t = timed(lambda: hip.check(Lb.tmjx_lstm_decoder_jacobian(C.byref(desc), x.data_ptr(), n, D_IN, h_in.data_ptr(), c_in.data_ptr(), L * H, None, n, None, 0, None, 0,
                                                                  ctrl.data_ptr(), None, gain.data_ptr(), col2.data_ptr(), row2.data_ptr(), None, None, cgain.data_ptr(),
                                                                  jsums.data_ptr(), ws.data_ptr(), None), "tmjx_lstm_decoder_jacobian"))
        print(f"{tag:<34s} tmjx_lstm_decoder_jacobian {med(t)}   (A {A}, {Z} columns: the one-step linearisation at the same rows)", flush=True)
        del ws, keep, wp, bp, h_in, c_in, x, jsums
        torch.cuda.empty_cache()


def qr_share(shape: str) -> str:
    """One call of `shape` under rocprofv3 --kernel-trace --stats: the kernels' times by name."""
    if shutil.which("rocprofv3") is None:
        return "# share: rocprofv3 not found: not measured\n"
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "dyn", "--", sys.executable, __file__, "--step", "--once", "--shapes", shape]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT // 3)
        except subprocess.TimeoutExpired:
            return "# share: the traced run ran past its limit: not measured\n"
        files = sorted(Path(d).rglob("*kernel_stats.csv"))
        if res.returncode != 0 or not files:
            return f"# share: the traced run failed ({res.returncode}): not measured\n"
        rows = [r for r in csv.DictReader(files[0].open()) if "k_lst_" in r.get("Name", "")]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    if not total:
        return "# share: no k_lst_ kernel in the trace: not measured\n"
    out = f"# share of the kernels' time in one traced call of {shape} (rocprofv3 --kernel-trace --stats, a run of its own; the host's launches are not in it):\n"
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        out += f"#   {r['Name'].split('(')[0]:<28s} {int(r['Calls']):7d} calls {float(r['TotalDurationNs']) / 1e6:10.3f} ms  {100 * float(r['TotalDurationNs']) / total:5.1f} %\n"
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lstm_dynamics_bench.txt"))
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    ap.add_argument("--once", action="store_true", help="(internal) one tmjx_lstm_lyapunov call of the first shape, for a trace")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in d.split(",")) for d in args.shapes.split("/")]
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("lstm_dynamics_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step(shapes, args.once)
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step", "--shapes", args.shapes], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"lstm_dynamics_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"lstm_dynamics_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/lstm_dynamics_bench.py\n" + res.stdout + qr_share(args.shapes.split("/")[0])
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
