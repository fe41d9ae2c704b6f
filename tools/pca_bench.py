#!/usr/bin/env python3
"""Times of the GPU PCA (track_mjx_amd/analysis/pca.py) and of the progression panel, with sklearn and matplotlib on the host for context.

  fit     fit + transform (k = 4) of 210 000 x 60 and 210 000 x 128 float32 rows: moments (two passes with their reductions) and Jacobi from the
          device events tmjx_pca_fit records, the transform between two device events over LOOPS calls; median of 5 repeats, the shapes alternating
  panel   the panel of 250 frames at 640 x 480, k = 4, window 530: tmjx_plot_strips per 64 frames between two device events, and
          plot_pca_progression end to end (with the copy of the frames to the host) by the host clock
  host    sklearn.decomposition.PCA(svd_solver="full") fit + transform at the same shapes and one matplotlib figure per frame over a pool of 16
          processes, where they import: context, not a comparison of like with like

  wide    the wide fit (tmjx_pca_fit_wide: block Jacobi, 129 <= d <= 1024) + transform (k = 4) of 210 000 x 256, x 512 and x 1024: moments and
          the block iteration from the call's device events, the transform between two device events; the generator's spectrum (decay 0.7) and, at
          1024, a slowly decaying one (0.98); then sklearn's full SVD on the host at the same shapes where it imports.  Not one of the default
          steps; it writes its own file, profiles/pca_wide_bench.txt (--wide-out)

usage: python tools/pca_bench.py [--out profiles/pca_bench.txt] [--steps fit,panel,host] [--wide-out profiles/pca_wide_bench.txt]
Every step is a child process under its own time limit; a step that fails or runs out of time ends the run.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

N, DS, K, REPEATS, LOOPS = 210_000, (60, 128), 4, 5, 20
FRAMES, PW, PH, WINDOW = 250, 640, 480, 530
LIMITS = {"fit": 300, "panel": 200, "host": 400, "wide": 300, "widehost": 400}
WIDE, WIDE_REPEATS, WIDE_LOOPS = ((256, 0.7), (512, 0.7), (1024, 0.7), (1024, 0.98)), 3, 5      # (d, decay of the spectrum)


def med(v):
    return f"{statistics.median(v):9.3f} ms  ({min(v):.3f} .. {max(v):.3f})"


def data(d, torch, decay=0.7):
    g = torch.Generator(device="cuda").manual_seed(d)
    z = torch.randn((N, d), generator=g, device="cuda") * (decay ** torch.arange(d, device="cuda")).sqrt()
    q, _ = torch.linalg.qr(torch.randn((d, d), generator=g, device="cuda"))
    return (z @ q.T + 3.0).contiguous()


def step_fit():
    import torch
    from track_mjx_amd import hip
    from track_mjx_amd.analysis import pca as P
    xs = {d: data(d, torch) for d in DS}
    t = {d: {"moments": [], "jacobi": [], "transform": [], "fit + transform": []} for d in DS}
    sweeps = {}
    for d in DS:                                   # warm-up of every shape
        P.PCA(K).fit_transform(xs[d])
    torch.cuda.synchronize()
    for _ in range(REPEATS):
        for d in DS:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            p = P.PCA(K).fit(xs[d])
            e[1].record()
            p.transform(xs[d])
            e[2].record()
            for _ in range(LOOPS):
                p._b.transform(xs[d], p.mean_, p.components_)
            e[3].record()
            e[3].synchronize()
            t[d]["moments"].append(p.moments_ms_); t[d]["jacobi"].append(p.jacobi_ms_)
            t[d]["transform"].append(e[2].elapsed_time(e[3]) / LOOPS)
            t[d]["fit + transform"].append(e[0].elapsed_time(e[2]))
            sweeps[d] = p.n_sweeps_
    print(f"# fit: {N} rows, k = {K}, median of {REPEATS} alternating repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    for d in DS:
        for what, v in t[d].items():
            note = f"  {sweeps[d]} sweeps" if what == "jacobi" else ("  (with allocation, the copies of the result and the call's wait)" if "+" in what else "")
            print(f"{N} x {d:<3d} {what:16s} {med(v)}{note}")
        flop, byts = 2.0 * N * d * d, 2.0 * 4 * N * d
        m = statistics.median(t[d]["moments"]) * 1e-3
        print(f"{N} x {d:<3d} moments: {flop / m / 1e12:.2f} TFLOP/s of Gram FMAs, {byts / m / 1e9:.0f} GB/s of x read twice")


def step_wide():
    import torch
    from track_mjx_amd import hip
    from track_mjx_amd.analysis import pca as P
    print(f"# wide fit: {N} rows, k = {K}, median of {WIDE_REPEATS} repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    for d, decay in WIDE:
        x = data(d, torch, decay)
        P.PCA(K).fit_transform(x)                  # warm-up
        torch.cuda.synchronize()
        t = {"moments": [], "block iteration": [], "transform": [], "fit + transform": []}
        for _ in range(WIDE_REPEATS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            p = P.PCA(K).fit(x)
            e[1].record()
            p.transform(x)
            e[2].record()
            for _ in range(WIDE_LOOPS):
                p._b.transform_wide(x, p.mean_, p.components_)
            e[3].record()
            e[3].synchronize()
            t["moments"].append(p.moments_ms_); t["block iteration"].append(p.jacobi_ms_)
            t["transform"].append(e[2].elapsed_time(e[3]) / WIDE_LOOPS)
            t["fit + transform"].append(e[0].elapsed_time(e[2]))
        tag = f"{N} x {d:<4d} decay {decay:<4}"
        for what, v in t.items():
            note = f"  {p.n_block_sweeps_} block sweeps, off / norm {p.off_rel_:.1e}" if what == "block iteration" else (
                "  (with allocation, the copies of the result and the call's waits)" if "+" in what else "")
            print(f"{tag} {what:16s} {med(v)}{note}")
        m = statistics.median(t["moments"]) * 1e-3
        print(f"{tag} moments: {N * d * (d + 128.0) / m / 1e12:.2f} TFLOP/s of Gram FMAs (the tiles with j >= i)")
        del x, p
        torch.cuda.empty_cache()


def step_widehost():
    import numpy as np
    print("# host, 16 CPUs, for context")
    try:
        from sklearn.decomposition import PCA
    except ImportError:
        print("sklearn does not import: not measured")
        return
    for d, decay in WIDE:
        x = (np.random.default_rng(d).standard_normal((N, d), dtype=np.float32) * np.sqrt(decay ** np.arange(d)).astype(np.float32) + np.float32(3.0))
        t0 = time.perf_counter()
        PCA(K, svd_solver="full").fit(x).transform(x)
        print(f"sklearn PCA(svd_solver='full') fit + transform {N} x {d:<4d} decay {decay:<4} {(time.perf_counter() - t0) * 1e3:9.0f} ms  (one run)", flush=True)


def step_panel():
    import ctypes as C
    import numpy as np
    import torch
    from track_mjx_amd import hip
    from track_mjx_amd.analysis import pca as P
    from track_mjx_amd.analysis import render as R
    rng = np.random.default_rng(0)
    proj = np.cumsum(rng.standard_normal((FRAMES, K)).astype(np.float32) * 0.2, 0)
    idx = np.arange(FRAMES)
    b, L, st = P.HipBackend("cuda"), hip.lib(), P.strip_style(PW, PH)
    pd, fi, fl = b.asarray(proj), torch.as_tensor(idx.astype(np.int32), device="cuda"), torch.zeros(FRAMES, dtype=torch.uint8, device="cuda")
    out = torch.empty((R.MAX_FRAMES_PER_CALL, PH, PW, 4), dtype=torch.uint8, device="cuda")

    def run():
        for i in range(0, FRAMES, R.MAX_FRAMES_PER_CALL):
            n = min(R.MAX_FRAMES_PER_CALL, FRAMES - i)
            hip.check(L.tmjx_plot_strips(pd.data_ptr(), FRAMES, K, K, fi[i:].data_ptr(), fl[i:].data_ptr(), n, float(proj.min()) - 0.2, float(proj.max()) + 0.2,
                                         WINDOW, C.byref(st), PW, PH, out.data_ptr(), None), "tmjx_plot_strips")
    run()
    R.plot_pca_progression(proj, idx, K, WINDOW, (PW, PH))
    torch.cuda.synchronize()
    dev, e2e = [], []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LOOPS):
            run()
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) / LOOPS)
        t0 = time.perf_counter()
        R.plot_pca_progression(proj, idx, K, WINDOW, (PW, PH))
        e2e.append((time.perf_counter() - t0) * 1e3)
    print(f"# panel: {FRAMES} frames at {PW} x {PH}, k = {K}, window {WINDOW}; median of {REPEATS} repeats (min .. max)")
    print(f"tmjx_plot_strips, device       {med(dev)}  {FRAMES / statistics.median(dev) * 1e3:.0f} panels/s")
    print(f"plot_pca_progression, to host  {med(e2e)}  {FRAMES / statistics.median(e2e) * 1e3:.0f} panels/s")


def _figure(i):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    proj = np.cumsum(np.random.default_rng(0).standard_normal((FRAMES, K)) * 0.2, 0)
    fig = plt.figure(figsize=(6.4, 4.8))
    for c in range(K):
        plt.plot(proj[:i, c], label=f"PC {c}")
        plt.scatter(i, proj[i - 1, c])
    plt.xlim(0, WINDOW); plt.ylim(proj.min() - 0.2, proj.max() + 0.2); plt.legend(loc="upper right"); plt.xlabel("Timestep")
    canvas = FigureCanvasAgg(fig)
    canvas.draw()
    n = len(canvas.buffer_rgba())
    plt.close(fig)
    return n


def step_host():
    import multiprocessing as mp
    import numpy as np
    print("# host, 16 CPUs, for context")
    try:
        from sklearn.decomposition import PCA
        for d in DS:
            x = (np.random.default_rng(d).standard_normal((N, d)) * np.sqrt(0.7 ** np.arange(d)) + 3.0).astype(np.float32)
            PCA(K, svd_solver="full").fit(x[:1000])
            v = []
            for _ in range(3):
                t0 = time.perf_counter()
                PCA(K, svd_solver="full").fit(x).transform(x)
                v.append((time.perf_counter() - t0) * 1e3)
            print(f"sklearn PCA(svd_solver='full') fit + transform {N} x {d:<3d} {med(v)}")
    except ImportError:
        print("sklearn does not import: not measured")
    try:
        import matplotlib  # noqa: F401
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(_figure, range(1, 17))                      # every worker has imported matplotlib
            t0 = time.perf_counter()
            pool.map(_figure, range(1, FRAMES + 1))
            dt = (time.perf_counter() - t0) * 1e3
        print(f"matplotlib, one figure per frame, pool of 16: {FRAMES} frames at 640 x 480 in {dt:.0f} ms  {FRAMES / dt * 1e3:.0f} panels/s")
    except ImportError:
        print("matplotlib does not import: not measured")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pca_bench.txt"))
    ap.add_argument("--steps", default="fit,panel,host")
    ap.add_argument("--wide-out", default=str(ROOT / "profiles" / "pca_wide_bench.txt"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        if args.step not in ("host", "widehost"):
            import torch
            if not torch.cuda.is_available():
                print("pca_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
                return 1
        {"fit": step_fit, "panel": step_panel, "host": step_host, "wide": step_wide, "widehost": step_widehost}[args.step]()
        return 0
    text, wide_text = "# tools/pca_bench.py\n", "# tools/pca_bench.py --steps wide\n"
    steps = [c for s in args.steps.split(",") for c in (("wide", "widehost") if s == "wide" else (s,))]
    for s in steps:
        try:
            res = subprocess.run([sys.executable, __file__, "--step", s], capture_output=True, text=True, timeout=LIMITS[s])
        except subprocess.TimeoutExpired:
            print(f"pca_bench: step {s} ran past its {LIMITS[s]} s limit; stopping", file=sys.stderr)
            return 1
        if res.returncode != 0:
            print(f"pca_bench: step {s} failed ({res.returncode}); stopping\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
            return 1
        if s.startswith("wide"):
            wide_text += res.stdout
        else:
            text += res.stdout
    if any(not s.startswith("wide") for s in steps):
        Path(args.out).write_text(text)
        print(text, end="")
    if any(s.startswith("wide") for s in steps):
        Path(args.wide_out).write_text(wide_text)
        print(wide_text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
