#!/usr/bin/env python3
"""Frames per second of the roll-out renderer (track_mjx_amd/analysis/render.py) on a 250-frame synthetic clip with the ghost, at 640 x 480 and at
152 x 113, camera close_profile: the median of 5 repeats with their spread, the repeats of all variants alternating.  One timed repeat is the whole
clip through Renderer.render_device (tmjx_render per chunk of frames, rgba only), LOOPS times over so that the window is a third of a second,
between two device events, after a warm-up of every shape.

usage: python tools/render_bench.py [--variant name=<path to an alternative build of libtmjx_hip.so>]... [--out profiles/render_bench.txt]
A variant is another build of the library timed in the same process (e.g. the 8 x 8 wave tile: TMJX_EXTRA_HIPCC_FLAGS=-DTMJX_RENDER_TILE_X=8);
its pixels are compared bit for bit with the product build's before anything is timed.
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from track_mjx_amd import clips as _clips  # noqa: E402
from track_mjx_amd import config as _config  # noqa: E402
from track_mjx_amd import hip  # noqa: E402
from track_mjx_amd import walker as _walker  # noqa: E402
from track_mjx_amd.analysis import render as R  # noqa: E402

SIZES = ((640, 480), (152, 113))
LOOPS = {(640, 480): 8, (152, 113): 80}      # passes over the clip per timed repeat
FRAMES, REPEATS = 250, 5


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", action="append", default=[])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "render_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("render_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
        return 1
    w = _walker.Rodent(**_config.default_config()["walker_config"])
    clip = _clips.make_synthetic_clips(w.model, 2, n_frames=FRAMES, seed=0)
    qpos = np.concatenate([clip.position, clip.quaternion, clip.joints], -1).astype(np.float32)
    q, g = torch.from_numpy(qpos[0]).cuda(), torch.from_numpy(qpos[1]).cuda()
    g[:, 0:3] = q[:, 0:3] + torch.tensor([0.02, 0.03, 0.0], device="cuda")
    libs = [("product", hip.lib())] + [(v.split("=", 1)[0], hip.load(Path(v.split("=", 1)[1]))) for v in args.variant]
    lines = [f"# tools/render_bench.py: {FRAMES}-frame synthetic clip with ghost, camera close_profile, rgba only; frames per second, median of {REPEATS} "
             f"alternating repeats (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}"]

    def run(r):
        for i in range(0, FRAMES, R.MAX_FRAMES_PER_CALL):
            r.render_device(q[i:i + R.MAX_FRAMES_PER_CALL], g[i:i + R.MAX_FRAMES_PER_CALL], depth=False, ids=False)

    for W, H in SIZES:
        rs = [(name, R.Renderer(w, "cuda", height=H, width=W, lib=L)) for name, L in libs]
        base = None
        for name, r in rs:      # same pixels, ids and depths from every variant before any timing (and the warm-up of this shape)
            out = [x.cpu() for x in r.render_device(q[:8], g[:8])]
            base = out if base is None else base
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(out, base))
            if not same:
                lines.append(f"{W}x{H} {name}: OUTPUT DIFFERS from product")
            run(r)
        torch.cuda.synchronize()
        fps = {name: [] for name, _ in rs}
        for _ in range(REPEATS):
            for name, r in rs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LOOPS[(W, H)]):
                    run(r)
                e1.record()
                e1.synchronize()
                fps[name].append(LOOPS[(W, H)] * FRAMES / (e0.elapsed_time(e1) * 1e-3))
        for name, v in fps.items():
            lines.append(f"{W}x{H} {name:10s} {statistics.median(v):10.1f} fps  ({min(v):.1f} .. {max(v):.1f})  "
                         f"{statistics.median(v) * W * H * r.info(1, True).nprim / 1e9:.2f} G ray-primitive tests/s")
    text = "\n".join(lines) + "\n"
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
