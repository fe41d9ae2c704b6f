#!/usr/bin/env python3
"""What one tmjx_intervene launch costs a roll-out control step: 1024 clips of the default configuration (rodent-full-clips network sizes, random
weights), the policy step's launch list + tmjx_step, with and without a K = 16 subspace intervention on the widest layer.

Both launch lists are built on the same env from the same build and timed in alternating blocks of STEPS control steps between two device
events (REPEATS blocks each, after a warm-up block of each); the recorder's two launches per step are not part of either.  The physics state
moves on between blocks, the same for both.  Writes the two per-step times, their spread and the difference to profiles/intervene_bench.txt.

usage: python tools/intervene_bench.py [--clips 1024] [--out profiles/intervene_bench.txt]
The measurement runs in one child process under its own time limit; the timings are recorded, not asserted.
"""
import argparse
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

K, STEPS, REPEATS, LIMIT = 16, 25, 8, 400


def med(v):
    return f"{statistics.median(v):9.2f} us  ({min(v):.2f} .. {max(v):.2f})"


def step(n: int):
    import numpy as np
    import torch
    from tests.common import StubEnv
    from track_mjx_amd import config as _config
    from track_mjx_amd import hip
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.agent.ppo import PPOLearner
    from track_mjx_amd.analysis.intervene import Intervention
    from track_mjx_amd.analysis.rollout import _PolicyStep, create_environment, reset_inputs
    cfg = _config.load_config(None, [f"n_synthetic_clips={n}"], name="rodent-full-clips")
    nc = cfg["network_config"]
    ln = PPOLearner(StubEnv(512), encoder_layers=nc["encoder_layer_sizes"], decoder_layers=nc["decoder_layer_sizes"], critic_layers=[64, 64],
                    latents=nc["intention_size"], unroll_length=4, batch_size=256, num_minibatches=8, num_updates_per_batch=1, use_graph=False, seed=3)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        ln.normalizer.mean.copy_(torch.randn(ln.normalizer.mean.shape, generator=g) * 0.3)
        ln.normalizer.std.copy_(0.4 + torch.rand(ln.normalizer.std.shape, generator=g))
    with tempfile.TemporaryDirectory() as d:
        ck.save_step_dir(d, 0, ln, config=cfg)
        fn = ck.load_inference_fn(cfg, ck.load_policy(d, cfg))
    env = create_environment(cfg, n, "cuda")
    nq, nv = int(env.layout.nq), int(env.layout.nv)
    qn, vn = np.empty((nq, n), np.float32), np.empty((nv, n), np.float32)
    for j in range(n):
        _, qn[:, j], vn[:, j] = reset_inputs(42, env._n_clips, nq, nv, env._reset_noise_scale, j)
    env.reset(None, torch.arange(n, dtype=torch.int32), start_frame=torch.zeros(n, dtype=torch.int32), qpos_noise=torch.from_numpy(qn),
              qvel_noise=torch.from_numpy(vn))
    plain = _PolicyStep(fn, n, env.obs_buf)
    widths = {f"{part}/{k}": v[2] for part in ("encoder", "decoder") for k, v in plain.acts[part].items() if k.startswith("layer_")}
    target = max(widths, key=widths.get)
    w = widths[target]
    iv = Intervention(target, "subspace", directions=np.random.default_rng(0).standard_normal((K, w)), gain=0.5, offset=0.1)
    edited = _PolicyStep(fn, n, env.obs_buf, intervention=iv, gates=iv.per_clip(n))
    L, p = hip.lib(), lambda t: t.data_ptr()      # noqa: E731
    print(f"# control step of {n} clips, rodent-full-clips (encoder {nc['encoder_layer_sizes']}, decoder {nc['decoder_layer_sizes']}): launch list + tmjx_step, "
          f"per step over blocks of {STEPS} steps, median of {REPEATS} alternating blocks (min .. max); build {hip.build_id()}, {torch.cuda.get_device_name(0)}")
    print(f"# intervention: K = {K} subspace on {target} (w = {w}), every row ON; launches per step: {len(plain.ll.calls) + 2} and {len(edited.ll.calls) + 2}")

    def block(st):
        args = [p(env.state_buf), p(env.istate_buf), p(st.action_t), p(env.obs_buf), p(env.reward_buf), p(env.done_buf), p(env.trunc_buf), p(env.metrics_buf),
                p(env.workspace), n]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(STEPS):
            st.launch(t)
            hip.check(L.tmjx_step(env._handle, *args, st.stream), "tmjx_step")
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / STEPS

    block(plain); block(edited)                     # warm-up
    t = {"without": [], "with": []}
    for _ in range(REPEATS):
        t["without"].append(block(plain))
        t["with"].append(block(edited))
    for k, v in t.items():
        print(f"{k:8s} intervention {med(v)}")
    diff = [b - a for a, b in zip(t["without"], t["with"])]
    print(f"difference (with - without, block by block) {med(diff)}", flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "intervene_bench.txt"))
    ap.add_argument("--step", action="store_true", help="(internal) run the measurement in this process")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            print("intervene_bench: no GPU (a timing needs the device; nothing is measured on the CPU)", file=sys.stderr)
            return 1
        step(args.clips)
        return 0
    try:
        res = subprocess.run([sys.executable, __file__, "--step", "--clips", str(args.clips)], capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        print(f"intervene_bench: ran past its {LIMIT} s limit; stopping", file=sys.stderr)
        return 1
    if res.returncode != 0:
        print(f"intervene_bench: failed ({res.returncode})\n{res.stdout}{res.stderr[-3000:]}", file=sys.stderr)
        return 1
    text = "# tools/intervene_bench.py\n" + res.stdout
    Path(args.out).write_text(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
