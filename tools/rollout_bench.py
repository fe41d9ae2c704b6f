"""Time a whole-table checkpoint roll-out (track_mjx_amd.analysis.rollout): a policy with random weights and non-trivial normaliser statistics in
the rodent-full-clips network sizes, `--clips` synthetic clips rolled out at once with activations and metrics logged.  Prints one JSON line:
wall time of generate_rollout (first call = with setup, then `--repeats` timed calls), control steps, recorded bytes per env and step.

    python tools/rollout_bench.py --clips 1024 [--config-name rodent-full-clips] [--repeats 1]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/rollout_bench.py --clips 1024 --repeats 0    (the recorder's share of GPU time)
    --sensors: log_sensor_data=True as well (the recording physics kernel k_physics_wave_sensors instead of k_physics_wave)
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--config-name", default="rodent-full-clips")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--sensors", action="store_true", help="log_sensor_data=True (sensor readings and joint forces)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from tests.common import StubEnv
    from track_mjx_amd import config as _config
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.agent.ppo import PPOLearner
    from track_mjx_amd.analysis.rollout import create_environment, create_rollout_generator
    cfg = _config.load_config(None, [f"n_synthetic_clips={args.clips}"], name=args.config_name)
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
    env = create_environment(cfg, 1, "cuda")
    gen = create_rollout_generator(cfg, env, fn, log_activations=True, log_metrics=True, log_sensor_data=args.sensors)
    clips = list(range(args.clips))
    t0 = time.perf_counter()
    r = gen(clips)
    first = time.perf_counter() - t0
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = gen(clips)
        times.append(time.perf_counter() - t0)

    def nbytes(x):
        return sum(nbytes(v) for v in x.values()) if isinstance(x, dict) else (sum(nbytes(v) for v in x) if isinstance(x, tuple) else x.nbytes)
    rec = nbytes({k: v for k, v in r.items() if k != "qposes_ref"})
    steps = gen.T - 1
    print(json.dumps({"clips": args.clips, "config": args.config_name, "sensors": bool(args.sensors), "T": gen.T, "first_call_s": round(first, 3),
                      "timed_s": [round(t, 3) for t in times], "ms_per_control_step": round(1e3 * (min(times) if times else first) / steps, 3),
                      "recorded_bytes_per_env_step": int(rec / args.clips / steps)}), flush=True)


if __name__ == "__main__":
    main()
