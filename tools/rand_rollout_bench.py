"""Cost of per-env domain randomisation on the env roll-out: env.step of `--envs` envs (one launch of the physics kernel per control step + K3),
the same handle WITHOUT scales (k_physics_wave) and WITH uniformly drawn per-env scales (k_physics_wave_rand, csrc/tmjx_wave_rand.hip),
alternating, `--repeats` times each, `--steps` control steps per repeat timed with HIP events on the launch stream after `--warmup` steps.
Prints one JSON line with both env-steps/s figures (median of the repeats) and every repeat's.

    python tools/rand_rollout_bench.py [--envs 4096] [--steps 40] [--warmup 5] [--repeats 3] [--scale 0.3]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=0.3, help="standard deviation of the (clipped) normal actions")
    args = ap.parse_args()
    import torch
    from tests.common import make_env_and_oracle
    from track_mjx_amd.environment import uniform_scales
    n = args.envs
    env, _, _ = make_env_and_oracle(num_envs=n, n_clips=4, wrappers=True)
    dr = uniform_scales(n, 0, friction=(0.5, 1.5), actuator=(0.7, 1.3), damping=(0.5, 2.0))
    g = torch.Generator().manual_seed(0)
    acts = [(torch.randn((38, n), generator=g) * args.scale).clamp(-1, 1).to(env.device) for _ in range(8)]

    def run(scales):
        env.set_domain_randomization(scales)
        st = env.reset(torch.Generator().manual_seed(1))
        for t in range(args.warmup):
            st = env.step(st, acts[t % len(acts)])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for t in range(args.steps):
            st = env.step(st, acts[t % len(acts)])
        e1.record()
        torch.cuda.synchronize()
        return n * args.steps / (e0.elapsed_time(e1) * 1e-3)
    plain, rand = [], []
    for _ in range(args.repeats):
        plain.append(run(None)); rand.append(run(dr))
    print(json.dumps({"envs": n, "steps": args.steps, "action_scale": args.scale, "plain_env_steps_per_s": round(statistics.median(plain)),
                      "rand_env_steps_per_s": round(statistics.median(rand)), "rand_over_plain": round(statistics.median(rand) / statistics.median(plain), 4),
                      "plain_repeats": [round(x) for x in plain], "rand_repeats": [round(x) for x in rand]}), flush=True)


if __name__ == "__main__":
    main()
