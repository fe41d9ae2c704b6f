"""Cost of per-env domain randomisation on the env roll-out: env.step of `--envs` envs (one launch of the physics kernel per control step + K3),
the same handle in each of `--modes` — `plain` (no table: k_physics_wave), `scales` (uniformly drawn per-env friction / actuator / damping
scales: k_physics_wave_rand, csrc/tmjx_wave_rand.hip), `gravity` (a drawn per-env gravity table alone), `both` — alternating, `--repeats` times
each, `--steps` control steps per repeat timed with HIP events on the launch stream after `--warmup` steps.  Prints one JSON line with every
mode's env-steps/s (median of the repeats), every repeat's, and the spread (max - min) / median of each mode's repeats.  A library from before
the gravity table (TMJX_SO=<its path>) runs `--modes plain,scales`.

    python tools/rand_rollout_bench.py [--envs 4096] [--steps 40] [--warmup 5] [--repeats 3] [--scale 0.3] [--modes plain,scales,gravity,both]
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
    ap.add_argument("--modes", default="plain,scales,gravity,both", help="comma list of plain | scales | gravity | both, run in this order, alternating")
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    if not modes or set(modes) - {"plain", "scales", "gravity", "both"}:
        ap.error("--modes: a comma list of plain, scales, gravity, both")
    import torch
    from tests.common import make_env_and_oracle
    from track_mjx_amd.environment import DomainRandomization, uniform_scales
    n = args.envs
    env, _, _ = make_env_and_oracle(num_envs=n, n_clips=4, wrappers=True)
    ranges = dict(friction=(0.5, 1.5), actuator=(0.7, 1.3), damping=(0.5, 2.0))
    both = uniform_scales(n, 0, **ranges, gravity_scale=(0.5, 1.5), gravity_tilt_deg=(0.0, 15.0))
    tables = {"plain": None, "scales": uniform_scales(n, 0, **ranges), "gravity": DomainRandomization(gravity=both.gravity), "both": both}
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
    reps = {m: [] for m in modes}
    for _ in range(args.repeats):
        for m in modes:
            reps[m].append(run(tables[m]))
    out = {"envs": n, "steps": args.steps, "action_scale": args.scale}
    for m in modes:
        med = statistics.median(reps[m])
        out[f"{m}_env_steps_per_s"] = round(med)
        out[f"{m}_repeats"] = [round(x) for x in reps[m]]
        out[f"{m}_spread"] = round((max(reps[m]) - min(reps[m])) / med, 4)
        if m != "plain" and "plain" in reps:
            out[f"{m}_over_plain"] = round(med / statistics.median(reps["plain"]), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
