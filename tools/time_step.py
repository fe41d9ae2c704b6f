#!/usr/bin/env python3
"""Time tmjx_step (K2+K3 fused launch) at a given env count; prints env-steps/s. Used for kernel tuning.

--walker torque|position|both: the rodent-sps-per-actor configuration with the torque / 0.9 walker, the position-actuator / 0.8 walker
(affine actuator bias), or both built in this process and timed in alternating rounds (--rounds) with the same actions."""
import argparse
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tests.common import make_env_and_oracle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--blocks", type=str, default="")
    ap.add_argument("--walker", choices=("torque", "position", "both"), default=None)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.walker:
        return walkers(args)
    for blk in ([int(b) for b in args.blocks.split(",")] if args.blocks else [None]):
        if blk:
            os.environ["TMJX_BLOCK"] = str(blk)
        env, _, _ = make_env_and_oracle(num_envs=args.envs, n_clips=64, wrappers=True)
        g = torch.Generator().manual_seed(0)
        st = env.reset(g)
        acts = [(torch.randn((38, args.envs), generator=g) * args.scale).clamp(-1, 1).cuda() for _ in range(4)]
        for i in range(2):
            st = env.step(st, acts[i % 4])
        torch.cuda.synchronize()
        t0 = time.time()
        for i in range(args.steps):
            st = env.step(st, acts[i % 4])
        torch.cuda.synchronize()
        dt = (time.time() - t0) / args.steps
        print(f"block={blk} envs={args.envs} ms/step={dt * 1e3:.2f} env-steps/s={args.envs / dt:.0f} done_frac={st.done.mean().item():.3f}", flush=True)
        del env


def walker_env(kind, n):
    from track_mjx_amd import clips as _clips
    from track_mjx_amd import config as _config
    from track_mjx_amd.environment import MultiClipTracking, RewardConfig, wrap
    from track_mjx_amd.walker import Rodent
    ov = ["walker_config.torque_actuators=false", "walker_config.rescale_factor=0.8"] if kind == "position" else []
    cfg = _config.load_config(name="rodent-sps-per-actor", overrides=ov)
    w = Rodent(**cfg["walker_config"])
    cl = _clips.make_synthetic_clips(w.model, 64, seed=0)
    env = MultiClipTracking(cl, w, RewardConfig(**cfg["env_config"]["reward_weights"]), **cfg["env_config"]["env_args"], **cfg["reference_config"],
                            num_envs=n, device="cuda:0")
    print(w.describe(), flush=True)
    return wrap(env, episode_length=195)


def walkers(args):
    kinds = ["torque", "position"] if args.walker == "both" else [args.walker]
    envs = {k: walker_env(k, args.envs) for k in kinds}
    g = torch.Generator().manual_seed(0)
    acts = [(torch.randn((38, args.envs), generator=g) * args.scale).clamp(-1, 1).cuda() for _ in range(4)]
    sts = {}
    for k, env in envs.items():
        sts[k] = env.reset(torch.Generator().manual_seed(0))
        for i in range(2):
            sts[k] = env.step(sts[k], acts[i % 4])
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for k, env in envs.items():
            st = sts[k]
            t0 = time.time()
            for i in range(args.steps):
                st = env.step(st, acts[i % 4])
            torch.cuda.synchronize()
            dt = (time.time() - t0) / args.steps
            sts[k] = st
            print(f"round={r} walker={k} envs={args.envs} ms/step={dt * 1e3:.3f} env-steps/s={args.envs / dt:.0f} done_frac={st.done.mean().item():.3f}",
                  flush=True)


if __name__ == "__main__":
    main()
