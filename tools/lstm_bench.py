"""Numbers of the recurrent learner on one GPU: the recurrence kernels alone (rows x T of one SGD minibatch and of one acting group), ms per roll-out
step and per SGD minibatch step of the LSTM learner, and the mean reward of a short learning run next to the MLP learner's at the same settings.

  python tools/lstm_bench.py [--envs 4096] [--steps 20] [--out FILE.json]

Run it under `rocprofv3 --kernel-trace --stats` to get the recurrence kernels' share of the two phases (k_lstm_fwd / k_lstm_bwd)."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def kernel_times(rows: int, T: int, H: int = 128, reps: int = 20) -> dict:
    from track_mjx_amd.agent.lstm import lstm_seq_bwd, lstm_seq_fwd
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    xg = torch.randn(T, rows, 4 * H, device=dev, generator=g)
    Wh = torch.randn(4 * H, H, device=dev, generator=g) * H ** -0.5
    bh = torch.zeros(4 * H, device=dev)
    h0, c0 = torch.zeros(rows, H, device=dev), torch.zeros(rows, H, device=dev)
    reset = (torch.rand(T, rows, device=dev, generator=g) < 0.05).float()
    dh = torch.randn(T, rows, H, device=dev, generator=g)
    out = lstm_seq_fwd(xg, Wh, bh, h0, c0, reset, train=True)
    lstm_seq_bwd(dh, Wh, out[2], out[1], c0, reset)
    torch.cuda.synchronize()
    res = {}
    for name, fn in (("fwd", lambda: lstm_seq_fwd(xg, Wh, bh, h0, c0, reset, train=True)), ("bwd", lambda: lstm_seq_bwd(dh, Wh, out[2], out[1], c0, reset))):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res[f"{name}_us"] = round(e0.elapsed_time(e1) / reps * 1e3, 1)
    return res


def learner(use_lstm: bool, n: int, groups: int):
    from track_mjx_amd import clips as _clips, config as _config
    from track_mjx_amd.agent import ppo
    from track_mjx_amd.agent.lstm import LSTMPPOLearner
    from track_mjx_amd.environment import wrap
    from track_mjx_amd.train import build_env
    from track_mjx_amd.walker import Rodent
    c = _config.default_config()
    table = _clips.make_synthetic_clips(Rodent(**c["walker_config"]).model, 64, n_frames=c["reference_config"]["clip_length"], mocap_hz=c["env_config"]["env_args"]["mocap_hz"])
    sizes = ppo.group_sizes(n, groups)
    e0 = wrap(build_env(c, sizes[0], "cuda:0", reference_clip=table), episode_length=195)
    envs = [e0] + [wrap(build_env(c, sz, "cuda:0", reference_clip=table, share_clips_with=e0), episode_length=195) for sz in sizes[1:]]
    kw = dict(encoder_layers=(256, 256), decoder_layers=(256, 256), critic_layers=(256, 256), latents=60, unroll_length=20, batch_size=1024 * n // 4096,
              num_minibatches=16, num_updates_per_batch=4, kl_weight=1e-3, entropy_cost=1e-2, learning_rate=1e-4, discounting=0.98, seed=0)
    L = LSTMPPOLearner(envs if len(envs) > 1 else e0, hidden_state_size=128, hidden_layer_num=2, **kw) if use_lstm else ppo.PPOLearner(envs if len(envs) > 1 else e0, **kw)
    gen = torch.Generator().manual_seed(5)
    for k, e in enumerate(envs):
        L.states[k] = e.reset(gen)
    return L


def run(use_lstm: bool, n: int, groups: int, steps: int) -> dict:
    L = learner(use_lstm, n, groups)
    roll, sgd, rewards = [], [], []
    for s in range(steps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        L.collect()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        L.update(s)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        roll.append((t1 - t0) * 1e3 / (L.unrolls * L.T)); sgd.append((t2 - t1) * 1e3 / (L.num_updates * L.num_minibatches))
        rewards.append(float(L.buf["reward"].mean()))
    skip = min(2, steps - 1)       # warm-up steps (allocations, graph capture of the MLP learner)
    med = lambda v: sorted(v[skip:])[len(v[skip:]) // 2]  # noqa: E731
    return {"rollout_step_ms": round(med(roll), 3), "sgd_minibatch_ms": round(med(sgd), 3), "reward_first": round(rewards[0], 4),
            "reward_last5": round(sum(rewards[-5:]) / len(rewards[-5:]), 4), "rewards": [round(r, 4) for r in rewards]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"kernels": {f"{r}x{t}": kernel_times(r, t) for r, t in ((1024, 20), (1368, 1))}}
    if not a.kernels_only:
        res["lstm"] = run(True, a.envs, a.groups, a.steps)
        res["mlp"] = run(False, a.envs, a.groups, a.steps)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
