"""GPU: the recurrent learner (agent/lstm.py) — tmjx_lstm_seq_fwd / _bwd against a float64 restatement of flax's nn.LSTMCell, the policy module
against float64 autograd, the roll-out carry against the loss's sequence pass, training, checkpoints and the CLI switch.

Tolerances are relative to the magnitude of the float64 result (max |a - b| / max |b|): fp32 accumulation over K <= 320 products per gate and
over <= 20 480 rows per weight gradient stays near 1e-6; 1e-4 leaves room for the 20-step recurrence compounding it, nothing more."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parents[1]
TOL = 1e-4


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _ref_layer(xg, Wh, bh, h, c, reset):
    """float64 flax nn.LSTMCell over T steps; the carry is zeroed before step t where reset[t] != 0."""
    H = h.shape[-1]
    hs, cs = [], []
    for t in range(xg.shape[0]):
        keep = (reset[t] == 0).double()[:, None]
        h, c = h * keep, c * keep
        g = xg[t] + h @ Wh.t() + bh
        i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h); cs.append(c)
    return torch.stack(hs), torch.stack(cs)


@pytest.mark.parametrize("rows,T,H", [(1024, 20, 128), (1365, 1, 128), (1000, 20, 128), (17, 7, 128), (300, 5, 64)])
def test_lstm_kernels_match_float64(rows, T, H):
    from track_mjx_amd.agent.lstm import lstm_seq_bwd, lstm_seq_fwd
    from track_mjx_amd.agent.networks import gemm_dw, gemm_nn, gemm_nt
    g = torch.Generator().manual_seed(rows * 31 + T)
    K, Zc = 286, 60                                 # layer 0's input [z | egocentric obs]: only the latent columns are differentiated
    x = torch.randn(T, rows, K, generator=g, dtype=torch.float64)
    Wi = (torch.rand(4 * H, K, generator=g, dtype=torch.float64) * 2 - 1) * (3.0 / K) ** 0.5
    Wh = torch.cat([torch.linalg.qr(torch.randn(H, H, generator=g, dtype=torch.float64))[0] for _ in range(4)])
    bh = torch.randn(4 * H, generator=g, dtype=torch.float64) * 0.1
    h0 = torch.randn(rows, H, generator=g, dtype=torch.float64) * 0.5
    c0 = torch.randn(rows, H, generator=g, dtype=torch.float64) * 0.5
    reset = (torch.rand(T, rows, generator=g) < 0.1).double()
    G = torch.randn(T, rows, H, generator=g, dtype=torch.float64)
    # float64 reference with autograd
    xr, Wir, Whr, bhr, h0r, c0r = (t.clone().requires_grad_(True) for t in (x, Wi, Wh, bh, h0, c0))
    hr, cr = _ref_layer(xr @ Wir.t(), Whr, bhr, h0r, c0r, reset)
    (hr * G).sum().backward()
    # the kernels (+ the GEMM glue the learner uses)
    f = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    xd, Wid, Whd, bhd, h0d, c0d, rd, Gd = map(f, (x, Wi, Wh, bh, h0, c0, reset, G))
    xg = gemm_nt(xd.view(-1, K), Wid).view(T, rows, 4 * H)
    h, c, gates, h_prev = lstm_seq_fwd(xg, Whd, bhd, h0d, c0d, rd, train=True)
    dgates, dh0, dc0 = lstm_seq_bwd(Gd, Whd, gates, c, c0d, rd, want_carry_grad=True)
    dg2 = dgates.view(-1, 4 * H)
    dx = gemm_nn(dg2, Wid, Zc)[:, :Zc]
    dWi, _ = gemm_dw(dg2, xd.view(-1, K), False)
    dWh, db = gemm_dw(dg2, h_prev.view(-1, H), True)
    torch.cuda.synchronize()
    errs = {"h": _rel(h, hr.detach()), "c": _rel(c, cr.detach()), "dW_i": _rel(dWi, Wir.grad), "dW_h": _rel(dWh, Whr.grad), "db": _rel(db, bhr.grad),
            "dx": _rel(dx, xr.grad.view(-1, K)[:, :Zc]), "dh0": _rel(dh0, h0r.grad), "dc0": _rel(dc0, c0r.grad)}
    assert all(np.isfinite(v) and v <= TOL for v in errs.values()), errs


def _ref_policy(pol, obs, h0, c0, reset):
    """float64 restatement of lstm_ppo scan_policy_fn over the module's parameters (Dense -> SiLU -> LayerNorm, z = mean, stacked cells, projection)."""
    P = {n: p.detach().double().cpu().requires_grad_(True) for n, p in pol.named_parameters()}
    x = obs[..., :pol.reference_obs_size]
    for i in range(len(pol.encoder)):
        x = torch.nn.functional.silu(x @ P[f"encoder.{i}.dense.weight"].t() + P[f"encoder.{i}.dense.bias"])
        x = torch.nn.functional.layer_norm(x, (x.shape[-1],), P[f"encoder.{i}.norm.weight"], P[f"encoder.{i}.norm.bias"], 1e-6)
    fc2 = x @ P["fc2.weight"].t() + P["fc2.bias"]
    x = torch.cat([fc2[..., :pol.latents], obs[..., pol.reference_obs_size:]], -1)
    for k in range(pol.hidden_layer_num):
        x = _ref_layer(x @ P[f"w_ih.{k}"].t(), P[f"w_hh.{k}"], P[f"b_hh.{k}"], h0[:, k], c0[:, k], reset)[0]
    return x @ P["projection.weight"].t() + P["projection.bias"], fc2, P


def test_lstm_policy_module_matches_float64_autograd():
    from track_mjx_amd.agent.lstm import LSTMIntentionPolicy
    torch.manual_seed(0)
    W, ref, A, Z, T, B, L, H = 96, 60, 6, 8, 6, 50, 2, 128
    pol = LSTMIntentionPolicy(W, ref, A, Z, (64, 64), H, L).to(DEV)
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(T, B, W, generator=g, dtype=torch.float64)
    h0, c0 = torch.randn(B, L, H, generator=g, dtype=torch.float64) * 0.5, torch.randn(B, L, H, generator=g, dtype=torch.float64) * 0.5
    reset = (torch.rand(T, B, generator=g) < 0.1).double()
    R1, R2 = torch.randn(T, B, 2 * A, generator=g, dtype=torch.float64), torch.randn(T, B, 2 * Z, generator=g, dtype=torch.float64)
    lr, fr, P = _ref_policy(pol, obs, h0, c0, reset)
    ((lr * R1).sum() + (fr * R2).sum()).backward()
    f = lambda t: t.float().to(DEV).contiguous()  # noqa: E731
    logits, fc2 = pol(f(obs), f(h0), f(c0), f(reset))
    grads = torch.autograd.grad((logits * f(R1)).sum() + (fc2 * f(R2)).sum(), list(pol.parameters()))
    assert _rel(logits.detach(), lr.detach()) <= TOL and _rel(fc2.detach(), fr.detach()) <= TOL
    bad = {n: e for (n, _), gd in zip(pol.named_parameters(), grads) if (e := _rel(gd, P[n].grad)) > TOL}
    assert not bad, bad


def _learner(n_groups: int, episode_length: int = 195, n: int = 4096, **kw):
    from track_mjx_amd import clips as _clips, config as _config
    from track_mjx_amd.agent import ppo
    from track_mjx_amd.agent.lstm import LSTMPPOLearner
    from track_mjx_amd.environment import wrap
    from track_mjx_amd.train import build_env
    from track_mjx_amd.walker import Rodent
    c = _config.default_config()
    table = _clips.make_synthetic_clips(Rodent(**c["walker_config"]).model, 16, n_frames=c["reference_config"]["clip_length"], mocap_hz=c["env_config"]["env_args"]["mocap_hz"])
    sizes = ppo.group_sizes(n, n_groups)
    e0 = wrap(build_env(c, sizes[0], DEV, reference_clip=table), episode_length=episode_length)
    envs = [e0] + [wrap(build_env(c, sz, DEV, reference_clip=table, share_clips_with=e0), episode_length=episode_length) for sz in sizes[1:]]
    L = LSTMPPOLearner(envs if len(envs) > 1 else e0, encoder_layers=(256, 256), decoder_layers=(256, 256), critic_layers=(256, 256), latents=60,
                       unroll_length=20, batch_size=1024, num_minibatches=16, num_updates_per_batch=1, kl_weight=1e-3, seed=0, **kw)
    gen = torch.Generator().manual_seed(5)
    for k, e in enumerate(envs):
        L.states[k] = e.reset(gen)
    return L


class _StopUpdate(Exception):
    pass


def _logp_gaps(L, mode: str = "ok") -> torch.Tensor:
    """|target log-prob of the loss's sequence pass - behaviour log-prob of the roll-out| [T, rows] with the learner's CURRENT normaliser and
    parameters.  mode "zero_h0": start every row from a zero carry; "no_reset": ignore the episode ends inside the unroll (controls)."""
    from track_mjx_amd.agent.networks import NormalTanh
    rows = L.buf["discount"].shape[1]
    out = []
    with torch.no_grad():
        for lo in range(0, rows, 1024):
            idx = torch.arange(lo, min(lo + 1024, rows), device=DEV)
            data, obs, logits, _ = L.sequence_outputs(idx, zero_h0=(mode == "zero_h0"))
            if mode == "no_reset":
                logits, _ = L.policy(obs, L.h0_store.index_select(0, idx), L.c0_store.index_select(0, idx), None)
            out.append((NormalTanh.log_prob(logits, data["raw_action"]) - L.buf["log_prob"][:, idx]).abs())
    return torch.cat(out, 1)


def _within(d: torch.Tensor) -> bool:
    return float(d.median()) <= 1e-4 and float(d.max()) <= 1e-2


def test_rollout_carry_matches_loss_sequence_pass():
    """After one training step (a non-zero carry at the unroll start), the loss's sequence pass AS update() RUNS IT — from the stored h0 / c0, with the
    normaliser update() uses, before its first optimiser step — reproduces the behaviour log-probs of the roll-out on every T x B row.  Acting (T = 1
    launches, gemm_nt + tmjx_silu_ln_fwd encoder) and the SGD pass (fused block GEMMs) round differently, and a log-prob sums 38 terms of |.| up to
    ~1e2: median |d| <= 1e-4, max <= 1e-2.  Controls, each of which must break that bound: a zero carry at t = 0 (checked on the t = 0 rows), no
    reset after an episode end (checked on the rows right after one), and the MLP learner's order — the normaliser updated before the SGD epochs."""
    L = _learner(3, episode_length=30)
    L.training_step()
    assert float(L.h_carry.abs().max()) > 0
    L.collect()
    disc = L.buf["discount"]
    assert float((1 - disc).sum()) > 100, "episodes must end inside the unroll"
    seen = {}

    def first_minibatch(idx, kl_w):          # stands in for update()'s first minibatch step: records, then stops update() before any optimiser step
        seen.update(ok=_logp_gaps(L), zero_h0=_logp_gaps(L, "zero_h0"), no_reset=_logp_gaps(L, "no_reset"))
        raise _StopUpdate

    L._lstm_minibatch_grads = first_minibatch
    with pytest.raises(_StopUpdate):
        L.update()
    d_ok = seen["ok"]
    assert _within(d_ok), (float(d_ok.median()), float(d_ok.max()))
    # the controls, row by row where a carry bug would show
    t0 = seen["zero_h0"][0]
    after_reset = torch.zeros_like(disc, dtype=torch.bool)
    after_reset[1:] = disc[:-1] == 0
    assert int(after_reset.sum()) > 100
    assert not _within(seen["zero_h0"]) and float(t0.median()) > 1e-3, float(t0.median())
    assert not _within(seen["no_reset"]) and float(seen["no_reset"][after_reset].median()) > 1e-3, float(seen["no_reset"][after_reset].median())
    # the normaliser-first order of the MLP learner would have the SGD pass read statistics the roll-out did not act with
    L.normalizer.update(L.buf["observation"])
    d_mlp = _logp_gaps(L)
    assert not _within(d_mlp), (float(d_mlp.median()), float(d_mlp.max()))


@pytest.mark.parametrize("groups", [1, 3])
def test_lstm_training_steps_and_checkpoint(groups, tmp_path):
    from track_mjx_amd.agent import checkpoint as ckpt
    from track_mjx_amd.agent.lstm import plain_kl
    L = _learner(groups)
    for it in range(3):
        m = L.training_step(it)
        assert all(np.isfinite(float(v)) for v in m.values()), m
    assert float(L.h_carry.abs().max()) > 0 and float(L.c_carry.abs().max()) > 0
    # the KL term: -0.5 mean(1 + logvar - mean^2 - exp(logvar)) over every row and latent of the minibatch (no AR(1) prior, no schedule), restated here
    # in float64 from the minibatch's fc2; and it is the ONLY latent-KL gradient: d loss / d fc2 at weight w minus at weight 0 (same entropy noise) is
    # w times the plain KL's gradient — a KL left on in the fused head would add its AR(1) term's.  (w = 10: the KL part of the gradient then dwarfs
    # the rounding of the sum it is added to)
    idx = torch.randperm(L.buf["reward"].shape[1], device=DEV)[:L.local_batch]
    noise = torch.randn(L.buf["raw_action"][:, :L.local_batch].shape, device=DEV)
    w = 10.0
    tot1, m1, fc2_1 = L.lstm_loss(idx, w, noise)
    g1 = torch.autograd.grad(tot1, fc2_1)[0]
    tot0, m0, fc2_0 = L.lstm_loss(idx, 0.0, noise)
    g0 = torch.autograd.grad(tot0, fc2_0)[0]
    f = fc2_1.detach().double()
    Z = f.shape[-1] // 2
    mu, lv = f[..., :Z], f[..., Z:]
    want = w * float(-0.5 * torch.mean(1 + lv - mu * mu - torch.exp(lv)))
    assert abs(float(m1[3]) - want) <= 1e-5 * abs(want), (float(m1[3]), want)
    assert float(m0[3]) == 0.0 and torch.equal(fc2_0, fc2_1)
    assert abs(float(m1[0] - m0[0]) - want) <= 1e-4 * abs(want) + 1e-6       # the total carries the same term once
    N = mu.numel()
    dkl = torch.cat([w * mu / N, -0.5 * w * (1 - torch.exp(lv)) / N], -1)
    assert _rel(g1 - g0, dkl) <= 1e-3, _rel(g1 - g0, dkl)
    # checkpoint save -> restore: identical parameters and carry
    L.settle_carry()
    snap = [p.detach().clone() for p in L.params] + [L.h_carry.clone(), L.c_carry.clone()]
    path = tmp_path / "lstm.npz"
    ckpt.save_npz(path, L)
    with torch.no_grad():
        L.opt.flat.zero_(); L.h_carry.zero_(); L.c_carry.fill_(1.0)
    ckpt.load_npz(path, L)
    after = [p.detach() for p in L.params] + [L.h_carry, L.c_carry]
    assert all(torch.equal(a, b) for a, b in zip(snap, after))


def test_cli_use_lstm_trains():
    env = {k: v for k, v in os.environ.items()}
    res = subprocess.run([sys.executable, "-m", "track_mjx_amd.train", "train_setup.train_config.use_lstm=true", "max_training_steps=2",
                          "train_setup.train_config.num_eval_envs=0", "n_synthetic_clips=8"],
                         cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert lines[0].startswith("[train] config=") and lines[1] == "[train] learner=lstm_ppo hidden_state_size=128 hidden_layer_num=2"
    assert any("training/kl_latent_loss" in ln for ln in lines)
