"""GPU: training a new encoder on a frozen pretrained decoder (the reference's ppo.train(checkpoint_to_restore=..., freeze_decoder=True),
track_mjx/agent/mlp_ppo/ppo.py:558-617,357-377).  The two launches against the unmasked ones, then end to end through train.main:
pretrain one step, train two frozen steps from it, resume the frozen run."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from track_mjx_amd import hip

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("lo,hi", [(1_000_000, 1_600_000), (800, 800), (0, 4096), (2_500_000 - 4096, 2_500_000), (0, 2_500_000)])
def test_adam_frozen_matches_unmasked_outside_the_range(lo, hi):
    """tmjx_adam_clip_norm_frozen vs tmjx_adam_clip_norm on identical seeded buffers of 2.5 M floats: parameters outside [lo, hi) and both
    moments bit-identical everywhere, parameters inside untouched, the same global norm (over ALL gradients: the clip is active here)."""
    L, dev = hip.lib(), torch.device("cuda:0")
    n = 2_500_000
    g = torch.Generator(device=dev).manual_seed(7)
    p0, grad = torch.randn(n, generator=g, device=dev), torch.randn(n, generator=g, device=dev) * 0.5
    m0, v0 = torch.randn(n, generator=g, device=dev) * 0.1, torch.rand(n, generator=g, device=dev) * 0.01
    out = []
    for frozen in (False, True):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        scratch, norm = torch.empty(L.tmjx_adam_norm_floats(), device=dev), torch.zeros(1, device=dev)
        args = (1e-3, 0.9, 0.999, 1e-8, 1 - 0.9 ** 3, 1 - 0.999 ** 3, 10.0, None)
        if frozen:
            rc = L.tmjx_adam_clip_norm_frozen(_p(p), _p(grad), _p(m), _p(v), _p(scratch), _p(norm), n, lo, hi, *args)
        else:
            rc = L.tmjx_adam_clip_norm(_p(p), _p(grad), _p(m), _p(v), _p(scratch), _p(norm), n, *args)
        assert rc == 0, L.tmjx_last_error()
        torch.cuda.synchronize()
        out.append((p, m, v, norm))
    (pa, ma, va, na), (pb, mb, vb, nb) = out
    assert float(na) > 10.0 and torch.equal(na, nb)
    assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert torch.equal(pa[:lo], pb[:lo]) and torch.equal(pa[hi:], pb[hi:])
    assert torch.equal(pb[lo:hi], p0[lo:hi])
    if hi > lo:
        assert not torch.equal(pa[lo:hi], p0[lo:hi])


@pytest.mark.parametrize("pin_lo", [470, 0, 696])
def test_stats_pinned_matches_unpinned_below_pin_lo(pin_lo):
    """tmjx_stats_apply_pinned vs tmjx_stats_apply: columns below pin_lo bit-identical, columns from pin_lo on untouched, the same count."""
    L, dev = hip.lib(), torch.device("cuda:0")
    W = 696
    g = torch.Generator(device=dev).manual_seed(3)
    sums = torch.randn(2 * W, generator=g, device=dev) * 50
    sums[W:] = sums[W:].abs() * 40
    st0 = {"count": torch.full((), 1000.0, device=dev), "mean": torch.randn(W, generator=g, device=dev),
           "sv": torch.rand(W, generator=g, device=dev) * 900 + 1, "std": torch.rand(W, generator=g, device=dev) + 0.5}
    out = []
    for pinned in (False, True):
        s = {k: v.clone() for k, v in st0.items()}
        ptr = [_p(s[k]) for k in ("count", "mean", "sv", "std")]
        if pinned:
            rc = L.tmjx_stats_apply_pinned(_p(sums), 2048.0, *ptr, W, pin_lo, 1e-6, 1e6, None)
        else:
            rc = L.tmjx_stats_apply(_p(sums), 2048.0, *ptr, W, 1e-6, 1e6, None)
        assert rc == 0, L.tmjx_last_error()
        torch.cuda.synchronize()
        out.append(s)
    a, b = out
    assert torch.equal(a["count"], b["count"]) and float(b["count"]) == 3048.0
    for k in ("mean", "sv", "std"):
        assert torch.equal(a[k][:pin_lo], b[k][:pin_lo]), k
        assert torch.equal(b[k][pin_lo:], st0[k][pin_lo:]), k
        if pin_lo < W:
            assert not torch.equal(a[k][pin_lo:], st0[k][pin_lo:]), k


_BASE = ["train_setup.train_config.num_envs=256", "train_setup.train_config.batch_size=64", "train_setup.train_config.num_minibatches=4",
         "train_setup.train_config.unroll_length=5", "train_setup.train_config.num_updates_per_batch=2", "train_setup.train_config.num_timesteps=6400",
         "train_setup.eval_every=640", "train_setup.reset_every=640", "n_synthetic_clips=4", "train_setup.train_config.num_eval_envs=0"]
_VARIANTS = {"64": ["network_config.encoder_layer_sizes=[64,64]", "network_config.decoder_layer_sizes=[64,64]", "network_config.critic_layer_sizes=[64,64]"],
             "2x256": ["network_config.encoder_layer_sizes=[256,256]", "network_config.decoder_layer_sizes=[256,256]",
                       "network_config.critic_layer_sizes=[256,256]"]}
_VARIANTS["2x256-bf16"] = _VARIANTS["2x256"] + ["mlp_gemm_inputs=bf16"]


def _policy(step_dir):
    with np.load(os.path.join(step_dir, "policy.npz")) as z:
        return {k: z[k] for k in z.files}


def _check_frozen(pre, run_dir, steps, ref):
    dec = {k: v for k, v in pre.items() if k.startswith("1/params/decoder/")}
    assert len(dec) >= 5
    for s in steps:
        got = _policy(os.path.join(run_dir, str(s)))
        for k, v in dec.items():
            assert np.array_equal(got[k], v), (s, k)
        for k in ("mean", "summed_variance", "std"):
            assert np.array_equal(got[f"0/{k}"][ref:], pre[f"0/{k}"][ref:]), (s, k)
    return dec


def _losses(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("[train] steps=")]
    vals = [float(v) for ln in lines for k, v in re.findall(r"(training/\w+_loss)=(\S+)", ln)]
    assert lines and vals
    return vals


@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_train_frozen_decoder_end_to_end(tmp_path, capsys, variant):
    """train.main: pretrain one step into a checkpoint, then two steps with train_setup.checkpoint_to_restore + train_setup.freeze_decoder:
    in every saved step of the frozen run the decoder and head are bit-equal to the pretrained ones, so is the normaliser's proprioceptive
    tail; the encoder moves, every loss is finite, the log names what was frozen.  Variants: 64-wide layers (fp32 layer path), 2 x 256 fp32
    (the chain kernels), 2 x 256 with bf16 GEMM inputs."""
    from track_mjx_amd import train
    base = _BASE + _VARIANTS[variant]
    pre_dir, run_dir = tmp_path / "pre", tmp_path / "frozen"
    train.main(base + [f"checkpoint_path={pre_dir}", "max_training_steps=1"])
    assert sorted(int(x) for x in os.listdir(pre_dir)) == [0, 1]
    pre = _policy(pre_dir / "1")
    ref = pre["1/params/encoder/hidden_0/kernel"].shape[0]
    W = pre["0/mean"].shape[-1]
    capsys.readouterr()
    train.main(base + [f"checkpoint_path={run_dir}", f"train_setup.checkpoint_to_restore={pre_dir}", "train_setup.freeze_decoder=true",
                       "max_training_steps=2", "train_setup.train_config.seed=5"])
    log = capsys.readouterr().out
    m = re.search(r"\[train\] freeze_decoder checkpoint=\S+ step=1 frozen_params=(\d+) pinned_obs_columns=\[(\d+), (\d+)\)", log)
    assert m, log
    assert (int(m.group(2)), int(m.group(3))) == (ref, W)
    dec = _check_frozen(pre, run_dir, [0, 1, 2], ref)
    assert int(m.group(1)) == sum(v.size for v in dec.values())
    assert all(np.isfinite(v) for v in _losses(log))
    first, last = _policy(run_dir / "0"), _policy(run_dir / "2")
    assert not np.array_equal(first["1/params/encoder/hidden_0/kernel"], last["1/params/encoder/hidden_0/kernel"])
    # a fresh run: the iteration and env_steps start at 0, the optimiser state is this run's own
    with np.load(run_dir / "2" / "train_state.npz") as z:
        assert int(z["iteration"]) == 2 and int(z["env_steps"]) == 2 * 64 * 4 * 5 and int(z["optimizer_state/count"]) == 2 * 2 * 4
    # the normaliser's count is not pinned: it grew from 0 with the rows seen
    assert float(last["0/count"]) == 2 * 5 * 256
    if variant == "64":
        # resume the frozen run: the whole state comes back, the decoder stays the pretrained one
        capsys.readouterr()
        train.main(base + [f"checkpoint_path={run_dir}", f"restore_from={run_dir}", "train_setup.freeze_decoder=true", "max_training_steps=1",
                           "train_setup.train_config.seed=5"])
        log = capsys.readouterr().out
        assert "[train] freeze_decoder checkpoint=" in log and " step=2 " in log
        assert sorted(int(x) for x in os.listdir(run_dir)) == [0, 1, 2, 3]
        _check_frozen(pre, run_dir, [3], ref)
        assert all(np.isfinite(v) for v in _losses(log))
        assert not np.array_equal(_policy(run_dir / "3")["1/params/encoder/hidden_0/kernel"], last["1/params/encoder/hidden_0/kernel"])
