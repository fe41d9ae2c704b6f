"""CPU: training a new encoder on a frozen pretrained decoder (the reference's ppo.train(checkpoint_to_restore=..., freeze_decoder=True),
track_mjx/agent/mlp_ppo/ppo.py:558-617,357-377; CLI keys train_setup.checkpoint_to_restore / train_setup.freeze_decoder, train.py:306-314).

The C-ABI refusals of the two new launches (tmjx_adam_clip_norm_frozen, tmjx_stats_apply_pinned) without a device, the learner's torch branch
(the same rule as the kernels: global norm over every gradient, Adam moments everywhere, no parameter update in the decoder's range, the
normaliser's proprioceptive columns pinned) against a float64 restatement, the refusals of ppo.train and the learner, two gloo ranks, and
the CLI mapping."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from track_mjx_amd import hip

_T, _NLOC, _OBS, _REF, _NU = 3, 4, 24, 16, 3
_NETS = dict(encoder_layers=(12,), decoder_layers=(10,), critic_layers=(8,), latents=4)


# ---- C-ABI: bad ranges are refused before any launch, with a message (fake device addresses: nothing is touched)
def test_adam_frozen_refuses_bad_ranges_without_gpu():
    L = hip.lib()
    a = 0x10000
    ok = dict(param=a, grad=a, m=a, v=a, scratch=a, norm_out=None, n=1024, lo=256, hi=512)
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, 10.0, None)
    for bad, msg in ((dict(lo=512, hi=256), b"0 <= lo <= hi <= n"), (dict(hi=1028), b"0 <= lo <= hi <= n"), (dict(lo=-4), b"0 <= lo <= hi <= n"),
                     (dict(lo=258), b"multiples of 4"), (dict(hi=510), b"multiples of 4"), (dict(lo=2, hi=2), b"multiples of 4"),
                     (dict(param=None), b"null"), (dict(grad=None), b"null"), (dict(m=None), b"null"), (dict(v=None), b"null"),
                     (dict(scratch=None), b"null"), (dict(grad=a + 4), b"16-byte aligned"), (dict(n=0, lo=0, hi=0), b"bad n")):
        v = dict(ok, **bad)
        assert L.tmjx_adam_clip_norm_frozen(*v.values(), *tail) == -22, bad
        err = L.tmjx_last_error()
        assert b"tmjx_adam_clip_norm_frozen" in err and msg in err, (bad, err)


def test_stats_pinned_refuses_bad_columns_without_gpu():
    L = hip.lib()
    a = 0x10000
    ok = dict(sums=a, n_added=8.0, count=a, mean=a, sv=a, std=a, W=24, pin_lo=16)
    for bad, msg in ((dict(pin_lo=25), b"pin_lo"), (dict(pin_lo=-1), b"pin_lo"), (dict(W=0, pin_lo=0), b"W must be"), (dict(n_added=0.0), b"n_added"),
                     (dict(sums=None), b"null"), (dict(count=None), b"null"), (dict(mean=None), b"null"), (dict(sv=None), b"null"),
                     (dict(std=None), b"null")):
        v = dict(ok, **bad)
        assert L.tmjx_stats_apply_pinned(*v.values(), 1e-6, 1e6, None) == -22, bad
        err = L.tmjx_last_error()
        assert b"tmjx_stats_apply_pinned" in err and msg in err, (bad, err)


# ---- the learner (torch branch)
def _make_learner(seed, groups=1, world_batch=4, obs=_OBS, ref=_REF, **nets):
    from tests.common import StubEnv, torch_gae
    from track_mjx_amd.agent.ppo import PPOLearner
    envs = StubEnv(_NLOC, obs, ref, _NU) if groups == 1 else [StubEnv(_NLOC // groups, obs, ref, _NU) for _ in range(groups)]
    ln = PPOLearner(envs, **dict(_NETS, **nets), unroll_length=_T, batch_size=world_batch, num_minibatches=2, num_updates_per_batch=2,
                    learning_rate=1e-2, use_graph=False, seed=seed)
    ln.gae_fn = torch_gae
    return ln


def _fill(ln, seed):
    g = torch.Generator().manual_seed(seed)
    rows = ln.buf["reward"].shape[1]
    data = {"observation": torch.randn((_T, rows, _OBS), generator=g) * 2 + 0.5, "raw_action": torch.randn((_T, rows, _NU), generator=g),
            "log_prob": torch.randn((_T, rows), generator=g) * 0.1 - 2, "reward": torch.randn((_T, rows), generator=g),
            "discount": (torch.rand((_T, rows), generator=g) > 0.1).float(), "truncation": (torch.rand((_T, rows), generator=g) > 0.9).float(),
            "next_observation_last": torch.randn((rows, _OBS), generator=g)}
    for k, v in data.items():
        ln.buf[k].copy_(v)


def _pretrained(tmp_path):
    """Learner A after one update, its decoder and head perturbed (so they differ from any fresh initialisation), saved as step 5."""
    from track_mjx_amd.agent import checkpoint as ck
    a = _make_learner(3)
    _fill(a, 1)
    a.update()
    with torch.no_grad():
        g = torch.Generator().manual_seed(42)
        for p in ck.decoder_flax_params(a.policy).values():
            p.add_(torch.randn(p.shape, generator=g) * 0.3)
    d = tmp_path / "pre"
    ck.save_step_dir(d, 5, a, config={}, env_steps=123)
    return a, d


def _decoder_np(ln):
    from track_mjx_amd.agent import checkpoint as ck
    return {k: p.detach().cpu().numpy().copy() for k, p in ck.decoder_flax_params(ln.policy).items()}


def test_frozen_update_keeps_decoder_and_pinned_columns_and_matches_float64(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    a, d = _pretrained(tmp_path)
    dec_a = _decoder_np(a)
    tail = {k: getattr(a.normalizer, k)[_REF:].clone() for k in ("mean", "summed_variance", "std")}
    norm_tree, pol_tree, step = ck.load_freeze_source(d)
    assert step == 5
    b = _make_learner(4)
    fresh = b.opt.flat.clone()
    info = b.freeze_decoder(pol_tree, norm_tree)
    lo, hi = b.opt.frozen
    # the frozen range is exactly the decoder blocks + head: the last segments of the policy's bucket
    assert info["frozen_range"] == (lo, hi) and hi == b._bucket_split and 0 < lo < hi
    ids = {id(p) for p in ck.decoder_flax_params(b.policy).values()}
    assert lo == min(seg[0] for p, seg in zip(b.grads.params, b.grads.segs) if id(p) in ids)
    assert info["n_frozen"] == sum(p.numel() for p in ck.decoder_flax_params(b.policy).values())
    assert info["pinned_columns"] == (_REF, _OBS) and b._pin_lo == _REF
    # only the decoder came from the checkpoint: encoder, fc2 and the value net keep B's own initialisation; Adam starts fresh
    assert torch.equal(b.opt.flat[:lo], fresh[:lo]) and torch.equal(b.opt.flat[hi:], fresh[hi:])
    assert b.opt.t == 0 and not b.opt.exp_avg.any() and float(b.normalizer.count) == 0.0
    for k, v in _decoder_np(b).items():
        assert np.array_equal(v, dec_a[k]), k

    # float64 restatement of every optimiser step: clip by the global norm of ALL gradients, Adam, then the decoder's updates zeroed
    b1, b2 = b.opt.betas
    p64, m64, v64 = b.opt.flat.double().clone(), torch.zeros_like(b.opt.flat, dtype=torch.float64), torch.zeros_like(b.opt.flat, dtype=torch.float64)
    step_orig, t = b.opt.step, [0]

    def step():
        g = b.grads.flat.double()
        t[0] += 1
        nrm = torch.linalg.vector_norm(g)
        gs = g * (b.opt.max_norm / torch.clamp(nrm, min=b.opt.max_norm))
        m64.mul_(b1).add_(gs * (1 - b1)); v64.mul_(b2).add_(gs * gs * (1 - b2))
        upd = b.opt.lr / (1 - b1 ** t[0]) * m64 / (v64.sqrt() / (1 - b2 ** t[0]) ** 0.5 + b.opt.eps)
        upd[lo:hi] = 0
        p64.sub_(upd)
        return step_orig()
    b.opt.step = step
    rows = b.buf["reward"].shape[1]
    for k in range(2):
        _fill(b, 10 + k)
        b.update()
    assert t[0] == 2 * 2 * 2
    for k, v in _decoder_np(b).items():
        assert np.array_equal(v, dec_a[k]), f"decoder/{k} moved"
    with np.load(os.path.join(d, "5", "policy.npz")) as z:
        for k, v in _decoder_np(b).items():
            assert np.array_equal(v.T if k.endswith("kernel") else v, z["1/params/decoder/" + k]), k
    for k, v in tail.items():
        assert torch.equal(getattr(b.normalizer, k)[_REF:], v), k
    assert float(b.normalizer.count) == 2 * _T * rows
    assert not torch.equal(b.normalizer.mean[:_REF], torch.zeros(_REF))
    got = b.opt.flat.double()
    scale = float(p64.abs().max())
    for name, sl in (("encoder + fc2", slice(0, lo)), ("value", slice(hi, None))):
        assert float((got[sl] - fresh[sl].double()).abs().max()) > 1e-3, f"{name} did not move"
        assert float((got[sl] - p64[sl]).abs().max()) <= 1e-6 * scale, name
    # the decoder's moments are still updated (the freeze comes after adam), and agree with the restatement everywhere
    assert b.opt.exp_avg[lo:hi].abs().max() > 0 and b.opt.exp_avg_sq[lo:hi].abs().max() > 0
    assert float((b.opt.exp_avg.double() - m64).abs().max()) <= 1e-6 * float(m64.abs().max())
    assert float((b.opt.exp_avg_sq.double() - v64).abs().max()) <= 1e-6 * float(v64.abs().max())


def test_freeze_refuses_a_decoder_of_another_shape(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    _, d = _pretrained(tmp_path)
    norm_tree, pol_tree, _ = ck.load_freeze_source(d)
    for nets, name in ((dict(decoder_layers=(12,)), "decoder/hidden_0/kernel"), (dict(latents=6), "decoder/hidden_0/kernel"),
                       (dict(decoder_layers=(10, 10)), "decoder/hidden_1")):
        b = _make_learner(4, **nets)
        before = b.opt.flat.clone()
        with pytest.raises(ValueError, match=name):
            b.freeze_decoder(pol_tree, norm_tree)
        assert torch.equal(b.opt.flat, before) and b.opt.frozen is None and b._pin_lo is None     # nothing written
    # another proprioceptive width: the decoder's input width differs
    b = _make_learner(4, obs=_OBS + 4)
    with pytest.raises(ValueError, match=r"decoder/hidden_0/kernel has shape \(12, 10\), this run's has \(16, 10\)"):
        b.freeze_decoder(pol_tree, norm_tree)


def test_freeze_refusals():
    from track_mjx_amd.agent import ppo
    from track_mjx_amd.agent.lstm import LSTMPPOLearner
    with pytest.raises(ValueError, match="freeze_decoder needs a checkpoint"):
        ppo.train(None, 100, 10, freeze_decoder=True)
    with pytest.raises(ValueError, match="checkpoint_to_restore and restore_from"):
        ppo.train(None, 100, 10, checkpoint_to_restore="a", restore_from="b")
    with pytest.raises(ValueError, match="checkpoint_to_restore and restore_from"):
        ppo.train(None, 100, 10, checkpoint_to_restore="a", restore_from="b", freeze_decoder=True)
    with pytest.raises(NotImplementedError, match="LSTM"):
        ppo.train(None, 100, 10, checkpoint_to_restore="a", freeze_decoder=True, use_lstm=True)
    with pytest.raises(NotImplementedError, match="LSTM"):
        LSTMPPOLearner.freeze_decoder(object(), {}, {})
    # no proprioceptive columns: nothing for the decoder to read from the observation, nothing to pin (ppo.py:586-590)
    b = _make_learner(4, ref=_OBS)
    with pytest.raises(ValueError, match="proprioceptive observation size is 0"):
        b.freeze_decoder()


def test_resumed_frozen_run_pins_the_restored_columns(tmp_path):
    """freeze_decoder() without trees (restore_from + freeze_decoder): the restored decoder and normaliser tail stay as they are."""
    from track_mjx_amd.agent import checkpoint as ck
    a, d = _pretrained(tmp_path)
    b = _make_learner(4)
    ck.restore(d, b)
    dec, tail = _decoder_np(b), b.normalizer.mean[_REF:].clone()
    b.freeze_decoder()
    _fill(b, 20)
    b.update()
    assert all(np.array_equal(v, dec[k]) for k, v in _decoder_np(b).items())
    assert torch.equal(b.normalizer.mean[_REF:], tail) and not torch.equal(b.normalizer.mean[:_REF], a.normalizer.mean[:_REF])


# ---- two gloo ranks, two env groups each: every rank freezes from the same checkpoint, replicas stay bit-identical
def _rank_worker(rank, world, port, ckdir, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from track_mjx_amd.agent import checkpoint as ck
    ln = _make_learner(4, groups=2, world_batch=4 * world)
    norm_tree, pol_tree, _ = ck.load_freeze_source(ckdir)
    ln.freeze_decoder(pol_tree, norm_tree)
    _fill(ln, 100 + rank)
    ln.perm_fn = lambda upd, rows: torch.randperm(rows, generator=torch.Generator().manual_seed(1000 + 10 * rank + upd))
    ln.update()
    n = ln.normalizer
    q.put((rank, ln.opt.flat.clone().numpy(), n.mean.numpy().copy(), n.std.numpy().copy(), float(n.count), _decoder_np(ln), ln.opt.frozen))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_freeze_identically(tmp_path):
    a, d = _pretrained(tmp_path)
    dec_a = _decoder_np(a)
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33700 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, str(d), q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r = q.get(timeout=300)
        got[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])
    assert got[0][3] == got[1][3] == world * _T * 2 * _NLOC
    lo, hi = got[0][5]
    fresh = _make_learner(4, groups=2, world_batch=4 * world).opt.flat.numpy()
    assert np.abs(got[0][0][:lo] - fresh[:lo]).max() > 1e-3, "the encoder must have moved"
    for r in range(world):
        assert all(np.array_equal(v, dec_a[k]) for k, v in got[r][4].items()), r
        assert np.array_equal(got[r][1][_REF:], a.normalizer.mean[_REF:].numpy())


# ---- the CLI keys
def test_train_setup_keys_map_to_ppo_train_keywords():
    from track_mjx_amd import config as _config
    from track_mjx_amd import train
    cfg = _config.load_config(None, [])
    assert "checkpoint_to_restore" not in cfg["train_setup"] and "freeze_decoder" not in cfg["train_setup"]
    assert train.restore_options(cfg) == {}
    cfg = _config.load_config(None, ["train_setup.checkpoint_to_restore=/runs/pre", "train_setup.freeze_decoder=true"])
    assert train.restore_options(cfg) == {"checkpoint_to_restore": "/runs/pre", "freeze_decoder": True}
    cfg = _config.load_config(None, ["train_setup.checkpoint_to_restore=/runs/pre"])
    assert train.restore_options(cfg) == {"checkpoint_to_restore": "/runs/pre"}
    cfg = _config.load_config(None, ["train_setup.checkpoint_to_restore=null", "train_setup.freeze_decoder=false"])
    assert train.restore_options(cfg) == {}
    cfg = _config.load_config(None, ["train_setup.freeze_decoder=true"])
    assert train.restore_options(cfg) == {"freeze_decoder": True}
