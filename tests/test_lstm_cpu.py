"""CPU: the recurrent learner's host side — argument validation of the LSTM exports without a GPU, the use_lstm switch of train.py and its
refusals, the flax parameter names / shapes in a checkpoint, and the initialisers."""
import ctypes as C

import numpy as np
import pytest
import torch

from track_mjx_amd import config as _config, hip


def _fwd(**kw):
    a = dict(xg=16, ldx=512, Wh=16, ldw=128, bh=16, h0=16, c0=16, ld0=128, reset=None, ldr=0, h=32, c=48, ldo=128, gates=None, h_prev=None, T=2, rows=8, H=128)
    a.update(kw)
    return hip.LstmFwd(**a)


def _bwd(**kw):
    a = dict(dh=16, ldd=128, Wh=16, ldw=128, gates=16, c=16, ldo=128, c0=16, ld0=128, reset=None, ldr=0, dgates=16, dh0=None, dc0=None, T=2, rows=8, H=128)
    a.update(kw)
    return hip.LstmBwd(**a)


@pytest.mark.parametrize("bad", [dict(H=100), dict(H=512), dict(T=0), dict(rows=0), dict(ldx=511), dict(ldw=130), dict(Wh=20), dict(ld0=64),
                                 dict(xg=18), dict(reset=16, ldr=4), dict(h=None), dict(h=16, c=16)])
def test_lstm_fwd_refuses_bad_arguments_without_gpu(bad):
    L = hip.lib()
    assert L.tmjx_lstm_seq_fwd(C.byref(_fwd(**bad)), None) == -22          # TMJX_EINVAL before any device call
    assert b"tmjx_lstm_seq_fwd" in L.tmjx_last_error()


@pytest.mark.parametrize("bad", [dict(H=48), dict(T=0), dict(ldd=100), dict(dgates=None), dict(gates=6), dict(reset=16, ldr=7), dict(c0=None)])
def test_lstm_bwd_refuses_bad_arguments_without_gpu(bad):
    L = hip.lib()
    assert L.tmjx_lstm_seq_bwd(C.byref(_bwd(**bad)), None) == -22
    assert b"tmjx_lstm_seq_bwd" in L.tmjx_last_error()


def test_lstm_hidden_sizes():
    from track_mjx_amd.agent.lstm import LSTM_HIDDEN_SIZES
    L = hip.lib()
    assert [h for h in range(1, 600) if L.tmjx_lstm_hidden_ok(h)] == list(LSTM_HIDDEN_SIZES)


def test_use_lstm_selects_the_recurrent_learner():
    from track_mjx_amd.train import learner_options
    assert learner_options(_config.load_config(None, [])) == {}
    cfg = _config.load_config(None, ["train_setup.train_config.use_lstm=true"])
    assert learner_options(cfg) == {"use_lstm": True, "hidden_state_size": 128, "hidden_layer_num": 2}
    cfg = _config.load_config(None, ["train_setup.train_config.use_lstm=true", "network_config.hidden_state_size=64", "network_config.hidden_layer_num=3"])
    assert learner_options(cfg) == {"use_lstm": True, "hidden_state_size": 64, "hidden_layer_num": 3}
    import inspect
    from track_mjx_amd.agent import ppo
    sig = inspect.signature(ppo.train).parameters
    assert sig["use_lstm"].default is False and sig["hidden_state_size"].default == 128 and sig["hidden_layer_num"].default == 2


@pytest.mark.parametrize("over,msg", [(["mlp_gemm_inputs=bf16"], "bf16"), (["network_config.hidden_state_size=100"], "hidden_state_size"),
                                      (["network_config.hidden_layer_num=0"], "hidden_layer_num")])
def test_use_lstm_refusals(over, msg):
    from track_mjx_amd.train import learner_options
    cfg = _config.load_config(None, ["train_setup.train_config.use_lstm=true", *over])
    with pytest.raises(ValueError, match=msg):
        learner_options(cfg)
    from track_mjx_amd.agent.lstm import LSTMIntentionPolicy, check_lstm_config
    with pytest.raises(ValueError):
        check_lstm_config(128, 2, torch.bfloat16)
    with pytest.raises(ValueError):
        LSTMIntentionPolicy(40, 24, 4, 8, (16,), 96, 2)
    with pytest.raises(ValueError):
        LSTMIntentionPolicy(40, 24, 4, 8, (16,), 128, 0)


def _policy(H=32, L=2):
    from track_mjx_amd.agent.lstm import LSTMIntentionPolicy
    torch.manual_seed(0)
    return LSTMIntentionPolicy(40, 24, 4, 8, (16, 16), H, L)


def test_lstm_checkpoint_names_and_shapes():
    from track_mjx_amd.agent import checkpoint as ckpt
    pol = _policy()
    flat = ckpt.flatten(ckpt.policy_to_flax(pol))
    H, D = 32, 8 + 16
    want = {}
    for k, din in ((0, D), (1, H)):
        for g in "ifgo":
            want[f"params/lstm_decoder/lstm_{k}/i{g}/kernel"] = (din, H)
            want[f"params/lstm_decoder/lstm_{k}/h{g}/kernel"] = (H, H)
            want[f"params/lstm_decoder/lstm_{k}/h{g}/bias"] = (H,)
    want["params/lstm_decoder/lstm_projection/kernel"] = (H, 8)
    want["params/lstm_decoder/lstm_projection/bias"] = (8,)
    for i, (a, b) in enumerate(((24, 16), (16, 16))):
        want[f"params/encoder/hidden_{i}/kernel"] = (a, b)
        want[f"params/encoder/hidden_{i}/bias"] = (b,)
        want[f"params/encoder/LayerNorm_{i}/scale"] = (b,)
        want[f"params/encoder/LayerNorm_{i}/bias"] = (b,)
    for n in ("fc2_mean", "fc2_logvar"):
        want[f"params/encoder/{n}/kernel"] = (16, 8)
        want[f"params/encoder/{n}/bias"] = (8,)
    assert {k: tuple(v.shape) for k, v in flat.items()} == want
    # round trip into a differently initialised module
    other = _policy()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    ckpt.policy_from_flax(other, ckpt.unflatten(flat))
    assert all(torch.equal(a, b) for a, b in zip(pol.parameters(), other.parameters()))


def test_lstm_initialisers():
    pol = _policy(H=64, L=2)
    H = 64
    for k in range(2):
        wh, bh, wi = pol.w_hh[k].detach().double(), pol.b_hh[k].detach(), pol.w_ih[k].detach()
        for g in range(4):
            q = wh[g * H:(g + 1) * H]
            assert torch.allclose(q @ q.t(), torch.eye(H, dtype=torch.float64), atol=1e-5)       # flax orthogonal(): one per gate kernel
        assert torch.count_nonzero(bh) == 0
        lim = (3.0 / wi.shape[1]) ** 0.5                                                        # lecun_uniform, fan_in = input width
        assert float(wi.abs().max()) <= lim and float(wi.abs().max()) > 0.9 * lim
    assert torch.count_nonzero(pol.projection.bias) == 0


def test_lstm_policy_torch_branch_carry_and_resets():
    """CPU branch of the module: the acting step (T = 1, carry in place, reset) agrees with the sequence pass."""
    pol = _policy()
    g = torch.Generator().manual_seed(2)
    T, B = 5, 6
    obs = torch.randn(T, B, 40, generator=g)
    reset = torch.zeros(T, B)
    reset[3, 1] = 1.0
    h0, c0 = pol.zero_carry(B, "cpu")
    with torch.no_grad():
        seq, _ = pol(obs, h0, c0, reset)
        h, c = pol.zero_carry(B, "cpu")
        steps = [pol.step(obs[t], h, c, reset[t])[0] for t in range(T)]
    np.testing.assert_allclose(torch.stack(steps).numpy(), seq.numpy(), rtol=1e-5, atol=1e-6)
    assert float(h.abs().max()) > 0


def test_plain_kl_formula():
    """plain_kl = -0.5 mean(1 + logvar - mean^2 - exp(logvar)) over every element (lstm_ppo/losses.py), not the MLP learner's AR(1) prior."""
    from track_mjx_amd.agent.lstm import plain_kl
    g = np.random.default_rng(0)
    mu, lv = g.normal(size=(5, 7, 3)), g.normal(size=(5, 7, 3)) * 0.5
    want = -0.5 * np.mean(1 + lv - mu ** 2 - np.exp(lv))
    got = float(plain_kl(torch.from_numpy(np.concatenate([mu, lv], -1))))
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want))


def test_carried_policy_takes_done_by_keyword_only():
    import inspect
    from track_mjx_amd.agent.lstm import CarriedPolicy
    p = inspect.signature(CarriedPolicy.__call__).parameters
    assert p["done"].kind is inspect.Parameter.KEYWORD_ONLY
