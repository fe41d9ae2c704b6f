"""CPU: the decoder-only policy of an LSTM checkpoint (agent.checkpoint.make_lstm_decoder_policy_fn), HighLevelWrapper's carry handling on a stub
env, and the argument validation of tmjx_lstm_decoder_act without a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests.test_highlevel_cpu import _StubEnv
from track_mjx_amd import hip

_OBS, _REF, _NU, _Z, _H, _L = 24, 16, 3, 4, 32, 2
_PROP = _OBS - _REF


def _policy(seed=0, H=_H, L=_L):
    from track_mjx_amd.agent.lstm import LSTMIntentionPolicy
    torch.manual_seed(seed)
    pol = LSTMIntentionPolicy(_OBS, _REF, _NU, _Z, (12,), H, L)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.2)
    return pol


def _norm(seed=0):
    g = torch.Generator().manual_seed(seed + 200)
    mean, std = torch.randn(_OBS, generator=g) * 0.3, 0.4 + torch.rand(_OBS, generator=g) * 1.5
    return {"count": np.float32(77.0), "mean": mean.numpy(), "summed_variance": np.ones(_OBS, np.float32), "std": std.numpy()}, mean, std


def _save(directory, step, pol, norm, config=None):
    """<directory>/<step>/{policy.npz, config/metadata}: what save_step_dir writes of a policy."""
    from track_mjx_amd.agent import checkpoint as ck
    d = os.path.join(str(directory), str(step))
    os.makedirs(os.path.join(d, "config"), exist_ok=True)
    np.savez(os.path.join(d, "policy.npz"), **ck.flatten({"0": norm, "1": ck.policy_to_flax(pol)}))
    with open(os.path.join(d, "config", "metadata"), "w") as f:
        json.dump({} if config is None else config, f)
    return str(directory)


def test_lstm_decoder_policy_equals_the_full_policys_step(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    pol = _policy()
    norm, mean, std = _norm()
    d = _save(tmp_path / "run", 5, pol, norm)
    dp = ck.make_lstm_decoder_policy_fn(d, device="cpu")
    assert isinstance(dp, ck.LSTMDecoderPolicy)
    assert (dp.latent_size, dp.proprioceptive_obs_size, dp.action_size, dp.reference_obs_size) == (_Z, _PROP, _NU, _REF)
    assert (dp.hidden_layer_num, dp.hidden_state_size) == (_L, _H)
    g = torch.Generator().manual_seed(1)
    n = 7
    h, c = pol.zero_carry(n, "cpu")
    carry = None
    for t in range(4):
        raw = torch.randn((n, _OBS), generator=g) * 2 + 0.5
        logits, fc2 = pol.step((raw - mean) / std, h, c)                # (updates h, c in place)
        want = torch.tanh(logits[:, :_NU])
        x = torch.cat([fc2[:, :_Z], raw[:, _REF:]], dim=-1)
        act, extras, carry = dp(x, hidden_state=carry)
        # the same torch expressions in the same order: no round-off between the two
        assert extras == {} and act.shape == (n, _NU) and torch.equal(act, want), t
        assert torch.equal(carry[0], h) and torch.equal(carry[1], c), t
    assert float(carry[0].abs().max()) > 1e-3
    # the step directory and an explicit step give the same policy
    for src, kw in ((os.path.join(d, "5"), {}), (d, dict(step=5))):
        other = ck.make_lstm_decoder_policy_fn(src, device="cpu", **kw)
        assert torch.equal(other(x, hidden_state=None)[0], dp(x)[0])
    with pytest.raises(ValueError, match="latents \\+ proprioception"):
        dp(torch.zeros(2, _Z + _PROP + 1))
    with pytest.raises(ValueError, match="hidden_state must be"):
        dp(torch.zeros(2, _Z + _PROP), hidden_state=(torch.zeros(3, _L, _H), torch.zeros(3, _L, _H)))


def test_normaliser_columns_none_carry_and_reset(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    pol = _policy(1)
    norm, mean, std = _norm(1)
    d = _save(tmp_path / "run", 1, pol, norm)
    dp = ck.make_lstm_decoder_policy_fn(d, device="cpu")
    assert dp.mean.shape == (_PROP,) and torch.equal(dp.mean, mean[_REF:]) and torch.equal(dp.std, std[_REF:])
    g = torch.Generator().manual_seed(2)
    x = torch.randn((6, _Z + _PROP), generator=g)
    want = dp(x)
    # only the proprioceptive columns of the normaliser count
    n2 = dict(norm, mean=norm["mean"].copy(), std=norm["std"].copy())
    n2["mean"][:_REF] += 3.0; n2["std"][:_REF] *= 2.0
    _save(d, 2, pol, n2)
    assert torch.equal(ck.make_lstm_decoder_policy_fn(d, device="cpu")(x)[0], want[0])                 # (the latest step: 2)
    n2["mean"][_REF:] += 0.5
    _save(d, 3, pol, n2)
    assert not torch.equal(ck.make_lstm_decoder_policy_fn(d, device="cpu")(x)[0], want[0])
    # normalize_observations=false in the saved config: no normaliser, the raw columns go in
    _save(d, 4, pol, norm, {"train_setup": {"train_config": {"normalize_observations": False}}})
    raw_dp = ck.make_lstm_decoder_policy_fn(d, device="cpu")
    assert raw_dp.mean is None and raw_dp.std is None
    dp.mean, dp.std = torch.zeros(_PROP), torch.ones(_PROP)
    assert torch.equal(raw_dp(x)[0], dp(x)[0])
    dp.mean, dp.std = mean[_REF:], std[_REF:]
    # hidden_state=None is a zero carry
    z = dp.zero_carry(6)
    assert z[0].shape == (6, _L, _H) and not z[0].any() and not z[1].any()
    a0, _, (h0, c0) = dp(x, hidden_state=z)
    assert torch.equal(a0, want[0]) and torch.equal(h0, want[2][0]) and torch.equal(c0, want[2][1]) and not z[0].any()
    # reset zeroes exactly the flagged rows
    x2 = torch.randn((6, _Z + _PROP), generator=g)
    kept = dp(x2, hidden_state=(h0, c0))
    fresh = dp(x2)
    flags = torch.tensor([0., 1., 0., 0., 2., 0.])
    mixed = dp(x2, hidden_state=(h0, c0), reset=flags)
    on = flags != 0
    for got, k, f in ((mixed[0], kept[0], fresh[0]), (mixed[2][0], kept[2][0], fresh[2][0]), (mixed[2][1], kept[2][1], fresh[2][1])):
        assert torch.equal(got[on], f[on]) and torch.equal(got[~on], k[~on]) and not torch.equal(k[on], f[on])


def test_lstm_decoder_policy_refusals(tmp_path):
    from tests.test_highlevel_cpu import _ckpt
    from track_mjx_amd.agent import checkpoint as ck
    pol = _policy()
    norm, _, _ = _norm()
    tree = ck.policy_to_flax(pol)
    ck.lstm_decoder_policy_from_trees(norm, tree, device="cpu")
    _, d = _ckpt(tmp_path)                                                   # an MLP checkpoint
    with pytest.raises(ValueError, match="make_decoder_policy_fn"):
        ck.make_lstm_decoder_policy_fn(d, device="cpu")
    enc, dec = tree["params"]["encoder"], tree["params"]["lstm_decoder"]
    with pytest.raises(ValueError, match="no params/lstm_decoder"):
        ck.lstm_decoder_policy_from_trees(norm, {"params": {"encoder": enc}}, device="cpu")
    with pytest.raises(ValueError, match="no lstm_projection"):
        ck.lstm_decoder_policy_from_trees(norm, {"params": {"encoder": enc, "lstm_decoder": {k: v for k, v in dec.items() if k != "lstm_projection"}}},
                                          device="cpu")
    odd = dict(dec, lstm_projection={"kernel": np.zeros((_H, 2 * _NU + 1), np.float32), "bias": np.zeros(2 * _NU + 1, np.float32)})
    with pytest.raises(ValueError, match="odd head width 7"):
        ck.lstm_decoder_policy_from_trees(norm, {"params": {"encoder": enc, "lstm_decoder": odd}}, device="cpu")
    with pytest.raises(ValueError, match="fc2_mean"):
        ck.lstm_decoder_policy_from_trees(norm, {"params": {"encoder": {}, "lstm_decoder": dec}}, device="cpu")
    with pytest.raises(ValueError, match="no normaliser"):
        ck.lstm_decoder_policy_from_trees(None, tree, device="cpu")
    with pytest.raises(FileNotFoundError):
        ck.make_lstm_decoder_policy_fn(tmp_path / "nothing_here_dir" / "x.npz", device="cpu")


class _DoneEnv(_StubEnv):
    """The stub env with done flags the test sets."""

    def __init__(self, *a):
        super().__init__(*a)
        self.done = torch.zeros(self.num_envs)

    def _mk(self):
        return self.ns(obs=self.obs, reward=torch.zeros(self.num_envs), done=self.done.clone())


def test_wrapper_owns_the_carry_on_the_callable_path():
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.environment import HighLevelWrapper
    pol = _policy(2)
    norm, _, _ = _norm(2)
    dp = ck.lstm_decoder_policy_from_trees(norm, ck.policy_to_flax(pol), device="cpu")
    n = 5
    env = _DoneEnv(n, _OBS, _NU)
    hl = HighLevelWrapper(env, dp, _REF)
    assert hl.path == "callable" and hl.action_size == _Z and hl.reset_carry_on_done is True
    g = torch.Generator().manual_seed(3)
    lats = [torch.randn(n, _Z, generator=g) for _ in range(4)]
    xs = [torch.cat([l, env.obs[:, _REF:]], dim=-1) for l in lats]
    st = hl.reset(0)
    h, c = hl.hidden_state
    assert h.shape == (n, _L, _H) and not h.any() and not c.any()
    # the carry persists across steps
    st = hl.step(st, lats[0])
    a0, _, s0 = dp(xs[0])
    assert torch.equal(env.actions[0], a0) and torch.equal(hl.hidden_state[0], s0[0]) and torch.equal(hl.hidden_state[1], s0[1])
    st = hl.step(st, lats[1])
    a1, _, s1 = dp(xs[1], hidden_state=s0)
    assert torch.equal(env.actions[1], a1) and torch.equal(hl.hidden_state[0], s1[0]) and not torch.equal(a1, dp(xs[1])[0])
    # reset_carry_on_done: the done flags of the state that is stepped reset those rows' carry
    env.done = torch.tensor([0., 1., 0., 1., 0.])
    st = hl.step(st, lats[2])                    # (st.done is still all zero: the env reports the flags with the state it returns)
    s2 = dp(xs[2], hidden_state=s1)[2]
    assert torch.equal(hl.hidden_state[0], s2[0])
    st = hl.step(st, lats[3])
    a3, _, s3 = dp(xs[3], hidden_state=s2, reset=env.done)
    assert torch.equal(env.actions[3], a3) and torch.equal(hl.hidden_state[1], s3[1])
    assert not torch.equal(a3, dp(xs[3], hidden_state=s2)[0])
    # ... and is not with reset_carry_on_done=False
    hl2 = HighLevelWrapper(env, dp, _REF, reset_carry_on_done=False)
    st = hl2.reset(0)
    hl2.set_hidden_state(*s2)
    assert torch.equal(hl2.hidden_state[0], s2[0]) and torch.equal(hl2.hidden_state[1], s2[1])       # set_hidden_state round-trips
    hl2.step(st, lats[3])
    assert torch.equal(env.actions[-1], dp(xs[3], hidden_state=s2)[0])
    # reset() zeroes the carry
    hl2.reset(0)
    assert not hl2.hidden_state[0].any() and not hl2.hidden_state[1].any()
    hl2.step(st, lats[0])
    assert torch.equal(env.actions[-1], a0)
    with pytest.raises(ValueError, match="h and c must be"):
        hl2.set_hidden_state(torch.zeros(n, _L, _H + 1), torch.zeros(n, _L, _H + 1))
    for path in ("fused", "layers"):
        with pytest.raises(ValueError, match="on the env's device"):
            HighLevelWrapper(env, dp, _REF, path=path)
    # a generic callable has no carry
    with pytest.raises(TypeError, match="LSTMDecoderPolicy"):
        HighLevelWrapper(env, lambda x: (x[:, :_NU], {}), _REF).hidden_state


# ---- C-ABI: refused before any device call, with a message (fake device addresses: nothing is touched)
def _desc(n=4096, Z=60, obs_w=696, ref=470, L=2, H=128, A=38, ldw=None, **over):
    a = 1 << 20
    d = hip.LstmDecoderAct()
    d.latents, d.ldz, d.obs, d.obs_s0, d.obs_s1, d.mean, d.std, d.reset = a, Z, a, 1, n, a, a, a
    d.n, d.Z, d.obs_w, d.ref_w, d.L, d.H = n, Z, obs_w, ref, L, H
    k = Z + obs_w - ref
    for i in range(min(L, 4)):
        y = d.layer[i]
        y.Wi, y.Wh, y.bh, y.ldwi, y.ldwh = a, a, a, ((k + 3) // 4 * 4 if ldw is None else ldw), H
        k = H
    d.Wp, d.bp, d.ldwp, d.A = a, a, H, A
    d.h, d.c, d.ld = a, a, L * H
    d.action_t, d.ctrl, d.logits, d.ldl = a, a, a, 2 * A
    for key, v in over.items():
        setattr(d, key, v)
    return d


def test_lstm_decoder_act_validates_before_it_launches():
    L = hip.lib()
    assert C.sizeof(hip.LstmDecoderAct) == 296
    assert "tmjx_lstm_decoder_act" in hip.EXPORTS and "tmjx_lstm_decoder_act_ok" in hip.EXPORTS
    assert L.tmjx_lstm_decoder_act_ok(C.byref(_desc())) == 1                        # the default shape
    assert L.tmjx_lstm_decoder_act_ok(C.byref(_desc(n=1, L=1, mean=None, std=None, reset=None, ctrl=None, logits=None, ldl=0))) == 1
    assert L.tmjx_lstm_decoder_act_ok(C.byref(_desc(L=4, A=64, Z=94))) == 1         # Z + prop = 320, 2A = 128
    assert L.tmjx_lstm_decoder_act_ok(None) == 0 and L.tmjx_lstm_decoder_act(None, None) == -22
    bad = ((_desc(H=64), b"H must be 128"), (_desc(L=5), b"1 .. 4 LSTM layers"), (_desc(L=0), b"1 .. 4 LSTM layers"), (_desc(A=65), b"2A <= 128"),
           (_desc(ldw=287), b"ldw % 4 == 0"), (_desc(h=None), b"null carry"), (_desc(c=None), b"null carry"), (_desc(Z=98), b"at most 320"),
           (_desc(latents=None), b"null argument"), (_desc(mean=None), b"mean and std together"), (_desc(n=0), b"n >= 1"), (_desc(ldz=59), b"ldz"),
           (_desc(ld=255), b"ld >= L * H"), (_desc(ldl=75), b"ldl >= 2A"), (_desc(ldw=284), b"ldwi"), (_desc(action_t=(1 << 20) + 2), b"4-byte aligned"))
    assert _desc(A=65).A * 2 == 130 and _desc(Z=98).Z + 696 - 470 == 324
    for d, word in bad:
        assert L.tmjx_lstm_decoder_act_ok(C.byref(d)) == 0, word
        assert L.tmjx_lstm_decoder_act(C.byref(d), None) == -22, word
        err = L.tmjx_last_error()
        assert b"tmjx_lstm_decoder_act" in err and word in err, (word, err)


def test_both_decoder_launches_refuse_a_common_fault_with_the_same_words():
    """The checks the two descriptors share (csrc/decoder_io.h): one fault in an otherwise valid descriptor, the same reason behind either name."""
    from tests.test_highlevel_cpu import _desc as _mlp_desc
    L = hip.lib()
    faults = ((dict(std=None), b"mean and std together"), (dict(ldz=59), b"ldz >= Z"), (dict(ref_w=697), b"obs_w >= ref_w"),
              (dict(Z=95), b"at most 320"), (dict(A=65), b"2A <= 128"), (dict(ldl=75), b"ldl >= 2A"))
    assert _desc(Z=95).Z + 696 - 470 == 321 and _desc(A=65).A * 2 == 130 and _desc().logits and _mlp_desc().logits
    for over, word in faults:
        reasons = []
        for name, d in (("tmjx_decoder_act", _mlp_desc(**over)), ("tmjx_lstm_decoder_act", _desc(**over))):
            assert getattr(L, name + "_ok")(C.byref(d)) == 0, (name, over)
            assert getattr(L, name)(C.byref(d), None) == -22, (name, over)
            err = L.tmjx_last_error()
            assert err.startswith(name.encode() + b": "), err
            reasons.append(err[len(name) + 2:])
        assert reasons[0] == reasons[1] and word in reasons[0], (over, reasons)


def test_wrapper_reports_why_an_lstm_decoder_does_not_qualify():
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.environment.wrappers import lstm_decoder_act_why_not
    norm, _, _ = _norm()
    dp = ck.lstm_decoder_policy_from_trees(norm, ck.policy_to_flax(_policy()), device="cpu")
    assert "H must be 128" in lstm_decoder_act_why_not(dp, _OBS)
    wide = ck.lstm_decoder_policy_from_trees(norm, ck.policy_to_flax(_policy(H=128, L=1)), device="cpu")
    assert lstm_decoder_act_why_not(wide, _OBS, 3) is None
