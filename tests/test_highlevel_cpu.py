"""CPU: the decoder-only policy (agent.checkpoint.make_decoder_policy_fn, the reference's ppo_networks.py:193-238 / intention_network.py:194-222) and
HighLevelWrapper's host logic (environment/wrappers.py; the reference's wrappers.py:384-412) — the policy against the full IntentionPolicy's
deterministic action and a float64 restatement, the normaliser's slicing, the wrapper on a stub env with a generic callable, the refusals, and the
argument validation of tmjx_decoder_act / tmjx_decoder_input without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from track_mjx_amd import hip

_T, _NLOC, _OBS, _REF, _NU, _Z = 3, 4, 24, 16, 3, 4
_NETS = dict(encoder_layers=(12,), decoder_layers=(10, 9), critic_layers=(8,), latents=_Z)
TOL = 5e-5          # tests/test_gpu_rollout.py: the project's relative bound of a float32 policy against its float64 restatement


def _learner(seed, **over):
    from tests.common import StubEnv
    from track_mjx_amd.agent.ppo import PPOLearner
    ln = PPOLearner(StubEnv(_NLOC, _OBS, _REF, _NU), **dict(_NETS, **over), unroll_length=_T, batch_size=4, num_minibatches=2, num_updates_per_batch=2,
                    learning_rate=1e-2, use_graph=False, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in ln.policy.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.2)
        ln.normalizer.mean.copy_(torch.randn(_OBS, generator=g) * 0.3)
        ln.normalizer.std.copy_(0.4 + torch.rand(_OBS, generator=g) * 1.5)
        ln.normalizer.count.fill_(77.0)
    return ln


def _ckpt(tmp_path, seed=3, config=None, **over):
    from track_mjx_amd.agent import checkpoint as ck
    ln = _learner(seed, **over)
    d = tmp_path / f"run{seed}"
    ck.save_step_dir(d, 5, ln, config={} if config is None else config, env_steps=1)
    return ln, d


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _f64_decoder(net, x):
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    h = x.double()
    for blk in net.decoder:
        z = h @ d(blk.dense.weight).T + d(blk.dense.bias)
        h = torch.nn.functional.layer_norm(torch.nn.functional.silu(z), (z.shape[-1],), d(blk.norm.weight), d(blk.norm.bias), blk.norm.eps)
    logits = h @ d(net.head.weight).T + d(net.head.bias)
    return torch.tanh(logits[:, :net.head.out_features // 2])


def test_decoder_policy_equals_the_full_policys_deterministic_action(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    ln, d = _ckpt(tmp_path)
    dp = ck.make_decoder_policy_fn(d, device="cpu")
    assert (dp.latent_size, dp.proprioceptive_obs_size, dp.action_size, dp.reference_obs_size) == (_Z, _OBS - _REF, _NU, _REF)
    assert dp.decoder_layer_sizes == (10, 9)
    g = torch.Generator().manual_seed(0)
    raw = torch.randn((7, _OBS), generator=g) * 2 + 0.5
    nz = ln.normalizer
    with torch.no_grad():
        obs_n = (raw - nz.mean) / nz.std
        logits, mean, _ = ln.policy(obs_n, deterministic=True)
        want = torch.tanh(logits[:, :_NU])
    act, extras = dp(torch.cat([mean, raw[:, _REF:]], dim=-1))
    # the same modules (_Block, _Dense) and the same torch ops in the same order: no round-off between the two
    assert extras == {} and act.shape == (7, _NU) and torch.equal(act, want)
    # float64 restatement of the decoder on the normalised input
    x64 = torch.cat([mean.double(), (raw[:, _REF:].double() - nz.mean[_REF:].double()) / nz.std[_REF:].double()], dim=-1)
    assert _rel(act.numpy(), _f64_decoder(dp.net, x64).numpy()) < TOL
    # the run directory, the step directory, an explicit step and a save_npz file give the same policy
    ck.save_npz(tmp_path / "flat.npz", ln, config={}, iteration=5)
    for src, kw in ((d / "5", {}), (d, dict(step=5)), (tmp_path / "flat.npz", {})):
        other = ck.make_decoder_policy_fn(src, device="cpu", **kw)
        assert torch.equal(other(torch.cat([mean, raw[:, _REF:]], dim=-1))[0], want), src
    with pytest.raises(ValueError, match="columns"):
        dp(torch.zeros(2, _Z + _OBS - _REF + 1))


def test_only_the_proprioceptive_normaliser_columns_are_used(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    ln, d = _ckpt(tmp_path)
    dp = ck.make_decoder_policy_fn(d, device="cpu")
    assert dp.mean.shape == (_OBS - _REF,) and torch.equal(dp.mean, ln.normalizer.mean[_REF:]) and torch.equal(dp.std, ln.normalizer.std[_REF:])
    x = torch.randn((5, _Z + _OBS - _REF), generator=torch.Generator().manual_seed(1))
    want = dp(x)[0]
    with torch.no_grad():
        ln.normalizer.mean[:_REF].add_(3.0); ln.normalizer.std[:_REF].mul_(2.0)
    ck.save_step_dir(d, 6, ln, config={})
    assert torch.equal(ck.make_decoder_policy_fn(d, device="cpu")(x)[0], want)                       # (the latest step: 6)
    with torch.no_grad():
        ln.normalizer.mean[_REF:].add_(0.5)
    ck.save_step_dir(d, 7, ln, config={})
    assert not torch.equal(ck.make_decoder_policy_fn(d, device="cpu")(x)[0], want)
    # normalize_observations=false in the saved config: the raw columns go in
    ck.save_step_dir(d, 8, ln, config={"train_setup": {"train_config": {"normalize_observations": False}}})
    raw_dp = ck.make_decoder_policy_fn(d, device="cpu")
    assert raw_dp.mean is None and raw_dp.std is None
    with torch.no_grad():
        assert torch.equal(raw_dp(x)[0], torch.tanh(raw_dp.net(x)[:, :_NU]))


def test_decoder_policy_refusals(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    ln, d = _ckpt(tmp_path)
    norm, ptree = ck.load_policy(d)
    lstm_tree = {"params": {"encoder": ptree["params"]["encoder"], "lstm_decoder": {"lstm_projection": {}}}}
    with pytest.raises(NotImplementedError, match="lstm_decoder"):
        ck.decoder_policy_from_trees(norm, lstm_tree, device="cpu")
    with pytest.raises(ValueError, match="no params/decoder"):
        ck.decoder_policy_from_trees(norm, {"params": {"encoder": ptree["params"]["encoder"]}}, device="cpu")
    with pytest.raises(FileNotFoundError):
        ck.make_decoder_policy_fn(tmp_path / "nothing_here_dir" / "x.npz", device="cpu")
    with pytest.raises(FileNotFoundError):
        ck.make_decoder_policy_fn(d, step=99, device="cpu")


class _StubEnv:
    """An env that records what it is stepped with."""

    def __init__(self, n, obs_w, nu):
        from types import SimpleNamespace
        self.num_envs, self.observation_size, self.action_size, self.device = n, obs_w, nu, torch.device("cpu")
        self.obs = torch.arange(n * obs_w, dtype=torch.float32).reshape(n, obs_w) / 7
        self.actions, self.ns = [], SimpleNamespace

    def _mk(self):
        return self.ns(obs=self.obs, reward=torch.zeros(self.num_envs), done=torch.zeros(self.num_envs))

    def reset(self, rng=None):
        return self._mk()

    def step(self, state, action):
        self.actions.append(action)
        return self._mk()


def test_wrapper_feeds_the_callable_and_the_env():
    from track_mjx_amd.environment import HighLevelWrapper
    env = _StubEnv(5, _OBS, _NU)
    seen = []

    def fn(x):
        seen.append(x)
        return x[:, :_NU] * 2, {"note": 1}
    hl = HighLevelWrapper(env, fn, _REF)
    assert hl.path == "callable" and hl.observation_size == _OBS and hl.num_envs == 5
    st = hl.reset(0)
    lat = torch.randn(5, _Z)
    st2 = hl.step(st, lat)
    assert torch.equal(seen[0], torch.cat([lat, env.obs[:, _REF:]], dim=-1)) and torch.equal(env.actions[0], lat[:, :_NU] * 2)
    assert st2.obs is env.obs
    with pytest.raises(ValueError, match="one row per env"):
        hl.step(st, torch.zeros(4, _Z))
    with pytest.raises(ValueError, match="needs a DecoderPolicy"):
        HighLevelWrapper(env, fn, _REF, path="fused")
    with pytest.raises(ValueError, match="path must be"):
        HighLevelWrapper(env, fn, _REF, path="fastest")
    with pytest.raises(TypeError, match="callable"):
        HighLevelWrapper(env, None, _REF)


def test_wrapper_with_a_decoder_policy_on_the_cpu_and_its_refusals(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.environment import HighLevelWrapper
    _, d = _ckpt(tmp_path)
    dp = ck.make_decoder_policy_fn(d, device="cpu")
    env = _StubEnv(5, _OBS, _NU)
    hl = HighLevelWrapper(env, dp, _REF)
    assert hl.action_size == _Z and hl.path == "callable"          # no device buffers: the policy is called through torch
    lat = torch.randn(5, _Z)
    hl.step(hl.reset(0), lat)
    assert torch.equal(env.actions[0], dp(torch.cat([lat, env.obs[:, _REF:]], dim=-1))[0])
    with pytest.raises(ValueError, match="intention size is 4"):
        hl.step(None, torch.zeros(5, _Z + 1))
    with pytest.raises(ValueError, match="one row per env"):
        hl.step(None, torch.zeros(6, _Z))
    with pytest.raises(ValueError, match="reference_obs_size=12, but the decoder policy was built for 16"):
        HighLevelWrapper(env, dp, 12)
    with pytest.raises(ValueError, match="proprioceptive columns"):
        HighLevelWrapper(_StubEnv(5, _OBS + 2, _NU), dp, _REF)
    with pytest.raises(ValueError, match="controls"):
        HighLevelWrapper(_StubEnv(5, _OBS, _NU + 1), dp, _REF)
    for path in ("fused", "layers"):
        with pytest.raises(ValueError, match="on the env's device"):
            HighLevelWrapper(env, dp, _REF, path=path)


# ---- C-ABI: refused before any device call, with a message (fake device addresses: nothing is touched)
def _desc(n=4096, Z=60, obs_w=696, ref=470, widths=(256, 256), A=38, **over):
    a = 1 << 20
    d = hip.DecoderAct()
    d.latents, d.ldz, d.obs, d.obs_s0, d.obs_s1, d.mean, d.std = a, Z, a, 1, n, a, a
    d.n, d.Z, d.obs_w, d.ref_w, d.n_blocks = n, Z, obs_w, ref, len(widths)
    k = Z + obs_w - ref
    for i, w in enumerate(widths[:4]):
        b = d.block[i]
        b.W, b.bias, b.gamma, b.beta, b.width, b.ldw = a, a, a, a, w, (k + 3) // 4 * 4
        k = w
    d.Wf, d.bf, d.ldwf, d.A, d.eps = a, a, 256, A, 1e-6
    d.action_t, d.ctrl, d.logits, d.ldl = a, a, a, 2 * A
    for key, v in over.items():
        setattr(d, key, v)
    return d


def test_decoder_act_validates_before_it_launches():
    L = hip.lib()
    a = 1 << 20
    assert L.tmjx_decoder_act_ok(C.byref(_desc())) == 1
    assert L.tmjx_decoder_act_ok(C.byref(_desc(widths=(256,), mean=None, std=None, ctrl=None, logits=None, ldl=0))) == 1
    assert L.tmjx_decoder_act_ok(C.byref(_desc(n=1, widths=(256,) * 4))) == 1
    assert L.tmjx_decoder_act_ok(None) == 0 and L.tmjx_decoder_act(None, None) == -22

    def misaligned_block():
        d = _desc()
        d.block[1].W = a + 4
        return d

    def short_ldw():
        d = _desc()
        d.block[0].ldw = 284
        return d
    bad = ((_desc(latents=None), b"null"), (_desc(obs=None), b"null"), (_desc(action_t=None), b"null"), (_desc(Wf=None), b"null"),
           (_desc(mean=None), b"mean and std together"), (_desc(latents=a + 2), b"aligned"), (_desc(action_t=a + 1), b"aligned"),
           (misaligned_block(), b"16-byte aligned"), (short_ldw(), b"ldw"),
           (_desc(widths=(512, 256)), b"256 wide"), (_desc(widths=(256, 128)), b"256 wide"), (_desc(A=65), b"128"), (_desc(A=0), b"128"),
           (_desc(widths=(256,) * 5), b"1 .. 4"), (_desc(widths=()), b"1 .. 4"), (_desc(n=0), b"n >= 1"), (_desc(ldz=59), b"ldz"),
           (_desc(ref=700), b"obs_w"), (_desc(Z=200), b"320"), (_desc(ldl=70), b"ldl"), (_desc(ldwf=255), b"ldwf"))
    for d, word in bad:
        assert L.tmjx_decoder_act_ok(C.byref(d)) == 0, word
        assert L.tmjx_decoder_act(C.byref(d), None) == -22, word
        err = L.tmjx_last_error()
        assert b"tmjx_decoder_act" in err and word in err, (word, err)


def test_decoder_input_validates_before_it_launches():
    L = hip.lib()
    a = 0x10000
    ok = dict(lat=a, ldz=60, obs=a, s0=1, s1=4, mean=a, std=a, x=a, ldx=288, n=4, Z=60, W=696, ref=470)
    for bad in (dict(lat=None), dict(obs=None), dict(x=None), dict(mean=None), dict(ldz=59), dict(ldx=200), dict(n=0), dict(ref=696), dict(x=a + 2)):
        v = dict(ok, **bad)
        assert L.tmjx_decoder_input(*v.values(), None) == -22, bad
        assert b"tmjx_decoder_input" in L.tmjx_last_error()


def test_wrapper_reports_why_a_decoder_does_not_qualify(tmp_path):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.environment.wrappers import decoder_act_why_not
    _, d = _ckpt(tmp_path)
    dp = ck.make_decoder_policy_fn(d, device="cpu")
    assert "256 wide" in decoder_act_why_not(dp, _OBS)
