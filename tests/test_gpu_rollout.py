"""GPU: checkpoint roll-outs (track_mjx_amd.analysis.rollout) against what they must reproduce — the reference's output dict, the clip table,
an open-loop replay of the recorded controls through a plain env (bit-exact), a float64 restatement of the policy on the recorded normalised
observations (MLP and LSTM), batch independence, no torch op inside the step loop, and the CLI's .h5 files."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_CLIPS = 70
TOL = 5e-5


def _cfg(name=None, overrides=()):
    from track_mjx_amd import config as _config
    return _config.load_config(None, [f"n_synthetic_clips={N_CLIPS}", *overrides], name=name)


@torch.no_grad()
def _randomise(learner, seed):
    g = torch.Generator().manual_seed(seed)
    for p in learner.policy.parameters():
        p.add_((torch.randn(p.shape, generator=g) * 0.05).to(p.device))
    head = getattr(learner.policy, "head", None) or learner.policy.projection
    head.weight.mul_(0.1)          # moderate controls: the walker tracks for a while instead of flailing (a roll-out never resets)
    nz = learner.normalizer
    W = nz.mean.numel()
    nz.mean.copy_((torch.randn(W, generator=g) * 0.3).to(nz.mean.device))
    nz.std.copy_((0.4 + torch.rand(W, generator=g) * 1.5).to(nz.std.device))
    nz.count.fill_(1234.0)


@pytest.fixture(scope="module")
def mlp_ckpt(tmp_path_factory):
    from tests.common import StubEnv
    from track_mjx_amd.agent.checkpoint import save_step_dir
    from track_mjx_amd.agent.ppo import PPOLearner
    ln = PPOLearner(StubEnv(512), encoder_layers=[512, 256], decoder_layers=[256, 256], critic_layers=[64, 64], latents=60, unroll_length=4,
                    batch_size=256, num_minibatches=8, num_updates_per_batch=1, use_graph=False, seed=3)
    _randomise(ln, 11)
    d = tmp_path_factory.mktemp("mlp_ckpt")
    save_step_dir(d, 0, ln, config=_cfg())
    return str(d), ln


@pytest.fixture(scope="module")
def lstm_ckpt(tmp_path_factory):
    from track_mjx_amd.agent.checkpoint import save_step_dir
    from track_mjx_amd.agent.lstm import LSTMPPOLearner
    from track_mjx_amd.analysis.rollout import create_environment
    cfg = _cfg(overrides=["train_setup.train_config.use_lstm=true"])
    env = create_environment(cfg, 256, DEV)
    ln = LSTMPPOLearner(env, encoder_layers=(256, 256), decoder_layers=(256, 256), critic_layers=(64, 64), latents=60, unroll_length=4, batch_size=64,
                        num_minibatches=4, num_updates_per_batch=1, seed=0, hidden_state_size=128, hidden_layer_num=2)
    _randomise(ln, 12)
    d = tmp_path_factory.mktemp("lstm_ckpt")
    save_step_dir(d, 0, ln, config=cfg)
    return str(d), ln


def _generator(path, name=None, **kw):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import create_environment, create_rollout_generator
    cfg = ck.load_config_from_checkpoint(path)
    if name is not None:
        cfg = _cfg(name, ["train_setup.train_config.use_lstm=" + str(cfg["train_setup"]["train_config"]["use_lstm"]).lower()])
    fn = ck.load_inference_fn(cfg, ck.load_policy(path, cfg))
    env = create_environment(cfg, 1, DEV)
    return create_rollout_generator(cfg, env, fn, model=fn.model, log_activations=True, log_metrics=True, **kw), env, fn, cfg


_GEN: dict = {}


def _gen(path, name=None):
    if (path, name) not in _GEN:
        _GEN[(path, name)] = _generator(path, name)
    return _GEN[(path, name)]


@pytest.mark.parametrize("name,T", [("rodent-full-clips", 250), ("rodent-sps-per-actor", 500)])
def test_shapes_and_keys_match_the_reference_dict(mlp_ckpt, name, T):
    from track_mjx_amd.analysis.rollout import ROLLOUT_METRICS
    gen, env, fn, cfg = _gen(mlp_ckpt[0], name)
    r = gen(3)
    nq, nu = int(env.layout.nq), int(env.layout.nu)
    assert set(r) == {"qposes_ref", "qposes_rollout", "ctrl", "state_rewards", "rollout_metrics", "activations"}
    assert r["qposes_ref"].shape == (T, nq) and r["qposes_rollout"].shape == (T, nq) and r["ctrl"].shape == (T - 1, nu)
    assert r["state_rewards"].shape == (T,)
    assert set(r["rollout_metrics"]) == {f"{m}s" for m in ROLLOUT_METRICS} and all(v.shape == (T,) for v in r["rollout_metrics"].values())
    a = r["activations"]
    assert set(a) == {"encoder", "decoder", "egocentric_obs", "traj_obs", "intention"}
    assert set(a["encoder"]) == {"layer_0", "layer_1", "mean", "logvar"} and set(a["decoder"]) == {"layer_0", "layer_1"}
    assert a["encoder"]["layer_0"].shape == (T - 1, 512) and a["encoder"]["mean"].shape == (T - 1, 60) and a["decoder"]["layer_1"].shape == (T - 1, 256)
    assert a["traj_obs"].shape == (T - 1, 470) and a["egocentric_obs"].shape == (T - 1, 696 - 470) and a["intention"].shape == (T - 1, 60)
    for v in [r["qposes_rollout"], r["ctrl"], r["state_rewards"], a["encoder"]["mean"], a["intention"]]:
        # (finite over the first 50 steps: an untrained policy that is never reset may drive the fallen walker's physics to NaN later on,
        # as brax's pipeline would; the replay test compares bits, NaN included)
        assert v.dtype == np.float32 and np.isfinite(v[:50]).all()
    assert np.array_equal(a["intention"], a["encoder"]["mean"])            # z = latent_mean exactly
    assert (r["state_rewards"][0] == 0) and np.abs(r["state_rewards"][1:]).max() > 0


def test_reference_qpos_is_the_clip_table(mlp_ckpt):
    gen, env, _, _ = _gen(mlp_ckpt[0])
    for c in (0, 17):
        r = gen(c)
        t = env._reference_clips
        want = np.hstack([np.asarray(t.position[c], np.float32), np.asarray(t.quaternion[c], np.float32), np.asarray(t.joints[c], np.float32)])
        assert np.array_equal(r["qposes_ref"], want)


def _replay(env_cfg, rec, clips, seed=42):
    """A plain env with the roll-out's reset inputs, stepped with the recorded ctrl: (qpos [n, T, nq], reward [n, T], metrics, raw obs [n, T-1, W])."""
    from track_mjx_amd.analysis.rollout import create_environment, reset_inputs
    from track_mjx_amd.environment.task import METRIC_NAMES
    n = len(clips)
    env = create_environment(env_cfg, n, DEV)
    nq, nv = int(env.layout.nq), int(env.layout.nv)
    qn, vn = np.empty((nq, n), np.float32), np.empty((nv, n), np.float32)
    for j, c in enumerate(clips):
        _, qn[:, j], vn[:, j] = reset_inputs(seed, env._n_clips, nq, nv, env._reset_noise_scale, c)
    st = env.reset(None, torch.tensor(clips, dtype=torch.int32), start_frame=torch.zeros(n, dtype=torch.int32), qpos_noise=torch.from_numpy(qn),
                   qvel_noise=torch.from_numpy(vn))
    T = rec["ctrl"].shape[1] + 1
    qpos, rew, obs = [st.pipeline_state["qpos"].cpu().numpy().copy()], [st.reward.cpu().numpy().copy()], []
    mets = [env.metrics_buf.cpu().numpy().copy()]
    for t in range(T - 1):
        obs.append(st.obs.cpu().numpy().copy())
        st = env.step(st, torch.from_numpy(np.ascontiguousarray(rec["ctrl"][:, t])).to(DEV))
        qpos.append(st.pipeline_state["qpos"].cpu().numpy().copy()); rew.append(st.reward.cpu().numpy().copy())
        mets.append(env.metrics_buf.cpu().numpy().copy())
    m = np.stack(mets, 1)
    return np.stack(qpos, 1), np.stack(rew, 1), {name: m[i].T for i, name in enumerate(METRIC_NAMES)}, np.stack(obs, 1)


def test_open_loop_replay_is_bit_exact(mlp_ckpt):
    gen, env, fn, cfg = _gen(mlp_ckpt[0])
    clips = [2, 9]
    r = gen(clips)
    qpos, rew, mets, _ = _replay(cfg, r, clips)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)     # noqa: E731  (NaN == NaN when the bits are the same)
    assert np.array_equal(bits(r["qposes_rollout"]), bits(qpos))
    assert np.array_equal(bits(r["state_rewards"]), bits(rew))
    for k, v in r["rollout_metrics"].items():
        assert np.array_equal(bits(v), bits(mets[k[:-1]])), k


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _f64_encoder(pol, traj):
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    acts, h = {}, traj
    for i, blk in enumerate(pol.encoder):
        z = h @ d(blk.dense.weight).T + d(blk.dense.bias)
        h = torch.nn.functional.layer_norm(torch.nn.functional.silu(z), (z.shape[-1],), d(blk.norm.weight), d(blk.norm.bias), blk.norm.eps)
        acts[f"layer_{i}"] = h
    fc2 = h @ d(pol.fc2.weight).T + d(pol.fc2.bias)
    Z = pol.latents
    acts["mean"], acts["logvar"] = fc2[..., :Z], fc2[..., Z:]
    return acts


def test_teacher_forced_mlp_policy(mlp_ckpt):
    gen, env, fn, cfg = _gen(mlp_ckpt[0])
    clips = [5]
    r = gen(clips)
    _, _, _, obs = _replay(cfg, r, clips)
    a = r["activations"]
    pol = fn.policy
    mean, std = fn.mean.cpu().numpy(), fn.std.cpu().numpy()
    norm = (obs[0] - mean) / std
    assert np.array_equal(a["traj_obs"][0], norm[:, :470]) and np.array_equal(a["egocentric_obs"][0], norm[:, 470:])
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    enc = _f64_encoder(pol, torch.from_numpy(a["traj_obs"][0]).double())
    for k, v in enc.items():
        assert _rel(a["encoder"][k][0], v.numpy()) < TOL, k
    x = torch.cat([torch.from_numpy(a["intention"][0]).double(), torch.from_numpy(a["egocentric_obs"][0]).double()], -1)
    h = x
    for i, blk in enumerate(pol.decoder):
        z = h @ d(blk.dense.weight).T + d(blk.dense.bias)
        h = torch.nn.functional.layer_norm(torch.nn.functional.silu(z), (z.shape[-1],), d(blk.norm.weight), d(blk.norm.bias), blk.norm.eps)
        assert _rel(a["decoder"][f"layer_{i}"][0], h.numpy()) < TOL, i
        h = torch.from_numpy(a["decoder"][f"layer_{i}"][0]).double()           # teacher forcing: the next layer from the recorded one
    logits = h @ d(pol.head.weight).T + d(pol.head.bias)
    ctrl = torch.tanh(logits[:, :pol.action_size])
    assert _rel(r["ctrl"][0], ctrl.numpy()) < TOL


def test_teacher_forced_lstm_policy(lstm_ckpt):
    gen, env, fn, cfg = _gen(lstm_ckpt[0])
    r = gen([4])
    a = r["activations"]
    assert set(a) == {"encoder", "decoder", "intention", "hidden_state"} and set(a["decoder"]) == {"lstm_projection"}
    h_all, c_all = a["hidden_state"]
    T = r["ctrl"].shape[1] + 1
    assert h_all.shape == (1, T - 1, 2, 128) and c_all.shape == (1, T - 1, 2, 128)
    _, _, _, obs = _replay(cfg, r, [4])
    pol = fn.policy
    norm = (obs[0] - fn.mean.cpu().numpy()) / fn.std.cpu().numpy()
    traj = torch.from_numpy(norm[:, :470]).double()
    enc = _f64_encoder(pol, traj)
    for k, v in enc.items():
        assert _rel(a["encoder"][k][0], v.numpy()) < TOL, k
    assert np.array_equal(a["intention"][0], a["encoder"]["mean"][0])
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    x = torch.cat([torch.from_numpy(a["intention"][0]).double(), torch.from_numpy(norm[:, 470:]).double()], -1)
    h_rec, c_rec = torch.from_numpy(h_all[0]).double(), torch.from_numpy(c_all[0]).double()
    H = pol.hidden_state_size
    h_prev, c_prev = torch.zeros_like(h_rec), torch.zeros_like(c_rec)
    h_prev[1:], c_prev[1:] = h_rec[:-1], c_rec[:-1]                              # the recorded carry of the step before (zero at t = 0)
    inp = x
    for k in range(pol.hidden_layer_num):
        g = inp @ d(pol.w_ih[k]).T + h_prev[:, k] @ d(pol.w_hh[k]).T + d(pol.b_hh[k])
        i_, f_, g_, o_ = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c = f_ * c_prev[:, k] + i_ * g_
        h = o_ * torch.tanh(c)
        assert _rel(c_rec[:, k], c) < TOL and _rel(h_rec[:, k], h) < TOL, k
        inp = h_rec[:, k]
    logits = inp @ d(pol.projection.weight).T + d(pol.projection.bias)
    assert _rel(a["decoder"]["lstm_projection"][0], logits.numpy()) < TOL
    assert _rel(r["ctrl"][0], torch.tanh(logits[:, :pol.action_size]).numpy()) < TOL


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], path + "/" + k)
    elif isinstance(a, tuple):
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}/{i}")
    else:
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                          b.view(np.uint32) if b.dtype == np.float32 else b), path


def _pick(tree, j):
    if isinstance(tree, dict):
        return {k: _pick(v, j) for k, v in tree.items()}
    if isinstance(tree, tuple):
        return tuple(_pick(v, j) for v in tree)
    return tree[j]


@pytest.mark.parametrize("which", ["mlp", "lstm"])
def test_batch_independence(mlp_ckpt, lstm_ckpt, which):
    path = (mlp_ckpt if which == "mlp" else lstm_ckpt)[0]
    gen, _, _, _ = _gen(path)
    k = 7
    alone = gen(k)
    batch = gen(list(range(64)))
    perm = list(np.random.default_rng(1).permutation(64))
    pb = gen(perm)
    _same(alone, _pick(batch, k))
    _same(alone, _pick(pb, perm.index(k)))


def test_no_torch_ops_inside_the_step_loop(mlp_ckpt, monkeypatch):
    from torch.utils._python_dispatch import TorchDispatchMode
    from track_mjx_amd.analysis import rollout as ro

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))

    calls = []
    orig = ro._step_loop

    def counted(*a, **kw):
        with Count():
            orig(*a, **kw)
        calls.append(Count.n)

    monkeypatch.setattr(ro, "_step_loop", counted)
    gen, _, _, _ = _generator(mlp_ckpt[0])
    gen(list(range(64)))
    assert calls == [0]


def test_cli_writes_one_h5_per_clip(tmp_path):
    from track_mjx_amd import train
    from track_mjx_amd.analysis.utils import load_from_h5py
    d = tmp_path / "run"
    train.main(["train_setup.train_config.num_envs=256", "train_setup.train_config.batch_size=64", "train_setup.train_config.num_minibatches=4",
                "train_setup.train_config.unroll_length=5", "train_setup.train_config.num_updates_per_batch=1", "network_config.encoder_layer_sizes=[64,64]",
                "network_config.decoder_layer_sizes=[64,64]", "network_config.critic_layer_sizes=[64,64]", "train_setup.train_config.num_timesteps=6400",
                "train_setup.eval_every=640", "train_setup.reset_every=640", "n_synthetic_clips=4", "train_setup.train_config.num_eval_envs=0",
                f"checkpoint_path={d}", "max_training_steps=2"])
    out = tmp_path / "rollouts"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-m", "track_mjx_amd.analysis.rollout", f"checkpoint={d}", "clips=1,3", "seed=7", f"out={out}"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=root)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == ["clip_1.h5", "clip_3.h5"]
    gen, _, _, _ = _generator(str(d))
    for c in (1, 3):
        got = load_from_h5py(out / f"clip_{c}.h5")
        meta = got.pop("meta")
        assert int(meta["clip_idx"]) == c and int(meta["seed"]) == 7 and int(meta["checkpoint_step"]) == 2
        assert bytes(meta["rollout_gemm_inputs"]) == b"f32"
        _same_loaded(gen(c, seed=7), got)


def _same_loaded(want, got, path=""):
    if isinstance(want, dict):
        assert set(want) == set(got), (path, set(want) ^ set(got))
        for k in want:
            _same_loaded(want[k], got[k], path + "/" + k)
    else:
        w, g = np.asarray(want), np.asarray(got)
        assert w.dtype == g.dtype and w.shape == g.shape and w.tobytes() == g.tobytes(), path
