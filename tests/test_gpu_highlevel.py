"""GPU: the decoder policy inside the env (environment.wrappers.HighLevelWrapper) and the fused decoder launch (tmjx_decoder_act).

The fused kernel against the launches it replaces, bit for bit; the layered wrapper path against the roll-out's policy step and, closed loop, against a
recorded roll-out (bit for bit, NaN bits included); the fused path end to end against a float64 restatement; path selection; no torch op inside `step`;
the CLI's replay_latents."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_rollout import _cfg, _randomise, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5          # tests/test_gpu_rollout.py: the bound the layered kernels are held to against a float64 restatement
Z, W, REF, A = 60, 696, 470, 38
PROP = W - REF


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 5. kernel bits
@pytest.mark.parametrize("n", [1, 3, 257, 4096])
@pytest.mark.parametrize("normalise", [True, False])
@pytest.mark.parametrize("blocks", [1, 2])
def test_decoder_act_is_bit_identical_to_the_launches_it_replaces(n, normalise, blocks):
    from track_mjx_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(1000 * blocks + 10 * n + int(normalise))
    f32 = dict(dtype=torch.float32, device=DEV)
    r = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).to(DEV)      # noqa: E731
    K1, K1p = Z + PROP, (Z + PROP + 3) // 4 * 4
    lat2 = r(n, 2 * Z)                                        # latents in the first Z columns of an [n][2Z] buffer (tmjx_latent_concat_det: ldf >= 2Z)
    obs = (r(W, n, scale=2.0) + 0.5).contiguous()             # the env's layout: [obs][n_env]
    mean = r(W, scale=0.3) if normalise else None
    std = (0.4 + torch.rand(W, generator=g) * 1.5).to(DEV) if normalise else None
    Ws, bs, gs, bes = [], [], [], []
    for l in range(blocks):
        K = K1 if l == 0 else 256
        w = torch.zeros((256, K1p if l == 0 else 256), **f32)
        w[:, :K] = r(256, K, scale=K ** -0.5) + r(256, K, scale=0.05)
        Ws.append(w); bs.append(r(256, scale=0.05)); gs.append(1 + r(256, scale=0.05)); bes.append(r(256, scale=0.05))
    Wf, bf = r(2 * A, 256, scale=0.1 * 256 ** -0.5), r(2 * A, scale=0.05)
    p = lambda t: None if t is None else t.data_ptr()         # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    # ---- the reference: tmjx_latent_concat_det -> tmjx_chain_fwd (decoder blocks + head) -> tmjx_action_mode
    x = torch.full((n, K1p), 7.0, **f32)
    hip.check(L.tmjx_latent_concat_det(p(lat2), 2 * Z, p(obs), 1, n, p(mean), p(std), p(x), K1p, None, 0, n, Z, W, REF, s), "tmjx_latent_concat_det")
    rows = L.tmjx_chain_rows(n)
    d = hip.ChainFwd()
    d.A, d.lda, d.M, d.n_hidden, d.epi, d.eps, d.rows_alloc = p(x), K1p, n, blocks, 1, 1e-6, rows
    keep = []
    for l in range(blocks):
        z, y, st = torch.empty((rows, 256), **f32), torch.empty((rows, 256), **f32), torch.empty((rows, 2), **f32)
        keep += [z, y, st]
        h = d.hidden[l]
        h.W, h.bias, h.gamma, h.beta, h.z, h.y, h.stats, h.K, h.ldw = p(Ws[l]), p(bs[l]), p(gs[l]), p(bes[l]), p(z), p(y), p(st), (K1 if l == 0 else 256), Ws[l].shape[1]
    logits = torch.empty((n, 2 * A), **f32)
    d.Wf, d.bf, d.outf, d.Nf, d.ldwf, d.ldof = p(Wf), p(bf), p(logits), 2 * A, 256, 2 * A
    assert L.tmjx_chain_fwd_ok(C.byref(d)) == 1
    hip.check(L.tmjx_chain_fwd(C.byref(d), s), "tmjx_chain_fwd")
    ctrl, act_t = torch.empty((n, A), **f32), torch.empty((A, n), **f32)
    hip.check(L.tmjx_action_mode(p(logits), 2 * A, p(ctrl), p(act_t), n, A, s), "tmjx_action_mode")
    # ---- the fused launch on the same inputs
    logits2, ctrl2, act2 = torch.full((n, 2 * A), -9.0, **f32), torch.full((n, A), -9.0, **f32), torch.full((A, n), -9.0, **f32)
    e = hip.DecoderAct()
    e.latents, e.ldz, e.obs, e.obs_s0, e.obs_s1, e.mean, e.std = p(lat2), 2 * Z, p(obs), 1, n, p(mean), p(std)
    e.n, e.Z, e.obs_w, e.ref_w, e.n_blocks = n, Z, W, REF, blocks
    for l in range(blocks):
        b = e.block[l]
        b.W, b.bias, b.gamma, b.beta, b.width, b.ldw = p(Ws[l]), p(bs[l]), p(gs[l]), p(bes[l]), 256, Ws[l].shape[1]
    e.Wf, e.bf, e.ldwf, e.A, e.eps = p(Wf), p(bf), 256, A, 1e-6
    e.action_t, e.ctrl, e.logits, e.ldl = p(act2), p(ctrl2), p(logits2), 2 * A
    assert L.tmjx_decoder_act_ok(C.byref(e)) == 1
    hip.check(L.tmjx_decoder_act(C.byref(e), s), "tmjx_decoder_act")
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all() and float(ctrl.abs().max()) > 1e-3
    for name, got, want in (("logits", logits2, logits), ("ctrl", ctrl2, ctrl), ("action_t", act2, act_t)):
        diff = int((_bits(got) != _bits(want)).sum())
        print(f"n={n} normalise={normalise} blocks={blocks} {name}: {diff} of {want.numel()} words differ")
        assert diff == 0, name
    # the optional outputs off: action_t alone, the same bits
    act3 = torch.full((A, n), -9.0, **f32)
    e.action_t, e.ctrl, e.logits, e.ldl = p(act3), None, None, 0
    hip.check(L.tmjx_decoder_act(C.byref(e), s), "tmjx_decoder_act")
    torch.cuda.synchronize()
    assert torch.equal(_bits(act3), _bits(act_t))


# ---------------------------------------------------------------------------------------------------------------- checkpoints / envs
def _make_ckpt(tmp, decoder_layers, seed):
    from tests.common import StubEnv
    from track_mjx_amd.agent.checkpoint import save_step_dir
    from track_mjx_amd.agent.ppo import PPOLearner
    ln = PPOLearner(StubEnv(512), encoder_layers=[512, 256], decoder_layers=list(decoder_layers), critic_layers=[64, 64], latents=60, unroll_length=4,
                    batch_size=256, num_minibatches=8, num_updates_per_batch=1, use_graph=False, seed=3)
    _randomise(ln, seed)
    save_step_dir(tmp, 0, ln, config=_cfg())
    return str(tmp)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    return _make_ckpt(tmp_path_factory.mktemp("hl_ckpt"), (256, 256), 11)


@pytest.fixture(scope="module")
def wide_ckpt(tmp_path_factory):
    return _make_ckpt(tmp_path_factory.mktemp("hl_wide_ckpt"), (512, 256), 12)


def _reset(env, clips, seed=42):
    from track_mjx_amd.analysis.rollout import reset_inputs
    n = len(clips)
    nq, nv = int(env.layout.nq), int(env.layout.nv)
    qn, vn = np.empty((nq, n), np.float32), np.empty((nv, n), np.float32)
    for j, c in enumerate(clips):
        _, qn[:, j], vn[:, j] = reset_inputs(seed, env._n_clips, nq, nv, env._reset_noise_scale, c)
    return env.reset(None, torch.tensor(clips, dtype=torch.int32), start_frame=torch.zeros(n, dtype=torch.int32), qpos_noise=torch.from_numpy(qn),
                     qvel_noise=torch.from_numpy(vn))


def _setup(path, clips, hl_path):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import create_environment
    from track_mjx_amd.environment import HighLevelWrapper
    cfg = ck.load_config_from_checkpoint(path)
    dp = ck.make_decoder_policy_fn(path, device=DEV)
    env = create_environment(cfg, len(clips), DEV)
    hl = HighLevelWrapper(env, dp, dp.reference_obs_size, path=hl_path)
    return cfg, dp, env, hl


_REC: dict = {}


def _recording(path, clips):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import create_environment, create_rollout_generator
    key = (path, tuple(clips))
    if key not in _REC:
        cfg = ck.load_config_from_checkpoint(path)
        fn = ck.load_inference_fn(cfg, ck.load_policy(path, cfg))
        gen = create_rollout_generator(cfg, create_environment(cfg, 1, DEV), fn, model=fn.model, log_activations=True, log_metrics=True)
        _REC[key] = (gen(list(clips)), gen.T)
    return _REC[key]


def _np_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 6. layered path bits
def test_layered_path_reproduces_the_rollout_policys_ctrl(ckpt):
    from track_mjx_amd.agent import checkpoint as ck
    clips = [2, 9, 30]
    cfg, dp, env, hl = _setup(ckpt, clips, "layers")
    assert hl.path == "layers" and hl.action_size == Z and hl.observation_size == W
    fn = ck.load_inference_fn(cfg, ck.load_policy(ckpt, cfg))
    st = _reset(hl, clips)
    ctrl, extras = fn(st.obs.clone())
    intention = extras["activations"]["intention"].contiguous()
    hl.step(st, intention)
    torch.cuda.synchronize()
    assert float(ctrl.abs().max()) > 1e-3
    assert torch.equal(_bits(hl.last_ctrl), _bits(ctrl))


# ---------------------------------------------------------------------------------------------------------------- 7. closed loop
# Clips.  The checkpoint is tests/test_gpu_rollout.py's `mlp_ckpt` (same learner, same seeds, same config), whose roll-outs that file already
# characterises: clips 2 and 9 are its open-loop replay's (bits only: such an untrained, never reset policy may drive the fallen walker's physics to NaN,
# and the comparison includes the NaN bits); clip 3 is the one it holds finite over the first 50 steps, clip 5 the one whose whole roll-out it holds
# within TOL of float64 (so: finite throughout).  The bit-exact closed loop runs on both pairs; the fused path, whose trajectory is its own and which
# is asked to stay finite over that 50-step window, starts from the pair known to be finite there.
NAN_PRONE_CLIPS, FINITE_CLIPS = [2, 9], [3, 5]


@pytest.mark.parametrize("clips", [NAN_PRONE_CLIPS, FINITE_CLIPS])
def test_closed_loop_replay_of_recorded_intentions_is_bit_exact(ckpt, clips):
    from track_mjx_amd.environment.task import METRIC_NAMES
    r, T = _recording(ckpt, clips)
    cfg, dp, env, hl = _setup(ckpt, clips, "layers")
    assert T == int(cfg["reference_config"]["clip_length"] * env._steps_for_cur_frame) and r["ctrl"].shape[1] == T - 1
    lat = torch.from_numpy(np.ascontiguousarray(r["activations"]["intention"])).to(DEV)          # [n, T - 1, Z]
    st = _reset(hl, clips)
    qpos, rew, mets, ctrl = [st.pipeline_state["qpos"].cpu().numpy().copy()], [st.reward.cpu().numpy().copy()], [env.metrics_buf.cpu().numpy().copy()], []
    for t in range(T - 1):
        st = hl.step(st, lat[:, t])                       # (a strided view: rows (T - 1) * Z apart)
        qpos.append(st.pipeline_state["qpos"].cpu().numpy().copy()); rew.append(st.reward.cpu().numpy().copy())
        mets.append(env.metrics_buf.cpu().numpy().copy()); ctrl.append(hl.last_ctrl.cpu().numpy().copy())
    m = np.stack(mets, 1)
    assert np.array_equal(_np_bits(r["qposes_rollout"]), _np_bits(np.stack(qpos, 1)))
    assert np.array_equal(_np_bits(r["state_rewards"]), _np_bits(np.stack(rew, 1)))
    assert np.array_equal(_np_bits(r["ctrl"]), _np_bits(np.stack(ctrl, 1)))
    for k, v in r["rollout_metrics"].items():
        assert np.array_equal(_np_bits(v), _np_bits(m[METRIC_NAMES.index(k[:-1])].T)), k


# ---------------------------------------------------------------------------------------------------------------- 8. fused path end to end
def _first_bad(a):
    """Per clip: the first step at which a [n, T, ...] record is not finite (T if never)."""
    ok = np.isfinite(a.reshape(a.shape[0], a.shape[1], -1)).all(axis=2)
    return [int(np.argmin(row)) if not row.all() else a.shape[1] for row in ok]


def test_fused_path_end_to_end(ckpt):
    clips = FINITE_CLIPS
    r, T = _recording(ckpt, clips)
    # the premise of the clip choice, on the recording itself (the layer-by-layer roll-out): finite over the window asked of the fused path
    print(f"recorded roll-out of clips {clips}: first non-finite step of qpos {_first_bad(r['qposes_rollout'])}, ctrl {_first_bad(r['ctrl'])} (T = {T})")
    assert np.isfinite(r["qposes_rollout"][:, :50]).all() and np.isfinite(r["ctrl"][:, :50]).all()
    cfg, dp, env, hl = _setup(ckpt, clips, "fused")
    assert hl.path == "fused"
    lat = torch.from_numpy(np.ascontiguousarray(r["activations"]["intention"])).to(DEV)
    st = _reset(hl, clips)
    obs0 = st.obs.cpu().double()
    d = lambda t: t.detach().double().cpu()               # noqa: E731
    h = torch.cat([lat[:, 0].cpu().double(), (obs0[:, REF:] - d(dp.mean)) / d(dp.std)], dim=-1)
    for blk in dp.net.decoder:
        z = h @ d(blk.dense.weight).T + d(blk.dense.bias)
        h = torch.nn.functional.layer_norm(torch.nn.functional.silu(z), (z.shape[-1],), d(blk.norm.weight), d(blk.norm.bias), blk.norm.eps)
    want = torch.tanh((h @ d(dp.net.head.weight).T + d(dp.net.head.bias))[:, :A]).numpy()
    qpos, rew, ctrl = [], [], []
    for t in range(T - 1):
        st = hl.step(st, lat[:, t])
        qpos.append(st.pipeline_state["qpos"].cpu().numpy().copy()); rew.append(st.reward.cpu().numpy().copy()); ctrl.append(hl.last_ctrl.cpu().numpy().copy())
    err = _rel(ctrl[0], want)
    print(f"fused path, first step's action against float64: rel err {err:.3e} (bound {TOL})")
    assert err < TOL
    assert len(ctrl) == T - 1
    print(f"fused path: first non-finite step of qpos {_first_bad(np.stack(qpos, 1))}, ctrl {_first_bad(np.stack(ctrl, 1))}; "
          f"max |ctrl - recorded ctrl| over the first 50 steps {float(np.abs(np.stack(ctrl, 1)[:, :50] - r['ctrl'][:, :50]).max()):.3e}")
    for v in (np.stack(qpos, 1), np.stack(rew, 1), np.stack(ctrl, 1)):
        # (finite over the first 50 steps: an untrained policy that is never reset may drive the fallen walker's physics to NaN later on)
        assert v.dtype == np.float32 and np.isfinite(v[:, :50]).all()
    # the generic-callable path (torch concat, the policy's modules, env.step) acts within the same bound on that first observation
    from track_mjx_amd.environment import HighLevelWrapper
    slow = HighLevelWrapper(env, lambda x: dp(x), dp.reference_obs_size)
    st = _reset(slow, clips)
    act, _ = dp(torch.cat([lat[:, 0], st.obs[:, REF:]], dim=-1))
    assert slow.path == "callable" and _rel(act.cpu().numpy(), want) < TOL
    slow.step(st, lat[:, 0])


# ---------------------------------------------------------------------------------------------------------------- 9. path selection
def test_path_selection(ckpt, wide_ckpt):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.environment import HighLevelWrapper
    cfg, dp, env, hl = _setup(ckpt, [0, 1], "auto")
    # "auto" is the fused launch where it qualifies — as long as the measurement keeps it the default (HighLevelWrapper.AUTO_PREFERS_FUSED)
    assert hl.path == ("fused" if HighLevelWrapper.AUTO_PREFERS_FUSED else "layers")
    assert HighLevelWrapper(env, dp, dp.reference_obs_size, path="fused").path == "fused"
    wide = ck.make_decoder_policy_fn(wide_ckpt, device=DEV)
    assert wide.decoder_layer_sizes == (512, 256)
    assert HighLevelWrapper(env, wide, wide.reference_obs_size, path="auto").path == "layers"
    with pytest.raises(ValueError, match="256 wide"):
        HighLevelWrapper(env, wide, wide.reference_obs_size, path="fused")
    with pytest.raises(ValueError, match="intention size is 60"):
        hl.step(None, torch.zeros((2, 61), device=DEV))
    with pytest.raises(ValueError, match="one row per env"):
        hl.step(None, torch.zeros((3, 60), device=DEV))
    with pytest.raises(ValueError, match="latents are on cpu"):
        hl.step(None, torch.zeros((2, 60)))
    # the wide decoder steps through the layered list
    hw = HighLevelWrapper(env, wide, wide.reference_obs_size)
    st = _reset(hw, [0, 1])
    lat = torch.randn((2, 60), generator=torch.Generator().manual_seed(0)).to(DEV) * 0.3
    want, _ = wide(torch.cat([lat, st.obs[:, REF:]], dim=-1))
    hw.step(st, lat)
    torch.cuda.synchronize()
    assert _rel(hw.last_ctrl.cpu().numpy(), want.cpu().numpy()) < 2 * TOL          # (two float32 paths, each within TOL of the exact decoder)


# ---------------------------------------------------------------------------------------------------------------- 10. no torch op in step
@pytest.mark.parametrize("hl_path", ["layers", "fused"])
def test_no_torch_ops_inside_step_after_the_first_call(ckpt, hl_path):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))

    clips = [1, 4, 6]
    cfg, dp, env, hl = _setup(ckpt, clips, hl_path)
    st = _reset(hl, clips)
    lats = [(torch.randn((3, 60), generator=torch.Generator().manual_seed(i)) * 0.3).to(DEV) for i in range(6)]
    st = hl.step(st, lats[0])
    Count.n = 0
    with Count():
        for lat in lats[1:]:
            st2 = hl.step(st, lat)
    assert Count.n == 0 and st2 is st
    torch.cuda.synchronize()
    assert torch.isfinite(st.obs).all()


# ---------------------------------------------------------------------------------------------------------------- 11. CLI
def test_cli_replay_latents_reproduces_the_rollout(tmp_path):
    from track_mjx_amd import train
    from track_mjx_amd.analysis.utils import load_from_h5py
    d = tmp_path / "run"
    train.main(["train_setup.train_config.num_envs=256", "train_setup.train_config.batch_size=64", "train_setup.train_config.num_minibatches=4",
                "train_setup.train_config.unroll_length=5", "train_setup.train_config.num_updates_per_batch=1", "network_config.encoder_layer_sizes=[64,64]",
                "network_config.decoder_layer_sizes=[64,64]", "network_config.critic_layer_sizes=[64,64]", "train_setup.train_config.num_timesteps=6400",
                "train_setup.eval_every=640", "train_setup.reset_every=640", "n_synthetic_clips=4", "train_setup.train_config.num_eval_envs=0",
                f"checkpoint_path={d}", "max_training_steps=2"])
    out, out2 = tmp_path / "rollouts", tmp_path / "replayed"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = lambda *a: subprocess.run([sys.executable, "-m", "track_mjx_amd.analysis.rollout", f"checkpoint={d}", "seed=7", *a],      # noqa: E731
                                    capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=root)
    res = run("clips=1,3", f"out={out}")
    assert res.returncode == 0, res.stderr[-3000:]
    res = run(f"replay_latents={out}", f"out={out2}", "path=layers")
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out2)) == ["clip_1.h5", "clip_3.h5"]
    for c in (1, 3):
        a, b = load_from_h5py(out / f"clip_{c}.h5"), load_from_h5py(out2 / f"clip_{c}.h5")
        for k in ("qposes_rollout", "ctrl", "state_rewards", "qposes_ref"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (c, k)
        assert set(b["activations"]) == {"intention"} and np.asarray(b["activations"]["intention"]).tobytes() == np.asarray(a["activations"]["intention"]).tobytes()
        assert int(b["meta"]["clip_idx"]) == c and float(b["meta"]["latent_scale"]) == 1.0
    res = run(f"replay_latents={out}", f"out={tmp_path / 'scaled'}", "path=layers", "latent_scale=0.5")
    assert res.returncode == 0, res.stderr[-3000:]
    s = load_from_h5py(tmp_path / "scaled" / "clip_1.h5")
    assert np.asarray(s["ctrl"]).tobytes() != np.asarray(load_from_h5py(out / "clip_1.h5")["ctrl"]).tobytes()
