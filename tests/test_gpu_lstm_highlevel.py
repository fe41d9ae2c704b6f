"""GPU: the LSTM decoder policy inside the env (HighLevelWrapper with an LSTMDecoderPolicy) and the fused launch tmjx_lstm_decoder_act.

The fused kernel and the layered launch list against a float64 restatement over carried steps with resets (and what they must not write); the layered
wrapper path against the roll-out's LSTM policy step and, closed loop, against a recorded roll-out (bit for bit); the fused path end to end against
float64; path selection; no torch op inside `step`; the CLI's replay_latents on a use_lstm run."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_highlevel import _bits, _make_ckpt, _np_bits, _recording, _reset
from tests.test_gpu_rollout import _cfg, _rel, lstm_ckpt  # noqa: F401  (lstm_ckpt: the module-scoped use_lstm checkpoint fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 5e-5          # tests/test_gpu_rollout.py: the bound the project's policy kernels are held to against a float64 restatement
Z, W, REF, A, H = 60, 696, 470, 38, 128
PROP = W - REF
POISON = -7.0


def _f64_step(x, layers, wp, bp, h, c, reset):
    """One decoder step in float64 on the CPU: x [n, K1] (already normalised), the carry h / c [n, L, H] updated in place."""
    if reset is not None:
        keep = (reset == 0).double()[:, None, None]
        h.mul_(keep); c.mul_(keep)
    a = x
    for k, (wi, wh, bh) in enumerate(layers):
        g = a @ wi.T + h[:, k] @ wh.T + bh
        i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c[:, k] = f * c[:, k] + i * gg
        h[:, k] = o * torch.tanh(c[:, k])
        a = h[:, k].clone()
    return a @ wp.T + bp


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("n", [1, 3, 33, 257])
@pytest.mark.parametrize("normalise", [True, False])
@pytest.mark.parametrize("L", [1, 2])
def test_lstm_decoder_act_against_float64_over_carried_steps(n, normalise, L):
    from track_mjx_amd import hip
    lib = hip.lib()
    g = torch.Generator().manual_seed(1000 * L + 10 * n + int(normalise))
    f32 = dict(dtype=torch.float32, device=DEV)
    r = lambda *s, scale=1.0: torch.randn(s, generator=g) * scale      # noqa: E731
    p = lambda t: None if t is None else t.data_ptr()                  # noqa: E731
    K1, K1p, ld, ldl, ldz, STEPS = Z + PROP, (Z + PROP + 3) // 4 * 4, L * H + 4, 2 * A + 4, Z + 4, 6
    mean = r(W, scale=0.3) if normalise else None
    std = (0.4 + torch.rand(W, generator=g) * 1.5) if normalise else None
    layers = []
    for k in range(L):
        K = K1 if k == 0 else H
        layers.append((r(4 * H, K, scale=K ** -0.5), r(4 * H, H, scale=H ** -0.5), r(4 * H, scale=0.1)))
    wp, bp = r(2 * A, H, scale=H ** -0.5), r(2 * A, scale=0.05)
    lats = [r(n, Z) for _ in range(STEPS)]
    obss = [r(W, n, scale=2.0) + 0.5 for _ in range(STEPS)]            # the env's layout: [obs][n_env]
    flags = (torch.arange(n) % 3 == 0).float()
    resets = [flags if t in (2, 4) else None for t in range(STEPS)]
    # ---- float64 on the CPU
    h64, c64 = torch.zeros((n, L, H), dtype=torch.float64), torch.zeros((n, L, H), dtype=torch.float64)
    l64 = [tuple(t.double() for t in y) for y in layers]
    want = []
    for t in range(STEPS):
        prop = obss[t].double().T[:, REF:]
        if normalise:
            prop = (prop - mean.double()[REF:]) / std.double()[REF:]
        lg = _f64_step(torch.cat([lats[t].double(), prop], dim=-1), l64, wp.double(), bp.double(), h64, c64, resets[t])
        want.append((lg.clone(), torch.tanh(lg[:, :A]), h64.clone(), c64.clone()))
    # ---- device operands
    dev = lambda t: None if t is None else t.to(DEV).contiguous()      # noqa: E731
    mean_d, std_d, wp_d, bp_d, flags_d = dev(mean), dev(std), dev(wp), dev(bp), dev(flags)
    wi_d, wh_d, bh_d = [], [], []
    for k, (wi, wh, bh) in enumerate(layers):
        buf = torch.zeros((4 * H, K1p if k == 0 else H), **f32)
        buf[:, :wi.shape[1]] = wi.to(DEV)
        wi_d.append(buf); wh_d.append(dev(wh)); bh_d.append(dev(bh))
    lat_d = torch.full((n, ldz), 3.0, **f32)
    obs_d = torch.empty((W, n), **f32)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def guarded(rows, cols):          # a [rows][cols] view at the front of a poisoned allocation with 64 guard floats behind it
        flat = torch.full((rows * cols + 64,), POISON, **f32)
        return flat, flat[:rows * cols].view(rows, cols)
    out = {k: guarded(*shape) for k, shape in (("h", (n, ld)), ("c", (n, ld)), ("logits", (n, ldl)), ("ctrl", (n, A)), ("action_t", (A, n)))}
    hF, cF, lgF, ctF, atF = (out[k][1] for k in ("h", "c", "logits", "ctrl", "action_t"))
    hF[:, :L * H] = 0; cF[:, :L * H] = 0
    e = hip.LstmDecoderAct()
    e.latents, e.ldz, e.obs, e.obs_s0, e.obs_s1, e.mean, e.std = p(lat_d), ldz, p(obs_d), 1, n, p(mean_d), p(std_d)
    e.n, e.Z, e.obs_w, e.ref_w, e.L, e.H = n, Z, W, REF, L, H
    for k in range(L):
        y = e.layer[k]
        y.Wi, y.Wh, y.bh, y.ldwi, y.ldwh = p(wi_d[k]), p(wh_d[k]), p(bh_d[k]), wi_d[k].shape[1], H
    e.Wp, e.bp, e.ldwp, e.A = p(wp_d), p(bp_d), H, A
    e.h, e.c, e.ld = p(hF), p(cF), ld
    e.action_t, e.ctrl, e.logits, e.ldl = p(atF), p(ctF), p(lgF), ldl
    assert lib.tmjx_lstm_decoder_act_ok(C.byref(e)) == 1
    # ---- the layered list (existing kernels) on its own carry
    hL, cL = torch.zeros((n, ld), **f32), torch.zeros((n, ld), **f32)
    x, xg = torch.zeros((n, K1p), **f32), torch.empty((n, 4 * H), **f32)
    lgL, ctL, atL = torch.empty((n, 2 * A), **f32), torch.empty((n, A), **f32), torch.empty((A, n), **f32)
    worst = {"fused": 0.0, "layered": 0.0}
    differ = total = 0
    for t in range(STEPS):
        lat_d[:, :Z] = lats[t].to(DEV); obs_d.copy_(obss[t])
        rp = p(flags_d) if resets[t] is not None else None
        e.reset = rp
        hip.check(lib.tmjx_lstm_decoder_act(C.byref(e), s), "tmjx_lstm_decoder_act")
        hip.check(lib.tmjx_decoder_input(p(lat_d), ldz, p(obs_d), 1, n, p(mean_d), p(std_d), p(x), K1p, n, Z, W, REF, s), "tmjx_decoder_input")
        a, lda = x, K1p
        for k in range(L):
            hip.check(lib.tmjx_linear_nolds(p(a), lda, 1, p(wi_d[k]), None, p(xg), n, 4 * H, wi_d[k].shape[1], s), "tmjx_linear_nolds")
            hk, ck = hL[:, k * H:], cL[:, k * H:]
            args = hip.LstmFwd(p(xg), 4 * H, p(wh_d[k]), H, p(bh_d[k]), p(hk), p(ck), ld, rp, n, p(hk), p(ck), ld, None, None, 1, n, H)
            hip.check(lib.tmjx_lstm_seq_fwd(C.byref(args), s), "tmjx_lstm_seq_fwd")
            a, lda = hk, ld
        hip.check(lib.tmjx_linear_nolds(p(a), lda, 1, p(wp_d), p(bp_d), p(lgL), n, 2 * A, H, s), "tmjx_linear_nolds")
        hip.check(lib.tmjx_action_mode(p(lgL), 2 * A, p(ctL), p(atL), n, A, s), "tmjx_action_mode")
        torch.cuda.synchronize()
        lg64, act64, hw, cw = want[t]
        for which, got in (("fused", (lgF[:, :2 * A], ctF, hF[:, :L * H], cF[:, :L * H])), ("layered", (lgL, ctL, hL[:, :L * H], cL[:, :L * H]))):
            errs = [_rel(got[0].cpu().numpy(), lg64.numpy()), _rel(got[1].cpu().numpy(), act64.numpy()),
                    _rel(got[2].cpu().numpy(), hw.reshape(n, -1).numpy()), _rel(got[3].cpu().numpy(), cw.reshape(n, -1).numpy())]
            worst[which] = max(worst[which], *errs)
            assert all(np.isfinite(v) for v in errs)
        assert torch.equal(_bits(atF), _bits(ctF.t().contiguous()))                  # action_t is the transpose of ctrl, exactly
        for a_, b_ in ((lgF[:, :2 * A], lgL), (ctF, ctL), (hF[:, :L * H], hL[:, :L * H]), (cF[:, :L * H], cL[:, :L * H])):
            differ += int((_bits(a_) != _bits(b_)).sum()); total += a_.numel()
    print(f"n={n} normalise={normalise} L={L}: worst rel err against float64 over {STEPS} steps: fused {worst['fused']:.3e}, layered {worst['layered']:.3e} "
          f"(bound {TOL}); fused and layered differ in {differ} of {total} words")
    assert float(ctF.abs().max()) > 1e-3 and float(hF[:, :L * H].abs().max()) > 1e-3
    assert worst["layered"] < TOL, "the inputs are too wild for the float32 kernels"
    assert worst["fused"] < TOL
    # nothing outside the documented extents was written: pad columns, guard floats behind the last row
    assert bool((hF[:, L * H:] == POISON).all()) and bool((cF[:, L * H:] == POISON).all()) and bool((lgF[:, 2 * A:] == POISON).all())
    for k, (flat, view) in out.items():
        assert bool((flat[view.numel():] == POISON).all()), k
    # the optional outputs off: action_t and the carry alone
    flat2, at2 = guarded(A, n)
    e.action_t, e.ctrl, e.logits, e.ldl, e.reset = p(at2), None, None, 0, None
    hip.check(lib.tmjx_lstm_decoder_act(C.byref(e), s), "tmjx_lstm_decoder_act")
    torch.cuda.synchronize()
    assert torch.isfinite(at2).all() and bool((flat2[A * n:] == POISON).all()) and bool((lgF[:, 2 * A:] == POISON).all())


# ---------------------------------------------------------------------------------------------------------------- checkpoints / envs
def _setup(path, clips, hl_path, **kw):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import create_environment
    from track_mjx_amd.environment import HighLevelWrapper
    cfg = ck.load_config_from_checkpoint(path)
    dp = ck.make_lstm_decoder_policy_fn(path, device=DEV)
    env = create_environment(cfg, len(clips), DEV)
    hl = HighLevelWrapper(env, dp, dp.reference_obs_size, path=hl_path, **kw)
    return cfg, dp, env, hl


@pytest.fixture(scope="module")
def h64_ckpt(tmp_path_factory):
    """A use_lstm checkpoint with H = 64 (policy.npz + config/metadata of a step directory): the fused launch does not take it."""
    from tests.test_lstm_highlevel_cpu import _save
    from track_mjx_amd.agent.lstm import LSTMIntentionPolicy
    torch.manual_seed(5)
    pol = LSTMIntentionPolicy(W, REF, A, Z, (64,), 64, 2)
    g = torch.Generator().manual_seed(6)
    norm = {"count": np.float32(9.0), "mean": (torch.randn(W, generator=g) * 0.3).numpy(), "summed_variance": np.ones(W, np.float32),
            "std": (0.4 + torch.rand(W, generator=g) * 1.5).numpy()}
    return _save(tmp_path_factory.mktemp("lstm_h64_ckpt"), 0, pol, norm, _cfg(overrides=["train_setup.train_config.use_lstm=true"]))


# ---------------------------------------------------------------------------------------------------------------- layered path bits
def test_layered_path_reproduces_the_rollout_lstm_policy_step(lstm_ckpt):  # noqa: F811
    from track_mjx_amd.agent import checkpoint as ck
    path = lstm_ckpt[0]
    clips = [2, 9, 30, 1, 4, 6, 11, 17]
    cfg, dp, env, hl = _setup(path, clips, "layers", reset_carry_on_done=False)
    assert hl.path == "layers" and hl.action_size == Z and hl.observation_size == W and (dp.hidden_layer_num, dp.hidden_state_size) == (2, H)
    fn = ck.load_inference_fn(cfg, ck.load_policy(path, cfg))
    st = _reset(hl, clips)
    carry = None
    for t in range(3):
        ctrl, extras, carry = fn(st.obs.clone(), hidden_state=carry)
        intention = extras["activations"]["intention"].contiguous()
        st = hl.step(st, intention)
        torch.cuda.synchronize()
        assert float(ctrl.abs().max()) > 1e-3
        assert torch.equal(_bits(hl.last_ctrl), _bits(ctrl)), t
        assert torch.equal(_bits(hl.hidden_state[0]), _bits(carry[0])) and torch.equal(_bits(hl.hidden_state[1]), _bits(carry[1])), t
    assert float(carry[0].abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- closed loop
def test_closed_loop_replay_of_a_recorded_lstm_rollout_is_bit_exact(lstm_ckpt):  # noqa: F811
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import replay_latents
    path = lstm_ckpt[0]
    clips = [2, 9]
    r, T = _recording(path, clips)
    cfg = ck.load_config_from_checkpoint(path)
    dp = ck.make_lstm_decoder_policy_fn(path, device=DEV)
    res = replay_latents(cfg, dp, clips, np.ascontiguousarray(r["activations"]["intention"]), path="layers")
    assert res["path"] == "layers" and res["ctrl"].shape == r["ctrl"].shape and r["ctrl"].shape[1] == T - 1
    assert np.array_equal(_np_bits(r["qposes_rollout"]), _np_bits(res["qposes_rollout"]))
    assert np.array_equal(_np_bits(r["ctrl"]), _np_bits(res["ctrl"]))
    assert np.array_equal(_np_bits(r["state_rewards"]), _np_bits(res["state_rewards"]))


# ---------------------------------------------------------------------------------------------------------------- fused path end to end
def test_fused_path_end_to_end(lstm_ckpt):  # noqa: F811
    clips = [3, 5, 2, 9, 30, 1, 4, 6]
    cfg, dp, env, hl = _setup(lstm_ckpt[0], clips, "fused")
    assert hl.path == "fused" and hl.reset_carry_on_done
    st = _reset(hl, clips)
    g = torch.Generator().manual_seed(0)
    carry = dp.zero_carry(len(clips), "cpu", torch.float64)
    worst = 0.0
    for t in range(6):
        lat = (torch.randn((len(clips), Z), generator=g) * 0.3).to(DEV)
        obs, done = st.obs.clone(), env.done_buf.clone()
        lg, carry = dp.logits(torch.cat([lat, obs[:, REF:]], dim=-1), hidden_state=carry, reset=done, dtype=torch.float64)
        want = torch.tanh(lg[:, :A]).numpy()
        st = hl.step(st, lat)
        torch.cuda.synchronize()
        got = hl.last_ctrl.cpu().numpy()
        err = _rel(got, want)
        worst = max(worst, err)
        print(f"fused LSTM path, step {t}: action against float64 rel err {err:.3e} (bound {TOL})")
        assert np.isfinite(got).all() and np.abs(got).max() <= 1.0 and np.isfinite(st.obs.cpu().numpy()).all()
        assert torch.isfinite(hl.hidden_state[0]).all() and torch.isfinite(hl.hidden_state[1]).all()
    assert worst < TOL
    assert _rel(hl.hidden_state[0].cpu().numpy(), carry[0].numpy()) < TOL and _rel(hl.hidden_state[1].cpu().numpy(), carry[1].numpy()) < TOL
    # reset() zeroes the device carry; set_hidden_state round-trips
    h_keep = hl.hidden_state[0].clone()
    _reset(hl, clips)
    assert not hl.hidden_state[0].any() and not hl.hidden_state[1].any()
    hl.set_hidden_state(h_keep, h_keep)
    assert torch.equal(hl.hidden_state[1], h_keep)


# ---------------------------------------------------------------------------------------------------------------- path selection
def test_path_selection(lstm_ckpt, h64_ckpt, tmp_path):  # noqa: F811
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.environment import HighLevelWrapper
    cfg, dp, env, hl = _setup(lstm_ckpt[0], [0, 1], "auto")
    assert hl.path == ("fused" if HighLevelWrapper.AUTO_PREFERS_FUSED_LSTM else "layers")
    assert HighLevelWrapper(env, dp, dp.reference_obs_size, path="fused").path == "fused"
    assert HighLevelWrapper(env, dp, dp.reference_obs_size, path="layers").path == "layers"
    small = ck.make_lstm_decoder_policy_fn(h64_ckpt, device=DEV)
    assert small.hidden_state_size == 64
    assert HighLevelWrapper(env, small, small.reference_obs_size, path="auto").path == "layers"
    with pytest.raises(ValueError, match="H must be 128"):
        HighLevelWrapper(env, small, small.reference_obs_size, path="fused")
    # the H = 64 decoder steps through the layered list, within the float32 bound of its own float64 evaluation
    hs = HighLevelWrapper(env, small, small.reference_obs_size)
    st = _reset(hs, [0, 1])
    lat = (torch.randn((2, Z), generator=torch.Generator().manual_seed(0)) * 0.3).to(DEV)
    lg, _ = small.logits(torch.cat([lat, st.obs[:, REF:]], dim=-1), dtype=torch.float64)
    hs.step(st, lat)
    torch.cuda.synchronize()
    assert _rel(hs.last_ctrl.cpu().numpy(), torch.tanh(lg[:, :A]).numpy()) < TOL
    # an MLP DecoderPolicy still selects what it did
    mlp = ck.make_decoder_policy_fn(_make_ckpt(tmp_path, (256, 256), 11), device=DEV)
    assert HighLevelWrapper(env, mlp, mlp.reference_obs_size, path="auto").path == ("fused" if HighLevelWrapper.AUTO_PREFERS_FUSED else "layers")
    assert HighLevelWrapper(env, mlp, mlp.reference_obs_size, path="fused").path == "fused"
    with pytest.raises(TypeError, match="LSTMDecoderPolicy"):
        HighLevelWrapper(env, mlp, mlp.reference_obs_size).hidden_state


# ---------------------------------------------------------------------------------------------------------------- no torch op in step
@pytest.mark.parametrize("hl_path", ["layers", "fused"])
def test_no_torch_ops_inside_step_after_the_first_call(lstm_ckpt, hl_path):  # noqa: F811
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))

    clips = [1, 4, 6]
    cfg, dp, env, hl = _setup(lstm_ckpt[0], clips, hl_path)
    st = _reset(hl, clips)
    lats = [(torch.randn((3, Z), generator=torch.Generator().manual_seed(i)) * 0.3).to(DEV) for i in range(6)]
    st = hl.step(st, lats[0])
    Count.n = 0
    with Count():
        for lat in lats[1:]:
            st2 = hl.step(st, lat)
    assert Count.n == 0 and st2 is st
    torch.cuda.synchronize()
    assert torch.isfinite(st.obs).all() and float(hl.hidden_state[0].abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- CLI
def test_cli_replay_latents_reproduces_an_lstm_rollout(lstm_ckpt, tmp_path):  # noqa: F811
    from track_mjx_amd.analysis.utils import load_from_h5py
    d = lstm_ckpt[0]
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
        model, used = b["meta"]["model"], b["meta"]["decoder_path"]
        assert (model.decode() if isinstance(model, bytes) else str(model)) == "lstm"
        assert (used.decode() if isinstance(used, bytes) else str(used)) == "layers"
