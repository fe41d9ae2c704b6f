"""GPU: activation interventions — the kernel (tmjx_intervene) against the host emulation (bits) and float64 (the derived bound of
tests/intervene_ref.py) at the edge cases; roll-outs with an intervention: an empty gate is a no-op, causality and effect of projecting a subspace
out of the intention, batch invariance; one policy step against torch float64 with the same edit; the replay paths; the command line.  The
checkpoints are tests/test_gpu_rollout.py's (its smallest policies and its 70-clip synthetic table)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import intervene_ref as R
from tests.hostemu import intervene_emu as E
from tests.test_gpu_rollout import DEV, TOL, _f64_encoder, _rel, _same, _pick, lstm_ckpt, mlp_ckpt  # noqa: F401
from track_mjx_amd import h5lite, hip
from track_mjx_amd.analysis.intervene import Intervention

pytestmark = pytest.mark.gpu
CLIPS = [3, 5, 17]
bits = R.bits


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def gpu_run(buf, c0, w, mode, gain, offset, dose, t_on, t_off, t, dirs=None, center=None, want_proj=False):
    """tests.hostemu.intervene_emu.run on the device: the same arguments, the library's tmjx_intervene on copies in device memory."""
    n, ld = buf.shape
    up = lambda a, dt: None if a is None else torch.from_numpy(np.array(a, dt)).to(DEV)      # noqa: E731  (a copy: the shared inputs are read-only)
    dbuf, g, o, d, c, v = up(buf, np.float32), up(gain, np.float32), up(offset, np.float32), up(dose, np.float32), up(center, np.float32), up(dirs, np.float32)
    on, off = up(t_on, np.int32), up(t_off, np.int32)
    K = 0 if dirs is None else dirs.shape[0]
    proj = torch.full((n, K + 1), -7.25, dtype=torch.float32, device=DEV) if want_proj else None
    desc = E.descriptor(dbuf.data_ptr() + 4 * c0, ld, w, n, mode, g, o, d, on, off, v, K, 0 if dirs is None else dirs.shape[1], c, proj, K + 1 if want_proj else 0)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    hip.check(hip.lib().tmjx_intervene(C.byref(desc), int(t), stream), "tmjx_intervene")
    torch.cuda.synchronize()
    buf[...] = dbuf.cpu().numpy()
    if want_proj:
        p = proj.cpu().numpy()
        assert (p[:, K] == -7.25).all(), "the kernel wrote behind a proj row"
        return p[:, :K].copy()
    return None


@pytest.mark.parametrize("w", R.WIDTHS)
def test_kernel_against_emulation_and_float64(w):
    worst = R.check_width(w, gpu_run, "kernel", other=E.run)
    print(f"w = {w}: largest kernel error / bound {worst:.3f}")
    assert worst <= 1.0


def test_kernel_gate_bits_and_two_calls():
    h, v, g, o, dose, t_on, t_off, on = R.gate_problem()
    w = h.shape[1]
    got, emu = R.framed(h), R.framed(h)
    p_gpu = gpu_run(got, R.C0, w, R.SUBSPACE, g, o, dose, t_on, t_off, 5, dirs=v, want_proj=True)
    p_emu = E.run(emu, R.C0, w, R.SUBSPACE, g, o, dose, t_on, t_off, 5, dirs=v, want_proj=True)
    assert (bits(got) == bits(emu)).all() and (bits(p_gpu) == bits(p_emu)).all()
    assert (bits(got[~on, R.C0:R.C0 + w]) == bits(h[~on])).all() and (bits(got[on, R.C0:R.C0 + w]) != bits(h[on])).any(axis=1).all()
    again = R.framed(h)
    p2 = gpu_run(again, R.C0, w, R.SUBSPACE, g, o, dose, t_on, t_off, 5, dirs=v, want_proj=True)
    assert (bits(again) == bits(got)).all() and (bits(p2) == bits(p_gpu)).all()
    got, emu = R.framed(h), R.framed(h)
    gpu_run(got, R.C0, w, R.UNITS, np.zeros(w), np.ones(w), dose, t_on, t_off, 5)
    E.run(emu, R.C0, w, R.UNITS, np.zeros(w), np.ones(w), dose, t_on, t_off, 5)
    assert (bits(got) == bits(emu)).all() and (bits(got[~on, R.C0:R.C0 + w]) == bits(h[~on])).all()
    # a row alone and in the middle of 130, on the device
    n, w, K = 130, 1023, 16
    hh, vv, cc = R.rows_of(n, w, seed=5), R.directions(K, w), R.center_of(w)
    dd = R.doses_of(n)
    full = R.framed(hh)
    pf = gpu_run(full, R.C0, w, R.SUBSPACE, np.full(K, 0.5), np.full(K, R.S), dd, np.zeros(n), np.full(n, 9), 4, dirs=vv, center=cc, want_proj=True)
    for r in (0, 64, 77, 129):
        one = R.framed(hh[r:r + 1])
        p1 = gpu_run(one, R.C0, w, R.SUBSPACE, np.full(K, 0.5), np.full(K, R.S), dd[r:r + 1], np.zeros(1), np.full(1, 9), 4, dirs=vv, center=cc, want_proj=True)
        assert (bits(one[0]) == bits(full[r])).all() and (bits(p1[0]) == bits(pf[r])).all(), r


# ---------------------------------------------------------------------------------------------------------------- roll-outs
_GEN: dict = {}


def _gen(path, intervention=None, key=None):
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import create_environment, create_rollout_generator
    if (path, key) not in _GEN:
        cfg = ck.load_config_from_checkpoint(path)
        fn = ck.load_inference_fn(cfg, ck.load_policy(path, cfg))
        env = create_environment(cfg, 1, DEV)
        _GEN[(path, key)] = (create_rollout_generator(cfg, env, fn, model=fn.model, log_activations=True, log_metrics=True, intervention=intervention), fn, cfg)
    return _GEN[(path, key)]


_BASE: dict = {}


def _baseline(path):
    if path not in _BASE:
        _BASE[path] = _gen(path)[0](CLIPS)
    return _BASE[path]


def _directions(seed=0, K=2, w=60):
    return np.random.default_rng(seed).standard_normal((K, w))


@pytest.mark.parametrize("gate", ["window", "dose"])
def test_an_empty_gate_is_a_no_op(mlp_ckpt, gate):  # noqa: F811
    path = mlp_ckpt[0]
    base = _baseline(path)
    T = base["qposes_rollout"].shape[1]
    kw = dict(window=(T, T)) if gate == "window" else dict(dose=0.0)
    iv = Intervention("intention", "subspace", directions=_directions(), gain=0.0, offset=3.0, **kw)
    got = dict(_gen(path, iv, gate)[0](CLIPS))
    group = got.pop("intervention")
    _same(base, got)
    assert group["projection"].shape == (3, T - 1, 2) and group["window"].shape == (3, 2) and group["dose"].shape == (3,)
    if gate == "window":
        assert group["window"].tolist() == [[T, T]] * 3
    else:
        assert group["dose"].tolist() == [0, 0, 0]


def test_causality_and_effect_of_projecting_out_of_the_intention(mlp_ckpt):  # noqa: F811
    path = mlp_ckpt[0]
    base = _baseline(path)
    iv = Intervention("intention", "subspace", directions=_directions(), window=(5, 12))
    got = _gen(path, iv, "project")[0](CLIPS)
    a0, a1 = base["activations"], got["activations"]
    # before step 5: the same bits everywhere (state t + 1 is the state after control step t)
    cut = lambda tree, k: {key: cut(v, k) for key, v in tree.items()} if isinstance(tree, dict) else tree[:, :k]      # noqa: E731
    _same(cut({"ctrl": base["ctrl"], "a": a0}, 5), cut({"ctrl": got["ctrl"], "a": a1}, 5))
    _same(cut({k: base[k] for k in ("qposes_rollout", "state_rewards", "rollout_metrics")}, 6), cut({k: got[k] for k in ("qposes_rollout", "state_rewards", "rollout_metrics")}, 6))
    for j in range(3):
        assert (bits(base["qposes_rollout"][j, 6:]) != bits(got["qposes_rollout"][j, 6:])).any(), j
        assert (bits(base["ctrl"][j, 5]) != bits(got["ctrl"][j, 5])).any(), j
    # within the window the recorded intention is the edited one: its coordinates along the directions are zero up to rounding.  With h = the
    # encoder's mean (recorded before the edit) the float64 result h'_64 = h - sum_m p_m v_m has (h'_64 . v_k) = -sum_m p_m (G - I)_mk, G the Gram
    # matrix of the float32 directions, |G - I| <= K 2^-22 (tests/test_intervene_cpu.py); the kernel's h' is within the derived bound b of h'_64:
    #   |h' . v_k| <= sum_j b_j |v_kj| + K 2^-22 sum_m |p_m|
    v, K = iv.directions.astype(np.float64), 2
    for j in range(3):
        h = a1["encoder"]["mean"][j, 5:12]
        x = a1["intention"][j, 5:12]
        assert np.isfinite(h).all() and (bits(x) != bits(h)).any()
        bh, _ = R.bounds_subspace(h, iv.directions, None, iv.gain, iv.offset, np.ones(len(h)))
        p = np.abs(h.astype(np.float64) @ v.T)
        limit = bh @ np.abs(v).T + K * 2.0 ** -22 * p.sum(1, keepdims=True)
        resid = np.abs(x.astype(np.float64) @ v.T)
        print(f"clip {CLIPS[j]}: |p| before {p.max():.3e}, after {resid.max():.3e}, largest residual / bound {np.max(resid / limit):.3f}")
        assert (resid <= limit).all() and p.max() > 1e3 * resid.max()
        # outside the window the intention is the encoder's mean, as in any roll-out
        assert (bits(a1["intention"][j, :5]) == bits(a1["encoder"]["mean"][j, :5])).all() and (bits(a1["intention"][j, 12:]) == bits(a1["encoder"]["mean"][j, 12:])).all()
    # the recorded projection: the float32 coordinates of the (baseline's) intention at steps < 5, the emulation's bits
    group = got["intervention"]
    assert group["window"].tolist() == [[5, 12]] * 3 and group["dose"].tolist() == [1, 1, 1] and bytes(group["target"][0]) == b"intention"
    for j in range(3):
        rows = np.ascontiguousarray(a0["intention"][j, :5])
        want = E.run(rows.copy(), 0, 60, R.SUBSPACE, iv.gain, iv.offset, np.ones(5), np.full(5, 9), np.full(5, 9), 0, dirs=iv.directions, want_proj=True)
        assert (bits(group["projection"][j, :5]) == bits(want)).all(), j
    # and inside the window, of the pre-edit value of THIS roll-out
    rows = np.ascontiguousarray(a1["encoder"]["mean"][1, 5:12])
    want = E.run(rows.copy(), 0, 60, R.SUBSPACE, iv.gain, iv.offset, np.ones(7), np.full(7, 9), np.full(7, 9), 0, dirs=iv.directions, want_proj=True)
    assert (bits(group["projection"][1, 5:12]) == bits(want)).all()


def test_batch_invariance(mlp_ckpt):  # noqa: F811
    path = mlp_ckpt[0]
    d = _directions(1)
    alone = Intervention("intention", "subspace", directions=d, gain=0.0, offset=1.0, window=(5, 12), dose=0.5)
    batch = Intervention("intention", "subspace", directions=d, gain=0.0, offset=1.0, window=[(0, 3), (5, 12), (7, None)], dose=[1.0, 0.5, 0.25])
    one = _gen(path, alone, "alone")[0]([CLIPS[1]])
    three = _gen(path, batch, "batch")[0](CLIPS)
    _same(_pick(one, 0), _pick(three, 1))
    assert (bits(_baseline(path)["qposes_rollout"][1]) != bits(three["qposes_rollout"][1])).any()
    assert three["intervention"]["dose"].tolist() == [1.0, 0.5, 0.25] and three["intervention"]["window"][2].tolist() == [7, 2 ** 31 - 1]
    # a clip repeated with different doses: a dose-response in one batch (dose 0 = the baseline)
    rep = _gen(path, Intervention("intention", "subspace", directions=d, gain=0.0, offset=1.0, window=(5, 12), dose=[0.0, 0.5]), "doses")[0]([CLIPS[1]] * 2)
    assert (bits(rep["qposes_rollout"][0]) == bits(_baseline(path)["qposes_rollout"][1])).all()
    assert (bits(rep["qposes_rollout"][1]) == bits(one["qposes_rollout"][0])).all()


# ---------------------------------------------------------------------------------------------------------------- 5. one policy step
def _obs(cfg, clips):
    from tests.test_gpu_highlevel import _reset
    from track_mjx_amd.analysis.rollout import create_environment
    env = create_environment(cfg, len(clips), DEV)
    return _reset(env, clips).obs.clone()


def _edit64(h, iv, dose=1.0):
    c = np.zeros(h.shape[1]) if iv.center is None else iv.center
    if iv.mode == "subspace":
        return torch.from_numpy(R.subspace(h.numpy(), iv.directions, c, iv.gain, iv.offset, np.full(len(h), dose))[0])
    g, o = np.ones(h.shape[1]), np.zeros(h.shape[1])
    g[iv.units], o[iv.units] = iv.gain, iv.offset
    return torch.from_numpy(R.units(h.numpy(), c, g, o, np.full(len(h), dose)))


@pytest.mark.parametrize("mode", ["subspace", "units"])
def test_one_mlp_policy_step_against_torch_float64(mlp_ckpt, mode):  # noqa: F811
    _, fn, cfg = _gen(mlp_ckpt[0])
    pol = fn.policy
    rng = np.random.default_rng(4)
    center = rng.standard_normal(256).astype(np.float32) * 0.1
    if mode == "subspace":
        iv = Intervention("decoder/layer_0", "subspace", directions=rng.standard_normal((3, 256)), center=center, gain=[0.0, 1.0, 0.5], offset=[0.5, 2.0, 0.0])
    else:
        iv = Intervention.units("decoder/layer_0", [3, 100, 255], center=center, gain=0.0, offset=[0.0, 1.0, -1.0])
    obs = _obs(cfg, CLIPS)
    ctrl, extras = fn(obs, intervention=iv, t=0)
    plain, _ = fn(obs)
    a = {k: v.cpu().numpy() for k, v in extras["activations"].items()}
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    norm = (obs.cpu().double() - d(fn.mean)) / d(fn.std)
    enc = _f64_encoder(pol, norm[:, :470])
    h = torch.cat([enc["mean"], norm[:, 470:]], -1)
    for i, blk in enumerate(pol.decoder):
        z = h @ d(blk.dense.weight).T + d(blk.dense.bias)
        h = torch.nn.functional.layer_norm(torch.nn.functional.silu(z), (z.shape[-1],), d(blk.norm.weight), d(blk.norm.bias), blk.norm.eps)
        if i == 0:
            before = h
            h = _edit64(h, iv)
        assert _rel(a[f"decoder/layer_{i}"], h.numpy()) < TOL, i          # the recorded layer_0 is the edited one
    want = torch.tanh((h @ d(pol.head.weight).T + d(pol.head.bias))[:, :pol.action_size])
    assert _rel(ctrl.cpu().numpy(), want.numpy()) < TOL
    assert _rel(before.numpy(), _edit64(before, iv).numpy()) > 1e-2 and _rel(plain.cpu().numpy(), want.numpy()) > 10 * TOL      # the edit matters
    off, _ = fn(obs, intervention=iv, t=-1)                                  # before the window: the plain step's bits
    assert torch.equal(off.view(torch.int32), plain.view(torch.int32))


def test_one_lstm_policy_step_against_torch_float64(lstm_ckpt):  # noqa: F811
    _, fn, cfg = _gen(lstm_ckpt[0])
    pol = fn.policy
    H, Lk = pol.hidden_state_size, pol.hidden_layer_num
    rng = np.random.default_rng(5)
    iv = Intervention("hidden_state/h:0", "subspace", directions=rng.standard_normal((2, H)), gain=1.0, offset=[0.5, -0.5])
    obs = _obs(cfg, CLIPS)
    n = len(CLIPS)
    g = torch.Generator().manual_seed(1)
    h0, c0 = (torch.randn((n, Lk, H), generator=g) * 0.3).to(DEV), (torch.randn((n, Lk, H), generator=g) * 0.3).to(DEV)
    ctrl, extras, (h1, c1) = fn(obs, hidden_state=(h0, c0), intervention=iv, t=0)
    plain, _, (hp, _) = fn(obs, hidden_state=(h0, c0))
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    norm = (obs.cpu().double() - d(fn.mean)) / d(fn.std)
    enc = _f64_encoder(pol, norm[:, :470])
    inp = torch.cat([enc["mean"], norm[:, 470:]], -1)
    for k in range(Lk):
        gt = inp @ d(pol.w_ih[k]).T + d(h0)[:, k] @ d(pol.w_hh[k]).T + d(pol.b_hh[k])
        i_, f_, g_, o_ = torch.sigmoid(gt[:, :H]), torch.sigmoid(gt[:, H:2 * H]), torch.tanh(gt[:, 2 * H:3 * H]), torch.sigmoid(gt[:, 3 * H:])
        c = f_ * d(c0)[:, k] + i_ * g_
        h = o_ * torch.tanh(c)
        if k == 0:
            assert _rel(hp[:, 0].cpu().numpy(), h.numpy()) < TOL
            h = _edit64(h, iv)                                              # the next layer's input AND the carry into the next step
        assert _rel(h1[:, k].cpu().numpy(), h.numpy()) < TOL and _rel(c1[:, k].cpu().numpy(), c.numpy()) < TOL, k
        inp = h
    want = torch.tanh((inp @ d(pol.projection.weight).T + d(pol.projection.bias))[:, :pol.action_size])
    assert _rel(ctrl.cpu().numpy(), want.numpy()) < TOL and _rel(plain.cpu().numpy(), want.numpy()) > 10 * TOL
    assert _rel(extras["activations"]["hidden_state/h"][:, 0].cpu().numpy(), h1[:, 0].cpu().numpy()) == 0


# ---------------------------------------------------------------------------------------------------------------- 6. replay paths
def test_replay_paths(mlp_ckpt):  # noqa: F811
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis.rollout import replay_latents
    path = mlp_ckpt[0]
    base = _baseline(path)
    cfg = ck.load_config_from_checkpoint(path)
    dp = ck.make_decoder_policy_fn(path, device=DEV)
    lat = np.ascontiguousarray(base["activations"]["intention"][:2])
    clips = CLIPS[:2]
    iv = Intervention.units("decoder/layer_0", [1, 50, 200], gain=0.0, offset=2.0, window=(5, 12))
    got = replay_latents(cfg, dp, clips, lat, path="layers", intervention=iv)
    assert got["path"] == "layers" and set(got["intervention"]) == {"target", "mode", "units", "gain", "offset", "window", "dose"}
    assert (bits(got["qposes_rollout"][:, :6]) == bits(base["qposes_rollout"][:2, :6])).all() and (bits(got["ctrl"][:, :5]) == bits(base["ctrl"][:2, :5])).all()
    for j in range(2):
        assert (bits(got["ctrl"][j, 5]) != bits(base["ctrl"][j, 5])).any() and (bits(got["qposes_rollout"][j, 6:]) != bits(base["qposes_rollout"][j, 6:])).any()
    with pytest.raises(ValueError, match="path='fused' cannot run an intervention: the fused decoder launch has no seam"):
        replay_latents(cfg, dp, clips, lat, path="fused", intervention=iv)
    sub = Intervention("intention", "subspace", directions=_directions(), window=(5, 12))
    # fed the pre-edit intentions (the encoder's means) of the roll-out that ran with this intervention, the replay applies the same edit to the same
    # rows: that roll-out, reproduced in closed loop
    want = _gen(path, sub, "project")[0](CLIPS)
    auto = replay_latents(cfg, dp, clips, np.ascontiguousarray(want["activations"]["encoder"]["mean"][:2]), path="auto", intervention=sub)
    assert auto["path"] == "layers" and auto["intervention"]["projection"].shape == (2, lat.shape[1], 2)
    assert (bits(auto["ctrl"]) == bits(want["ctrl"][:2])).all() and (bits(auto["qposes_rollout"]) == bits(want["qposes_rollout"][:2])).all()
    assert (bits(auto["intervention"]["projection"]) == bits(want["intervention"]["projection"][:2])).all()


# ---------------------------------------------------------------------------------------------------------------- 7. command line
def test_cli_writes_the_intervention_group_and_usage_errors_return_2(mlp_ckpt, tmp_path, capsys):  # noqa: F811
    from track_mjx_amd.analysis import rollout as ro
    from track_mjx_amd.analysis.utils import load_from_h5py
    path = mlp_ckpt[0]
    comp, _ = np.linalg.qr(np.random.default_rng(7).standard_normal((60, 4)))
    pca = tmp_path / "pca.h5"
    h5lite.write_tree(str(pca), {"mean": np.full(60, 0.01, np.float32), "components": comp.T.astype(np.float32), "feature": "intention"})
    out = tmp_path / "rollouts"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-m", "track_mjx_amd.analysis.rollout", f"checkpoint={path}", "clips=3,5", f"out={out}", f"intervene_pca={pca}",
                          "intervene_components=0:2", "intervene_window=5:12", "intervene_dose=1,0.5", "log_metrics=false"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ), cwd=root)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == ["clip_3.h5", "clip_5.h5"]
    iv = Intervention.from_pca(pca, "0:2", window=(5, 12), dose=[1, 0.5])
    want = _gen(path, iv, "cli")[0]([3, 5])
    for j, c in enumerate((3, 5)):
        got = load_from_h5py(out / f"clip_{c}.h5")
        g = got["intervention"]
        assert bytes(g["target"]) == b"intention" and bytes(g["mode"]) == b"subspace" and g["window"].tolist() == [5, 12] and float(g["dose"]) == (1, 0.5)[j]
        assert g["directions"].shape == (2, 60) and g["center"].shape == (60,) and g["gain"].tolist() == [0, 0] and g["offset"].tolist() == [0, 0]
        assert (bits(g["projection"]) == bits(want["intervention"]["projection"][j])).all()
        assert (bits(got["qposes_rollout"]) == bits(want["qposes_rollout"][j])).all()
    # the same options on replay_latents= (in-process), here a units edit with one dose per clip
    rep = tmp_path / "replays"
    assert ro.main([f"checkpoint={path}", f"replay_latents={out}", f"out={rep}", "intervene_units=decoder/layer_0:1,50,200", "intervene_offset=2",
                    "intervene_window=5:12", "intervene_dose=0,1"]) == 0
    capsys.readouterr()
    r3, r5 = load_from_h5py(rep / "clip_3.h5"), load_from_h5py(rep / "clip_5.h5")
    assert bytes(r5["intervention"]["mode"]) == b"units" and r5["intervention"]["units"].tolist() == [1, 50, 200] and float(r3["intervention"]["dose"]) == 0
    assert bytes(r5["meta"]["decoder_path"]) == b"layers"
    assert (bits(r3["qposes_rollout"]) == bits(want["qposes_rollout"][0])).all()            # dose 0: the recorded roll-out, closed loop
    assert (bits(r5["qposes_rollout"][:6]) == bits(want["qposes_rollout"][1][:6])).all() and (bits(r5["qposes_rollout"][6:]) != bits(want["qposes_rollout"][1][6:])).any()
    # usage errors: exit code 2 and one line, no traceback (in-process: nothing reaches the device)
    for extra, word in ((["intervene_gain=1"], "no intervention is given"), ([f"intervene_pca={pca}", "intervene_units=intention:1"], "exactly one of"),
                        ([f"intervene_pca={pca}", "intervene_columns=0:2"], "intervene_columns goes with intervene_readout"),
                        ([f"intervene_pca={tmp_path / 'missing.h5'}"], "intervene_pca"), (["intervene_units=encoder/mean:1"], "not supported"),
                        ([f"intervene_pca={pca}", "intervene_components=2:9"], "selects"), ([f"intervene_pca={pca}", "intervene_window=5"], "intervene_window=a:b"),
                        ([f"intervene_pca={pca}", f"replay_latents={out}", "path=fused"], "path=fused cannot run an intervention")):
        assert ro.main([f"checkpoint={path}", f"out={tmp_path / 'none'}", *extra]) == 2, extra
        assert word in capsys.readouterr().err, extra
    assert ro.main([f"checkpoint={path}", "clips=3,5,17", f"out={tmp_path / 'none'}", f"intervene_pca={pca}", "intervene_dose=1,2"]) == 2
    assert "intervene_dose: 2 values for 3 clips (one value, or one per clip)" in capsys.readouterr().err
    assert ro.main([f"checkpoint={path}", "clips=3", f"out={tmp_path / 'none'}", "intervene_units=decoder/layer_7:1"]) == 2
    assert "does not exist in this policy step" in capsys.readouterr().err
