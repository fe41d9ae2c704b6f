"""Activation interventions on the CPU: the host emulation of tmjx_intervene (tests/hostemu/intervene_emu.cpp) against the float64 statement of
tests/intervene_ref.py under the derived bound, the bit-level properties of the gate, the refusals (the emulation's and the product library's: no
GPU is touched), analysis.intervene.Intervention, the launch lists with and without an intervention, the effect-summary tool, and the emulation
as a stand-alone program under the sanitizers."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import intervene_ref as R
from tests.hostemu import intervene_emu as E
from track_mjx_amd import h5lite, hip
from track_mjx_amd.analysis import intervene as IV
from track_mjx_amd.analysis.intervene import Intervention

ROOT = Path(__file__).resolve().parents[1]
bits = R.bits


# ------------------------------------------------------------------------------------------------------------------ 1, 2: emulation against float64
@pytest.mark.parametrize("w", R.WIDTHS)
def test_emu_against_float64_under_the_derived_bound(w):
    worst = R.check_width(w, E.run, "emulation")
    print(f"w = {w}: largest error / bound {worst:.3f}")
    assert worst <= 1.0


def test_the_edits_do_what_they_say():
    """Project out, clamp, stimulate and scale, read off the coordinates of the edited rows (float64 of the float32 result)."""
    w, K, n = 256, 2, 3
    h, v, c = R.rows_of(n, w), R.directions(K, w), R.center_of(w)
    p0 = (h.astype(np.float64) - c) @ v.astype(np.float64).T
    for (g, o), want in zip(R.GAIN_OFFSET, (0 * p0, 0 * p0 + R.S, p0 + R.S, 0.5 * p0)):
        buf = R.framed(h)
        E.run(buf, R.C0, w, R.SUBSPACE, np.full(K, g), np.full(K, o), np.ones(n), np.zeros(n), np.full(n, 9), 0, dirs=v, center=c)
        p1 = (buf[:, R.C0:R.C0 + w].astype(np.float64) - c) @ v.astype(np.float64).T
        assert np.abs(p1 - want).max() < 1e-4, (g, o)
    gw, ow = np.ones(w, np.float32), np.zeros(w, np.float32)
    gw[[3, 77]], ow[[3, 77]] = 0.0, 0.5
    buf = R.framed(h)
    E.run(buf, R.C0, w, R.UNITS, gw, ow, np.ones(n), np.zeros(n), np.full(n, 9), 0, center=c)
    got = buf[:, R.C0:R.C0 + w]
    assert np.allclose(got[:, [3, 77]], c[[3, 77]] + 0.5, atol=1e-6)                     # a unit at gain 0 is set to c + o
    keep = np.setdiff1d(np.arange(w), [3, 77])
    assert (got[:, keep] == h[:, keep]).all()                                           # gain 1, offset 0 leaves a unit alone


# ------------------------------------------------------------------------------------------------------------------ 3: bit-level properties
def test_off_rows_keep_their_bits_and_proj_is_written_for_every_row():
    h, v, g, o, dose, t_on, t_off, on = R.gate_problem()
    w = h.shape[1]
    buf = R.framed(h)
    proj = E.run(buf, R.C0, w, R.SUBSPACE, g, o, dose, t_on, t_off, 5, dirs=v, want_proj=True)
    got = buf[:, R.C0:R.C0 + w]
    assert (bits(got[~on]) == bits(h[~on])).all()                                       # NaN and -0 included
    assert np.signbit(got[~on, 0]).all() and np.isnan(got[~on, w // 2]).all()
    assert (bits(got[on]) != bits(h[on])).any(axis=1).all()
    frame = R.framed(h)
    frame[:, R.C0:R.C0 + w] = got
    assert (bits(frame) == bits(buf)).all()                                             # the canaries around the target
    assert np.isnan(proj).all()                                                         # (every row has a NaN planted: its projection is NaN, OFF rows too)
    clean = h.copy()
    clean[:, w // 2] = 1.0
    buf = R.framed(clean)
    proj = E.run(buf, R.C0, w, R.SUBSPACE, g, o, dose, t_on, t_off, 5, dirs=v, want_proj=True)
    p64 = clean.astype(np.float64) @ v.astype(np.float64).T
    assert np.abs(proj - p64).max() < 1e-4 and (proj != -7.25).all()                     # written for the OFF rows too
    assert (bits(buf[~on, R.C0:R.C0 + w]) == bits(clean[~on])).all()
    # units mode: the same gates
    buf = R.framed(h)
    E.run(buf, R.C0, w, R.UNITS, np.zeros(w), np.ones(w), dose, t_on, t_off, 5)
    assert (bits(buf[~on, R.C0:R.C0 + w]) == bits(h[~on])).all()
    assert np.allclose(buf[on, R.C0 + 1], h[on, 1] + dose[on] * (1.0 - h[on, 1]), atol=1e-6)         # gain 0, offset 1, no centre: towards 1 by the dose


@pytest.mark.parametrize("mode", (R.SUBSPACE, R.UNITS))
def test_a_row_is_the_same_alone_and_anywhere_in_a_batch(mode):
    w, K, n = 1023, 16, 130
    h, v, c = R.rows_of(n, w, seed=5), R.directions(K, w), R.center_of(w)
    rng = np.random.default_rng(0)
    dose = rng.choice([0.0, 0.25, 1.0], n).astype(np.float32)
    t_on, t_off = rng.integers(0, 6, n).astype(np.int32), rng.integers(3, 9, n).astype(np.int32)
    g, o = (np.full(K, 0.5), np.full(K, R.S)) if mode == R.SUBSPACE else (rng.standard_normal(w), rng.standard_normal(w))
    kw = dict(dirs=v, want_proj=True) if mode == R.SUBSPACE else {}
    buf = R.framed(h)
    proj = E.run(buf, R.C0, w, mode, g, o, dose, t_on, t_off, 4, center=c, **kw)
    for r in (0, 1, 63, 64, 129):
        one = R.framed(h[r:r + 1])
        kw1 = dict(kw)
        p1 = E.run(one, R.C0, w, mode, g, o, np.full(1, dose[r]), t_on[r:r + 1], t_off[r:r + 1], 4, center=c, **kw1)
        assert (bits(one[0]) == bits(buf[r])).all(), r
        if proj is not None:
            assert (bits(p1[0]) == bits(proj[r])).all(), r


# ------------------------------------------------------------------------------------------------------------------ 4: refusals
def _refusals(desc, ok, call, last_error):
    one = 1 << 20
    base = dict(h=one, ld=40, w=32, n=5, mode=R.SUBSPACE, gain=one, offset=one, dose=one, t_on=one, t_off=one, dirs=one, K=3, ldv=32, center=None,
                proj=one, ldp=3)
    good = desc(**base)
    assert ok(good)
    units = dict(base, mode=R.UNITS, proj=None, dirs=None, K=0, ldv=0, ldp=0)
    assert ok(desc(**units))
    cases = [(dict(h=None), "null argument"), (dict(gain=None), "null argument"), (dict(offset=None), "null argument"), (dict(dose=None), "null argument"),
             (dict(t_on=None), "null argument"), (dict(t_off=None), "null argument"), (dict(dirs=None), "null argument"),
             (dict(h=one + 2), "4-byte aligned"), (dict(dirs=one + 1), "4-byte aligned"), (dict(center=one + 3), "4-byte aligned"),
             (dict(proj=one + 2), "4-byte aligned"), (dict(t_on=one + 2), "4-byte aligned"), (dict(dose=one + 1), "4-byte aligned"),
             (dict(w=0), "w = 0 outside 1 .. 1024"), (dict(w=1025, ld=1025, ldv=1025), "w = 1025 outside 1 .. 1024"),
             (dict(K=0), "K = 0 outside 1 .. 16"), (dict(K=17, ldp=17), "K = 17 outside 1 .. 16"), (dict(ld=31), "ld = 31 is smaller than w = 32"),
             (dict(ldv=31), "ldv = 31 is smaller than w = 32"), (dict(ldp=2), "ldp = 2 is smaller than K = 3"), (dict(n=0), "n must be >= 1 (got 0)"),
             (dict(mode=2), "unknown mode 2"), (dict(mode=-1), "unknown mode -1")]
    for change, word in cases:
        d = desc(**dict(base, **change))
        assert not ok(d) and word in last_error(), (change, last_error())
        assert call(d) == -22 and word in last_error(), (change, last_error())
    d = desc(**dict(units, proj=one, ldp=3))
    assert not ok(d) and "proj is given in units mode" in last_error()
    assert call(d) == -22
    assert call(None) == -22 and "null descriptor" in last_error()


def test_emu_refusals():
    L = E._lib()
    _refusals(E.descriptor, E.intervene_ok, lambda d: L.ivemu_intervene(None if d is None else C.byref(d), 0), E.last_error)


def test_library_refuses_before_any_device_call():
    """The product library's own checks: the dummy pointers are never dereferenced and no GPU is touched."""
    L = hip.lib()
    _refusals(E.descriptor, lambda d: bool(L.tmjx_intervene_ok(C.byref(d))), lambda d: L.tmjx_intervene(None if d is None else C.byref(d), 0, None),
              lambda: L.tmjx_last_error().decode())


def test_abi_declares_the_intervention():
    header = (ROOT / "include" / "tmjx.h").read_text()
    core = (ROOT / "track_mjx_amd" / "csrc" / "intervene_core.h").read_text()
    assert {"tmjx_intervene_ok", "tmjx_intervene"} <= set(hip.EXPORTS) and any(p.name == "tmjx_intervene.hip" for p in hip.SOURCES)
    for text in ("int tmjx_intervene_ok(const tmjx_intervene_t *d);", "int tmjx_intervene(const tmjx_intervene_t *d, int t, void *stream);",
                 f"#define TMJX_INTERVENE_SUBSPACE {hip.INTERVENE_SUBSPACE}", f"#define TMJX_INTERVENE_UNITS {hip.INTERVENE_UNITS}"):
        assert text in header
    assert f"#define IV_MAX_W {hip.INTERVENE_MAX_W}" in core and f"#define IV_MAX_K {hip.INTERVENE_MAX_K}" in core
    assert (IV.MAX_W, IV.MAX_K) == (hip.INTERVENE_MAX_W, hip.INTERVENE_MAX_K)
    assert C.sizeof(hip.Intervene) == 104


def test_emulation_as_a_stand_alone_program_under_sanitizers(tmp_path):
    exe = E.build_main(tmp_path / "intervene_emu", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "checksum" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr
    assert "130 x 1023" in out.stdout


# ------------------------------------------------------------------------------------------------------------------ 5: Intervention
def test_orthonormalisation_and_rank_refusal():
    rng = np.random.default_rng(1)
    for K, w in ((1, 1), (2, 60), (16, 256), (16, 1024), (3, 3)):
        raw = rng.standard_normal((K, w)) * rng.uniform(0.1, 30.0, (K, 1)) + 0.7      # far from orthonormal: a shared offset, different norms
        iv = Intervention("decoder/layer_0", "subspace", directions=raw)
        q = iv.directions
        assert q.dtype == np.float32 and q.shape == (K, w)
        gram = q.astype(np.float64) @ q.astype(np.float64).T
        assert np.abs(gram - np.eye(K)).max() <= K * 2.0 ** -22
        # the same nested spans: row k of the input lies in the span of the first k + 1 stored rows
        resid = raw - (raw @ q.astype(np.float64).T) @ q.astype(np.float64)
        assert np.abs(resid).max() <= 1e-5 * np.abs(raw).max()
        assert np.abs(np.triu(raw @ q.astype(np.float64).T, 1)).max() <= 1e-5 * np.abs(raw).max()
    a = rng.standard_normal(60)
    for bad in ([a, 2 * a], [a, rng.standard_normal(60), a * (1 + 1e-9)], [a * 0], np.ones((2, 1))):
        with pytest.raises(ValueError, match="rank below"):
            Intervention("intention", "subspace", directions=bad)
    with pytest.raises(ValueError, match="1 .. 16 directions"):
        Intervention("intention", "subspace", directions=rng.standard_normal((17, 60)))
    with pytest.raises(ValueError, match="1 .. 1024 features"):
        Intervention("intention", "subspace", directions=rng.standard_normal((2, 1025)))


def test_gain_offset_window_and_dose_rules():
    v = np.eye(3, 60)
    iv = Intervention("intention", "subspace", directions=v, gain=[0, 1, 0.5], offset=2.0)
    assert iv.gain.tolist() == [0, 1, 0.5] and iv.offset.tolist() == [2, 2, 2]
    with pytest.raises(ValueError, match="gain: 2 values for 3 directions"):
        Intervention("intention", "subspace", directions=v, gain=[0, 1])
    with pytest.raises(ValueError, match="offset: 2 values for 3 listed units"):
        Intervention.units("decoder/layer_0", [1, 2, 3], offset=[0, 1])
    win, dose = iv.per_clip(4)
    assert win.tolist() == [[0, IV.T_END]] * 4 and dose.tolist() == [1, 1, 1, 1]
    iv = Intervention("intention", "subspace", directions=v, window=[(5, 12), (0, None), (3, 3)], dose=[0, 0.25, 1])
    win, dose = iv.per_clip(3)
    assert win.tolist() == [[5, 12], [0, IV.T_END], [3, 3]] and dose.tolist() == [0, 0.25, 1]
    with pytest.raises(ValueError, match=r"window: 3 values for 2 clips \(one value, or one per clip\)"):
        iv.per_clip(2)
    iv = Intervention("intention", "subspace", directions=v, dose=[1, 2])
    with pytest.raises(ValueError, match=r"dose: 2 values for 3 clips \(one value, or one per clip\)"):
        iv.per_clip(3)
    with pytest.raises(ValueError, match="window must be"):
        Intervention("intention", "subspace", directions=v, window=(1, 2, 3))
    with pytest.raises(ValueError, match="mode must be"):
        Intervention("intention", "rotate", directions=v)
    with pytest.raises(ValueError, match="distinct indices"):
        Intervention.units("decoder/layer_0", [1, 1])


@pytest.mark.parametrize("target", ("encoder/mean", "encoder/logvar", "egocentric_obs", "traj_obs", "decoder/lstm_projection", "hidden_state/c",
                                    "hidden_state/h", "decoder/layer_x", "nonsense"))
def test_unsupported_targets(target):
    with pytest.raises(ValueError, match="not supported; supported: intention, encoder/layer_<i>, decoder/layer_<i>, hidden_state/h:<k>"):
        Intervention(target, "subspace", directions=np.eye(2, 8))
    with pytest.raises(ValueError, match="not supported"):
        Intervention.units(target, [0])


def test_from_pca_from_readout_and_units(tmp_path):
    rng = np.random.default_rng(2)
    comp, _ = np.linalg.qr(rng.standard_normal((60, 5)))
    mean = rng.standard_normal(60).astype(np.float32)
    pca = tmp_path / "pca.h5"
    h5lite.write_tree(str(pca), {"mean": mean, "components": comp.T.astype(np.float32), "feature": "intention", "n_samples": np.int64(10)})
    iv = Intervention.from_pca(pca, components="1:3", window=(100, 300))
    assert iv.target == "intention" and iv.mode == "subspace" and iv.K == 2 and (iv.center == mean).all()
    assert np.abs(iv.directions - comp.T[1:3]).max() < 1e-6 and iv.per_clip(1)[0].tolist() == [[100, 300]]
    assert Intervention.from_pca(pca).K == 2 and Intervention.from_pca(pca, components="0,4").K == 2
    with pytest.raises(ValueError, match="components='3:9' selects"):
        Intervention.from_pca(pca, components="3:9")
    coef = rng.standard_normal((256, 4)).astype(np.float32)
    ro = tmp_path / "readout.h5"
    h5lite.write_tree(str(ro), {"coef": coef, "mean_x": np.arange(256, dtype=np.float32), "feature": "decoder/layer_0", "target": "qposes_rollout"})
    iv = Intervention.from_readout(ro, columns="0:3", gain=1.0, offset=0.5)
    assert iv.target == "decoder/layer_0" and iv.K == 3 and iv.center[7] == 7 and iv.gain.tolist() == [1, 1, 1]
    c0 = coef[:, 0] / np.linalg.norm(coef[:, 0])
    assert np.abs(iv.directions[0] - c0).max() < 1e-6                                  # the first direction is the first column, normalised
    h5lite.write_tree(str(tmp_path / "pca2.h5"), {"mean": np.ones(256, np.float32), "components": np.eye(2, 256, dtype=np.float32), "feature": "decoder/layer_0"})
    iv = Intervention.units("decoder/layer_0", [3, 9, 200], center=tmp_path / "pca2.h5")
    assert iv.mode == "units" and iv.units.tolist() == [3, 9, 200] and (iv.center == 1).all() and iv.gain.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="the PCA of 'intention'"):
        Intervention.units("decoder/layer_0", [3], center=pca)
    rec = iv.record(*iv.per_clip(2))
    assert set(rec) == {"target", "mode", "units", "center", "gain", "offset", "window", "dose"} and rec["units"].shape == (2, 3)


def test_command_line_options(tmp_path):
    pca = tmp_path / "pca.h5"
    h5lite.write_tree(str(pca), {"mean": np.zeros(60, np.float32), "components": np.eye(4, 60, dtype=np.float32), "feature": "intention"})
    assert IV.from_cli({"checkpoint": "x"}) is None
    iv = IV.from_cli({"intervene_pca": str(pca), "intervene_components": "0:3", "intervene_window": "5:12", "intervene_dose": "0,0.5,1", "intervene_gain": "1",
                      "intervene_offset": "0.5"})
    assert iv.K == 3 and iv.per_clip(3)[0][0].tolist() == [5, 12] and iv.per_clip(3)[1].tolist() == [0, 0.5, 1] and iv.gain.tolist() == [1, 1, 1]
    iv = IV.from_cli({"intervene_units": "hidden_state/h:1:4,5", "intervene_window": "7:"})
    assert iv.target == "hidden_state/h:1" and iv.units.tolist() == [4, 5] and iv.per_clip(1)[0].tolist() == [[7, IV.T_END]]
    for bad, word in (({"intervene_pca": str(pca), "intervene_units": "intention:1"}, "exactly one of"), ({"intervene_gain": "1"}, "no intervention is given"),
                      ({"intervene_pca": str(pca), "intervene_columns": "0:1"}, "intervene_columns goes with intervene_readout"),
                      ({"intervene_units": "decoder/layer_0"}, "intervene_units=<target>:i,j,k"), ({"intervene_pca": str(tmp_path / "none.h5")}, "intervene_pca"),
                      ({"intervene_units": "encoder/mean:1,2"}, "not supported"), ({"intervene_pca": str(pca), "intervene_window": "5"}, "intervene_window=a:b")):
        with pytest.raises(ValueError, match=word):
            IV.from_cli(bad)


# ------------------------------------------------------------------------------------------------------------------ 6: launch lists
def _names(ll):
    return [name for name, _ in ll.calls]


def _mlp_step(intervention=None, n=3):
    from track_mjx_amd.agent.networks import IntentionPolicy
    from track_mjx_amd.analysis.rollout import RolloutPolicy, _PolicyStep
    torch.manual_seed(0)
    pol = IntentionPolicy(40, 24, 6, latents=8, encoder_layers=(32, 20), decoder_layers=(28, 16))
    rp = RolloutPolicy(pol, torch.zeros(40), torch.ones(40), "mlp")
    gates = None if intervention is None else intervention.per_clip(n)
    return _PolicyStep(rp, n, torch.zeros((40, n)), record=False, intervention=intervention, gates=gates)


def _lstm_step(intervention=None, n=3):
    from track_mjx_amd.agent.lstm import LSTMIntentionPolicy
    from track_mjx_amd.analysis.rollout import RolloutPolicy, _PolicyStep
    torch.manual_seed(0)
    pol = LSTMIntentionPolicy(40, 24, 6, latents=8, encoder_layers=(32, 20), hidden_state_size=32, hidden_layer_num=2)
    rp = RolloutPolicy(pol, torch.zeros(40), torch.ones(40), "lstm")
    gates = None if intervention is None else intervention.per_clip(n)
    return _PolicyStep(rp, n, torch.zeros((40, n)), record=False, intervention=intervention, gates=gates)


BLOCK0, BLOCK = ["tmjx_linear_nolds_norm", "tmjx_silu_ln_fwd"], ["tmjx_linear_nolds", "tmjx_silu_ln_fwd"]
ENCODER = BLOCK0 + BLOCK + ["tmjx_linear_nolds", "tmjx_latent_concat_det"]
MLP_CALLS = ENCODER + BLOCK + BLOCK + ["tmjx_linear_nolds", "tmjx_action_mode"]
LSTM_CALLS = ENCODER + ["tmjx_linear_nolds", "tmjx_lstm_seq_fwd"] * 2 + ["tmjx_linear_nolds", "tmjx_action_mode"]


def test_without_an_intervention_the_launch_lists_are_what_they_were():
    assert _names(_mlp_step().ll) == MLP_CALLS
    assert _names(_lstm_step().ll) == LSTM_CALLS


@pytest.mark.parametrize("target,w,after", [("intention", 8, 5), ("encoder/layer_0", 32, 1), ("encoder/layer_1", 20, 3), ("decoder/layer_0", 28, 7),
                                            ("decoder/layer_1", 16, 9)])
def test_one_intervene_call_directly_behind_the_producer_mlp(target, w, after):
    base = _mlp_step()
    step = _mlp_step(Intervention(target, "subspace", directions=np.eye(2, w)))
    names = _names(step.ll)
    assert names.count("tmjx_intervene") == 1 and names.index("tmjx_intervene") == after + 1
    assert names[:after + 1] + names[after + 2:] == MLP_CALLS == _names(base.ll)
    entry = step.ll.calls[after + 1]
    assert entry is step.iv_entry and entry[1][1] == 0
    d = entry[1][0]._obj
    buf, c0, ww, ld = (step.acts["intention"] if target == "intention" else step.acts[target.split("/")[0]][target.split("/")[1]])
    assert (d.h, d.w, d.ld, d.n, d.K, d.mode) == (buf.data_ptr() + 4 * c0, w, ld, 3, 2, hip.INTERVENE_SUBSPACE) and ww == w
    assert d.proj == step.iv.proj.data_ptr() and d.ldp == 2
    # units mode on the same target
    step = _mlp_step(Intervention.units(target, [0, w - 1]))
    d = step.iv_entry[1][0]._obj
    assert _names(step.ll).index("tmjx_intervene") == after + 1 and d.mode == hip.INTERVENE_UNITS and d.proj is None and d.w == w
    assert step.iv.gain.tolist() == [0.0] + [1.0] * (w - 2) + [0.0]


@pytest.mark.parametrize("target,w,after", [("intention", 8, 5), ("hidden_state/h:0", 32, 7), ("hidden_state/h:1", 32, 9)])
def test_one_intervene_call_directly_behind_the_producer_lstm(target, w, after):
    step = _lstm_step(Intervention(target, "subspace", directions=np.eye(3, w)))
    names = _names(step.ll)
    assert names.count("tmjx_intervene") == 1 and names.index("tmjx_intervene") == after + 1
    assert names[:after + 1] + names[after + 2:] == LSTM_CALLS
    d = step.iv_entry[1][0]._obj
    if target.startswith("hidden_state"):
        k = int(target[-1])
        assert (d.h, d.w, d.ld) == (step.h.data_ptr() + 4 * 32 * k, 32, 64)
    else:
        assert (d.h, d.w, d.ld) == (step.x.data_ptr(), 8, step.x.shape[1])


def test_targets_and_widths_the_step_refuses():
    with pytest.raises(ValueError, match="does not exist in this policy step; it has: intention, encoder/layer_0, encoder/layer_1, decoder/layer_0, decoder/layer_1"):
        _mlp_step(Intervention("decoder/layer_2", "subspace", directions=np.eye(2, 16)))
    with pytest.raises(ValueError, match="does not exist in this policy step"):
        _mlp_step(Intervention("hidden_state/h:0", "subspace", directions=np.eye(2, 32)))
    with pytest.raises(ValueError, match="hidden_state/h:0, hidden_state/h:1"):
        _lstm_step(Intervention("hidden_state/h:2", "subspace", directions=np.eye(2, 32)))
    with pytest.raises(ValueError, match="directions are 9 wide, the target intention is 8 wide"):
        _mlp_step(Intervention("intention", "subspace", directions=np.eye(2, 9)))
    with pytest.raises(ValueError, match="unit 28 outside the 28 units of decoder/layer_0"):
        _mlp_step(Intervention.units("decoder/layer_0", [28]))
    with pytest.raises(ValueError, match="center has 5 entries"):
        _mlp_step(Intervention.units("decoder/layer_0", [2], center=np.zeros(5)))


def test_decoder_step_launch_lists():
    """environment.wrappers._DecoderStep (HighLevelWrapper's decoder): the layers path with and without an intervention, and the fused refusal."""
    from track_mjx_amd.agent.checkpoint import DecoderPolicy
    from track_mjx_amd.agent.networks import DecoderNet
    from track_mjx_amd.environment.wrappers import HighLevelWrapper, _DecoderStep
    torch.manual_seed(0)
    dp = DecoderPolicy(DecoderNet(8 + 16, 6, (28, 16)), torch.zeros(16), torch.ones(16), 8, 24)
    obs = torch.zeros((40, 3))
    plain = ["tmjx_decoder_input"] + BLOCK + BLOCK + ["tmjx_linear_nolds", "tmjx_action_mode"]
    assert _names(_DecoderStep(dp, 3, obs, "layers").ll) == plain
    for target, w, after in (("intention", 8, 0), ("decoder/layer_0", 28, 2), ("decoder/layer_1", 16, 4)):
        iv = Intervention(target, "subspace", directions=np.eye(2, w), window=(2, 4))
        step = _DecoderStep(dp, 3, obs, "layers", intervention=iv, gates=iv.per_clip(3))
        names = _names(step.ll)
        assert names.index("tmjx_intervene") == after + 1 and names[:after + 1] + names[after + 2:] == plain
        assert step.iv.t_on.tolist() == [2, 2, 2] and step.iv.t_off.tolist() == [4, 4, 4]
    iv = Intervention("encoder/layer_0", "subspace", directions=np.eye(2, 32))
    with pytest.raises(ValueError, match="does not exist in this policy step; it has: intention, decoder/layer_0, decoder/layer_1"):
        _DecoderStep(dp, 3, obs, "layers", intervention=iv, gates=iv.per_clip(3))
    iv = Intervention("decoder/layer_0", "subspace", directions=np.eye(2, 28))
    with pytest.raises(ValueError, match="path='fused' cannot run an intervention: the fused decoder launch has no seam"):
        HighLevelWrapper(object(), dp, 24, path="fused", intervention=iv)


# ------------------------------------------------------------------------------------------------------------------ 7: effect summary
def test_effect_summary_tool(tmp_path, capsys):
    from track_mjx_amd.analysis.utils import load_from_h5py, save_to_h5py
    rng = np.random.default_rng(3)
    T, nq = 12, 74
    base, pert = tmp_path / "base", tmp_path / "pert"
    base.mkdir(); pert.mkdir()
    iv = Intervention("intention", "subspace", directions=np.eye(2, 60), window=(5, 9))
    want = {}
    for c in (0, 3, 4):
        q = rng.standard_normal((T, nq)).astype(np.float32)
        r = rng.random(T).astype(np.float32)
        m = {"pos_rewards": rng.random(T).astype(np.float32), "falls": np.zeros(T, np.float32)}
        save_to_h5py(base / f"clip_{c}.h5", {"qposes_rollout": q, "state_rewards": r, "rollout_metrics": m})
        if c == 4:
            continue                                                                    # (only in the baseline: not summarised)
        q2, r2, m2 = q.copy(), r.copy(), {k: v.copy() for k, v in m.items()}
        if c == 3:
            q2[6:, 0] += 0.5; q2[7:, 10] -= 0.25; r2[6:] -= 0.125; m2["pos_rewards"][6:] -= 0.5
        rec = {k: v[0] for k, v in iv.record(*iv.per_clip(1), np.zeros((1, T - 1, 2), np.float32)).items()}
        save_to_h5py(pert / f"clip_{c}.h5", {"qposes_rollout": q2, "state_rewards": r2, "rollout_metrics": m2, "intervention": rec})
        want[c] = (q, q2, r, r2)
    save_to_h5py(pert / "clip_9.h5", {"qposes_rollout": q, "state_rewards": r})
    out = tmp_path / "sub" / "effect.h5"
    assert IV.main([f"baseline={base}", f"perturbed={pert}", f"out={out}"]) == 0
    assert "2 clips; diverged: 1 (first step: 6)" in capsys.readouterr().out
    got = load_from_h5py(out)
    assert set(got) == {"clip_0", "clip_3"}
    g0, g3 = got["clip_0"], got["clip_3"]
    assert int(g0["first_divergence"]) == -1 and float(g0["reward_mean_difference"]) == 0 and not g0["root_distance"].any() and not g0["joint_distance"].any()
    q, q2, r, r2 = want[3]
    assert int(g3["first_divergence"]) == 6
    assert abs(float(g3["reward_mean_difference"]) - (-0.125 * 6 / T)) < 1e-7
    assert abs(float(g3["reward_mean_baseline"]) - r.astype(np.float64).mean()) < 1e-12 and abs(float(g3["reward_mean_perturbed"]) - r2.astype(np.float64).mean()) < 1e-12
    assert g3["root_distance"].shape == (T,) and np.allclose(g3["root_distance"], [0] * 6 + [0.5] * 6)
    assert np.allclose(g3["joint_distance"], [0] * 7 + [0.25] * 5)
    assert abs(float(g3["metric_mean_difference"]["pos_rewards"]) + 0.25) < 1e-7 and float(g3["metric_mean_difference"]["falls"]) == 0
    ivg = g3["intervention"]
    assert bytes(ivg["target"]) == b"intention" and ivg["window"].tolist() == [5, 9] and ivg["projection"].shape == (T - 1, 2) and ivg["directions"].shape == (2, 60)
    assert IV.main([f"baseline={base}"]) == 2
    assert IV.main([f"baseline={base}", f"perturbed={tmp_path / 'sub'}", f"out={out}"]) == 2
    assert "no clip_<i>.h5 present in both" in capsys.readouterr().err
