"""The LSTM-decoder-dynamics kernels (csrc/tmjx_lstm_tangent.hip) through the C-ABI against the float64 reference (tests/lstm_dynamics_ref.py): every
output of every case, the tangent step across a pass, the exact properties (repeatability, a sequence alone, among others and permuted, the
prefix of a K-run, cut and continued sequences, decoupled layers, a zero column, row strides), the refusals, the tool against the emulation's
file, and one real path: a freshly initialised use_lstm checkpoint, analysis.rollout of two clips with log_decoder_input=true, and the tool on
them (the recomputed forward is the recorded one, row 0 of every clip is evaluated with a zero carry).  tests/test_lstm_dynamics_cpu.py runs the
same checks on the host emulation of the same kernel bodies."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import lstm_dynamics_ref as R
from tests.test_gpu_rollout import lstm_ckpt  # noqa: F401
from track_mjx_amd import hip
from track_mjx_amd.analysis import pca as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(None)
def backend():
    return P.HipBackend(DEV)


@pytest.mark.parametrize("case", R.CASES, ids=[str(i) for i in range(len(R.CASES))])
def test_case_against_float64(case):
    R.check_case(case, backend(), "kernel")


def test_tangent_step_across_a_pass_against_float64():
    R.check_step(backend(), "kernel")


def test_decoupled_layers_follow_the_closed_form():
    R.check_decoupled(backend(), "kernel")


def test_exact_properties():
    R.check_properties(backend(), "kernel")


def test_refusals_launch_nothing():
    def alloc(shape, dtype, fill):
        return torch.full(tuple(shape), fill, dtype=getattr(torch, np.dtype(dtype).name), device=DEV)

    def untouched(t, fill):
        torch.cuda.synchronize()
        return bool((t == fill).all())
    R.check_refusals(hip.lib(), alloc, lambda t: t.data_ptr(), untouched, "kernel")


def test_tool_on_three_synthetic_lstm_clips(tmp_path, capsys):
    R.check_tool(tmp_path, backend(), capsys)


def test_tool_writes_the_emulations_file_within_the_bounds(tmp_path, capsys):
    from tests.hostemu import lstm_dynamics_emu as T
    R.check_tool_files_agree(tmp_path, backend(), T.B, capsys)


def test_real_path_checkpoint_rollout_dynamics(lstm_ckpt, tmp_path, capsys):  # noqa: F811
    """What a freshly initialised policy gives is reported, not asserted."""
    from track_mjx_amd.analysis import dynamics as DT
    from track_mjx_amd.analysis import jacobian as JT
    from track_mjx_amd.analysis import rollout as ro
    from track_mjx_amd.analysis.utils import load_from_h5py
    path, out, dyn = lstm_ckpt[0], tmp_path / "rollouts", tmp_path / "dynamics.h5"
    assert ro.main([f"checkpoint={path}", "clips=3,5", f"out={out}", "log_activations=true", "log_metrics=false", "log_decoder_input=true"]) == 0
    capsys.readouterr()
    assert DT.main([f"checkpoint={path}", f"rollouts={out}", f"out={dyn}", "k=16", "warmup=25", "rate=50"]) == 0
    text = capsys.readouterr()
    f = load_from_h5py(dyn)
    recs = [load_from_h5py(out / f"clip_{c}.h5") for c in (3, 5)]
    T, L, H, K = recs[0]["ctrl"].shape[0] + 1, 2, 128, 16
    with capsys.disabled():
        print(f"[lstm dynamics real path] forward mismatch {float(f['forward_mismatch']):.3g} over {int(f['rows'])} rows ({int(f['counted_rows'])} counted) in "
              f"{len(f['status'])} sequences of 2 clips; spectrum per step {np.array2string(f['exponents'], precision=4)}; memory half-life "
              f"{float(f['memory_halflife_steps']):.4g} steps = {float(f['memory_halflife_seconds']):.4g} s; Kaplan-Yorke dimension {float(f['kaplan_yorke_dimension']):.4g}")
    assert float(f["forward_mismatch"]) < JT.MISMATCH_WARN and "forward" not in text.err      # the recomputed forward is the recorded one
    assert f["local_exponents"]["clip_3"].shape == (T - 1, K) and np.isfinite(f["local_exponents"]["clip_3"]).all()
    assert f["exponents"].shape == (K,) and np.isfinite(f["exponents"]).all() and f["final_basis"]["clip_5"].shape == (K, 2 * L * H)
    assert bytes(f["model"]) == b"lstm" and f["clips"].tolist() == [3, 5] and (f["status"] == 0).all()
    # row 0 of every clip equals, bit for bit, a direct call on that row with a zero carry
    layers, _ = JT.lstm_decoder_weights(path)
    b, zero = backend(), np.zeros((1, L * H), np.float32)
    for c, r in zip((3, 5), recs):
        x0 = np.concatenate([r["activations"]["intention"][:1], r["activations"]["egocentric_obs"][:1]], 1)
        one = b.lstm_lyapunov(b.asarray(x0), b.asarray(zero), b.asarray(zero), layers, np.array([0, 1], np.int32), DT.first_basis(2 * L * H, K, 0), 0, ("local",))
        assert R.same_bits(one["local"][0], f["local_exponents"][f"clip_{c}"][0]), c
