"""The LSTM-decoder-Jacobian kernels (csrc/tmjx_lstm_jacobian.hip) through the C-ABI against the float64 reference (tests/lstm_jacobian_ref.py): every
output of every case in both modes, the exact properties (zero rows, a saturated tanh, W_hh = 0, permuted and repeated rows, repeatability, row
strides, a row alone, an index out of range, the input side with and without the carry outputs), the refusals, the tool against the emulation's
file, and one real path: a freshly initialised use_lstm checkpoint, analysis.rollout of two clips with log_decoder_input=true (the recorded
egocentric_obs is the normalised observation; without the option the recorded set is what it was), and the tool on them (the recomputed forward is
the recorded one, row 0 of every clip is evaluated with a zero carry).  tests/test_lstm_jacobian_cpu.py runs the same checks on the host emulation of
the same kernel bodies."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from tests import lstm_jacobian_ref as R
from tests.test_gpu_rollout import lstm_ckpt  # noqa: F401
from track_mjx_amd import hip
from track_mjx_amd.analysis import pca as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(None)
def backend():
    return P.HipBackend(DEV)


def strided(a):
    buf = torch.full((a.shape[0], a.shape[1] + 5), 1e6, dtype=torch.float32, device=DEV)
    buf[:, 3:3 + a.shape[1]] = torch.from_numpy(np.array(a))
    xs = buf[:, 3:3 + a.shape[1]]
    assert backend().asarray(xs).data_ptr() == xs.data_ptr() and xs.stride(0) == a.shape[1] + 5      # no copy
    return xs


@pytest.mark.parametrize("case", R.CASES, ids=[str(i) for i in range(len(R.CASES))])
def test_case_against_float64(case):
    R.check_case(case, backend(), "kernel")


def test_exact_properties():
    R.check_properties(backend(), strided, "kernel")


def test_a_row_alone_has_the_bits_it_has_in_either_pass():
    R.check_rows_across_passes(backend())


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
    from tests.hostemu import lstm_jacobian_emu as T
    R.check_tool_files_agree(tmp_path, backend(), T.B, capsys)


def test_real_path_checkpoint_rollout_with_decoder_input_jacobian(lstm_ckpt, tmp_path, capsys):  # noqa: F811
    from tests.test_gpu_rollout import _gen, _replay
    from track_mjx_amd.agent import checkpoint as ck
    from track_mjx_amd.analysis import jacobian as JT
    from track_mjx_amd.analysis import rollout as ro
    from track_mjx_amd.analysis.utils import load_from_h5py
    path, out, jac = lstm_ckpt[0], tmp_path / "rollouts", tmp_path / "jacobian.h5"
    assert ro.main([f"checkpoint={path}", "clips=3,5", f"out={out}", "log_activations=true", "log_metrics=false", "log_decoder_input=true"]) == 0
    assert sorted(os.listdir(out)) == ["clip_3.h5", "clip_5.h5"]
    recs = [load_from_h5py(out / f"clip_{c}.h5") for c in (3, 5)]
    # the option adds egocentric_obs, the normalised proprioceptive columns of the observation, and nothing else
    gen, _, fn, cfg = _gen(path)
    assert all(set(r["activations"]) == {"encoder", "decoder", "intention", "hidden_state", "egocentric_obs"} for r in recs)
    _, _, _, obs = _replay(cfg, {"ctrl": np.stack([r["ctrl"] for r in recs])}, [3, 5])
    norm = (obs - fn.mean.cpu().numpy()) / fn.std.cpu().numpy()
    for j, r in enumerate(recs):
        assert np.array_equal(np.ascontiguousarray(r["activations"]["egocentric_obs"]).view(np.uint32), np.ascontiguousarray(norm[j][:, 470:]).view(np.uint32)), j
    plain = gen([3])      # (the module's generator: log_activations without the option)
    assert set(plain["activations"]) == {"encoder", "decoder", "intention", "hidden_state"}
    assert np.array_equal(plain["ctrl"][0].view(np.uint32), recs[0]["ctrl"].view(np.uint32))
    # the tool on the result
    assert JT.main([f"checkpoint={path}", f"rollouts={out}", f"out={jac}", "store=true"]) == 0
    f = load_from_h5py(jac)
    T, L, H = recs[0]["ctrl"].shape[0] + 1, 2, 128
    with capsys.disabled():
        print(f"[lstm jacobian real path] forward mismatch {float(f['forward_mismatch']):.3g} over {int(f['rows'])} rows of 2 clips; mean memory sensitivity "
              f"{np.nanmean(f['memory_sensitivity']['clip_3'], 0)}, mean gain {float(np.trace(f['gram_in'])):.3g}")
    assert float(f["forward_mismatch"]) < JT.MISMATCH_WARN and "warning" not in capsys.readouterr().err      # the recomputed forward is the recorded one
    assert f["mean_jacobian"].shape == (38, 60) and bytes(f["model"]) == b"lstm" and f["clips"].tolist() == [3, 5] and f["mean_carry_jacobian"].shape == (38, 2 * L * H)
    ms = f["memory_sensitivity"]["clip_3"]
    assert ms.shape == (T - 1, 2 * L) and np.isfinite(ms).all() and float(ms.sum()) > 0
    # row 0 of every clip is evaluated with a zero carry: its stored rows are those of its input row against zeros
    layers, head = JT.lstm_decoder_weights(path)
    for c, r in zip((3, 5), recs):
        x0 = np.concatenate([r["activations"]["intention"][:1], r["activations"]["egocentric_obs"][:1]], 1)
        zero = np.zeros((1, L * H), np.float32)
        b = backend()
        one = b.lstm_decoder_jacobian(b.asarray(x0), b.asarray(zero), b.asarray(zero), layers, head, (0, 60), carry_scale=f["carry_std"])
        assert R.same_bits(one["jac"][0], f["jacobian"][f"clip_{c}"][0]) and R.same_bits(one["carry_jac"][0], f["carry_jacobian"][f"clip_{c}"][0]), c
        assert R.same_bits(one["carry_gain"][0], f["memory_sensitivity"][f"clip_{c}"][0]), c
