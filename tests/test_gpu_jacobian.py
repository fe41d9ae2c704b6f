"""The decoder-Jacobian kernels (csrc/tmjx_jacobian.hip) through the C-ABI against the float64 reference (tests/jacobian_ref.py): every output of
every case in both modes, the exact properties (zero rows, gamma = 0, a saturated tanh, permuted and repeated rows, repeatability, row strides, a
row alone), the refusals, the tool against the emulation's file, and one real path: a freshly initialised checkpoint, analysis.rollout of two
clips with the activations recorded, the tool on them (the recomputed forward is the recorded one), and a roll-out that projects out the
directions it found.  tests/test_jacobian_cpu.py runs the same checks on the host emulation of the same kernel bodies."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from tests import jacobian_ref as R
from tests.test_gpu_rollout import mlp_ckpt  # noqa: F401
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


def test_tool_on_three_synthetic_clips(tmp_path, capsys):
    R.check_tool(tmp_path, backend(), capsys)


def test_tool_writes_the_emulations_file_within_the_bounds(tmp_path, capsys):
    from tests.hostemu import jacobian_emu as T
    R.check_tool_files_agree(tmp_path, backend(), T.B, capsys)


def test_real_path_checkpoint_rollout_jacobian_intervention(mlp_ckpt, tmp_path, capsys):  # noqa: F811
    from track_mjx_amd.analysis import jacobian as JT
    from track_mjx_amd.analysis import rollout as ro
    from track_mjx_amd.analysis.utils import load_from_h5py
    path, out, jac = mlp_ckpt[0], tmp_path / "rollouts", tmp_path / "jacobian.h5"
    assert ro.main([f"checkpoint={path}", "clips=3,5", f"out={out}", "log_activations=true", "log_metrics=false"]) == 0
    assert sorted(os.listdir(out)) == ["clip_3.h5", "clip_5.h5"]
    assert JT.main([f"checkpoint={path}", f"rollouts={out}", f"out={jac}"]) == 0
    f = load_from_h5py(jac)
    with capsys.disabled():
        print(f"[jacobian real path] forward mismatch {float(f['forward_mismatch']):.3g} over {int(f['rows'])} rows of 2 clips")
    assert float(f["forward_mismatch"]) < JT.MISMATCH_WARN and "warning" not in capsys.readouterr().err      # the recomputed forward is the recorded one
    assert f["mean_jacobian"].shape == (38, 60) and f["components"].shape == (60, 60) and bytes(f["feature"]) == b"intention" and f["clips"].tolist() == [3, 5]
    assert int(f["rows"]) > 100 and np.isfinite(f["gram_in"]).all() and float(np.trace(f["gram_in"])) > 0
    assert ro.main([f"checkpoint={path}", "clips=3", f"out={tmp_path / 'projected'}", f"intervene_pca={jac}", "intervene_components=0:2",
                    "log_activations=false", "log_metrics=false"]) == 0
    g = load_from_h5py(tmp_path / "projected" / "clip_3.h5")["intervention"]
    assert bytes(g["target"]) == b"intention" and g["directions"].shape == (2, 60)
