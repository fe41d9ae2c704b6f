"""The behaviour-map kernels (csrc/tmjx_tsne.hip) through the C-ABI against the float64 reference (tests/tsne_ref.py): the kNN cases, the exact
grid, ties and self, the affinities, the gradient, the update, the fit as its steps, placement, the bit-level properties (repeatability, row
strides), the refusals, `TSNE` on the planted blobs (ten separated motifs that the first two PCs cannot show) and the command-line tool.
tests/test_embed_cpu.py runs the same checks on the host emulation of the same kernel bodies."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import tsne_ref as R
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


@pytest.mark.parametrize("case", R.KNN_CASES)
def test_knn_against_float64(case):
    R.check_knn(case, backend(), "kernel")


def test_knn_exact_grid_ties_and_self():
    R.check_knn_exact(backend())
    R.check_knn_duplicates(backend())
    R.check_knn_self(backend())


def test_knn_two_calls_and_strided_rows_give_the_same_bits():
    R.check_knn_repeat_and_strides(backend(), strided, "kernel")


@pytest.mark.parametrize("k", R.AFFINITY_K)
def test_affinities_against_float64(k):
    R.check_affinities(k, backend(), "kernel")


@pytest.mark.parametrize("scale", R.GRADIENT_SCALES)
@pytest.mark.parametrize("n", R.GRADIENT_N)
def test_gradient_against_float64(n, scale):
    R.check_gradient(n, scale, backend(), "kernel")


@pytest.mark.parametrize("n", (2, 257, 1000))
def test_update_is_exact(n):
    R.check_update(n, backend(), "kernel")


def test_fit_is_its_steps():
    R.check_fit_steps(backend(), "kernel")


def test_place_is_exact_and_inside_the_hull():
    R.check_place(backend(), "kernel")


def test_model_level_on_the_planted_blobs():
    R.check_model(backend(), "kernel")


def test_transform_places_held_out_rows_in_their_blob():
    R.check_transform(backend(), "kernel")


def test_tsne_on_numpy_and_strided_device_tensors():
    R.check_tsne_inputs(backend(), strided, "kernel")


def test_refusals_launch_nothing():
    def alloc(shape, dtype, fill):
        return torch.full(tuple(shape), fill, dtype=getattr(torch, np.dtype(dtype).name), device=DEV)

    def untouched(t, fill):
        torch.cuda.synchronize()
        return bool((t == fill).all())
    R.check_refusals(hip.lib(), alloc, lambda t: t.data_ptr(), untouched, "kernel")


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, backend(), capsys)
