"""The representation-comparison kernels (csrc/tmjx_compare.hip) through the C-ABI against the float64 reference (tests/compare_ref.py): CKA
against float64 and its exact properties, the RDM correlation under every metric pair, its special rows and its pair count, the CCA on the
planted cases and its properties, the decomposition on its own, the bit-level properties (repeatability, row strides), the refusals and the
command-line tool.  tests/test_compare_cpu.py runs the same checks on the host emulation of the same kernel bodies."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import compare_ref as R
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


@pytest.mark.parametrize("offset", (0.0, 1e3))
@pytest.mark.parametrize("case", R.CKA_CASES)
def test_cka_against_float64(case, offset):
    R.check_cka(case, offset, backend(), "kernel")


def test_cka_exact_properties():
    R.check_cka_properties(backend(), "kernel")


@pytest.mark.parametrize("case", R.RDM_CASES)
def test_rdm_against_float64(case):
    R.check_rdm(case, backend(), "kernel")


@pytest.mark.parametrize("case", R.RDM_OFFSET_CASES)
def test_rdm_far_from_the_origin(case):
    R.check_rdm_offset(case, backend(), "kernel")


def test_rdm_rows_without_variance_duplicates_labels_and_self():
    R.check_rdm_special(backend(), "kernel")


@pytest.mark.parametrize("n", R.COUNT_N)
def test_rdm_counts_every_pair_once(n):
    R.check_rdm_count(n, backend())


@pytest.mark.parametrize("case", R.CCA_CASES)
def test_cca_against_float64(case):
    R.check_cca(case, backend(), "kernel")


def test_cca_properties():
    R.check_cca_properties(backend(), "kernel")


@pytest.mark.parametrize("shape", R.SVD_SHAPES)
def test_svd_known_singular_values(shape):
    R.check_svd(shape, backend(), "kernel")


def test_two_calls_and_strided_rows_give_the_same_bits():
    R.check_repeat_and_strides(backend(), strided, "kernel")


def test_refusals_launch_nothing():
    def alloc(shape, dtype, fill):
        return torch.full(tuple(shape), fill, dtype=getattr(torch, np.dtype(dtype).name), device=DEV)

    def untouched(t, fill):
        torch.cuda.synchronize()
        return bool((t == fill).all())
    R.check_refusals(hip.lib(), alloc, lambda t: t.data_ptr(), untouched, "kernel")


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, backend(), capsys)
