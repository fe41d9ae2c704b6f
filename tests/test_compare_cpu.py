"""The representation-comparison kernels on the CPU: the bodies of csrc/compare_core.h compiled for the host (tests/hostemu/compare_emu.cpp),
called through analysis.backend.Backend and checked against the float64 reference (tests/compare_ref.py): CKA against float64 and its exact
properties, the RDM correlation under every metric pair, its special rows and its pair count, the CCA on the planted cases and its properties,
the decomposition on its own, the bit-level properties, the command line and the refusals (on the emulation and, with host arrays, on the
product library, which checks before it launches).  The stand-alone emulation runs under the address and undefined-behaviour sanitizers with
buffers of exactly the contract's sizes.  tests/test_gpu_compare.py runs the same checks through the C-ABI on the device."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import compare_ref as R
from tests.hostemu import compare_emu as T

B = T.B


def strided(a):
    buf = np.full((a.shape[0], a.shape[1] + 5), 1e6, np.float32)
    buf[:, 3:3 + a.shape[1]] = a
    xs = buf[:, 3:3 + a.shape[1]]
    assert B.asarray(xs) is xs or B.asarray(xs).ctypes.data == xs.ctypes.data      # no copy
    return xs


@pytest.mark.parametrize("offset", (0.0, 1e3))
@pytest.mark.parametrize("case", R.CKA_CASES)
def test_cka_against_float64(case, offset):
    R.check_cka(case, offset, B, "emulation")


def test_cka_exact_properties():
    R.check_cka_properties(B, "emulation")


@pytest.mark.parametrize("case", R.RDM_CASES)
def test_rdm_against_float64(case):
    R.check_rdm(case, B, "emulation")


@pytest.mark.parametrize("case", R.RDM_OFFSET_CASES)
def test_rdm_far_from_the_origin(case):
    R.check_rdm_offset(case, B, "emulation")


def test_rdm_rows_without_variance_duplicates_labels_and_self():
    R.check_rdm_special(B, "emulation")


@pytest.mark.parametrize("n", R.COUNT_N)
def test_rdm_counts_every_pair_once(n):
    R.check_rdm_count(n, B)


@pytest.mark.parametrize("case", R.CCA_CASES)
def test_cca_against_float64(case):
    R.check_cca(case, B, "emulation")


def test_cca_properties():
    R.check_cca_properties(B, "emulation")


@pytest.mark.parametrize("shape", R.SVD_SHAPES)
def test_svd_known_singular_values(shape):
    R.check_svd(shape, B, "emulation")


def test_two_calls_and_strided_rows_give_the_same_bits():
    R.check_repeat_and_strides(B, strided, "emulation")


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, B, capsys)


def _numpy_alloc():
    keep = []

    def alloc(shape, dtype, fill):
        raw = np.empty(int(np.prod(shape)) * np.dtype(dtype).itemsize + 16, np.uint8)
        start = (-raw.ctypes.data) % 16
        a = raw[start:start + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
        a[...] = fill
        keep.append(raw)
        return a
    return alloc


def test_refusals_on_the_emulation():
    R.check_refusals(T.ARRAYS.library, _numpy_alloc(), lambda a: a.ctypes.data, lambda a, fill: bool((a == fill).all()), "emulation")
    # through the backend: the guards and sentinels of NumpyArrays come back clean
    x, y = R.cka_data(R.CKA_CASES[1], 0.0)
    for entry, subs, call in (("tmjx_cka_linear", dict(n=2), lambda b: b.cka_linear(b.asarray(x), b.asarray(y))),
                              ("tmjx_cka_linear", dict(misalign=True), lambda b: b.cka_linear(b.asarray(x), b.asarray(y))),
                              ("tmjx_rdm_corr", dict(metric_x=7), lambda b: b.rdm_corr(b.asarray(x), 0, b.asarray(y), 0)),
                              ("tmjx_cca", dict(var_keep=0.0), lambda b: b.cca(b.asarray(x), b.asarray(y)))):
        with pytest.raises(ValueError):
            call(T.over(entry, **subs))


def test_refusals_on_the_product_library_launch_nothing():
    from track_mjx_amd import hip
    R.check_refusals(hip.lib(), _numpy_alloc(), lambda a: a.ctypes.data, lambda a, fill: bool((a == fill).all()), "product, host arrays")


def test_emulation_under_sanitizers(tmp_path):
    exe = T.build_main(tmp_path / "compare_emu", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for args in ((), ("513", "40", "130"), ("3", "1", "1"), ("259", "129", "2")):
        res = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert res.returncode == 0 and "rebuild their matrices: 1" in res.stdout, res.stdout + res.stderr
