"""The behaviour-map kernels on the CPU: the bodies of csrc/tsne_core.h compiled for the host (tests/hostemu/tsne_emu.cpp), called through
analysis.backend.Backend and checked against the float64 reference (tests/tsne_ref.py): the kNN cases, the exact grid, ties and self, the
affinities, the gradient, the update, the fit as its steps, placement, the planted blobs, `TSNE`, the host map, the command line and the refusals
(on the emulation and, with host arrays, on the product library, which checks before it launches).  The stand-alone emulation runs under the
address and undefined-behaviour sanitizers with buffers of exactly the contract's sizes.  tests/test_gpu_embed.py runs the same checks through
the C-ABI on the device."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import tsne_ref as R
from tests.hostemu import tsne_emu as T

B = T.B


def strided(a):
    buf = np.full((a.shape[0], a.shape[1] + 5), 1e6, np.float32)
    buf[:, 3:3 + a.shape[1]] = a
    xs = buf[:, 3:3 + a.shape[1]]
    assert B.asarray(xs) is xs or B.asarray(xs).ctypes.data == xs.ctypes.data      # no copy
    return xs


@pytest.mark.parametrize("case", R.KNN_CASES)
def test_knn_against_float64(case):
    R.check_knn(case, B, "emulation")


def test_knn_exact_grid_ties_and_self():
    R.check_knn_exact(B)
    R.check_knn_duplicates(B)
    R.check_knn_self(B)


def test_knn_two_calls_and_strided_rows_give_the_same_bits():
    R.check_knn_repeat_and_strides(B, strided, "emulation")


@pytest.mark.parametrize("k", R.AFFINITY_K)
def test_affinities_against_float64(k):
    R.check_affinities(k, B, "emulation")


@pytest.mark.parametrize("scale", R.GRADIENT_SCALES)
@pytest.mark.parametrize("n", R.GRADIENT_N)
def test_gradient_against_float64(n, scale):
    R.check_gradient(n, scale, B, "emulation")


@pytest.mark.parametrize("n", (2, 257, 1000))
def test_update_is_exact(n):
    R.check_update(n, B, "emulation")


def test_fit_is_its_steps():
    R.check_fit_steps(B, "emulation")


def test_place_is_exact_and_inside_the_hull():
    R.check_place(B, "emulation")


def test_model_level_on_the_planted_blobs():
    R.check_model(B, "emulation")


def test_transform_places_held_out_rows_in_their_blob():
    R.check_transform(B, "emulation")


def test_tsne_on_numpy_and_strided_inputs():
    R.check_tsne_inputs(B, strided, "emulation")


def test_density_and_watershed():
    R.check_density_and_watershed()


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
    x, _ = R.knn_data(R.KNN_CASES[5])
    for entry, subs, call in (("tmjx_knn", dict(k=129), lambda b: b.knn(b.asarray(x), None, 128, exclude_self=True)),
                              ("tmjx_knn", dict(misalign=True), lambda b: b.knn(b.asarray(x), None, 8, exclude_self=True)),
                              ("tmjx_tsne_affinities", dict(perplexity=8.0), lambda b: b.tsne_affinities(np.ones((4, 8), np.float32), 3.0)),
                              ("tmjx_tsne_gradient", dict(nnz=3), lambda b: b.tsne_gradient(*R.gradient_case(3, 1.0))),
                              ("tmjx_tsne_update", dict(eta=-1.0), lambda b: b.tsne_update(*[np.ones((3, 2), np.float32)] * 4, 0.5, 50.0))):
        with pytest.raises(ValueError):
            call(T.over(entry, **subs))
    idx, dist2 = B.knn(B.asarray(x), None, 128, exclude_self=True)      # k at its ceiling is served
    assert idx.shape == (130, 128)


def test_refusals_on_the_product_library_launch_nothing():
    from track_mjx_amd import hip
    R.check_refusals(hip.lib(), _numpy_alloc(), lambda a: a.ctypes.data, lambda a, fill: bool((a == fill).all()), "product, host arrays")


def test_emulation_under_sanitizers(tmp_path):
    exe = T.build_main(tmp_path / "tsne_emu", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for args in ((), ("513", "40", "128"), ("3", "1", "2"), ("259", "33", "7")):
        res = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert res.returncode == 0 and "the fit equals its steps: 1" in res.stdout, res.stdout + res.stderr
