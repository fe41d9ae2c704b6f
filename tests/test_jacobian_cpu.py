"""The decoder-Jacobian kernels on the CPU: the bodies of csrc/jacobian_core.h compiled for the host (tests/hostemu/jacobian_emu.cpp), called
through analysis.backend.Backend and checked against the float64 reference (tests/jacobian_ref.py): the reference itself against torch autograd,
every output of every case in both modes, the exact properties, the refusals (on the emulation and, with host arrays, on the product library,
which checks before it launches), and the tool on three synthetic clips.  The stand-alone emulation runs the first four cases under the address
and undefined-behaviour sanitizers with buffers of exactly the contract's sizes.  tests/test_gpu_jacobian.py runs the same checks through the
C-ABI on the device."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import jacobian_ref as R
from tests.hostemu import jacobian_emu as T

B = T.B


def strided(a):
    buf = np.full((a.shape[0], a.shape[1] + 5), 1e6, np.float32)
    buf[:, 3:3 + a.shape[1]] = a
    xs = buf[:, 3:3 + a.shape[1]]
    assert B.asarray(xs).ctypes.data == xs.ctypes.data      # no copy
    return xs


def test_reference_against_torch_autograd():
    R.check_reference_against_autograd()


@pytest.mark.parametrize("case", R.CASES, ids=[str(i) for i in range(len(R.CASES))])
def test_case_against_float64(case):
    R.check_case(case, B, "emulation")


def test_exact_properties():
    R.check_properties(B, strided, "emulation")


def test_a_row_alone_has_the_bits_it_has_in_either_pass():
    R.check_rows_across_passes(B)


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
    net, x, scale = R.problem(R.PROPERTY_CASE)
    for subs in (dict(m=0), dict(mode=3), dict(misalign=True), dict(ldx=8), dict(sums=None)):
        with pytest.raises(ValueError):
            R.run(T.over("tmjx_decoder_jacobian", **subs), net, x, R.PROPERTY_CASE[2], 0, scale)


def test_refusals_on_the_product_library_launch_nothing():
    from track_mjx_amd import hip
    R.check_refusals(hip.lib(), _numpy_alloc(), lambda a: a.ctypes.data, lambda a, fill: bool((a == fill).all()), "product, host arrays")


def test_tool_on_three_synthetic_clips(tmp_path, capsys):
    R.check_tool(tmp_path, B, capsys)


def test_emulation_under_sanitizers(tmp_path):
    exe = T.build_main(tmp_path / "jacobian_emu", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for m, d_in, (c0, Z), widths, A, ldx in R.CASES[:4]:
        res = subprocess.run([str(exe), *[str(v) for v in (m, d_in, c0, Z, A, ldx or d_in, *widths)]], capture_output=True, text=True)
        assert res.returncode == 0 and "finite: 1" in res.stdout, res.stdout + res.stderr
