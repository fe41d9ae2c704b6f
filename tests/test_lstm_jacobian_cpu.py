"""The LSTM-decoder-Jacobian kernels on the CPU: the bodies of csrc/lstm_jacobian_core.h and csrc/jacobian_core.h compiled for the host
(tests/hostemu/lstm_jacobian_emu.cpp), called through analysis.backend.Backend and checked against the float64 reference
(tests/lstm_jacobian_ref.py): the reference itself against torch autograd, every output of every case in both modes, the exact properties, the
refusals (on the emulation and, with host arrays, on the product library, which checks before it launches), the marshalling, and the tool on
three synthetic LSTM clips.  The stand-alone emulation runs the first four cases under the address and undefined-behaviour sanitizers with buffers
of exactly the contract's sizes.  tests/test_gpu_lstm_jacobian.py runs the same checks through the C-ABI on the device."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import lstm_jacobian_ref as R
from tests.hostemu import lstm_jacobian_emu as T

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
    net, x, h, c, scale, cs = R.problem(R.PROPERTY_CASE)
    for subs in (dict(m=0), dict(mode=3), dict(misalign=True), dict(ldx=8), dict(ld_carry=63), dict(sums=None), dict(h_in=None)):
        with pytest.raises(ValueError):
            R.run(T.over("tmjx_lstm_decoder_jacobian", **subs), net, x, h, c, R.PROPERTY_CASE[2], 0, scale, cs)


def test_refusals_on_the_product_library_launch_nothing():
    from track_mjx_amd import hip
    R.check_refusals(hip.lib(), _numpy_alloc(), lambda a: a.ctypes.data, lambda a, fill: bool((a == fill).all()), "product, host arrays")


def test_backend_marshalling():
    """What the backend refuses before the library sees it, and what it hands over: the carry's one row stride, the layers' shapes, carry_scale's
    length; `want` selects the optional outputs, the sums always come."""
    net, x, h, c, scale, cs = R.problem(R.PROPERTY_CASE)
    m, d_in, wrt, H, L, A, _, _ = R.PROPERTY_CASE
    got = R.run(B, net, x, h, c, wrt, 0, None, None, want=("gain",))
    assert set(got) == {"gain", "mean_sum", "gram_in", "gram_out", "carry_sum"} and got["carry_sum"].shape == (A, 2 * L * H) and got["carry_sum"].dtype == np.float64
    full = R.run(B, net, x, h, c, wrt, 0, scale, cs)
    assert full["carry_jac"].shape == (m, A, 2 * L * H) and full["carry_gain"].shape == (m, 2 * L) and full["action_var"].shape == (m, A)
    assert R.same_bits(full["gain"], got["gain"]) and R.same_bits(full["carry_sum"], got["carry_sum"])
    with pytest.raises(ValueError, match="row strides"):
        R.run(B, net, x, strided(h), c, wrt)
    with pytest.raises(ValueError, match="h_in has shape"):
        R.run(B, net, x, h[:, :-1], c, wrt)
    with pytest.raises(ValueError, match="carry_scale holds"):
        R.run(B, net, x, h, c, wrt, carry_scale=cs[:-1])
    with pytest.raises(ValueError, match="LSTM layer 1"):
        R.run(B, R._variant(net, w_hh=(1, np.zeros((4 * H, H + 1), np.float32))), x, h, c, wrt)
    five = R.Net(d_in, H, 5, A, 1)
    with pytest.raises(ValueError, match="5 LSTM layers"):
        R.run(B, five, x, np.zeros((m, 5 * H), np.float32), np.zeros((m, 5 * H), np.float32), wrt)


def test_tool_on_three_synthetic_lstm_clips(tmp_path, capsys):
    R.check_tool(tmp_path, B, capsys)


def test_emulation_under_sanitizers(tmp_path):
    exe = T.build_main(tmp_path / "lstm_jacobian_emu", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for m, d_in, (c0, Z), H, L, A, ldx, ldc in R.CASES[:4]:
        res = subprocess.run([str(exe), *[str(v) for v in (m, d_in, c0, Z, H, L, A, ldx or d_in, ldc or L * H)]], capture_output=True, text=True)
        assert res.returncode == 0 and "finite: 1" in res.stdout, res.stdout + res.stderr
