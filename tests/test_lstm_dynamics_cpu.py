"""The LSTM-decoder-dynamics kernels on the CPU: the bodies of csrc/lstm_tangent_core.h, csrc/lstm_jacobian_core.h and csrc/jacobian_core.h compiled
for the host (tests/hostemu/lstm_dynamics_emu.cpp), called through analysis.backend.Backend and checked against the float64 reference
(tests/lstm_dynamics_ref.py): the reference itself against torch autograd and against the condition it puts on its own inputs, every output of
every case, the tangent step across a pass, the exact properties, the refusals (on the emulation and, with host arrays, on the product library,
which checks before it launches), the marshalling, and the tool on three synthetic LSTM clips.  The stand-alone emulation runs the first four
cases under the address and undefined-behaviour sanitizers with buffers of exactly the contract's sizes.  tests/test_gpu_lstm_dynamics.py runs
the same checks through the C-ABI on the device."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import lstm_dynamics_ref as R
from tests.hostemu import lstm_dynamics_emu as T

B = T.B


def test_reference_against_torch_autograd():
    R.check_reference_against_autograd()


def test_reference_inputs_are_well_conditioned():
    R.check_conditioning()


@pytest.mark.parametrize("case", R.CASES, ids=[str(i) for i in range(len(R.CASES))])
def test_case_against_float64(case):
    R.check_case(case, B, "emulation")


def test_tangent_step_across_a_pass_against_float64():
    R.check_step(B, "emulation")


def test_decoupled_layers_follow_the_closed_form():
    R.check_decoupled(B, "emulation")


def test_exact_properties():
    R.check_properties(B, "emulation")


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
    net, x, h, c, seq, q0 = R.problem(R.PROPERTY_CASE)
    for subs in (dict(K=0), dict(warmup=-1), dict(misalign=True), dict(ldx=8), dict(ld_carry=63), dict(sums=None), dict(h_in=None), dict(S=2), dict(q0_per_seq=2)):
        with pytest.raises(ValueError):
            R.run(T.over("tmjx_lstm_lyapunov", **subs), net, x, h, c, seq, q0)
    snet, sx, sh, sc, sv = R.step_problem()
    for subs in (dict(K=33), dict(misalign=True), dict(ldx=6), dict(out=None), dict(n=0)):
        with pytest.raises(ValueError):
            R.step(T.over("tmjx_lstm_tangent_step", **subs), snet, sx[:3], sh[:3], sc[:3], sv[:3])


def test_refusals_on_the_product_library_launch_nothing():
    from track_mjx_amd import hip
    R.check_refusals(hip.lib(), _numpy_alloc(), lambda a: a.ctypes.data, lambda a, fill: bool((a == fill).all()), "product, host arrays")


def test_backend_marshalling():
    """What the backend refuses before the library sees it, and what it hands over: the carry's one row stride, the layers' shapes, the shapes of the
    tangents and of the first basis; `want` selects the optional outputs, the sums always come."""
    net, x, h, c, seq, q0 = R.problem(R.PROPERTY_CASE)
    H, L, d_in, K, lens, _, _ = R.PROPERTY_CASE
    got = R.run(B, net, x, h, c, seq, q0, want=("status",))
    assert set(got) == {"status", "sums"} and got["sums"].shape == (len(lens), K) and got["sums"].dtype == np.float64 and got["status"].dtype == np.int32
    with pytest.raises(ValueError, match="row strides"):
        R.run(B, net, x, R._slice_of(h, L * H + 4), c, seq, q0)
    with pytest.raises(ValueError, match="h_in has shape"):
        R.run(B, net, x, h[:, :-1], c, seq, q0)
    with pytest.raises(ValueError, match="q0 has shape"):
        R.run(B, net, x, h, c, seq, q0[:, :-1])
    with pytest.raises(ValueError, match="q0 has shape"):
        R.run(B, net, x, h, c, seq, np.broadcast_to(q0[None], (2, *q0.shape)))
    with pytest.raises(ValueError, match="v has shape"):
        B.lstm_tangent_step(B.asarray(x), B.asarray(h), B.asarray(c), net.layers, np.zeros((x.shape[0], 2, 5), np.float32))
    five = R.make_net(d_in, H, 5, 1)
    with pytest.raises(ValueError, match="5 LSTM layers"):
        R.run(B, five, x, np.zeros((x.shape[0], 5 * H), np.float32), np.zeros((x.shape[0], 5 * H), np.float32), seq, q0)


def test_tool_on_three_synthetic_lstm_clips(tmp_path, capsys):
    R.check_tool(tmp_path, B, capsys)


def test_emulation_under_sanitizers(tmp_path):
    exe = T.build_main(tmp_path / "lstm_dynamics_emu", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    for H, L, d_in, K, lens, ldx, ldc in R.CASES[:4]:
        res = subprocess.run([str(exe), *[str(v) for v in (d_in, H, L, K, ldx or d_in, ldc or L * H, *lens)]], capture_output=True, text=True)
        assert res.returncode == 0 and "finite: 1" in res.stdout, res.stdout + res.stderr
