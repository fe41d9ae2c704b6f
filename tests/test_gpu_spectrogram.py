"""The spectrogram kernels (csrc/tmjx_spectrogram.hip) through the C-ABI against the float64 reference (tests/spectrogram_ref.py): every case within
the derived bound, strided rows and padded outputs, analysis, sequences of one row, the bit-level properties (repeatability, a sequence alone, first,
last and between sequences of NaN), the refusals, the planted rhythm and the command-line tool.  tests/test_spectrogram_cpu.py runs the same checks on
the host emulation of the same kernel bodies."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import spectrogram_ref as R
from track_mjx_amd import hip
from track_mjx_amd.analysis import pca as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [pytest.param(R.EDGE, True, False, id="edge"), pytest.param(R.EDGE, False, False, id="edge-no-detrend"), pytest.param(R.EDGE, True, True, id="edge-log"),
         pytest.param(R.F1, True, False, id="F1"), pytest.param(R.F64, True, False, id="F64"), pytest.param(R.PRODUCT, True, False, id="product")]


@functools.lru_cache(None)
def backend():
    return P.HipBackend(DEV)


def test_the_bank_builder():
    R.check_bank(backend())


@pytest.mark.parametrize("case,detrend,log", CASES)
def test_against_float64(case, detrend, log):
    R.check(*R.run(backend(), case, detrend, log), R.reference(case, detrend, log), "kernel")


@pytest.mark.parametrize("case", R.CHANNEL_CASES, ids=[f"C{c[1]}" for c in R.CHANNEL_CASES])
def test_channel_counts_with_strided_rows_and_padded_output(case):
    lengths, Cn, freqs = case
    x, n, F = R.signal(case), sum(lengths), len(freqs)
    xbuf = torch.full((n, Cn + 5), 1e6, dtype=torch.float32, device=DEV)
    xbuf[:, 2:2 + Cn] = torch.from_numpy(np.array(x))
    xs = xbuf[:, 2:2 + Cn]
    assert backend().asarray(xs).data_ptr() == xs.data_ptr() and xs.stride(0) == Cn + 5      # no copy
    obuf = torch.full((n, F * Cn + 3), -7.25, dtype=torch.float32, device=DEV)
    out, cov = R.run(backend(), case, x=xs, out=obuf[:, :F * Cn])
    assert (obuf[:, F * Cn:] == -7.25).all()
    R.check(out, cov, R.reference(case), f"kernel, C = {Cn}")
    np.testing.assert_array_equal(R.bits(R.run(backend(), case)[0]), R.bits(out))      # the strides change no bit


def test_analysis():
    b = backend()
    bank = b.wavelet_bank(R.RATE, R.DEFAULT_BANK)
    for j in (6, 18):
        out, cov = b.spectrogram(b.asarray(R.sinusoid(j)), [0, 1000], *bank)
        R.check_analysis(b.to_numpy(out), b.to_numpy(cov), j, "kernel")


def test_sequences_of_one_row():
    R.check_length_one(backend(), "kernel")


def test_bit_level_properties():
    R.check_bits(backend(), "kernel")


def test_refusals_launch_nothing():
    L = hip.lib()
    n, Cn, F, S = 187, 3, 2, 2
    bank, offset, radius = backend().wavelet_bank(R.RATE, [3.0, 12.5])
    x = torch.zeros((n, Cn), dtype=torch.float32, device=DEV)
    bk = torch.from_numpy(bank).to(DEV)
    out, cov = torch.full((n, F * Cn), -5.0, dtype=torch.float32, device=DEV), torch.full((n, F), -5.0, dtype=torch.float32, device=DEV)
    floats = C.c_int64(0)
    assert L.tmjx_spectrogram_workspace(n, Cn, F, S, C.byref(floats)) == 0 and floats.value > 0
    ws = torch.zeros(int(floats.value) + 4, dtype=torch.float32, device=DEV)
    i32 = lambda v: (C.c_int32 * len(v))(*[int(e) for e in v])      # noqa: E731
    seq, off, rad = i32([0, 37, 187]), i32(offset), i32(radius)
    err = lambda: L.tmjx_last_error()      # noqa: E731

    def call(n=n, Cn=Cn, F=F, S=S, ldx=Cn, ldo=F * Cn, x=x.data_ptr(), seq=seq, bank=bk.data_ptr(), off=off, rad=rad, kind=0, floor=1e-3, out=out.data_ptr(),
             cov=cov.data_ptr(), ws=ws.data_ptr()):
        return L.tmjx_spectrogram(x, n, Cn, ldx, seq, S, bank, off, rad, F, 1, kind, floor, out, ldo, cov, ws, None)
    big, off2 = list(radius), list(offset)
    big[0], off2[1] = 4097, off2[1] + 3
    for kw, word in ((dict(n=0), b"n must be >= 1"), (dict(Cn=0, ldx=0), b"C must be >= 1"), (dict(Cn=1025, ldx=1025), b"limit of 1024"), (dict(F=0), b"F must be >= 1"),
                     (dict(F=65), b"limit of 64"), (dict(S=0), b"S must be >= 1"), (dict(S=188), b"every sequence has a row"), (dict(ldx=2), b"ldx = 2"),
                     (dict(ldo=5), b"ldo = 5"), (dict(rad=i32(big)), b"outside 0 .. 4096"), (dict(off=i32(off2)), b"does not follow"),
                     (dict(seq=i32([1, 37, 187])), b"seq_start[0] = 1"), (dict(seq=i32([0, 37, 37])), b"strictly increasing"),
                     (dict(seq=i32([0, 37, 186])), b"seq_start[S] = 186"), (dict(kind=2), b"output_kind = 2"), (dict(kind=1, floor=0.0), b"log_floor"),
                     (dict(ws=ws.data_ptr() + 4), b"16-byte"), (dict(x=None), b"null"), (dict(seq=None), b"null"), (dict(bank=None), b"null"), (dict(off=None), b"null"),
                     (dict(rad=None), b"null"), (dict(out=None), b"null"), (dict(cov=None), b"null"), (dict(ws=None), b"null")):
        assert call(**kw) == -22 and word in err(), (kw, err())
    assert L.tmjx_spectrogram_workspace(n, 1025, F, S, C.byref(floats)) == -22 and L.tmjx_spectrogram_workspace(n, Cn, F, S, None) == -22
    dbl = lambda v: (C.c_double * len(v))(*v)      # noqa: E731
    for rate, fr, nf, om, sup, word in ((50.0, [26.0], 1, 5.0, 4.0, b"rate / 2"), (50.0, [0.0], 1, 5.0, 4.0, b"rate / 2"), (50.0, [0.02], 1, 5.0, 4.0, b"limit of 4096"),
                                        (50.0, [5.0], 1, 0.0, 4.0, b"omega0"), (50.0, [5.0], 1, 5.0, -1.0, b"support"), (0.0, [5.0], 1, 5.0, 4.0, b"rate"),
                                        (50.0, [5.0] * 65, 65, 5.0, 4.0, b"limit of 64"), (50.0, [5.0], 0, 5.0, 4.0, b"F must be >= 1")):
        assert L.tmjx_wavelet_bank_size(rate, dbl(fr), nf, om, sup, C.byref(floats)) == -22 and word in err(), (fr, err())
    assert L.tmjx_wavelet_bank_size(50.0, None, 1, 5.0, 4.0, C.byref(floats)) == -22 and L.tmjx_wavelet_bank(50.0, dbl([5.0]), 1, 5.0, 4.0, None, off, rad) == -22
    torch.cuda.synchronize()
    assert (out == -5).all() and (cov == -5).all() and float(ws.abs().sum().item()) == 0.0


def test_spectrogram_on_device_tensors_stays_on_the_device():
    from track_mjx_amd.analysis.spectrogram import Spectrogram
    x = R.signal(R.F1)
    xbuf = torch.full((240, 7), 1e6, dtype=torch.float32, device=DEV)
    xbuf[:, 3:5] = torch.from_numpy(np.array(x))
    sp = Spectrogram(R.RATE, n_freqs=6, device=DEV)
    a, ca = sp.transform(xbuf[:, 3:5], (40, 200))
    b, cb = sp.transform(np.array(x), (40, 200))
    assert isinstance(a, torch.Tensor) and a.device.type == "cuda" and isinstance(b, np.ndarray) and a.shape == (240, 12) and ca.shape == (240, 6)
    np.testing.assert_array_equal(R.bits(a.cpu().numpy()), R.bits(b))
    np.testing.assert_array_equal(R.bits(ca.cpu().numpy()), R.bits(cb))


def test_the_feature_earns_its_place():
    R.check_planted(backend(), "kernel")


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, backend(), capsys)
