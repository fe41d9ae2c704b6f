"""CPU: the spectrogram kernel bodies (csrc/spectrogram_core.h) compiled into the host emulation (tests/hostemu/spectrogram_emu.cpp),
called through the shared analysis backend (tests/hostemu/analysis_emu.py), against the
float64 reference (tests/spectrogram_ref.py): the reference against analysis first, the float32 numpy restatement alone against the derived bound
(and three wrong variants of it that must break it), the emulation at every case, the bit-level properties, the refusals, the planted rhythm, the
command-line tool, and the emulation as a stand-alone program under AddressSanitizer and UBSan.  tests/test_gpu_spectrogram.py runs the same checks
through the C-ABI."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import spectrogram_ref as R
from tests.hostemu import analysis_emu as E
from track_mjx_amd import hip

B = E.B
CASES = [pytest.param(R.EDGE, True, False, id="edge"), pytest.param(R.EDGE, False, False, id="edge-no-detrend"), pytest.param(R.EDGE, True, True, id="edge-log"),
         pytest.param(R.F1, True, False, id="F1"), pytest.param(R.F64, True, False, id="F64"), pytest.param(R.PRODUCT, True, False, id="product")]


def test_limits_are_exported_and_the_entry_points_declared():
    assert (hip.SPECTROGRAM_MAX_C, hip.SPECTROGRAM_MAX_F, hip.SPECTROGRAM_MAX_R) == (1024, 64, 4096)
    for name in ("tmjx_wavelet_bank_size", "tmjx_wavelet_bank", "tmjx_spectrogram_workspace", "tmjx_spectrogram"):
        assert name in hip.EXPORTS
    assert any(s.name == "tmjx_spectrogram.hip" for s in hip.SOURCES)


def test_the_reference_against_analysis():
    for j in (0, 6, 12, 18):      # 1 .. 11.2 Hz: at most rate / 4
        assert R.DEFAULT_BANK[j] <= R.RATE / 4
        out, cov, _ = R.spectrogram64(R.sinusoid(j), (1000,), R.DEFAULT_BANK)
        R.check_analysis(out, cov, j, "float64 definition", exact=False)


def test_the_bank_builder():
    R.check_bank(B)
    assert int(B.wavelet_bank(50.0, [0.05])[2][0]) == 3184


@pytest.mark.parametrize("case,detrend,log", CASES)
def test_restatement_and_emulation_against_float64(case, detrend, log):
    ref = R.reference(case, detrend, log)
    x = R.signal(case)
    R.check(*R.spectrogram32(x, case[0], case[2], detrend, log), ref, "restatement")
    R.check(*R.run(B, case, detrend, log), ref, "emulation")


def test_the_bound_has_teeth():
    """Each of three wrong restatements breaks the bound on at least one case."""
    for variant in ("shift", "no_renorm", "mean_left_in"):
        worst = 0.0
        for case in (R.EDGE, R.F1):
            out, cov = R.spectrogram32(R.signal(case), case[0], case[2], True, False, variant=variant)
            worst = max(worst, R.worst_ratio(out, cov, R.reference(case))[0])
        print(f"[spectrogram] wrong variant {variant}: worst error / bound {worst:.1f}")
        assert worst > 1.0, variant


@pytest.mark.parametrize("case", R.CHANNEL_CASES, ids=[f"C{c[1]}" for c in R.CHANNEL_CASES])
def test_channel_counts_with_strided_rows_and_padded_output(case):
    lengths, C, freqs = case
    x, n, F = R.signal(case), sum(lengths), len(freqs)
    xbuf = np.full((n, C + 5), 1e6, np.float32)
    xbuf[:, 2:2 + C] = x
    obuf = np.full((n, F * C + 3), -7.25, np.float32)
    out, cov = R.run(B, case, x=xbuf[:, 2:2 + C], out=obuf[:, :F * C])
    assert (obuf[:, F * C:] == -7.25).all() and out.base is obuf
    R.check(out, cov, R.reference(case), f"emulation, C = {C}")
    np.testing.assert_array_equal(R.bits(R.run(B, case)[0]), R.bits(out))      # the strides change no bit


def test_analysis_on_the_emulation():
    bank = B.wavelet_bank(R.RATE, R.DEFAULT_BANK)
    for j in (6, 18):
        out, cov = B.spectrogram(R.sinusoid(j), [0, 1000], *bank)
        R.check_analysis(out, cov, j, "emulation")


def test_sequences_of_one_row():
    R.check_length_one(B, "emulation")


def test_bit_level_properties():
    R.check_bits(B, "emulation")


def test_refusals_leave_out_untouched():
    case = ((37, 150), 3, np.array([3.0, 12.5]))
    x, seq = R.signal(case), R.seq_of(case[0])
    bank, offset, radius = B.wavelet_bank(R.RATE, case[2])
    out = np.full((187, 6), -7.25, np.float32)

    def call(**kw):
        a = dict(seq_start=seq, offset=offset, radius=radius)
        a.update({k: kw.pop(k) for k in list(kw) if k in a and kw[k] is not None})      # (None: a null pointer, substituted below)
        own = {k: kw.pop(k) for k in list(kw) if k in ("log", "floor")}      # (the method's own arguments; the rest substitutes tmjx_spectrogram's)
        return E.over("tmjx_spectrogram", **kw).spectrogram(x, a["seq_start"], bank, a["offset"], a["radius"], out=out, **own)
    big = np.array(radius)
    big[0] = 4097
    off2 = np.array(offset)
    off2[1] += 3
    for kw, word in ((dict(n=0), "n must be >= 1"), (dict(C=0), "C must be >= 1"), (dict(C=1025, ldx=1025), "limit of 1024"), (dict(F=0), "F must be >= 1"),
                     (dict(F=65), "limit of 64"), (dict(S=0), "S must be >= 1"), (dict(ldx=2), "ldx = 2"), (dict(ldo=5), "ldo = 5"),
                     (dict(radius=big), "outside 0 .. 4096"), (dict(offset=off2), "does not follow"), (dict(seq_start=[1, 37, 187]), r"seq_start\[0\] = 1"),
                     (dict(seq_start=[0, 37, 37]), "strictly increasing"), (dict(seq_start=[0, 37, 186]), r"seq_start\[S\] = 186"), (dict(output_kind=2), "output_kind = 2"),
                     (dict(log=True, floor=0.0), "log_floor"), (dict(log=True, floor=float("nan")), "log_floor"), (dict(misalign=True), "16-byte"),
                     *[({name: None}, "null") for name in ("x", "seq_start", "bank", "offset", "radius", "out", "coverage", "workspace")]):
        with pytest.raises(ValueError, match=word):
            call(**kw)
        assert (out == -7.25).all(), kw
    for kw, word in ((dict(freqs=[26.0]), "rate / 2"), (dict(freqs=[0.0]), "rate / 2"), (dict(freqs=[float("nan")]), "rate / 2"), (dict(freqs=[0.02]), "limit of 4096"),
                     (dict(freqs=[5.0], omega0=0.0), "omega0"), (dict(freqs=[5.0], support=-1.0), "support"), (dict(freqs=[5.0], rate=0.0), "rate"),
                     (dict(freqs=[5.0] * 65), "limit of 64"), (dict(freqs=[5.0], over=dict(F=0)), "F must be >= 1"), (dict(freqs=[5.0], over=dict(freqs=None)), "null")):
        kw = dict(kw)
        with pytest.raises(ValueError, match=word):
            E.over("tmjx_wavelet_bank_size", **kw.pop("over", {})).wavelet_bank(kw.pop("rate", 50.0), kw.pop("freqs"), **kw)


def test_workspace_does_not_scale_with_n():
    assert E.workspace("tmjx_spectrogram_workspace", 210000, 67, 25, 840) == E.workspace("tmjx_spectrogram_workspace", 1000, 67, 25, 840) <= 840 * 67 + 2 * 25 * 8194 + 4096


def test_spectrogram_class_argument_checks():
    from track_mjx_amd.analysis import spectrogram as SP
    np.testing.assert_allclose(SP.dyadic_frequencies(1.0, 25.0, 5), R.FIVE, rtol=1e-15)
    sp = SP.Spectrogram(50.0, backend=B)
    assert sp.n_freqs_ == 25 and sp.frequencies_[0] == 1.0 and sp.frequencies_[-1] == 25.0 and int(sp.radius_[0]) == 160 and int(sp.radius_[-1]) == 7
    for kw in (dict(rate=0.0), dict(rate=50.0, f_max=26.0), dict(rate=50.0, frequencies=[0.0, 1.0]), dict(rate=50.0, n_freqs=65), dict(rate=50.0, output="power"),
               dict(rate=50.0, omega0=0.0), dict(rate=50.0, floor=0.0), dict(rate=50.0, f_min=0.001)):
        with pytest.raises(ValueError):
            SP.Spectrogram(backend=B, **kw)
    with pytest.raises(ValueError, match="lengths"):
        sp.transform(np.zeros((10, 2), np.float32), [4, 5])
    with pytest.raises(KeyError, match="unknown source"):
        SP.transform_rollouts([{"ctrl": np.zeros((9, 2), np.float32)}], "speed", backend=B)
    spec, feats, cov = SP.transform_rollouts([{"ctrl": np.ones((9, 2), np.float32)}, {"ctrl": np.ones((4, 2), np.float32)}], "ctrl", cols="1:", n_freqs=3, backend=B)
    assert [f.shape for f in feats] == [(9, 3), (4, 3)] and [c.shape for c in cov] == [(9, 3), (4, 3)] and spec.clips_ == [0, 1] and (feats[0] == 0).all()


def test_the_feature_earns_its_place():
    R.check_planted(B, "emulation")


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, B, capsys)


def test_emulation_runs_clean_under_sanitizers(tmp_path):
    exe = E.build_main("spectrogram", tmp_path / "spectrogram_emu_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for args in ((), ("1", "1", "1", "0", "1"), ("67", "3", "0", "1", "249", "5"), ("130", "2", "1", "0", "1", "64", "65"), ("4", "64", "1", "0", "300")):
        res = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert res.returncode == 0 and "checksum" in res.stdout and not res.stderr, res.stdout + res.stderr
