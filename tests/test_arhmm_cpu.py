"""CPU: the autoregressive-HMM kernel bodies (csrc/arhmm_core.h) compiled into the host emulation (tests/hostemu/arhmm_emu.cpp), called through the
shared analysis backend (tests/hostemu/arhmm_emu.py), against the float64 reference (tests/arhmm_ref.py): emission, moments and solve at the five
cases (every limit with 300 rows here), the exact grids, the Gaussian chain, sequence boundaries, the fit as its steps, repeatability and
strides, the refusals, `ARHMM` on the planted rotations, the command-line tool, and the emulation as a stand-alone program under AddressSanitizer
and UBSan.  tests/test_gpu_arhmm.py runs the same checks through the C-ABI."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import arhmm_ref as R
from tests.hostemu import arhmm_emu as E
from track_mjx_amd import hip

B = E.B
CASES = R.CASES[:4] + (R.CPU_LIMIT,)


def test_limits_are_exported_and_the_entry_points_declared():
    assert (hip.ARHMM_MAX_D, hip.ARHMM_MAX_LAGS) == (32, 4)
    for name in ("workspace", "emission", "moments", "solve", "fit"):
        assert f"tmjx_arhmm_{name}" in hip.EXPORTS
    assert any(s.name == "tmjx_arhmm.hip" for s in hip.SOURCES)
    assert [f[0] for f in hip.ArhmmInfo._fields_] == ["n_iter", "converged", "loglik", "emission_ms", "fb_ms", "mstep_ms", "viterbi_ms", "n_singular", "pad_"]


def test_cases_are_cut_into_the_sequences_the_kernels_can_get_wrong():
    for n, d, L, k in R.CASES[1:] + (R.CPU_LIMIT,):
        lengths = R.lengths_of(n, L)
        assert sum(lengths) == n and 1 in lengths and L + 1 in lengths and (L == 0 or L in lengths) and max(lengths) > 128
    assert R.lengths_of(1, 0) == (1,)


@pytest.mark.parametrize("case", CASES)
def test_emission_against_float64(case):
    R.check_emission(case, B, "emulation")


@pytest.mark.parametrize("case", CASES)
def test_moments_and_solve_against_float64(case):
    M, w = R.check_moments(case, B, "emulation")
    R.check_solve(case, B, M, w, "emulation")


def test_exact_grids():
    R.check_emission_exact(B)
    R.check_moments_exact(B)


def test_unscored_rows_and_other_sequences_add_nothing_to_the_moments():
    R.check_moments_ignore_unscored_rows(B)


def test_light_and_singular_states_keep_their_bits():
    R.check_light_and_singular(B, "emulation")


def test_lags_zero_is_the_gaussian_emission_chain():
    R.check_gaussian_chain(B)


def test_no_lag_crosses_a_boundary():
    R.check_boundaries(B)
    R.check_short_sequences_are_unscored(B)


def test_fit_is_its_steps_and_the_loglik_never_falls():
    R.check_fit_steps(B, "emulation")


def test_strided_rows_and_two_calls_give_the_same_bits():
    def strided(x):
        buf = np.full((x.shape[0], x.shape[1] + 5), 1e6, np.float32)
        buf[:, 3:-2] = x
        xs = buf[:, 3:-2]
        assert B.asarray(xs) is xs
        return xs
    R.check_repeat_and_strides(B, strided, "emulation")


def test_refusals():
    import ctypes as C
    lib = E.ARRAYS.library
    keep = []

    def alloc(shape, dtype, fill):
        raw = np.empty(int(np.prod(shape)) * np.dtype(dtype).itemsize + 16, np.uint8)
        a = raw[(-raw.ctypes.data) % 16:][:int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
        a[...] = fill
        keep.append(raw)
        return a
    R.check_refusals(lib, alloc, lambda a: a.ctypes.data, lambda a, fill: bool((a == fill).all()), "emulation")
    x, seq, center, W, var, g = R.case_data(R.CASES[1])
    with pytest.raises(ValueError, match="warmup = 0 is smaller than lags = 1"):      # and through the backend's marshalling
        B.arhmm_emission(x, seq, 1, 0, center, W, var)
    with pytest.raises(ValueError, match="16-byte"):
        E.over("tmjx_arhmm_moments", misalign=True).arhmm_moments(x, seq, 1, 1, center, g)
    assert C.sizeof(hip.ArhmmInfo) == 40


def test_workspace_reports_the_reused_hmm_steps_and_a_row_split_of_n_k_q():
    from tests.hostemu import analysis_emu as A
    small = E.workspace(210000, 10, 3, 16, 840)
    assert small >= A.workspace("tmjx_hmm_workspace", 210000, 1, 16, 840)
    assert E.workspace(210000, 10, 3, 16, 1) <= small <= E.workspace(210000, 10, 3, 16, 1) + 844      # S sizes its own offsets only
    big = E.workspace(210000, 32, 4, 128, 840)
    parts = 8 * 128 * 161 * 161 * 2      # eight row parts of [k][q][q] float64 at the limits, whatever n is
    assert parts <= big - A.workspace("tmjx_hmm_workspace", 210000, 1, 128, 840) <= parts + 2 * 128 * (161 * 161 + 129 * 129 + 32 * 129 + 200) + 2 * 210000 + 4096
    assert E.workspace(420000, 32, 4, 128, 840) - A.workspace("tmjx_hmm_workspace", 420000, 1, 128, 840) - 210000 == big - A.workspace("tmjx_hmm_workspace", 210000, 1, 128, 840)


def test_model_level_on_the_planted_rotations():
    R.check_model(B, "emulation")


def test_arhmm_argument_checks():
    from track_mjx_amd.analysis import arhmm as AR
    x, lengths, _ = R.rotations()
    for kw in (dict(n_states=0), dict(n_states=129), dict(n_states=3, lags=5), dict(n_states=3, lags=-1), dict(n_states=3, lags=2, warmup=1), dict(n_states=3, ridge=-1),
               dict(n_states=3, tol=-1)):
        with pytest.raises(ValueError):
            AR.ARHMM(backend=B, **kw)
    with pytest.raises(ValueError, match="lengths"):
        AR.ARHMM(3, backend=B).fit(x, [10, 20])
    with pytest.raises(ValueError, match="not fitted"):
        AR.ARHMM(3, backend=B).predict(x, lengths)
    with pytest.raises(ValueError, match="analysis.pca"):
        AR.ARHMM(3, backend=B).fit(np.zeros((50, 33), np.float32), [50])
    assert AR.companion_eigenvalues(np.zeros((2, 3, 1), np.float32), 3, 0).shape == (2, 0)
    rot = np.array([[[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0]]])
    ev = AR.companion_eigenvalues(rot, 2, 1)
    assert np.allclose(np.abs(ev), 1.0) and np.allclose(np.abs(np.angle(ev)), 0.3)


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, B, capsys)


def test_emulation_runs_clean_under_sanitizers(tmp_path):
    exe = E.build_main(tmp_path / "arhmm_emu_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for args in ((), ("1", "0", "1", "1"), ("32", "4", "3", "1", "4", "5", "300"), ("10", "3", "7", "37", "300", "5")):
        res = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert res.returncode == 0 and "checksum" in res.stdout and not res.stderr, res.stdout + res.stderr
