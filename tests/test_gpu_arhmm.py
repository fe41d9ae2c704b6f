"""The autoregressive-HMM kernels (csrc/tmjx_arhmm.hip) through the C-ABI against the float64 reference (tests/arhmm_ref.py): emission, moments and
solve at the five cases, the exact grids, the Gaussian chain, sequence boundaries, the bit-level properties (repeatability, row strides, the fit
as its steps), the refusals, `ARHMM` on the planted rotations (the motifs nothing else in the repository can find) and the command-line tool.
tests/test_arhmm_cpu.py runs the same checks on the host emulation of the same kernel bodies."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import arhmm_ref as R
from track_mjx_amd import hip
from track_mjx_amd.analysis import pca as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(None)
def backend():
    return P.HipBackend(DEV)


@pytest.mark.parametrize("case", R.CASES)
def test_emission_against_float64(case):
    R.check_emission(case, backend(), "kernel")


@pytest.mark.parametrize("case", R.CASES)
def test_moments_and_solve_against_float64(case):
    M, w = R.check_moments(case, backend(), "kernel")
    R.check_solve(case, backend(), M, w, "kernel")


def test_exact_grids():
    R.check_emission_exact(backend())
    R.check_moments_exact(backend())


def test_unscored_rows_and_other_sequences_add_nothing_to_the_moments():
    R.check_moments_ignore_unscored_rows(backend())


def test_light_and_singular_states_keep_their_bits():
    R.check_light_and_singular(backend(), "kernel")


def test_lags_zero_is_the_gaussian_emission_chain():
    R.check_gaussian_chain(backend())


def test_no_lag_crosses_a_boundary():
    R.check_boundaries(backend())
    R.check_short_sequences_are_unscored(backend())


def test_fit_is_its_steps_and_the_loglik_never_falls():
    R.check_fit_steps(backend(), "kernel")


def test_two_calls_and_strided_rows_give_the_same_bits():
    def strided(a):
        buf = torch.full((a.shape[0], a.shape[1] + 5), 1e6, dtype=torch.float32, device=DEV)
        buf[:, 3:3 + a.shape[1]] = torch.from_numpy(np.array(a))
        xs = buf[:, 3:3 + a.shape[1]]
        assert backend().asarray(xs).data_ptr() == xs.data_ptr() and xs.stride(0) == a.shape[1] + 5      # no copy
        return xs
    R.check_repeat_and_strides(backend(), strided, "kernel")


def test_refusals_launch_nothing():
    def alloc(shape, dtype, fill):
        return torch.full(tuple(shape), fill, dtype=getattr(torch, np.dtype(dtype).name), device=DEV)

    def untouched(t, fill):
        torch.cuda.synchronize()
        return bool((t == fill).all())
    R.check_refusals(hip.lib(), alloc, lambda t: t.data_ptr(), untouched, "kernel")


def test_model_level_on_the_planted_rotations():
    R.check_model(backend(), "kernel")


def test_arhmm_on_device_tensors():
    from track_mjx_amd.analysis import arhmm as AR
    x, lengths, _ = R.rotations()
    buf = torch.full((900, 7), 1e6, dtype=torch.float32, device=DEV)
    buf[:, 2:4] = torch.from_numpy(np.array(x[:900]))
    a = AR.ARHMM(3, lags=2, warmup=3, max_iter=5, n_init=1, device=DEV).fit(buf[:, 2:4], (300, 300, 300))
    c = AR.ARHMM(3, lags=2, warmup=3, max_iter=5, n_init=1, device=DEV).fit(np.array(x[:900]), (300, 300, 300))
    for name in ("weights_", "vars_", "means_", "transmat_", "startprob_", "labels_", "status_"):
        np.testing.assert_array_equal(R.bits(getattr(a, name)), R.bits(getattr(c, name)))
    assert a.loglik_ == c.loglik_ and a.weights_.shape == (3, 2, 5) and (np.diff(a.counts_) <= 0).all() and a.n_scored_ == 891


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, backend(), capsys)
