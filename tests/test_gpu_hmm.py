"""The hidden-Markov-model kernels (csrc/tmjx_hmm.hip) through the C-ABI against the float64 reference (tests/hmm_ref.py): emission,
forward-backward, M-step and Viterbi at the five cases of each kind, the exact grids, the bit-level properties (repeatability, row strides, the fit
as its steps), sequence boundaries, the zero-probability sequence, the refusals, `GaussianHMM` on the planted chain and the command-line tool.
tests/test_hmm_cpu.py runs the same checks on the host emulation of the same kernel bodies."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import hmm_ref as R
from track_mjx_amd import hip
from track_mjx_amd.analysis import pca as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(None)
def backend():
    return P.HipBackend(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


@pytest.mark.parametrize("case", R.EMISSION_CASES)
def test_emission_against_float64(case):
    x, mu, var = R.emission_data(case)
    R.check_emission(x, mu, var, backend().hmm_emission(backend().asarray(x), mu, var), "kernel")


@pytest.mark.parametrize("case", R.SEQ_CASES)
def test_forward_backward_against_float64(case):
    _, _, _, A, pi, seq, logb = R.seq_data(case)
    R.check_fb(logb, seq, A, pi, backend().hmm_forward_backward(logb, seq, A, pi), "kernel")


@pytest.mark.parametrize("case", R.EMISSION_CASES)
@pytest.mark.parametrize("kind", ["onehot", "soft"])
def test_mstep_against_float64(case, kind):
    x, mu, var = R.emission_data(case)
    gamma = R.onehot_gamma(case) if kind == "onehot" else R.soft_gamma(case)
    R.check_mstep(x, gamma, mu, var, backend().hmm_mstep(backend().asarray(x), gamma, mu, var, 1e-6, 1e-3), 1e-6, 1e-3, f"kernel, {kind}")


def test_mstep_floor_and_light_states():
    x, mu, var = R.emission_data(R.EMISSION_CASES[2])
    gamma = np.array(R.soft_gamma(R.EMISSION_CASES[2]))
    gamma[:, 3] = 0
    gamma[1:, 5] = 0
    out = backend().hmm_mstep(backend().asarray(x), gamma, mu, var, 2.0, 1.5)
    assert out[2][3] == 0 and out[2][5] < 1.5 and (out[1] == np.float32(2.0)).any()
    R.check_mstep(x, gamma, mu, var, out, 2.0, 1.5, "kernel, a floor that binds and two light states")


def test_transitions():
    r = np.random.default_rng(4)
    xi, start = r.uniform(0, 5, (7, 7)), r.uniform(0, 2, 7)
    xi[3] = 0
    A0, p0 = R.sticky_chain(r, 7)
    A, pi = backend().hmm_transitions(xi, start, 0.0, 0.0, A0, p0)
    rA, rpi = R.transitions64(xi, start, 0.0, 0.0, A0, p0)
    np.testing.assert_array_equal(bits(A[3]), bits(A0[3]))      # a row without mass keeps its bits
    np.testing.assert_array_equal(A, R.f32(rA))
    np.testing.assert_array_equal(pi, R.f32(rpi))
    A, pi = backend().hmm_transitions(xi, start, 0.1, 4.0, A0, p0)
    np.testing.assert_array_equal(A, R.f32(R.transitions64(xi, start, 0.1, 4.0, A0, p0)[0]))


@pytest.mark.parametrize("case", R.SEQ_CASES)
def test_viterbi_against_float64(case):
    _, _, _, A, pi, seq, logb = R.seq_data(case)
    R.check_viterbi(logb, seq, A, pi, *backend().hmm_viterbi(logb, seq, A, pi), "kernel")


def test_viterbi_never_takes_a_zero_entry_while_a_finite_path_exists():
    _, _, _, A, pi, seq, logb = R.seq_data(R.SEQ_CASES[2])
    A, pi = np.array(A), np.array(pi)
    A[:, 0], A[0, 0], pi[0] = 0, 1, 0      # state 0 can only be entered at the start, and nothing starts there
    labels, path = backend().hmm_viterbi(logb, seq, A, pi)
    assert (labels != 0).all() and np.isfinite(path).all()
    R.check_viterbi(logb, seq, A, pi, labels, path, "kernel, a forbidden state")


def test_exact_grids():
    R.check_viterbi_exact(backend())
    R.check_emission_exact(backend())


def strided(a, pad_left, pad_right):
    buf = torch.full((a.shape[0], a.shape[1] + pad_left + pad_right), 1e6, dtype=torch.float32, device=DEV)
    buf[:, pad_left:pad_left + a.shape[1]] = torch.from_numpy(np.array(a))
    return buf[:, pad_left:pad_left + a.shape[1]]


def test_two_calls_and_strided_rows_give_the_same_bits():
    b = backend()
    case = R.EMISSION_CASES[3]
    x, mu, var = R.emission_data(case)
    xa, xs = b.asarray(x), strided(x, 3, 2)
    assert b.asarray(xs).data_ptr() == xs.data_ptr() and xs.stride(0) == case[1] + 5      # no copy
    gamma = R.soft_gamma(case)
    _, _, _, A, pi, seq, logb = R.seq_data(R.SEQ_CASES[3])
    xq, muq, varq = R.seq_data(R.SEQ_CASES[3])[:3]
    fit_args = (seq, muq, varq, A, pi, 4, 0.0, 0.1, 0.5, 1e-3, 1e-3)
    want = ((b.hmm_emission(xa, mu, var),), b.hmm_mstep(xa, gamma, mu, var, 1e-6, 1e-3), b.hmm_forward_backward(logb, seq, A, pi)[:4],
            b.hmm_viterbi(logb, seq, A, pi), b.hmm_fit(b.asarray(xq), *fit_args)[:6])
    for rows, rq in ((xa, b.asarray(xq)), (xs, strided(xq, 1, 4))):
        got = ((b.hmm_emission(rows, mu, var),), b.hmm_mstep(rows, gamma, mu, var, 1e-6, 1e-3), b.hmm_forward_backward(logb, seq, A, pi)[:4],
               b.hmm_viterbi(logb, seq, A, pi), b.hmm_fit(rq, *fit_args)[:6])
        for g, w in zip(got, want):
            for u_, v_ in zip(g, w):
                np.testing.assert_array_equal(bits(np.asarray(u_)), bits(np.asarray(v_)))


def test_no_transition_crosses_a_boundary():
    R.check_split(backend(), "kernel")


def test_zero_probability_sequence():
    R.check_zero_probability(backend())


def test_fit_is_its_steps_and_the_loglik_never_falls():
    R.check_fit_steps(backend(), "kernel")


def test_refusals_launch_nothing():
    L = hip.lib()
    n, d, k, S = 300, 8, 4, 3
    f32 = lambda shape, v: torch.full(shape, v, dtype=torch.float32, device=DEV)      # noqa: E731
    f64 = lambda shape, v: torch.full(shape, v, dtype=torch.float64, device=DEV)      # noqa: E731
    x, mu, var, A, pi = f32((n, d), 0.0), f32((k, d), -5.0), f32((k, d), -5.0), f32((k, k), -5.0), f32((k,), -5.0)
    logb, gamma, lab = f32((n, k), -5.0), f32((n, k), -5.0), torch.full((n,), -5, dtype=torch.int32, device=DEV)
    xi, start, ll, total, weight, path = f64((k, k), -5.0), f64((k,), -5.0), f64((S,), -5.0), f64((1,), -5.0), f64((k,), -5.0), f64((S,), -5.0)
    floats = C.c_int64(0)
    assert L.tmjx_hmm_workspace(n, d, k, S, C.byref(floats)) == 0 and floats.value > 4 * n * k
    ws = torch.zeros(int(floats.value) + 4, dtype=torch.float32, device=DEV)
    seq = (C.c_int32 * 4)(0, 100, 200, 300)
    X, W = x.data_ptr(), ws.data_ptr()
    err = lambda: L.tmjx_last_error()      # noqa: E731

    def emission(n=n, d=d, ldx=d, k=k, x=X, means=mu.data_ptr(), vars=var.data_ptr(), out=logb.data_ptr(), ws=W):
        return L.tmjx_hmm_emission(x, n, d, ldx, means, vars, k, out, ws, None)
    for kw, word in ((dict(n=0), b"n must be >= 1"), (dict(d=0, ldx=0), b"d must be >= 1"), (dict(d=1025, ldx=1025), b"limit of 1024"), (dict(k=0), b"k must be >= 1"),
                     (dict(k=129), b"limit of 128"), (dict(ldx=7), b"ldx = 7"), (dict(x=None), b"null"), (dict(means=None), b"null"), (dict(out=None), b"null"),
                     (dict(ws=None), b"null"), (dict(ws=W + 4), b"16-byte")):
        assert emission(**kw) == -22 and word in err(), (kw, err())

    def fb(seq=seq, S=S, logb=logb.data_ptr(), gamma=gamma.data_ptr(), xi=xi.data_ptr(), total=total.data_ptr(), ws=W):
        return L.tmjx_hmm_forward_backward(logb, n, k, seq, S, A.data_ptr(), pi.data_ptr(), gamma, xi, start.data_ptr(), ll.data_ptr(), total, ws, None)
    for kw, word in ((dict(S=0), b"S must be >= 1"), (dict(seq=(C.c_int32 * 4)(1, 100, 200, 300)), b"seq_start[0] = 1"),
                     (dict(seq=(C.c_int32 * 4)(0, 200, 200, 300)), b"strictly increasing"), (dict(seq=(C.c_int32 * 4)(0, 100, 200, 299)), b"seq_start[S] = 299"),
                     (dict(seq=None), b"null"), (dict(gamma=None), b"null"), (dict(xi=None), b"null"), (dict(total=None), b"null"), (dict(ws=W + 4), b"16-byte")):
        assert fb(**kw) == -22 and word in err(), (kw, err())
    assert L.tmjx_hmm_viterbi(logb.data_ptr(), n, k, (C.c_int32 * 4)(0, 100, 100, 300), S, A.data_ptr(), pi.data_ptr(), 0, lab.data_ptr(), path.data_ptr(), W,
                              None) == -22 and b"strictly increasing" in err()
    assert L.tmjx_hmm_viterbi(logb.data_ptr(), n, k, seq, S, A.data_ptr(), pi.data_ptr(), 0, None, path.data_ptr(), W, None) == -22 and b"null" in err()
    for mv, mw, word in ((-1.0, 0.0, b"min_var"), (float("nan"), 0.0, b"min_var"), (0.0, -1.0, b"min_weight")):
        assert L.tmjx_hmm_mstep(X, n, d, d, gamma.data_ptr(), k, mv, mw, mu.data_ptr(), var.data_ptr(), weight.data_ptr(), W, None) == -22 and word in err()
    assert L.tmjx_hmm_mstep(X, n, d, d, gamma.data_ptr(), k, 0.0, 0.0, mu.data_ptr(), var.data_ptr(), None, W, None) == -22 and b"null" in err()
    for prior, kappa, word in ((-0.1, 0.0, b"prior"), (0.0, float("nan"), b"kappa")):
        assert L.tmjx_hmm_transitions(xi.data_ptr(), start.data_ptr(), k, prior, kappa, A.data_ptr(), pi.data_ptr(), None) == -22 and word in err()
    info = hip.HmmInfo()

    def fit(max_iter=5, tol=1e-4, prior=0.1, kappa=0.0, min_var=1e-3, min_weight=1e-3, info=C.byref(info), labels=lab.data_ptr(), seq=seq):
        return L.tmjx_hmm_fit(X, n, d, d, seq, S, k, mu.data_ptr(), var.data_ptr(), A.data_ptr(), pi.data_ptr(), gamma.data_ptr(), labels, max_iter, tol, prior, kappa,
                              min_var, min_weight, info, W, None)
    for kw, word in ((dict(max_iter=0), b"max_iter"), (dict(tol=-1.0), b"tol"), (dict(tol=float("nan")), b"tol"), (dict(prior=-1.0), b"prior"),
                     (dict(kappa=-1.0), b"kappa"), (dict(min_var=float("nan")), b"min_var"), (dict(min_weight=-1.0), b"min_weight"), (dict(info=None), b"null"),
                     (dict(labels=None), b"null"), (dict(seq=(C.c_int32 * 4)(0, 100, 300, 300)), b"strictly increasing")):
        assert fit(**kw) == -22 and word in err(), (kw, err())
    assert L.tmjx_hmm_workspace(n, d, 129, S, C.byref(floats)) == -22 and L.tmjx_hmm_workspace(n, d, k, S, None) == -22
    assert L.tmjx_hmm_workspace(n, d, k, n + 1, C.byref(floats)) == -22
    torch.cuda.synchronize()
    for t in (mu, var, A, pi, logb, gamma, xi, start, ll, total, weight, path):
        assert (t == -5).all()
    assert (lab == -5).all() and float(ws.abs().sum().item()) == 0.0


def test_model_level_on_the_planted_chain():
    R.check_model(backend(), "kernel")


def test_gaussian_hmm_on_device_tensors():
    from track_mjx_amd.analysis import hmm as H
    x, lengths, _ = R.planted()
    xs = strided(x[:900], 2, 3)
    a = H.GaussianHMM(4, max_iter=5, n_init=1, device=DEV).fit(xs, (300, 300, 300))
    c = H.GaussianHMM(4, max_iter=5, n_init=1, device=DEV).fit(np.array(x[:900]), (300, 300, 300))
    for name in ("means_", "vars_", "transmat_", "startprob_", "labels_"):
        np.testing.assert_array_equal(bits(getattr(a, name)), bits(getattr(c, name)))
    assert a.loglik_ == c.loglik_ and a.means_.shape == (4, 2) and (np.diff(a.counts_) <= 0).all()


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, backend(), capsys)
