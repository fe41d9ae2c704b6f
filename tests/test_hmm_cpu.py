"""CPU: the hidden-Markov-model kernel bodies (csrc/hmm_core.h) compiled into the host emulation (tests/hostemu/hmm_emu.cpp),
called through the shared analysis backend (tests/hostemu/analysis_emu.py), against the float64
reference (tests/hmm_ref.py): emission, forward-backward, M-step and Viterbi at the five cases of each kind, the float32 numpy restatement alone
against the same bounds, the exact grids, the properties (sequence boundaries, the zero-probability sequence, the fit as its steps), the refusals,
`GaussianHMM` on the planted chain, the command-line tool, and the emulation as a stand-alone program under AddressSanitizer and UBSan.
tests/test_gpu_hmm.py runs the same checks through the C-ABI."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import hmm_ref as R
from tests.hostemu import analysis_emu as E
from track_mjx_amd import hip

B = E.B
f32, f64 = R.f32, R.f64
BIG = R.EMISSION_CASES[4]


def test_limits_are_exported_and_the_entry_points_declared():
    assert (hip.HMM_MAX_D, hip.HMM_MAX_K) == (1024, 128)
    for name in ("workspace", "emission", "forward_backward", "mstep", "transitions", "viterbi", "fit"):
        assert f"tmjx_hmm_{name}" in hip.EXPORTS
    assert any(s.name == "tmjx_hmm.hip" for s in hip.SOURCES)
    assert [f[0] for f in hip.HmmInfo._fields_] == ["n_iter", "converged", "loglik", "emission_ms", "fb_ms", "mstep_ms", "viterbi_ms"]


def test_sequence_inputs_meet_the_conditions_of_the_bounds():
    for case in R.SEQ_CASES:
        _, _, var, A, pi, seq, logb = R.seq_data(case)
        assert A.min() >= 2.0 ** -10 and pi.min() >= 2.0 ** -10 and 0.25 <= var.min() and var.max() <= 4.0
        assert np.abs(f64(A).sum(1) - 1).max() < 2.0 ** -20 and list(np.diff(seq)) == list(case[0])


@pytest.mark.parametrize("case", R.EMISSION_CASES)
def test_emission_against_float64(case):
    x, mu, var = R.emission_data(case)
    R.check_emission(x, mu, var, R.emission32(x, mu, var), "restatement")
    R.check_emission(x, mu, var, B.hmm_emission(x, mu, var), "emulation")


@pytest.mark.parametrize("case", R.SEQ_CASES)
def test_forward_backward_against_float64(case):
    _, _, _, A, pi, seq, logb = R.seq_data(case)
    g, xi, st, ll = R.fb64(logb, seq, A, pi, np.float32)
    R.check_fb(logb, seq, A, pi, (g, xi, st, ll, float(np.add.accumulate(ll)[-1])), "restatement")
    R.check_fb(logb, seq, A, pi, B.hmm_forward_backward(logb, seq, A, pi), "emulation")


@pytest.mark.parametrize("case", R.EMISSION_CASES)
@pytest.mark.parametrize("kind", ["onehot", "soft"])
def test_mstep_against_float64(case, kind):
    x, mu, var = R.emission_data(case)
    gamma = R.onehot_gamma(case) if kind == "onehot" else R.soft_gamma(case)
    if case != BIG:      # (the restatement holds [n, d] float64 temporaries per state: at both limits the emulation alone)
        R.check_mstep(x, gamma, mu, var, R.mstep32(x, gamma, mu, var, 1e-6, 1e-3), 1e-6, 1e-3, f"restatement, {kind}")
    R.check_mstep(x, gamma, mu, var, B.hmm_mstep(x, gamma, mu, var, 1e-6, 1e-3), 1e-6, 1e-3, f"emulation, {kind}")


def test_mstep_restatement_at_both_limits():
    x, mu, var = R.emission_data(BIG)
    gamma = R.soft_gamma(BIG)
    R.check_mstep(x, gamma, mu, var, R.mstep32(x, gamma, mu, var, 1e-6, 1e-3), 1e-6, 1e-3, "restatement, soft")


def test_mstep_floor_and_light_states():
    x, mu, var = R.emission_data(R.EMISSION_CASES[2])
    gamma = np.array(R.soft_gamma(R.EMISSION_CASES[2]))
    gamma[:, 3] = 0
    gamma[1:, 5] = 0
    out = B.hmm_mstep(x, gamma, mu, var, 2.0, 1.5)
    assert out[2][3] == 0 and out[2][5] < 1.5 and (out[1][[0, 1, 2, 4, 6]] >= f32(2.0)).all() and (out[1] == f32(2.0)).any()
    R.check_mstep(x, gamma, mu, var, out, 2.0, 1.5, "emulation, a floor that binds and two light states")


def test_transitions():
    r = np.random.default_rng(4)
    xi, start = r.uniform(0, 5, (7, 7)), r.uniform(0, 2, 7)
    xi[3] = 0
    A0, p0 = R.sticky_chain(r, 7)
    A, pi = B.hmm_transitions(xi, start, 0.0, 0.0, A0, p0)
    rA, rpi = R.transitions64(xi, start, 0.0, 0.0, A0, p0)
    np.testing.assert_array_equal(A[3].view(np.uint32), A0[3].view(np.uint32))      # a row without mass keeps its bits
    np.testing.assert_array_equal(A, f32(rA))
    np.testing.assert_array_equal(pi, f32(rpi))
    A, pi = B.hmm_transitions(xi, start, 0.1, 4.0, A0, p0)
    rA, rpi = R.transitions64(xi, start, 0.1, 4.0, A0, p0)
    np.testing.assert_array_equal(A, f32(rA))
    assert A[3, 3] == f32(4.1 / 4.7) and (np.diag(A) > np.diag(f32(R.transitions64(xi, start, 0.1, 0.0, A0, p0)[0]))).all()
    same = B.hmm_transitions(np.zeros((7, 7)), np.zeros(7), 0.0, 0.0, A0, p0)
    np.testing.assert_array_equal(same[0], A0)
    np.testing.assert_array_equal(same[1], p0)


@pytest.mark.parametrize("case", R.SEQ_CASES)
def test_viterbi_against_float64(case):
    _, _, _, A, pi, seq, logb = R.seq_data(case)
    with np.errstate(divide="ignore"):
        lab, score, _, _ = R.viterbi64(logb, seq, np.log(A), np.log(pi), np.float32)
    R.check_viterbi(logb, seq, A, pi, lab, score, "restatement")
    R.check_viterbi(logb, seq, A, pi, *B.hmm_viterbi(logb, seq, A, pi), "emulation")


def test_viterbi_never_takes_a_zero_entry_while_a_finite_path_exists():
    _, _, _, A, pi, seq, logb = R.seq_data(R.SEQ_CASES[2])
    A = np.array(A)
    A[:, 0] = 0
    A[0, 0] = 1      # state 0 can only be entered at the start
    pi = np.array(pi)
    pi[0] = 0
    labels, path = B.hmm_viterbi(logb, seq, A, pi)
    assert (labels != 0).all() and np.isfinite(path).all()
    R.check_viterbi(logb, seq, A, pi, labels, path, "emulation, a forbidden state")


def test_exact_grids():
    R.check_viterbi_exact(B)
    R.check_emission_exact(B)


def test_strided_rows_and_two_calls_give_the_same_bits():
    x, mu, var = R.emission_data(R.EMISSION_CASES[3])
    buf = np.full((x.shape[0], x.shape[1] + 5), 1e6, np.float32)
    buf[:, 3:-2] = x
    xs = buf[:, 3:-2]
    assert B.asarray(xs) is xs
    gamma = R.soft_gamma(R.EMISSION_CASES[3])
    want = (B.hmm_emission(x, mu, var), *B.hmm_mstep(x, gamma, mu, var, 1e-6, 1e-3))
    for rows in (x, xs):
        got = (B.hmm_emission(rows, mu, var), *B.hmm_mstep(rows, gamma, mu, var, 1e-6, 1e-3))
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_no_transition_crosses_a_boundary():
    R.check_split(B, "emulation")


def test_zero_probability_sequence():
    R.check_zero_probability(B)


def test_fit_is_its_steps_and_the_loglik_never_falls():
    R.check_fit_steps(B, "emulation")


def test_fit_without_gamma():
    x, mu, var, A, pi, seq, _ = R.seq_data(R.SEQ_CASES[2])
    a, b = B.hmm_fit(x, seq, mu, var, A, pi, 3, 0.0, 0.1, 1.0, 1e-3, 1e-3), E.over("tmjx_hmm_fit", gamma=None).hmm_fit(x, seq, mu, var, A, pi, 3, 0.0, 0.1, 1.0, 1e-3, 1e-3)
    for u, v in zip(a[:4] + a[5:6], b[:4] + b[5:6]):
        np.testing.assert_array_equal(u, v)
    assert a[6].n_iter == 3 and not a[6].converged and a[6].loglik == b[6].loglik


def test_refusals():
    x, mu, var, A, pi, seq, logb = R.seq_data(R.SEQ_CASES[2])
    for kw, word in ((dict(n=0), "n must be >= 1"), (dict(d=1025, ldx=1025), "limit of 1024"), (dict(k=129), "limit of 128"), (dict(k=0), "k must be >= 1"),
                     (dict(ldx=2), "ldx = 2"), (dict(misalign=True), "16-byte")):
        with pytest.raises(ValueError, match=word):
            E.over("tmjx_hmm_emission", **kw).hmm_emission(x, mu, var)
    for bad, word in (([1, 37, 342], r"seq_start\[0\] = 1"), ([0, 37, 37, 342], "strictly increasing"), ([0, 37, 300], r"seq_start\[S\] = 300")):
        with pytest.raises(ValueError, match=word):
            B.hmm_forward_backward(logb, bad, A, pi)
        with pytest.raises(ValueError, match=word):
            B.hmm_viterbi(logb, bad, A, pi)
    with pytest.raises(ValueError, match="S must be >= 1"):
        B.hmm_forward_backward(logb, [0], A, pi)
    for kw, word in ((dict(max_iter=0), "max_iter"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"), (dict(prior=-0.5), "prior"),
                     (dict(kappa=float("nan")), "kappa"), (dict(min_var=-1e-3), "min_var"), (dict(min_weight=-1.0), "min_weight")):
        with pytest.raises(ValueError, match=word):
            B.hmm_fit(x, seq, mu, var, A, pi, **kw)
    with pytest.raises(ValueError, match="prior"):
        B.hmm_transitions(np.zeros((7, 7)), np.zeros(7), -1.0, 0.0, A, pi)
    with pytest.raises(ValueError, match="min_var"):
        B.hmm_mstep(x, np.ones((342, 7), np.float32), mu, var, float("nan"), 0.0)


def test_workspace_scales_with_n_k_and_not_with_n_k_d():
    small, big = E.workspace("tmjx_hmm_workspace", 210000, 60, 16, 840), E.workspace("tmjx_hmm_workspace", 210000, 1024, 128, 840)
    assert 4 * 210000 * 16 <= small <= 6 * 210000 * 16 + (1 << 24)
    assert 4.25 * 210000 * 128 <= big <= 4.25 * 210000 * 128 + 3 * (1 << 24)
    assert E.workspace("tmjx_hmm_workspace", 210000, 60, 16, 1) == small      # the number of sequences sizes nothing


def test_model_level_on_the_planted_chain():
    R.check_model(B, "emulation")


def test_gaussian_hmm_argument_checks():
    from track_mjx_amd.analysis import hmm as H
    x, lengths, _ = R.planted()
    for kw in (dict(n_states=0), dict(n_states=129), dict(n_states=3, tol=-1), dict(n_states=3, kappa=-1), dict(n_states=3, max_iter=0)):
        with pytest.raises(ValueError):
            H.GaussianHMM(backend=B, **kw)
    with pytest.raises(ValueError, match="lengths"):
        H.GaussianHMM(3, backend=B).fit(x, [10, 20])
    with pytest.raises(ValueError, match="not fitted"):
        H.GaussianHMM(3, backend=B).predict(x, lengths)


def test_cli_round_trip(tmp_path, capsys):
    R.check_cli(tmp_path, B, capsys)


def test_emulation_runs_clean_under_sanitizers(tmp_path):
    exe = E.build_main("hmm", tmp_path / "hmm_emu_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for args in ((), ("1", "1", "1"), ("3", "2", "1", "2", "1"), ("60", "7", "37", "300", "5")):
        res = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert res.returncode == 0 and "checksum" in res.stdout and not res.stderr, res.stdout + res.stderr
