"""CPU: conditions on the reference of tests/lstm_ref.py alone, for the exact case lists tests/test_gpu_lstm_kernels.py compares the recurrence
kernels on.  They must hold before a GPU comparison against this reference means anything: the float32 restatement of every case stays under the
conditioning cap 2^-10 in every compared array (a case above it would let max(4 e32, 2^-20) hide a wrong kernel); the hand-written backward pass
equals float64 autograd through the forward pass; the product's CPU branch computes the same cell; T steps equal T one-step passes; the reset
flags mean what the kernels' `!= 0.f` means; the hard family has the rows it promises."""
import pytest
import torch

from tests import lstm_ref as R


def _close(a, b, tol=1e-12):
    return R.array_error(a, b.double()) <= tol


def test_case_lists_are_the_ones_the_comparison_was_specified_on():
    assert len(R.CASES) == 2 * 4 * 5 * 3 and len(set(R.CASES)) == len(R.CASES)
    assert {c[0] for c in R.CASES} == {"plain", "hard"} and {c[1] for c in R.CASES} == {1, 7, 8, 9, 17}
    assert {c[2] for c in R.CASES} == {1, 2, 20} and {c[3] for c in R.CASES} == {32, 64, 128, 256}
    assert R.LARGE_CASES == (("plain", 257, 20, 256), ("hard", 1365, 2, 32), ("plain", 1365, 3, 128))
    assert R.ARRAYS == ("h", "c", "gates", "h_prev", "dgates", "dh0", "dc0") and R.CAP == 2.0 ** -10 and R.bound(0.0) == 2.0 ** -20 and R.bound(1e-3) == 4e-3


@pytest.mark.parametrize("H", R.HIDDEN_SIZES)
def test_every_case_is_under_the_conditioning_cap(H):
    bad = []
    for case in [c for c in R.CASES + R.LARGE_CASES if c[3] == H]:
        for name, e32 in R.e32_of(case).items():
            print(f"LSTM-ref | {R.case_id(case)} | {name} | e32 {e32:.2e}")
            if name in R.ARRAYS and not e32 <= R.CAP:
                bad.append((case, name, e32))
    assert not bad, bad


@pytest.mark.parametrize("case", [("hard", 17, 20, 64), ("hard", 9, 2, 256), ("plain", 17, 20, 32), ("hard", 7, 1, 128)], ids=R.case_id)
def test_hand_written_backward_equals_float64_autograd(case):
    inp, r64, _ = R.reference(*case)
    assert bool((inp["reset"] != 0).any()) and bool((inp["reset"] == 0).any())
    xg, Wh, bh, h0, c0 = (inp[k].double().requires_grad_(True) for k in ("xg", "Wh", "bh", "h0", "c0"))
    h = R.lstm_forward(xg, Wh, bh, h0, c0, inp["reset"])[0]
    dxg, dWh, dbh, dh0, dc0 = torch.autograd.grad(h, (xg, Wh, bh, h0, c0), inp["dh"].double())
    for name, want in (("dgates", dxg), ("dh0", dh0), ("dc0", dc0), ("dW_h", dWh), ("db", dbh)):
        err = R.array_error(r64[name], want)
        print(f"LSTM-ref | {R.case_id(case)} | {name} | hand-written vs autograd {err:.2e}")
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("case", [("hard", 17, 20, 64), ("plain", 9, 2, 256), ("plain", 8, 1, 32)], ids=R.case_id)
def test_product_cpu_branch_equals_the_reference(case):
    from track_mjx_amd.agent.lstm import _torch_lstm_layer
    inp, r64, _ = R.reference(*case)
    xg, Wh, bh, h0, c0 = (inp[k].double() for k in ("xg", "Wh", "bh", "h0", "c0"))
    h, c = _torch_lstm_layer(xg, Wh, bh, h0, c0, inp["reset"])
    assert _close(h, r64["h"]) and _close(c, r64["c"])
    h, c = _torch_lstm_layer(xg, Wh, bh, h0, c0, None)
    r = R.lstm_layer({**inp, "reset": None})
    assert _close(h, r["h"]) and _close(c, r["c"]) and not _close(h, r64["h"], 1e-3)


@pytest.mark.parametrize("case", [("hard", 17, 20, 64), ("plain", 9, 20, 256)], ids=R.case_id)
def test_T_steps_equal_T_one_step_passes(case):
    inp, r64, _ = R.reference(*case)
    h, c = inp["h0"].double(), inp["c0"].double()
    for t in range(case[2]):
        one = {"xg": inp["xg"][t:t + 1].double(), "Wh": inp["Wh"].double(), "bh": inp["bh"].double(), "h0": h, "c0": c, "reset": inp["reset"][t:t + 1]}
        r = R.lstm_layer(one)
        h, c = r["h"][0], r["c"][0]
        for name in ("h", "c", "gates", "h_prev"):
            assert _close(r[name][0], r64[name][t]), (name, t)


def test_reset_flags_behave_as_specified():
    fam, rows, T, H = case = ("hard", 9, 20, 32)
    inp, r64, _ = R.reference(*case)
    reset = inp["reset"]
    # -0.0 keeps the carry: the flag is there, the step reads the previous step's h, and nothing differs from the same case with +0.0 in its place
    t, row = R.neg_zero_index(fam, rows, T)
    assert float(reset[t, row]) == 0.0 and bool(torch.signbit(reset[t, row]))
    assert torch.equal(r64["h_prev"][t, row], r64["h"][t - 1, row]) and float(r64["h_prev"][t, row].abs().max()) > 0
    plus = reset.clone()
    plus[t, row] = 0.0
    rp = R.lstm_layer({**inp, "reset": plus})
    assert all(torch.equal(rp[k], r64[k]) for k in R.ARRAYS)
    # 2.0 and -1.0 zero it, 0.0 does not
    assert set(reset[0, ::3].tolist()) == {2.0} and set(reset[:, 1].tolist()) == {-1.0}
    flagged = reset != 0
    assert float(r64["h_prev"][flagged].abs().max()) == 0.0 and float(r64["c_prev"][flagged].abs().max()) == 0.0
    assert bool((r64["h_prev"][~flagged].abs().amax(-1) > 0).all())
    # the reset step's gates come from xg + bh alone
    H4 = inp["xg"].double()[0, 0] + inp["bh"].double()
    want = torch.cat([torch.sigmoid(H4[:H]), torch.sigmoid(H4[H:2 * H]), torch.tanh(H4[2 * H:3 * H]), torch.sigmoid(H4[3 * H:])])
    assert _close(r64["gates"][0, 0], want)
    # a row reset at every step: no carry in, no gradient out; d f-gate = dc * c_prev * ... = 0 there
    assert float(r64["h_prev"][:, 1].abs().max()) == 0.0 and float(r64["dh0"][1].abs().max()) == 0.0 and float(r64["dc0"][1].abs().max()) == 0.0
    assert float(r64["dgates"][:, 1, H:2 * H].abs().max()) == 0.0
    # rows reset at t = 0 get no carry gradient either; the others do
    at0 = reset[0] != 0
    assert float(r64["dh0"][at0].abs().max()) == 0.0 and float(r64["dc0"][at0].abs().max()) == 0.0
    assert bool((r64["dc0"][~at0].abs().amax(-1) > 0).all())
    # about half the rows are reset at the last step
    frac = float((R.reference("hard", 1365, 2, 32)[0]["reset"][-1] != 0).double().mean())
    assert 0.4 < frac < 0.7, frac


def test_hard_family_saturates_its_gates_exactly():
    case = ("hard", 17, 2, 64)
    inp, r64, r32 = R.reference(*case)
    xg = inp["xg"]
    assert 0.03 < float((xg == -100).double().mean()) < 0.07 and 0.03 < float((xg == 100).double().mean()) < 0.07
    assert float(inp["c0"].abs().max()) > 6.0
    pre = R.pre_activation(inp, r64)
    H = case[3]
    sig = torch.ones(4 * H, dtype=torch.bool)
    sig[2 * H:3 * H] = False
    lo, hi = pre < -90, pre > 90
    assert int(lo.sum()) > 100 and int(hi.sum()) > 100
    g = r32["gates"]          # the float32 restatement: exact 0 / 1 / -+1, as the kernel's must be
    assert bool((g[lo & sig] == 0).all()) and bool((g[hi & sig] == 1).all()) and bool((g[lo & ~sig] == -1).all()) and bool((g[hi & ~sig] == 1).all())
    assert all(bool(torch.isfinite(r32[k]).all()) for k in R.ARRAYS + R.WEIGHT_GRADS)
