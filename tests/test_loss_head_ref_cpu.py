"""CPU: conditions on the references of tests/loss_head_ref.py alone, for the exact case list tests/test_gpu_loss_head.py compares the kernels on.
They must hold before a GPU comparison against these references means anything: the clip-edge band is wide enough and nearly empty, both clip
branches occur, the float32 restatement is finite, and the GAE and Adam references agree with independent implementations."""
import math

import numpy as np
import pytest
import torch

from tests import loss_head_ref as R

HEAD_CASES = R.whole_head_cases()
_id = lambda c: f"{c[0]}-T{c[1]}-B{c[2]}-A{c[3]}-Z{c[4]}-norm{c[5]}"  # noqa: E731


def test_case_list_is_the_one_the_comparison_was_specified_on():
    assert [c[:4] for c in R.CASES] == [(1, 1, 38, 60), (1, 70, 38, 60), (2, 63, 38, 60), (7, 96, 38, 60), (24, 65, 38, 60), (24, 129, 38, 60),
                                        (3, 1025, 38, 60), (7, 96, 5, 3), (7, 96, 8, 16), (25, 65, 38, 60), (30, 130, 38, 60)]
    assert all(("phases" in c[4]) == (c[0] <= 24) and "one" in c[4] for c in R.CASES)
    assert len(HEAD_CASES) == 2 * (len(R.CASES) + len(R.NORMALIZE_CASES))


@pytest.mark.parametrize("case", HEAD_CASES, ids=_id)
def test_reference_conditions(case):
    fam, T, B, A, Z, norm, _ = case
    inp, cfg, r64, r32, near = R.reference(fam, T, B, A, Z, normalize_advantage=norm)
    N = T * B
    # near rows are few
    assert int(near.sum()) <= max(0.02 * N, 2), (int(near.sum()), N)
    # the band is wide enough: float32's relative error in rho is at most an eighth of it
    rho_err = float(((r32["rho"].double() - r64["rho"]).abs() / r64["rho"]).max())
    assert rho_err <= R.BAND / 8, rho_err
    # outside the band the two precisions take the same clip branch, and the float64 gradient is the branch it says it is
    assert torch.equal(r32["clipped"][~near], r64["clipped"][~near])
    W = 2 * A
    pick = torch.where(r64["clipped"][:, None], r64["dlogits_clipped"].reshape(N, W), r64["dlogits_unclipped"].reshape(N, W))
    assert R.array_error(pick, r64["dlogits"].reshape(N, W)) <= 1e-12
    # both clip branches occur
    if N >= 64:
        frac = float(r64["clipped"].double().mean())
        assert 0.10 <= frac <= 0.90, frac
        lo, hi = 1.0 - cfg["clip_eps"], 1.0 + cfg["clip_eps"]
        assert bool((r64["clipped"] & (r64["rho"] > hi)).any()) and bool((r64["clipped"] & (r64["rho"] < lo)).any())
    # everything finite, in both precisions
    for r in (r64, r32):
        for k in ("scalars", "vs", "adv", "dlogits", "dbaseline", "dfc2", "dlogits_unclipped", "dlogits_clipped"):
            assert bool(torch.isfinite(r[k]).all()), k
    print(f"near {int(near.sum())}/{N}  clipped {float(r64['clipped'].double().mean()):.3f}  rho err32 {rho_err:.2e}")


def test_hard_family_reaches_the_saturated_branches():
    """raw scale -30 (the min_std floor) and > 20 (softplus's linear branch), |action| > 10 (the branch inside fldj), log-variance at +-8"""
    inp = R.make_inputs("hard", 7, 96, 38, 60)
    raw_scale, lv = inp["logits"][..., 38:], inp["fc2"][..., 60:]
    assert bool((raw_scale == -30).any()) and bool((raw_scale > 20).any())
    assert bool((inp["raw_action"] > 10).any()) and bool((inp["raw_action"] < -10).any())
    assert bool((lv == 8).any()) and bool((lv == -8).any())


def test_zero_value_inputs_leave_the_entropy_gradient_alone():
    """reward = baseline = bootstrap = 0: every advantage is zero and dlogits is the entropy term only"""
    _, cfg, r64, _, _ = R.reference("hard", 7, 96, 38, 60, zero_value=True, normalize_advantage=0, entropy_cost=1.0, kl_weight=0.0)
    assert float(r64["adv"].abs().max()) == 0.0 and torch.equal(r64["dlogits"], r64["dlogits_clipped"])
    assert float(r64["dlogits"].abs().max()) > 0 and float(r64["dfc2"].abs().max()) == 0.0


def test_kl_gradient_by_hand_at_two_steps():
    """d kl / d m_0 has the prior term and the AR(1) term of step 1; d kl / d m_1 the AR(1) term alone"""
    T, B, A, Z = 2, 1, 1, 1
    inp = R.make_inputs("plain", T, B, A, Z)
    cfg = R.make_cfg(T, B, A, Z, kl_weight=1.0)
    r = R.loss_head(inp, cfg)
    m0, m1, lv0, lv1 = (float(inp["fc2"][t, 0, k]) for t, k in ((0, 0), (1, 0), (0, 1), (1, 1)))
    pv = 1 - 0.95 ** 2
    e = 0.95 * m0 - m1
    want = [[0.5 * (m0 + 0.95 * e / pv), -0.25 * (1 - math.exp(lv0))], [-0.5 * e / pv, 0.25 * (math.exp(lv1) / pv - 1)]]
    assert np.allclose(r["dfc2"].reshape(2, 2).numpy(), np.array(want), rtol=1e-12, atol=0)


@pytest.mark.parametrize("T,B", [(20, 1024), (1, 3)])
def test_gae_reference_agrees_with_the_oracle(T, B, oracle_built):
    from tests.common import default_blob, make_oracle
    rng = np.random.default_rng([T, B])
    trunc = (rng.random((T, B)) < 0.05).astype(np.float32); term = ((rng.random((T, B)) < 0.05) * (1 - trunc)).astype(np.float32)
    rew, val, boot = (rng.normal(size=s).astype(np.float32) for s in ((T, B), (T, B), (B,)))
    lam, disc = R.f32r(0.95), R.f32r(0.98)
    vs, adv = R.gae(*[torch.from_numpy(x).double() for x in (trunc, term, rew, val, boot)], lam, disc)
    scale = max(float(vs.abs().max()), float(adv.abs().max()))
    # the oracle computes in float32: at most six roundings per step of the recurrence, T steps (the float64 build: rounding of float64 alone)
    for precision, tol in (("f32", 6 * T * 2.0 ** -24), ("f64", 6 * T * 2.0 ** -53)):
        O = make_oracle(default_blob(), precision=precision)
        vs_o, adv_o = O.gae(trunc, term, rew, val, boot, lam, disc)
        assert np.abs(vs.numpy() - vs_o).max() <= tol * scale and np.abs(adv.numpy() - adv_o).max() <= tol * scale, precision


def test_adam_reference_agrees_with_torch_adam():
    """three steps (clip active, idle, active) against torch.optim.Adam + clip_grad_norm_ in float64 on 1 000 elements.  clip_grad_norm_ scales by
    max_norm / (norm + 1e-6): a relative 1e-6 in the clipped gradient, which Adam's update — invariant to the gradient's scale up to eps — passes on
    at far less than lr * 1e-6 per step."""
    hp = R.ADAM_HP
    rng = np.random.default_rng(3)
    p = torch.from_numpy(0.02 * rng.standard_normal(1000))
    ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([ref], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, gnorm in enumerate((3.0, 0.5, 7.0), 1):
        g = torch.from_numpy(rng.standard_normal(1000)); g = g / g.norm() * gnorm
        norm, p, m, v = R.adam_clip_step(p, g, m, v, lr=hp["lr"], b1=hp["b1"], b2=hp["b2"], eps=hp["eps"], bc1=1 - hp["b1"] ** step,
                                         bc2=1 - hp["b2"] ** step, max_norm=hp["max_norm"])
        ref.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([ref], hp["max_norm"])
        opt.step()
        assert abs(float(norm) - float(total)) <= 1e-12 * gnorm and abs(float(norm) - gnorm) <= 1e-12 * gnorm
        assert float((p - ref.detach()).abs().max()) <= step * hp["lr"] * 1e-6
    st = opt.state[ref]
    assert float((m - st["exp_avg"]).abs().max()) <= 1e-6 * float(m.abs().max()) and float((v - st["exp_avg_sq"]).abs().max()) <= 2e-6 * float(v.abs().max())
