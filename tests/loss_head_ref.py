"""Plain torch references for the kernels between the network outputs and the parameter update (csrc/ppo_kernels.h, csrc/tmjx_hip.hip):
the PPO loss head from RAW arrays (no networks: the kernels are compared per output row, not through a GEMM), the GAE recurrence of
tmjx_gae and one clip_by_global_norm -> adam step on flat arrays.  Every function takes the dtype to compute in: float64 is the reference,
the same code in float32 (the "restatement") gives the error a correct float32 evaluation has, which the tests' bounds are built on.

Semantics (header of csrc/ppo_kernels.h, agent/losses.py): NormalTanh with min_std 0.001; the entropy sample at loc + scale * noise; GAE with
termination = (1 - discount)(1 - truncation); vs and the advantages are constants for the gradient; advantage normalisation by the
population std + 1e-8; v_loss = 0.25 mean((vs - baseline)^2); AR(1) latent KL with alpha = 0.95, the t = 0 term against N(0, 1), the gradient
through both m_t and m_{t-1}.

The clip edge: min(rho A, clip(rho) A) has a gradient discontinuity at rho = 1 +- eps, so two correct evaluations in different precisions
can take different branches on a row whose rho is within rounding of an edge — which changes that whole dlogits row.  A row is NEAR when
|rho64 - (1 +- eps)| < BAND; the reference returns the gradient of both branches (`dlogits_unclipped`, `dlogits_clipped`) and
`dlogits_error` accepts either on near rows, under the same bound as every other row.  tests/test_loss_head_ref_cpu.py checks that near rows are
few and that the band is eight times wider than float32's error in rho."""
from __future__ import annotations

import math

import numpy as np
import torch

MIN_STD = 0.001
ALPHA = 0.95
BAND = 1e-3                      # |rho - (1 +- eps)| below which a row may take either clip branch
FLOOR = 2.0 ** -20               # eight float32 roundings at the array's largest magnitude
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
INPUT_KEYS = ("logits", "raw_action", "behaviour_logp", "noise", "baseline", "bootstrap", "reward", "discount", "truncation", "fc2")   # the C entry's order
SCALAR_NAMES = ("total", "policy", "v", "entropy_loss", "kl", "adv_mean", "adv_std", "entropy")                                        # the kernel's `out`
FAMILIES = ("plain", "hard")

# (T, B, A, Z, entries): tmjx_ppo_loss ("one") and tmjx_ppo_loss_phases with mask 15 ("phases", T <= 24 only).  T > 24 takes the single-block
# k_ppo_b, whose register path is for T <= 24 as well: through tmjx_ppo_loss both 25 and 30 steps run its generic loop.
CASES = (
    (1, 1, 38, 60, ("one", "phases")),
    (1, 70, 38, 60, ("one", "phases")),
    (2, 63, 38, 60, ("one", "phases")),
    (7, 96, 38, 60, ("one", "phases")),
    (24, 65, 38, 60, ("one", "phases")),
    (24, 129, 38, 60, ("one", "phases")),
    (3, 1025, 38, 60, ("one", "phases")),
    (7, 96, 5, 3, ("one", "phases")),
    (7, 96, 8, 16, ("one", "phases")),
    (25, 65, 38, 60, ("one",)),
    (30, 130, 38, 60, ("one",)),
)
NORMALIZE_CASES = ((7, 96, 38, 60), (24, 65, 38, 60))     # these also run with normalize_advantage = 0


def f32r(x: float) -> float:
    """A scalar as the C entry receives it: rounded to float32."""
    return float(np.float32(x))


def softplus(x):
    return torch.logaddexp(x, torch.zeros_like(x))


def fldj(x):
    """log |d tanh(x) / dx|"""
    return 2.0 * (math.log(2.0) - x - softplus(-2.0 * x))


def log_prob(logits, raw_action):
    A = raw_action.shape[-1]
    loc, scale = logits[..., :A], softplus(logits[..., A:]) + MIN_STD
    return (-0.5 * ((raw_action - loc) / scale) ** 2 - torch.log(scale) - HALF_LOG_2PI - fldj(raw_action)).sum(-1)


def gae(truncation, termination, rewards, values, bootstrap, lambda_, discount):
    """compute_gae as a reverse recurrence in the dtype of its inputs: (vs, advantages), both [T, B]."""
    T = rewards.shape[0]
    tm = 1.0 - truncation
    acc, vnext, vs = torch.zeros_like(bootstrap), bootstrap, [None] * T
    for t in range(T - 1, -1, -1):
        delta = (rewards[t] + discount * (1.0 - termination[t]) * vnext - values[t]) * tm[t]
        acc = delta + discount * (1.0 - termination[t]) * tm[t] * lambda_ * acc
        vs[t] = acc + values[t]
        vnext = values[t]
    vs = torch.stack(vs, 0)
    vs_next = torch.cat([vs[1:], bootstrap[None]], 0)
    adv = (rewards + discount * (1.0 - termination) * vs_next - values) * tm
    return vs, adv


def make_cfg(T, B, A, Z, family="plain", **over):
    """The PpoCfg scalars of a family, every float rounded to float32 (what the kernel is handed)."""
    c = dict(T=T, B=B, A=A, Z=Z, reward_scaling=1.0, discounting=0.95, gae_lambda=0.95, clip_eps=0.2, entropy_cost=1e-2, kl_weight=0.1,
             normalize_advantage=1)
    if family == "hard":
        c.update(reward_scaling=0.5, discounting=0.97, gae_lambda=0.9)
    c.update(over)
    return {k: (f32r(v) if isinstance(v, float) else int(v)) for k, v in c.items()}


def case_seed(family, T, B, A, Z, bump=0):
    return [FAMILIES.index(family), T, B, A, Z, bump]


def make_inputs(family, T, B, A, Z, bump=0):
    """float32 CPU tensors under INPUT_KEYS, seeded per case.  behaviour_logp = the float64 log-prob + 0.3 N(0, 1), so that the ratios straddle
    both clip edges."""
    rng = np.random.default_rng(case_seed(family, T, B, A, Z, bump))
    n = lambda *s: rng.standard_normal(s)  # noqa: E731
    if family == "plain":
        logits, raw, fc2 = 0.5 * n(T, B, 2 * A), 0.7 * n(T, B, A), 0.3 * n(T, B, 2 * Z)
        baseline, bootstrap = n(T, B), n(B)
    else:
        loc = 1.5 * n(T, B, A) * np.where(rng.random((T, B, A)) < 0.05, 8.0, 1.0)
        rs, u = 2.0 * n(T, B, A) - 1.0, rng.random((T, B, A))
        rs = np.where(u < 0.05, -30.0, np.where(u > 0.95, 25.0, rs))
        logits = np.concatenate([loc, rs], -1).astype(np.float32)
        scale = np.logaddexp(logits[..., A:].astype(np.float64), 0.0) + MIN_STD
        raw = logits[..., :A].astype(np.float64) + scale * n(T, B, A)          # as the acting policy samples it
        fc2 = np.concatenate([2.0 * n(T, B, Z), np.clip(3.0 * n(T, B, Z), -8.0, 8.0)], -1)
        baseline, bootstrap = 3.0 * n(T, B), 3.0 * n(B)
    noise, reward = n(T, B, A), np.abs(n(T, B))
    discount, trunc = (rng.random((T, B)) > 0.1), (rng.random((T, B)) > 0.9)
    out = {"logits": logits, "raw_action": raw, "noise": noise, "baseline": baseline, "bootstrap": bootstrap, "reward": reward, "discount": discount,
           "truncation": trunc, "fc2": fc2}
    out = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in out.items()}
    lp = log_prob(out["logits"].double(), out["raw_action"].double())
    out["behaviour_logp"] = (lp + 0.3 * torch.from_numpy(n(T, B))).float()
    return {k: out[k] for k in INPUT_KEYS}


def loss_head(inp: dict, cfg: dict, dtype=torch.float64) -> dict:
    """The loss head on the C entry's inputs, computed in `dtype` on the CPU.  Returns the eight scalars in the kernel's order, vs, adv (not
    normalised: what the kernel leaves in its scratch buffer), the three gradients by autograd, the two clip branches of dlogits, and per row:
    rho, the (normalised) advantage the surrogate used and whether the surrogate gradient is zero (`clipped`)."""
    T, B, A, Z = cfg["T"], cfg["B"], cfg["A"], cfg["Z"]
    x = {k: inp[k].to(dtype) for k in INPUT_KEYS}
    logits, baseline, fc2 = (x[k].clone().requires_grad_(True) for k in ("logits", "baseline", "fc2"))
    N = T * B
    # policy
    loc, scale = logits[..., :A], softplus(logits[..., A:]) + MIN_STD
    logp = log_prob(logits, x["raw_action"])
    ent_rows = (0.5 + HALF_LOG_2PI + torch.log(scale) + fldj(loc + scale * x["noise"])).sum(-1)
    entropy = ent_rows.mean()
    entropy_loss = -cfg["entropy_cost"] * entropy
    # GAE on constants
    with torch.no_grad():
        termination = (1.0 - x["discount"]) * (1.0 - x["truncation"])
        vs, adv = gae(x["truncation"], termination, x["reward"] * cfg["reward_scaling"], baseline.detach(), x["bootstrap"], cfg["gae_lambda"],
                      cfg["discounting"])
        adv_mean = adv.mean()
        adv_std = ((adv - adv_mean) ** 2).mean().sqrt()
        ad = (adv - adv_mean) / (adv_std + 1e-8) if cfg["normalize_advantage"] else adv
    rho = torch.exp(logp - x["behaviour_logp"])
    lo, hi = 1.0 - cfg["clip_eps"], 1.0 + cfg["clip_eps"]
    s1, s2 = rho * ad, rho.clamp(lo, hi) * ad
    surrogate = torch.where(s1 <= s2, s1, s2)      # inside the clip range s1 == s2 and s1's (full) gradient is taken
    policy = -surrogate.mean()
    v_loss = 0.25 * ((vs - baseline) ** 2).mean()
    # latent KL
    m, lv = fc2[..., :Z], fc2[..., Z:]
    pv = 1.0 - ALPHA ** 2
    kl = -0.5 * (1.0 + lv[0] - m[0] ** 2 - torch.exp(lv[0])).mean()
    if T > 1:
        kl_t = 0.5 * (torch.exp(lv[1:]) / pv + (ALPHA * m[:-1] - m[1:]) ** 2 / pv - 1.0 + math.log(pv) - lv[1:]).mean()
        kl = (kl + kl_t * (T - 1)) / T
    kl = cfg["kl_weight"] * kl
    total = policy + v_loss + entropy_loss + kl
    dlogits, dbaseline, dfc2 = torch.autograd.grad(total, (logits, baseline, fc2), retain_graph=True)
    d_ent, = torch.autograd.grad(entropy_loss, logits, retain_graph=True)
    d_unc, = torch.autograd.grad(-(rho * ad).mean(), logits)
    with torch.no_grad():
        clipped = ~((s1 <= s2) | ((rho >= lo) & (rho <= hi)))
    det = lambda t: t.detach()  # noqa: E731
    return {"scalars": torch.stack([det(t) for t in (total, policy, v_loss, entropy_loss, kl, adv_mean, adv_std, entropy)]),
            "vs": vs, "adv": adv, "dlogits": det(dlogits), "dbaseline": det(dbaseline), "dfc2": det(dfc2),
            "dlogits_unclipped": det(d_ent + d_unc), "dlogits_clipped": det(d_ent),
            "rho": det(rho).reshape(N), "ad": ad.reshape(N), "clipped": clipped.reshape(N), "logp": det(logp)}


def near_rows(rho64, clip_eps):
    """[N] bool: rows whose float64 rho lies within BAND of a clip edge."""
    return ((rho64 - (1.0 - clip_eps)).abs() < BAND) | ((rho64 - (1.0 + clip_eps)).abs() < BAND)


# ---- the metric and the bound ----------------------------------------------------------------------------------------------------------
def array_error(got, ref) -> float:
    """largest absolute error / largest reference magnitude (absolute where the reference is all zero)"""
    got, ref = torch.as_tensor(got).double().cpu(), ref.double()
    scale = float(ref.abs().max())
    d = float((got - ref).abs().max())
    return d / scale if scale > 0 else d


def scalar_error(got, ref) -> float:
    got, ref = torch.as_tensor(got).double().cpu(), ref.double()
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())


def dlogits_error(got, r64: dict, near, only_far: bool = False) -> float:
    """array_error for dlogits with the clip edge: a near row is compared with BOTH branches of the reference and the closer one counts;
    only_far: rows outside the band only (the float32 restatement's error e32)."""
    W = r64["dlogits"].shape[-1]
    rows = lambda t: torch.as_tensor(t).double().cpu().reshape(-1, W)  # noqa: E731
    g = rows(got)
    scale = float(r64["dlogits"].abs().max())
    d = (g - rows(r64["dlogits"])).abs().amax(-1)
    if only_far:
        d = d[~near]
    else:
        alt = torch.minimum((g - rows(r64["dlogits_unclipped"])).abs().amax(-1), (g - rows(r64["dlogits_clipped"])).abs().amax(-1))
        d = torch.where(near, alt, d)
    d = float(d.max()) if d.numel() else 0.0
    return d / scale if scale > 0 else d


def bound(e32: float) -> float:
    """4 x the float32 restatement's error, and never below eight float32 roundings"""
    return max(4.0 * e32, FLOOR)


# ---- optimiser ------------------------------------------------------------------------------------------------------------------------
def adam_clip_step(p, g, m, v, *, lr, b1, b2, eps, bc1, bc2, max_norm):
    """One optax.chain(clip_by_global_norm(max_norm), adam(lr)) step on flat arrays in their dtype: (norm, p, m, v).  bc1 / bc2 are the bias
    corrections 1 - beta^step of the step being taken."""
    norm = (g * g).sum().sqrt()
    gi = g * (max_norm / torch.clamp(norm, min=max_norm))          # g if ||g|| < max_norm else g / ||g|| * max_norm
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return norm, p, m, v


ADAM_HP = dict(lr=f32r(1e-2), b1=f32r(0.9), b2=f32r(0.999), eps=f32r(1e-8), max_norm=1.0)
ADAM_HP.update(bc1=f32r(1.0 - ADAM_HP["b1"] ** 3), bc2=f32r(1.0 - ADAM_HP["b2"] ** 3))       # step 3


def make_adam_inputs(n: int, grad_norm: float):
    """float32 flat arrays p, g, m, v (m, v nonzero: a step in the middle of training), ||g|| = grad_norm up to rounding.  p is small so
    that the update (~ lr) is a visible part of it."""
    rng = np.random.default_rng([n, int(round(grad_norm * 1000))])
    p, g, m = 0.02 * rng.standard_normal(n), rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    v = (0.1 * rng.standard_normal(n)) ** 2 + 1e-6
    g = g / np.sqrt((g * g).sum()) * grad_norm
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (p, g, m, v))


# ---- the case list shared by the CPU conditions and the GPU comparisons ---------------------------------------------------------------
def whole_head_cases():
    """(family, T, B, A, Z, normalize_advantage, entries) of every whole-head comparison"""
    out = []
    for fam in FAMILIES:
        for T, B, A, Z, entries in CASES:
            out.append((fam, T, B, A, Z, 1, entries))
            if (T, B, A, Z) in NORMALIZE_CASES:
                out.append((fam, T, B, A, Z, 0, entries))
    return out


_cache: dict = {}


def reference(family, T, B, A, Z, zero_value=False, **over):
    """(inputs, cfg, float64 result, float32 result, near rows) of a case, computed once per process and shared; callers must not write to it.
    zero_value: reward = baseline = bootstrap = 0 (every advantage is then zero)."""
    key = (family, T, B, A, Z, zero_value, tuple(sorted(over.items())))
    if key not in _cache:
        inp = make_inputs(family, T, B, A, Z)
        if zero_value:
            inp = {k: (torch.zeros_like(v) if k in ("reward", "baseline", "bootstrap") else v) for k, v in inp.items()}
        cfg = make_cfg(T, B, A, Z, family, **over)
        r64, r32 = loss_head(inp, cfg, torch.float64), loss_head(inp, cfg, torch.float32)
        _cache[key] = (inp, cfg, r64, r32, near_rows(r64["rho"], cfg["clip_eps"]))
    return _cache[key]
