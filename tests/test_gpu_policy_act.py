"""GPU: the acting policy as one launch (tmjx_policy_act, csrc/policy_act.h) against the launch sequence it replaces — tmjx_linear_act, tmjx_silu_ln_fwd,
tmjx_latent_concat, tmjx_sample_action — to the bit, against float64 torch within the tolerances of the layer-by-layer path, and through PPOLearner.

The flagship's reference width is 470 (not a multiple of 4): as the layer-by-layer path does, the kernel takes the first layer through weight rows
padded with zeros to K0 = 472, so tmjx_policy_act_ok asks for K0 == ref_w rounded up to 4 rather than refusing ref_w % 4 != 0 (which would refuse the
nets this kernel is written for); the refusal checked here is the UNPADDED row length."""
import ctypes as C

import pytest
import torch

from track_mjx_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OBS, REF, Z, A, H = 696, 470, 60, 38, 256
K0, WD = 472, 288                       # padded row lengths of the two first layers (470 -> 472, 60 + 226 = 286 -> 288)
LN_EPS = 1e-6
ROWS = (1, 15, 16, 17, 33, 1365)        # below, at and just past a 16-row tile edge, a ragged multi-tile case, the real group size
MAXROWS = max(ROWS)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Nets:
    """Random 2 x 256-style nets (n_enc / n_dec blocks per stack), a non-trivial normaliser with near-constant columns (std 1e-6) in both halves of the
    observation, observations and caller-supplied draws for MAXROWS rows.  Built once per stack depth and never modified."""

    def __init__(self, n_enc=2, n_dec=2, seed=0):
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731

        def block(k, kpad):
            w = torch.zeros(H, kpad)
            w[:, :k] = rn(H, k) / k ** 0.5
            return [w, 0.1 * rn(H), 1.0 + 0.1 * rn(H), 0.1 * rn(H)]
        self.enc = [block(REF, K0)] + [block(H, H) for _ in range(n_enc - 1)]
        self.dec = [block(Z + OBS - REF, WD)] + [block(H, H) for _ in range(n_dec - 1)]
        self.W2, self.b2 = rn(2 * Z, H) / H ** 0.5, 0.1 * rn(2 * Z)
        self.Wh, self.bh = rn(2 * A, H) / H ** 0.5, 0.1 * rn(2 * A)
        self.mean, self.std = 0.5 * rn(OBS), 0.5 + torch.rand(OBS, generator=g)
        self.obs = self.mean + self.std * rn(MAXROWS, OBS)
        for c in (7, 500):              # near-constant columns: one in the reference half, one in the proprioceptive half
            self.mean[c], self.std[c] = 0.25, 1e-6
            self.obs[:, c] = 0.25 + 1e-6 * rn(MAXROWS)
        self.fold_mean, self.fold_inv = torch.zeros(K0), torch.zeros(K0)
        self.fold_mean[:REF], self.fold_inv[:REF] = self.mean[:REF], 1.0 / self.std[:REF]
        self.eps, self.noise = rn(MAXROWS, Z), rn(MAXROWS, A)
        for k, v in list(vars(self).items()):
            if isinstance(v, torch.Tensor):
                setattr(self, k, v.to(DEV).contiguous())
            elif isinstance(v, list):
                setattr(self, k, [[t.to(DEV).contiguous() for t in b] for b in v])


_NETS = {}


def nets(n_enc=2, n_dec=2):
    if (n_enc, n_dec) not in _NETS:
        _NETS[(n_enc, n_dec)] = Nets(n_enc, n_dec)
    return _NETS[(n_enc, n_dec)]


def _outputs(M):
    f32 = dict(dtype=torch.float32, device=DEV)
    return dict(fc2=torch.full((M, 2 * Z), float("nan"), **f32), logits=torch.full((M, 2 * A), float("nan"), **f32), raw=torch.full((M, A), float("nan"), **f32),
                action_t=torch.full((A, M), float("nan"), **f32), logp=torch.full((M,), float("nan"), **f32))


def descriptor(N, M, out, eps=None, noise=None, seed=0, rng_state=None):
    d = hip.PolicyAct()
    d.obs, d.ldo, d.mean, d.inv_std, d.nmean, d.nstd = N.obs.data_ptr(), OBS, N.fold_mean.data_ptr(), N.fold_inv.data_ptr(), N.mean.data_ptr(), N.std.data_ptr()
    d.n, d.K0, d.Z, d.obs_w, d.ref_w, d.A, d.n_enc, d.n_dec = M, K0, Z, OBS, REF, A, len(N.enc), len(N.dec)
    for blocks, dst in ((N.enc, d.enc), (N.dec, d.dec)):
        for l, (w, b, g, be) in enumerate(blocks):
            dst[l] = hip.DecoderBlock(w.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr(), H, w.stride(0))
    d.W2, d.b2, d.ldw2, d.Wh, d.bh, d.ldwh, d.ln_eps = N.W2.data_ptr(), N.b2.data_ptr(), H, N.Wh.data_ptr(), N.bh.data_ptr(), H, LN_EPS
    d.eps, d.noise, d.seed = (eps.data_ptr() if eps is not None else None), (noise.data_ptr() if noise is not None else None), seed
    d.rng_state = rng_state.data_ptr() if rng_state is not None else None
    d.fc2, d.logits, d.raw, d.action_t, d.logp = (out[k].data_ptr() for k in ("fc2", "logits", "raw", "action_t", "logp"))
    return d


def run_new(N, M, eps=None, noise=None, seed=0, rng_state=None):
    out = _outputs(M)
    d = descriptor(N, M, out, eps, noise, seed, rng_state)
    L = hip.lib()
    assert L.tmjx_policy_act_ok(C.byref(d)) == 1
    hip.check(L.tmjx_policy_act(C.byref(d), None), "tmjx_policy_act")
    torch.cuda.synchronize()
    return out


def run_old(N, M, eps=None, noise=None, seed=0, rng_state=None):
    """The launches of PPOLearner._act_fused's LDS-free fp32 branch, one by one."""
    L, f32 = hip.lib(), dict(dtype=torch.float32, device=DEV)
    out = _outputs(M)

    def linear(a, lda, w, bias, n_out, mean=None, inv=None):
        assert L.tmjx_linear_act_ok(_p(a), lda, _p(w), w.stride(0), w.shape[1]) == 1
        o = torch.empty((M, n_out), **f32)
        hip.check(L.tmjx_linear_act(_p(a), lda, _p(w), w.stride(0), _p(bias), _p(o), M, n_out, w.shape[1], _p(mean), _p(inv), None), "tmjx_linear_act")
        return o

    def block(a, lda, blk, mean=None, inv=None):
        w, b, g, be = blk
        z = linear(a, lda, w, None, H, mean, inv)
        y, stats = torch.empty_like(z), torch.empty((M, 2), **f32)
        hip.check(L.tmjx_silu_ln_fwd(_p(z), _p(b), _p(g), _p(be), _p(y), _p(stats), M, H, LN_EPS, None), "tmjx_silu_ln_fwd")
        return y
    h = block(N.obs, OBS, N.enc[0], N.fold_mean, N.fold_inv)
    for blk in N.enc[1:]:
        h = block(h, H, blk)
    fc2 = linear(h, H, N.W2, N.b2, 2 * Z)
    x = torch.empty((M, WD), **f32)
    hip.check(L.tmjx_latent_concat(_p(fc2), _p(eps), _p(N.obs), _p(x), M, Z, OBS, REF, OBS, 1, _p(N.mean), _p(N.std), WD, seed, _p(rng_state), None), "tmjx_latent_concat")
    h = x
    for blk in N.dec:
        h = block(h, h.shape[1], blk)
    logits = linear(h, H, N.Wh, N.bh, 2 * A)
    hip.check(L.tmjx_sample_action(_p(logits), _p(noise), _p(out["raw"]), _p(out["action_t"]), _p(out["logp"]), M, A, seed, _p(rng_state), None), "tmjx_sample_action")
    torch.cuda.synchronize()
    out["fc2"], out["logits"] = fc2, logits
    return out


def assert_same(new, old, what):
    for k in ("fc2", "logits", "raw", "action_t", "logp"):
        assert torch.isfinite(old[k]).all(), (what, k)
        assert torch.equal(new[k], old[k]), (what, k, float((new[k] - old[k]).abs().max()), int((new[k] != old[k]).sum()))


@pytest.mark.parametrize("M", ROWS)
def test_equal_to_the_old_launches_with_the_callers_draws(M):
    N = nets()
    eps, noise = N.eps[:M].contiguous(), N.noise[:M].contiguous()
    assert_same(run_new(N, M, eps, noise), run_old(N, M, eps, noise), f"M = {M}")


# (the cases at counter 5 keep the ids they had before the counter became a parameter)
@pytest.mark.parametrize("M,ctr", [(M, c) for c in (5, 2 ** 32 + 5) for M in ROWS], ids=[f"{M}" if c == 5 else f"{M}-high-counter" for c in (5, 2 ** 32 + 5) for M in ROWS])
def test_equal_to_the_old_launches_with_the_device_stream(M, ctr):
    """Philox streams 2 / 3 on the device: the same draws, the same advance of the draw counter, and fresh noise on the next call; from a counter with
    its high word clear and set (tests/test_gpu_noise_gather.py states what the launch sequence draws, element for element)."""
    N = nets()
    seed = 0x1234567887654321
    st_new, st_old = (torch.tensor([ctr, 0], dtype=torch.long, device=DEV) for _ in range(2))
    new, old = run_new(N, M, seed=seed, rng_state=st_new), run_old(N, M, seed=seed, rng_state=st_old)
    assert_same(new, old, f"M = {M}, first call")
    assert st_new.tolist() == [ctr + 1, 0] and torch.equal(st_new, st_old)
    new2, old2 = run_new(N, M, seed=seed, rng_state=st_new), run_old(N, M, seed=seed, rng_state=st_old)
    assert_same(new2, old2, f"M = {M}, second call")
    assert st_new.tolist() == [ctr + 2, 0] and torch.equal(st_new, st_old)
    assert torch.equal(new2["fc2"], new["fc2"]) and not torch.equal(new2["raw"], new["raw"])      # same nets and observation, different noise
    if ctr >> 32:      # the counter's high word is part of the draw: the same low word alone gives other noise
        low = run_new(N, M, seed=seed, rng_state=torch.tensor([ctr & 0xFFFFFFFF, 0], dtype=torch.long, device=DEV))
        assert torch.equal(low["fc2"], new["fc2"]) and not torch.equal(low["raw"], new["raw"])


def test_whole_policy_against_float64_torch():
    """M = 33 against the policy written out in float64 torch, with the tolerances tests/test_gpu_parity.py::test_fused_inference_tail_matches_torch_path
    uses for its LDS-free arm (the same arithmetic): logits rtol 1e-3 / atol 2e-4, raw and action atol 3e-4."""
    M, N = 33, nets()
    eps, noise = N.eps[:M].contiguous(), N.noise[:M].contiguous()
    new = run_new(N, M, eps, noise)
    d = lambda t: t.double()  # noqa: E731
    x = (d(N.obs[:M]) - d(N.mean)) / d(N.std)

    def stack(h, blocks, k):
        for w, b, g, be in blocks:
            a = torch.nn.functional.silu(h @ d(w[:, :k]).T + d(b))
            h, k = torch.nn.functional.layer_norm(a, (H,), d(g), d(be), LN_EPS), H
        return h
    fc2 = stack(x[:, :REF], N.enc, REF) @ d(N.W2).T + d(N.b2)
    lat = fc2[:, :Z] + d(eps) * torch.exp(0.5 * fc2[:, Z:])
    logits = stack(torch.cat([lat, x[:, REF:]], 1), N.dec, Z + OBS - REF) @ d(N.Wh).T + d(N.bh)
    raw = logits[:, :A] + (torch.nn.functional.softplus(logits[:, A:]) + 0.001) * d(noise)
    print("max abs error: fc2 %.3g logits %.3g raw %.3g" % tuple(float((new[k].double() - r).abs().max()) for k, r in (("fc2", fc2), ("logits", logits), ("raw", raw))))
    assert torch.allclose(new["logits"].double(), logits, rtol=1e-3, atol=2e-4)
    assert torch.allclose(new["raw"].double(), raw, rtol=1e-3, atol=3e-4)
    assert torch.allclose(new["action_t"].t().double(), torch.tanh(raw), rtol=1e-3, atol=3e-4)


@pytest.mark.parametrize("nh", [1, 3])
def test_one_and_three_block_stacks(nh):
    M, N = 17, nets(nh, nh)
    eps, noise = N.eps[:M].contiguous(), N.noise[:M].contiguous()
    assert_same(run_new(N, M, eps, noise), run_old(N, M, eps, noise), f"{nh} blocks per stack")


def test_predicate_refuses_what_the_kernel_is_not_written_for():
    M, N, L = 17, nets(), hip.lib()
    out = _outputs(M)
    eps, noise = N.eps[:M].contiguous(), N.noise[:M].contiguous()

    def refused(word, **change):
        d = descriptor(N, M, out, eps, noise)
        for k, v in change.items():
            if k in ("enc_width", "dec_width"):
                getattr(d, k[:3])[1].width = v
            else:
                setattr(d, k, v)
        assert L.tmjx_policy_act_ok(C.byref(d)) == 0, change
        assert L.tmjx_policy_act(C.byref(d), None) == -22 and word in L.tmjx_last_error(), (change, L.tmjx_last_error())
    assert L.tmjx_policy_act_ok(C.byref(descriptor(N, M, out, eps, noise))) == 1
    refused(b"256 wide", enc_width=64)
    refused(b"256 wide", dec_width=512)
    refused(b"K0", K0=REF)                                     # the unpadded first-layer row: 470 is no multiple of 4
    refused(b"K0", ref_w=REF - 3, obs_w=OBS - 3)               # K0 is not ref_w rounded up to 4
    refused(b"aligned", obs=N.obs.data_ptr() + 4)              # misaligned rows
    refused(b"aligned", W2=N.W2.data_ptr() + 8)
    refused(b"blocks", n_enc=5)
    refused(b"288", Z=128, obs_w=OBS, ref_w=REF)               # 128 + 226 > 288
    refused(b"together", noise=None)
    assert all(torch.isnan(v).all() for v in out.values())     # nothing was launched


def _learner(envs, width, **kw):
    from track_mjx_amd.agent import ppo
    return ppo.PPOLearner(envs, encoder_layers=(width, width), decoder_layers=(width, width), critic_layers=(64, 64), latents=60, unroll_length=5,
                          batch_size=32, num_minibatches=4, num_updates_per_batch=2, seed=3, **kw)


def _spy(L):
    """Records what PPOLearner._policy_act_descriptor returned: a descriptor (the one-launch path ran) or None (the old launches)."""
    seen, inner = [], L._policy_act_descriptor

    def spy(*a, **k):
        seen.append(inner(*a, **k))
        return seen[-1]
    L._policy_act_descriptor = spy
    return seen


def test_learner_with_64_wide_nets_keeps_the_old_launches():
    from tests.common import make_env_and_oracle
    env = make_env_and_oracle(num_envs=64, n_clips=4, wrappers=True)[0]
    L = _learner(env, 64, use_graph=False)
    st = env.reset(torch.Generator().manual_seed(0))
    L.normalizer.update(st.obs.reshape(1, 64, -1) * 1.0)
    L.lds_free = True
    seen = _spy(L)
    action, extra = L.act(st.obs.contiguous())                 # row-major, as collect()'s staging copy: only the nets' width stands in the way
    torch.cuda.synchronize()
    assert torch.isfinite(action).all() and torch.isfinite(extra["log_prob"]).all()
    assert len(seen) >= 1 and all(d is None for d in seen)


def test_learner_rollout_and_update_equal_with_and_without_the_switch(monkeypatch):
    """Two learners over three env groups of (48, 44, 36) envs, 2 x 256 nets, the same seeds; one keeps the old launches (TMJX_NO_POLICY_ACT=1).  Every
    roll-out buffer after collect() and every parameter after update(1) must be equal to the bit."""
    from tests.common import make_env_and_oracle
    sizes, res = (48, 44, 36), {}
    for switch in ("1", None):
        if switch:
            monkeypatch.setenv("TMJX_NO_POLICY_ACT", switch)
        else:
            monkeypatch.delenv("TMJX_NO_POLICY_ACT", raising=False)
        envs = [make_env_and_oracle(num_envs=n, n_clips=4, wrappers=True, seed=k)[0] for k, n in enumerate(sizes)]
        L = _learner(envs, 256)
        assert L.lds_free
        seen = _spy(L)
        for k, e in enumerate(envs):
            L.states[k] = e.reset(torch.Generator().manual_seed(10 + k))
        L.collect()
        torch.cuda.synchronize()
        buf = {k: v.clone() for k, v in L.buf.items()}
        L.update(1)
        torch.cuda.synchronize()
        res[switch] = (buf, [p.detach().clone() for p in L.grads.params])
        assert (len(seen) == 0) if switch else (len(seen) > 0 and all(d is not None for d in seen)), (switch, len(seen))
    for k in res["1"][0]:
        assert torch.isfinite(res["1"][0][k]).all(), k
        assert torch.equal(res["1"][0][k], res[None][0][k]), k
    for a, b in zip(res["1"][1], res[None][1]):
        assert torch.equal(a, b)
