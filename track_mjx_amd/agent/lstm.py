"""The recurrent learner: PPO with the LSTM-decoder intention policy — mirror of track_mjx/agent/lstm_ppo/{intention_network,acting,losses,ppo}.py.

Network (intention_network.py): the MLP learner's encoder (Dense -> SiLU -> LayerNorm blocks, fc2_mean | fc2_logvar); z = latent_mean (no
reparameterisation in acting or in the loss); the decoder input [z | egocentric obs] feeds `hidden_layer_num` stacked flax nn.LSTMCell's of
`hidden_state_size` features (gate order i, f, g, o; input kernels without bias, recurrent kernels orthogonal with bias, no forget-gate offset) and one
Dense `lstm_projection` to the 2 nu action logits.  The decoder_layer_sizes other than the logits width are unused, as in the reference.

Kernels: per layer, the input projection x W_i^T is one GEMM over all T x rows rows (tmjx_gemm_nt, autograd through _HipDenseFn: dx = dgates W_i,
dW_i); the recurrence is ONE launch of tmjx_lstm_seq_fwd / _bwd (csrc/lstm_kernels.h) over the T steps; dW_h and db = the weight-gradient GEMM of
dgates against the reset-applied h_prev sequence.  The acting step is the same launch with T = 1 per layer, writing the roll-out carry in place.

Carry (acting.py:36-78, ppo.py:396-459): [n_env, L, H] (h, c) starting at zero, zeroed for every env whose episode ended (the reset mask of the next
step's launch), continued across unrolls, training steps and env resets; each transition row stores the carry the policy READ at t = 0 of its
unroll; the loss scans T steps from it, zeroing the carry after step t where 1 - discount[t] is set.  Loss (losses.py:105-297): the MLP learner's
loss with the plain KL -0.5 mean(1 + logvar - mean^2 - exp(logvar)) and no KL schedule.  The normaliser is updated AFTER the SGD epochs
(ppo.py:425-453).  GPU only: the SGD step needs tmjx_gae / tmjx_ppo_loss; CPU tensors take a torch restatement of the network only.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from .. import hip as _hip
from . import losses as _losses
from .networks import NormalTanh, _Block, _dense, _HipDenseFn, _lecun_normal_, _lecun_uniform_, gemm_dw
from .ppo import PPOLearner

LSTM_HIDDEN_SIZES = (32, 64, 128, 256)      # what tmjx_lstm_hidden_ok accepts


def check_lstm_config(hidden_state_size: int, hidden_layer_num: int, matmul_dtype=None) -> None:
    """Refuse what the recurrent learner does not build (before anything is allocated)."""
    if matmul_dtype is not None and matmul_dtype != torch.float32:
        raise ValueError("use_lstm: the LSTM learner is fp32 only; mlp_gemm_inputs=bf16 is not supported with use_lstm=true")
    if int(hidden_layer_num) < 1:
        raise ValueError(f"use_lstm: hidden_layer_num must be >= 1 (got {hidden_layer_num})")
    if int(hidden_state_size) not in LSTM_HIDDEN_SIZES:
        raise ValueError(f"use_lstm: hidden_state_size {hidden_state_size} is not supported by the LSTM kernels (one of {LSTM_HIDDEN_SIZES})")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _vp(t):
    return t.data_ptr() if t is not None else None


def lstm_seq_fwd(xg, Wh, bh, h0, c0, reset=None, out_h=None, out_c=None, train: bool = False):
    """One layer's T-step recurrence (tmjx_lstm_seq_fwd).  xg [T, rows, 4H] (row stride ldx), h0 / c0 [rows, H] with a common row stride (e.g. a
    layer slice of a [rows, L, H] carry), reset [T, rows] or None.  Returns (h [T, rows, H], c, gates, h_prev); gates / h_prev only with `train`.
    out_h / out_c: destinations with h0's row stride (T == 1: may be h0 / c0 themselves — the acting step updates the carry in place)."""
    T, rows, G4 = xg.shape
    H = G4 // 4
    dev = xg.device
    if xg.stride(2) != 1 or xg.stride(0) != rows * xg.stride(1) or h0.stride(-1) != 1 or c0.stride() != h0.stride() or Wh.stride(1) != 1:
        raise _hip.TmjxError("lstm_seq_fwd: unexpected operand layout")
    f32 = dict(dtype=torch.float32, device=dev)
    if out_h is None:
        out_h, out_c = torch.empty((T, rows, H), **f32), torch.empty((T, rows, H), **f32)
        ldo = H
    else:
        ldo = out_h.stride(-2)
        # (h_prev is written with the outputs' row stride: the in-place acting form has no training outputs)
        if T != 1 or train or out_c.stride() != out_h.stride():
            raise _hip.TmjxError("lstm_seq_fwd: out_h / out_c are for the T == 1 acting step (train=False) with matching strides")
    gates = torch.empty((T, rows, G4), **f32) if train else None
    h_prev = torch.empty((T, rows, H), **f32) if train else None
    if reset is not None:
        reset = reset.contiguous().float()
    a = _hip.LstmFwd(_vp(xg), xg.stride(1), _vp(Wh), Wh.stride(0), _vp(bh), _vp(h0), _vp(c0), h0.stride(-2), _vp(reset), rows,
                     _vp(out_h), _vp(out_c), ldo, _vp(gates), _vp(h_prev), T, rows, H)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().tmjx_lstm_seq_fwd(C.byref(a), _stream(dev)), "tmjx_lstm_seq_fwd")
    return out_h, out_c, gates, h_prev


def lstm_seq_bwd(dh, Wh, gates, c, c0, reset=None, want_carry_grad: bool = False):
    """The reverse recurrence (tmjx_lstm_seq_bwd): dh [T, rows, H] -> dgates [T, rows, 4H] (+ d h0, d c0 [rows, H] with `want_carry_grad`)."""
    T, rows, H = dh.shape
    dh = dh.contiguous()
    dev = dh.device
    dgates = torch.empty((T, rows, 4 * H), dtype=torch.float32, device=dev)
    dh0 = torch.empty((rows, H), dtype=torch.float32, device=dev) if want_carry_grad else None
    dc0 = torch.empty_like(dh0) if want_carry_grad else None
    c0 = c0 if c0.stride(-1) == 1 else c0.contiguous()
    ld0 = c0.stride(-2)
    if want_carry_grad and ld0 != H:
        c0 = c0.contiguous(); ld0 = H
    if reset is not None:
        reset = reset.contiguous().float()
    a = _hip.LstmBwd(_vp(dh), H, _vp(Wh), Wh.stride(0), _vp(gates), _vp(c), H, _vp(c0), ld0, _vp(reset), rows, _vp(dgates), _vp(dh0), _vp(dc0), T, rows, H)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().tmjx_lstm_seq_bwd(C.byref(a), _stream(dev)), "tmjx_lstm_seq_bwd")
    return dgates, dh0, dc0


class _LstmSeqFn(torch.autograd.Function):
    """h [T, rows, H] of one layer from its gate inputs xg = x W_i^T.  The initial carry and the reset mask are data (no gradient)."""

    @staticmethod
    def forward(ctx, xg, Wh, bh, h0, c0, reset):
        h, c, gates, h_prev = lstm_seq_fwd(xg, Wh, bh, h0, c0, reset, train=True)
        ctx.save_for_backward(Wh, gates, c, c0, reset if reset is not None else torch.empty(0, device=xg.device), h_prev)
        ctx.has_reset = reset is not None
        return h

    @staticmethod
    def backward(ctx, dh):
        Wh, gates, c, c0, reset, h_prev = ctx.saved_tensors
        dgates, _, _ = lstm_seq_bwd(dh, Wh, gates, c, c0, reset if ctx.has_reset else None)
        G4 = dgates.shape[-1]
        dWh, dbh = gemm_dw(dgates.view(-1, G4), h_prev.view(-1, h_prev.shape[-1]), True)
        return dgates, dWh, dbh, None, None, None


def _torch_lstm_layer(xg, Wh, bh, h, c, reset):
    """CPU tensors: the same recurrence in torch (flax nn.LSTMCell)."""
    hs, cs = [], []
    H = h.shape[-1]
    for t in range(xg.shape[0]):
        if reset is not None:
            keep = (reset[t] == 0).to(h.dtype)[:, None]
            h, c = h * keep, c * keep
        g = xg[t] + h @ Wh.t() + bh
        i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h); cs.append(c)
    return torch.stack(hs), torch.stack(cs)


class LSTMIntentionPolicy(nn.Module):
    """Encoder + stacked-LSTM decoder intention policy (lstm_ppo/intention_network.py).  Parameters of LSTM layer k (flax lstm_{k}):
    w_ih[k] [4H, in_k] = the four input kernels ii | if | ig | io transposed (no bias), w_hh[k] [4H, H] = hi | hf | hg | ho transposed, b_hh[k] [4H]."""

    def __init__(self, obs_size: int, reference_obs_size: int, action_size: int, latents: int = 60, encoder_layers=(1024, 1024),
                 hidden_state_size: int = 128, hidden_layer_num: int = 2):
        super().__init__()
        check_lstm_config(hidden_state_size, hidden_layer_num)
        self.reference_obs_size, self.latents, self.action_size = reference_obs_size, latents, action_size
        self.hidden_state_size, self.hidden_layer_num = H, L = int(hidden_state_size), int(hidden_layer_num)
        enc, d = [], reference_obs_size
        for h in encoder_layers:
            enc.append(_Block(d, h)); d = h
        self.encoder = nn.Sequential(*enc)
        self.fc2 = _dense(d, 2 * latents, _lecun_normal_)
        self.decoder_input_size = latents + (obs_size - reference_obs_size)
        self.w_ih, self.w_hh, self.b_hh = nn.ParameterList(), nn.ParameterList(), nn.ParameterList()
        d = self.decoder_input_size
        for _ in range(L):
            wi = torch.empty(4 * H, d)
            _lecun_uniform_(wi)                      # flax lecun_uniform on each [in, H] gate kernel: fan_in = in
            wh = torch.empty(4 * H, H)
            for g in range(4):                       # flax orthogonal() per [H, H] recurrent gate kernel
                nn.init.orthogonal_(wh[g * H:(g + 1) * H])
            self.w_ih.append(nn.Parameter(wi)); self.w_hh.append(nn.Parameter(wh)); self.b_hh.append(nn.Parameter(torch.zeros(4 * H)))
            d = H
        self.projection = _dense(H, 2 * action_size)   # lstm_projection (lecun_uniform, zero bias)

    def zero_carry(self, n: int, device) -> tuple[torch.Tensor, torch.Tensor]:
        shape = (n, self.hidden_layer_num, self.hidden_state_size)
        return torch.zeros(shape, dtype=torch.float32, device=device), torch.zeros(shape, dtype=torch.float32, device=device)

    def _encode(self, obs):
        fc2 = self.fc2(self.encoder(obs[..., :self.reference_obs_size]))
        x = torch.cat([fc2[..., :self.latents], obs[..., self.reference_obs_size:]], dim=-1)   # z = latent_mean
        return fc2, x

    def forward(self, obs: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor, reset: torch.Tensor | None = None):
        """The loss's sequence pass (losses.py scan_policy_fn).  obs [T, B, W] normalised, h0 / c0 [B, L, H] (data), reset [T, B]: non-zero = the
        carry is zeroed BEFORE step t.  Returns (logits [T, B, 2 nu], fc2 = latent mean | logvar [T, B, 2 latents])."""
        T, B = obs.shape[:2]
        fc2, x = self._encode(obs)
        for k in range(self.hidden_layer_num):
            w_i, w_h, b_h = self.w_ih[k], self.w_hh[k], self.b_hh[k]
            if obs.is_cuda:
                # the input part of every step's gates as one GEMM; layer 0: only the latent columns of the input need a gradient
                xg = _HipDenseFn.apply(x.reshape(T * B, -1), w_i, None, self.latents if k == 0 else None).view(T, B, -1)
                x = _LstmSeqFn.apply(xg, w_h, b_h, h0[:, k], c0[:, k], reset)
            else:
                x = _torch_lstm_layer(x @ w_i.t(), w_h, b_h, h0[:, k], c0[:, k], reset)[0]
        return self.projection(x), fc2

    @torch.no_grad()
    def step(self, obs: torch.Tensor, h: torch.Tensor, c: torch.Tensor, reset: torch.Tensor | None = None):
        """One acting step (acting.py actor_step): obs [n, W] normalised; the carry h / c [n, L, H] is read (zeroed first where `reset` [n] is set)
        and overwritten with the new carry in place.  Returns (logits [n, 2 nu], fc2 [n, 2 latents])."""
        fc2, x = self._encode(obs)
        for k in range(self.hidden_layer_num):
            w_i, w_h, b_h = self.w_ih[k], self.w_hh[k], self.b_hh[k]
            if obs.is_cuda:
                from .networks import gemm_nt
                xg = gemm_nt(x, w_i).view(1, x.shape[0], -1)
                hk, ck = h[:, k], c[:, k]
                lstm_seq_fwd(xg, w_h, b_h, hk, ck, None if reset is None else reset.view(1, -1), out_h=hk.unsqueeze(0), out_c=ck.unsqueeze(0))
                x = hk
            else:
                hn, cn = _torch_lstm_layer((x @ w_i.t()).unsqueeze(0), w_h, b_h, h[:, k], c[:, k], None if reset is None else reset.view(1, -1))
                h[:, k].copy_(hn[0]); c[:, k].copy_(cn[0])
                x = h[:, k]
        return self.projection(x), fc2


class CarriedPolicy:
    """An acting policy with its own [n, L, H] carry (acting.py:113-175, the evaluator / make_policy): call(obs, *, done=None) acts and carries;
    `done` = the env's done flags of the step that produced `obs` (the carry of those envs is zeroed first); reset_carry() starts over."""

    def __init__(self, learner, deterministic: bool = False, gen: torch.Generator | None = None):
        self.learner, self.deterministic, self.gen = learner, deterministic, gen
        self.h = self.c = None

    def reset_carry(self) -> None:
        self.h = self.c = None

    def __call__(self, obs: torch.Tensor, *, done: torch.Tensor | None = None):
        if done is not None and (not torch.is_tensor(done) or done.shape != obs.shape[:1] or not done.is_floating_point()):
            raise ValueError("CarriedPolicy: done must be the env's float done flags [n] of the step that produced obs")
        if self.h is None or self.h.shape[0] != obs.shape[0]:
            self.h, self.c = self.learner.policy.zero_carry(obs.shape[0], self.learner.dev)
        return self.learner.act_carried(obs, self.h, self.c, reset=done, deterministic=self.deterministic, gen=self.gen)


class LSTMPPOLearner(PPOLearner):
    """PPOLearner with the LSTM-decoder policy: its own roll-out (carry), SGD step (sequence pass from the stored carry, plain KL) and
    normaliser order.  Eager launches (no hipGraph capture); fp32 only."""

    def __init__(self, env, *, hidden_state_size: int = 128, hidden_layer_num: int = 2, **kw):
        check_lstm_config(hidden_state_size, hidden_layer_num, kw.get("matmul_dtype"))
        self.hidden_state_size, self.hidden_layer_num = int(hidden_state_size), int(hidden_layer_num)
        kw["use_graph"] = False
        super().__init__(env, **kw)
        if self.dev.type != "cuda":
            raise _hip.TmjxError("the LSTM learner runs on the GPU only (tmjx_lstm_seq_fwd / _bwd, tmjx_ppo_loss); there is no CPU fallback")
        self._streams = None                 # one stream: the groups' acting steps and env steps run in order
        self.h_carry, self.c_carry = self.policy.zero_carry(self.n_local, self.dev)
        self._pending_reset = torch.zeros(self.n_local, dtype=torch.float32, device=self.dev)   # done flags not yet applied to the carry
        rows = self.unrolls * self.n_local
        self.h0_store, self.c0_store = self.policy.zero_carry(rows, self.dev)

    def freeze_decoder(self, policy_tree=None, normalizer_tree=None) -> dict:
        raise NotImplementedError("freeze_decoder: the LSTM learner has no frozen-decoder training (the reference's lstm_ppo/ppo.py has none)")

    def _build_policy(self, obs, ref, action_size, latents, encoder_layers, decoder_layers):
        return LSTMIntentionPolicy(obs, ref, action_size, latents, encoder_layers, self.hidden_state_size, self.hidden_layer_num)

    # ---- acting
    @torch.no_grad()
    def settle_carry(self) -> None:
        """Apply the pending resets (the done flags of the last env step) to the roll-out carry: afterwards it is exactly the reference's
        TrainingState.hidden_state (what is checkpointed, what the next unroll stores as its t = 0 carry)."""
        keep = (1.0 - self._pending_reset)[:, None, None]
        self.h_carry.mul_(keep); self.c_carry.mul_(keep)
        self._pending_reset.zero_()

    @torch.no_grad()
    def act_carried(self, obs, h, c, reset=None, deterministic: bool = False, gen: torch.Generator | None = None):
        """One policy step on the carry (h, c) [n, L, H] (updated in place); `reset` [n]: zero the carry of these envs first."""
        gen = self.gen if gen is None else gen
        x = self.normalizer.normalize(obs) if self.normalize_observations else obs
        logits, fc2 = self.policy.step(x.contiguous(), h, c, reset)
        mean, logvar = torch.chunk(fc2, 2, dim=-1)
        if deterministic:
            return NormalTanh.mode(logits), {"latent_mean": mean, "latent_logvar": logvar}
        n, A = logits.shape[0], self.policy.action_size
        f32 = dict(dtype=torch.float32, device=self.dev)
        raw, action_t, logp = torch.empty((n, A), **f32), torch.empty((A, n), **f32), torch.empty(n, **f32)
        rs = self._act_rng_state(gen)          # the acting noise from the generator's device-side Philox stream (as the MLP learner's default)
        with torch.cuda.device(self.dev):
            _hip.check(_hip.lib().tmjx_sample_action(_vp(logits), None, _vp(raw), _vp(action_t), _vp(logp), n, A, rs[1], _vp(rs[0]), _stream(self.dev)),
                       "tmjx_sample_action")
        return action_t.t(), {"raw_action": raw, "log_prob": logp, "logits": logits, "latent_mean": mean, "latent_logvar": logvar}

    def act(self, obs: torch.Tensor, deterministic: bool = False, gen: torch.Generator | None = None, draws=None):
        """A carry-free call (a fresh zero carry): the recurrent policy's state lives in CarriedPolicy / the roll-out carry."""
        if draws is not None:
            raise ValueError("the LSTM learner draws its acting noise on the device only")
        h, c = self.policy.zero_carry(obs.shape[0], self.dev)
        return self.act_carried(obs, h, c, deterministic=deterministic, gen=gen)

    @torch.no_grad()
    def collect(self) -> None:
        T, n_local = self.T, self.n_local
        offs = [0]
        for e in self.envs:
            offs.append(offs[-1] + e.num_envs)
        for u in range(self.unrolls):
            self.settle_carry()
            rows_u = slice(u * n_local, (u + 1) * n_local)
            self.h0_store[rows_u].copy_(self.h_carry)          # the carry every row of this unroll starts from (Transition extras at t = 0)
            self.c0_store[rows_u].copy_(self.c_carry)
            for t in range(T):
                for g, env in enumerate(self.envs):
                    sl = slice(u * n_local + offs[g], u * n_local + offs[g + 1])
                    gl = slice(offs[g], offs[g + 1])
                    st = self.states[g]
                    if u == 0 and t == 0:
                        self.buf["observation"][0, sl] = st.obs
                    action, extra = self.act_carried(st.obs, self.h_carry[gl], self.c_carry[gl], reset=None if t == 0 else self._pending_reset[gl],
                                                     gen=self.gens[g])
                    st = env.step(st, action)
                    nxt = self.buf["observation"][t + 1, sl] if t + 1 < T else self.buf["next_observation_last"][sl]
                    nxt1 = self.buf["observation"][0, slice(sl.start + n_local, sl.stop + n_local)] if (t + 1 == T and u + 1 < self.unrolls) else None
                    self._store_transition(env, st, extra, nxt, nxt1, t, sl, None)
                    self._pending_reset[gl].copy_(st.done)          # zeroes these envs' carry in front of the next step
                    self.states[g] = st

    # ---- learning
    def sequence_outputs(self, idx: torch.Tensor, zero_h0: bool = False):
        """The loss's sequence pass over the roll-out rows `idx` from their stored t = 0 carry: (data, logits, fc2, baseline).  `zero_h0`: start
        from a zero carry instead (a control for tests)."""
        data = self._mb_data(idx)
        obs = data["observation_normalized"] if "observation_normalized" in data else self.normalizer.normalize(data["observation"])
        h0, c0 = self.h0_store.index_select(0, idx), self.c0_store.index_select(0, idx)
        if zero_h0:
            h0, c0 = torch.zeros_like(h0), torch.zeros_like(c0)
        disc = data["discount"]
        reset = torch.zeros_like(disc)
        reset[1:] = 1.0 - disc[:-1]          # the scan zeroes the carry after step t where 1 - discount[t]: i.e. before step t + 1
        logits, fc2 = self.policy(obs, h0, c0, reset)
        return data, obs, logits, fc2

    def lstm_loss(self, idx: torch.Tensor, kl_w: float, noise: torch.Tensor | None = None):
        """The minibatch loss of the rows `idx` with autograd: (total, the five METRIC_KEYS terms, fc2).  `noise`: the entropy sample (default:
        drawn from the learner's generator)."""
        data, obs, logits, fc2 = self.sequence_outputs(idx)
        baseline = self.value(obs)
        with torch.no_grad():
            nxt = data["next_observation_last_normalized"] if "next_observation_last_normalized" in data else self.normalizer.normalize(data["next_observation_last"])
            bootstrap = self.value(nxt)
            if noise is None:
                noise = torch.randn(data["raw_action"].shape, generator=self.gen, dtype=torch.float32, device=self.dev)   # entropy sample
        # the MLP learner's loss head for everything but the latent KL (kl_weight 0 there), the plain KL next to it (losses.py:105-297)
        cfg = dict(self.hp, kl_weight=0.0, normalize_advantage=True)
        head, out = _losses._FusedLossHead.apply(logits, baseline, fc2, data["raw_action"], data["log_prob"], noise, bootstrap, data["reward"],
                                                 data["discount"], data["truncation"], cfg)
        kl = kl_w * plain_kl(fc2)
        kld = kl.detach()
        return head + kl, torch.stack([out[0] + kld, out[1], out[2], kld, out[3]]), fc2      # METRIC_KEYS order

    def _lstm_minibatch_grads(self, idx: torch.Tensor, kl_w: float) -> torch.Tensor:
        total, metrics, _ = self.lstm_loss(idx, kl_w)
        self.grads.assign(torch.autograd.grad(total, self.grads.params))
        return metrics

    def update(self, it: int = 0, kl_schedule=None) -> dict:
        """SGD epochs with the normaliser of the roll-out, THEN the normaliser update (lstm_ppo/ppo.py:425-453).  No KL schedule."""
        kl_w = self.kl_weight
        rows = self.buf["reward"].shape[1]
        acc = torch.zeros(len(self.METRIC_KEYS), dtype=torch.float32, device=self.dev)
        for upd in range(self.num_updates):
            perm = torch.randperm(rows, generator=self.gen, device=self.dev) if self.perm_fn is None else self.perm_fn(upd, rows).to(self.dev)
            for mb in range(self.num_minibatches):
                acc += self._lstm_minibatch_grads(perm[mb * self.local_batch:(mb + 1) * self.local_batch], kl_w)
                self.grads.all_reduce_mean(self.group, force=self.collectives)
                self.opt.step()
        if self.normalize_observations:
            self.normalizer.update(self.buf["observation"], group=self.group, distributed=self.collectives)
        acc = acc / (self.num_updates * self.num_minibatches)
        res = {k: acc[i] for i, k in enumerate(self.METRIC_KEYS)}
        res["kl_weight"] = torch.as_tensor(kl_w)
        return res


def plain_kl(fc2: torch.Tensor) -> torch.Tensor:
    """-0.5 mean(1 + logvar - mean^2 - exp(logvar)) over every row and latent (lstm_ppo/losses.py:281-285)."""
    mean, logvar = torch.chunk(fc2, 2, dim=-1)
    return -0.5 * torch.mean(1 + logvar - mean * mean - torch.exp(logvar))
