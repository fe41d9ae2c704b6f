"""wrappers.wrap mirror (reference: track_mjx/environment/wrappers.py:18-56).

In the reference `wrap` stacks brax's EpisodeWrapper and VmapWrapper and then the
(LSTM)AutoResetWrapperTracking.  Here batching is native and the episode / auto-reset logic runs
inside the K3 kernel (csrc/env_core.h: tm_step_prologue / tm_step_post), so `wrap` only switches
those semantics on for the env's handle and returns the env itself.  `action_repeat` is brax EpisodeWrapper's: the env's own step
runs that many times per `step` with the same action, rewards summed, the step counter advanced by `action_repeat`
(include/tmjx.h: tmjx_set_action_repeat).

AutoAlignWrapperTracking (wrappers.py:328-381) and EvalClipWrapperTracking (wrappers.py:313-325) are the evaluation-side wrappers: the first
switches the handle to the align done-policy (include/tmjx.h: tmjx_set_done_policy; csrc/wave_align.h), the second pins reset to a clip's frame 0.

HighLevelWrapper (wrappers.py:384-412) puts a pretrained decoder INSIDE the env: step(state, latents) takes an intention vector per env instead of
joint controls.  With a DecoderPolicy (agent/checkpoint.py: make_decoder_policy_fn) the decoder runs as launches on the env's own device buffers —
one fused launch (include/tmjx.h: tmjx_decoder_act) where the decoder qualifies, else the roll-out policy step's decoder half, layer by layer.
With an LSTMDecoderPolicy (make_lstm_decoder_policy_fn) the wrapper also owns the decoder's carry (h, c) [n, L, H]; the launches are the LSTM
roll-out step's decoder half, or one tmjx_lstm_decoder_act launch.  Both policy kinds run through one _DecoderStep; its layer-by-layer list is built by
agent/launch_list.py, the builder of the roll-out's own policy step.
"""
from __future__ import annotations

import ctypes as C

from .task import MultiClipTracking


def wrap(env: MultiClipTracking, episode_length: int = 1000, action_repeat: int = 1, randomization_fn=None,
         use_lstm: bool = True, hidden_state_dim: int = 128, hidden_layer_num: int = 2) -> MultiClipTracking:
    """Episode (steps/truncation) + auto-reset semantics (wrappers.py:104-144, brax EpisodeWrapper).

    `use_lstm`, `hidden_state_dim`, `hidden_layer_num` are accepted for signature parity: the LSTM
    auto-reset wrapper differs from the plain one only by an unused `info["hidden_state"]`
    (wrappers.py:59-144 vs 278-310), which is not materialised."""
    env.configure_wrappers(int(episode_length), auto_reset=True, action_repeat=int(action_repeat))
    if randomization_fn is not None:
        # brax's DomainRandomizationVmapWrapper (wrappers.py:44-47) steps every env with its own copy of the mjx.Model; the physics kernel reads
        # ONE model from constant memory (csrc/dmodel.h) plus three per-env SCALARS and the env's gravity (csrc/tmjx_wave_rand.hip): randomization_fn(model) returns a
        # DomainRandomization (environment/randomization.py); a per-env model raises NotImplementedError
        from .randomization import apply_randomization_fn
        apply_randomization_fn(env, randomization_fn)
    return env


def AutoAlignWrapperTracking(env: MultiClipTracking, episode_length: int = 1000, action_repeat: int = 1, randomization_fn=None) -> MultiClipTracking:
    """Align-on-failure tracking (wrappers.py:328-381) with brax EpisodeWrapper's step counter / truncation underneath it, in the style of `wrap`:
    the handle is switched to the align done-policy and the env itself is returned.  An env whose step ends with done set (terminated or truncated
    at `episode_length`) is put onto the reference pose and velocities of the clip frame it has reached — kinematics and a fresh observation
    included, inside the same `step` — and tracking goes on; `state.done` of that step counts one re-alignment.  time is not rewound and
    prev_ctrl is not restored.  With `action_repeat` > 1 the alignment follows the last inner step.  Needs the clip set's velocity and
    joints_velocity (a ValueError / TmjxError otherwise).  `randomization_fn`: as in `wrap` (per-env scales; the alignment itself is kinematics and reads none)."""
    if not isinstance(env, MultiClipTracking):
        raise TypeError(f"AutoAlignWrapperTracking wraps a MultiClipTracking env, not {type(env).__name__}")
    if int(episode_length) < 1:
        raise ValueError("episode_length must be >= 1")
    if int(action_repeat) < 1:
        raise ValueError("action_repeat must be >= 1")
    env.configure_wrappers(int(episode_length), auto_reset=False, action_repeat=int(action_repeat), done_policy="align")
    if randomization_fn is not None:
        from .randomization import apply_randomization_fn
        apply_randomization_fn(env, randomization_fn)
    return env


class EvalClipWrapperTracking:
    """reset at frame 0 of a given clip (wrappers.py:313-325: reset_from_clip(rng, {clip_idx, start_frame: 0}, noise=False)); everything else is
    the wrapped env's.  As in the reference, noise=False zeroes the qvel noise ONLY: the qpos noise U(-reset_noise_scale, +reset_noise_scale) is
    still drawn and added (single_clip_tracking.py:153-161)."""

    def __init__(self, env: MultiClipTracking):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, rng=None, clip_idx=None):
        import torch
        e = self.env
        n = e.num_envs
        if clip_idx is None:
            raise ValueError("EvalClipWrapperTracking.reset needs clip_idx (an int for every env, or one per env)")
        ci = torch.as_tensor(clip_idx, dtype=torch.int32).reshape(-1)
        if ci.numel() == 1:
            ci = ci.expand(n).contiguous()
        if ci.numel() != n:
            raise ValueError(f"clip_idx must be one int or {n} of them")
        if int(ci.min()) < 0 or int(ci.max()) >= max(e._n_clips, 1):
            raise IndexError(f"clip_idx outside the table's {e._n_clips} clips")
        return e.reset(rng, ci, start_frame=torch.zeros(n, dtype=torch.int32), qvel_noise=torch.zeros((int(e.layout.nv), n)))


def _same_device(a, b) -> bool:
    import torch
    a, b = torch.device(a), torch.device(b)
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return True
    cur = torch.cuda.current_device() if (a.index is None or b.index is None) else 0
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


def _is_lstm(dp) -> bool:
    from ..agent.checkpoint import LSTMDecoderPolicy
    return isinstance(dp, LSTMDecoderPolicy)


def _fused_desc(dp, obs_w: int, n: int, p, **addr):
    """(entry point, descriptor) of the fused launch of a decoder policy on observations `obs_w` wide for `n` envs.  p(tensor, pad=False): the address
    the kernel reads one of the policy's tensors at (pad: as a copy with rows padded to ceil4 columns); addr: the other pointer fields, by name."""
    from .. import hip as _hip
    from ..agent.launch_list import ceil4
    lstm = _is_lstm(dp)
    d = (_hip.LstmDecoderAct if lstm else _hip.DecoderAct)()
    d.ldz, d.obs_s0, d.obs_s1 = dp.latent_size, 1, n
    d.n, d.Z, d.obs_w, d.ref_w, d.A = n, dp.latent_size, int(obs_w), dp.reference_obs_size, dp.action_size
    if lstm:
        d.L, d.H = dp.hidden_layer_num, dp.hidden_state_size
        for y, wi, wh, bh in zip(d.layer, dp.w_ih, dp.w_hh, dp.b_hh):       # (zip stops at the descriptor's 4 layers: a deeper decoder is refused by L)
            y.Wi, y.Wh, y.bh, y.ldwi, y.ldwh = p(wi, True), p(wh), p(bh), ceil4(wi.shape[1]), d.H
        d.Wp, d.bp, d.ldwp, d.ld = p(dp.w_p, True), p(dp.b_p), ceil4(d.H), d.L * d.H
    else:
        net = dp.net
        d.n_blocks = len(net.decoder)
        for b, blk in zip(d.block, net.decoder):                              # (likewise: refused by n_blocks)
            w = blk.dense.weight
            b.W, b.bias, b.gamma, b.beta, b.width, b.ldw = p(w, True), p(blk.dense.bias), p(blk.norm.weight), p(blk.norm.bias), w.shape[0], ceil4(w.shape[1])
        d.Wf, d.bf, d.ldwf = p(net.head.weight, True), p(net.head.bias), ceil4(net.head.weight.shape[1])
        d.eps = float(net.decoder[0].norm.eps) if d.n_blocks else 0.0
    for name, a in addr.items():
        setattr(d, name, a)
    return ("tmjx_lstm_decoder_act" if lstm else "tmjx_decoder_act"), d


def decoder_act_why_not(dp, obs_w: int, n: int = 1) -> str | None:
    """None if the fused launch (tmjx_decoder_act; tmjx_lstm_decoder_act for an LSTMDecoderPolicy) runs this decoder, else the library's reason
    (tmjx_*_decoder_act_ok on the descriptor the step would launch, every address a dummy: `dp` is a DecoderPolicy or an LSTMDecoderPolicy)."""
    from .. import hip as _hip
    a = 1 << 20                  # a non-null, 16-byte aligned dummy address: the check reads shapes and alignments, never memory
    carry = dict(h=a, c=a) if _is_lstm(dp) else {}
    entry, d = _fused_desc(dp, obs_w, n, lambda t, pad=False: a, latents=a, obs=a, action_t=a, **carry)
    L = _hip.lib()
    if getattr(L, entry + "_ok")(C.byref(d)) == 1:
        return None
    getattr(L, entry)(C.byref(d), None)          # (refused before any device call: records the reason)
    return L.tmjx_last_error().decode()


lstm_decoder_act_why_not = decoder_act_why_not


class _DecoderStep:
    """Preallocated buffers and the launch list of a decoder policy for `n` envs reading the env's raw observation buffer obs_soa [W][n] and writing
    the action as [nu][n] rows (what tmjx_step takes).  For an LSTMDecoderPolicy the carry h, c [n, L, H] lives here and is updated in place by the
    launches; `reset` (the env's done buffer [n], or None) zeroes a row's carry of every layer before the step.

    path "layers": tmjx_decoder_input (tmjx_latent_concat_det's kernel, for latents [n][ldz >= Z]), then the decoder half of the roll-out's policy step
    (agent/launch_list.py, which analysis.rollout._PolicyStep builds from too): its kernels, operand layouts and therefore its bits.
    path "fused": one tmjx_decoder_act / tmjx_lstm_decoder_act launch.

    `intervention` (analysis.intervene.Intervention) with `gates` = (window [n, 2], dose [n]), layers path only: one tmjx_intervene call directly
    behind the launch that produces its target (intention, decoder/layer_<i>, hidden_state/h:<k>)."""

    def __init__(self, dp, n: int, obs_soa, path: str, reset=None, intervention=None, gates=None):
        from ..agent.launch_list import LaunchList, ceil4, ptr
        ll = self.ll = LaunchList(n, dp.device)
        lstm = _is_lstm(dp)
        Z, prop, A, ref = dp.latent_size, dp.proprioceptive_obs_size, dp.action_size, dp.reference_obs_size
        W = int(obs_soa.shape[0])
        # the normaliser as tmjx_latent_concat_det / the fused launches index it: by observation column (the reference columns are never read)
        mean = std = None
        if dp.mean is not None:
            mean, std = ll.buf(W, zero=True), ll.buf(W).fill_(1.0)
            mean[ref:].copy_(dp.mean); std[ref:].copy_(dp.std)
        carry = {}
        self.h = self.c = self.desc = None
        if lstm:
            self.h, self.c = (ll.buf(n, dp.hidden_layer_num, dp.hidden_state_size, zero=True) for _ in range(2))
            carry = dict(h=ptr(self.h), c=ptr(self.c), reset=ptr(reset))
        if path == "fused":
            self.ctrl, self.action_t = ll.buf(n, A), ll.buf(A, n)
            ll.keep.append(reset)              # (the layers path: lstm_layers keeps it)

            def p(t, pad=False):
                t = ll.pad(t) if pad else t.detach().contiguous()
                ll.keep.append(t)
                return t.data_ptr()
            entry, self.desc = _fused_desc(dp, W, n, p, obs=ptr(obs_soa), mean=ptr(mean), std=ptr(std), action_t=ptr(self.action_t), ctrl=ptr(self.ctrl), **carry)
            ll.call(entry, C.byref(self.desc))
        else:
            x = ll.buf(n, ceil4(Z + prop), zero=True)
            ll.call("tmjx_decoder_input", None, None, ptr(obs_soa), 1, n, ptr(mean), ptr(std), ptr(x), x.shape[1], n, Z, W, ref)
            if lstm:
                out = ll.decoder(x, (), dp.w_p, dp.b_p, lstm=(dp.w_ih, dp.w_hh, dp.b_hh, self.h, self.c, reset))
            else:
                out = ll.decoder(x, dp.net.decoder, dp.net.head.weight, dp.net.head.bias)
            self.ctrl, self.action_t = out[2:]
        self.iv_entry = self.iv = None
        if intervention is not None:
            if path == "fused":
                raise ValueError("an intervention needs path='layers': the fused decoder launch has no seam between its layers")
            layers = {f"decoder/layer_{i}": y for i, y in enumerate(out[0])}
            self.iv_entry, self.iv = ll.place_intervention(intervention, gates[0], gates[1], x, Z, layers, self.h)

    def launch(self, lat_ptr: int, ldz: int, stream, t: int = 0) -> None:
        """The decoder's launches on `stream` (ctypes calls only: no torch operation); `t`: the control-step index an intervention's gate sees."""
        if self.iv_entry is not None:
            self.iv_entry[1][1] = t
        if self.desc is not None:
            self.desc.latents, self.desc.ldz = lat_ptr, ldz
        else:
            self.ll.calls[0][1][:2] = lat_ptr, ldz
        self.ll.run(stream)


class HighLevelWrapper:
    """step(state, latents): the decoder's action on concat([latents, state.obs[..., reference_obs_size:]]) drives the wrapped env
    (wrappers.py:384-412); reset and everything else are the wrapped env's, so it composes with wrap / AutoAlignWrapperTracking /
    EvalClipWrapperTracking.  action_size is the latent width.

    decoder_inference_fn: a DecoderPolicy on the env's device runs as launches on the env's buffers — after the first call `step` issues ctypes
    calls only (no torch op, no allocation, no host synchronisation) and returns the same State object, whose tensors are views of the buffers
    the kernels update in place.  `path`: "fused" (one tmjx_decoder_act launch; ValueError if the decoder does not qualify), "layers" (the
    roll-out policy step's decoder half, any decoder shape), "auto" (fused where tmjx_decoder_act_ok says so AND AUTO_PREFERS_FUSED, else layers).
    Any other callable fn(x) -> (action, extras) is called on the torch concat, as the reference does.

    An LSTMDecoderPolicy (agent.checkpoint.make_lstm_decoder_policy_fn) runs the same way; the wrapper then owns its carry (h, c) [n, L, H]: zeroed
    by reset(), read with `hidden_state`, set with set_hidden_state(h, c).  reset_carry_on_done (LSTMAutoResetWrapperTracking's semantics, what the
    roll-out's policy step does under align_on_fail): the env's done flags of the previous step go to the decoder as `reset`, so an env that ended
    and was reset or aligned starts from a zero carry; False: the carry is never reset by the wrapper.  "layers" is the LSTM roll-out step's decoder
    half, "fused" one tmjx_lstm_decoder_act launch, "auto" follows AUTO_PREFERS_FUSED_LSTM."""

    # "auto" takes the fused launch only once tools/decoder_act_bench.py has shown it faster than the layer-by-layer list at 4 096 AND 8 192 envs by
    # more than the spread of the alternating repeats.  That measurement has not been taken yet: "auto" means "layers", the fused
    # launch is selected with path="fused"
    AUTO_PREFERS_FUSED = False
    # the same rule for the LSTM decoder's fused launch, and that measurement HAS been taken (tools/lstm_decoder_act_bench.py,
    # profiles/lstm_decoder_act_bench.txt): 94.2 against 114.1 us per decoder step at 4 096 envs and 101.6 against 192.6 at 8 192,
    # the alternating repeats within 0.2 us of each other — "auto" takes tmjx_lstm_decoder_act where tmjx_lstm_decoder_act_ok says so
    AUTO_PREFERS_FUSED_LSTM = True

    def __init__(self, env, decoder_inference_fn, reference_obs_size: int, path: str = "auto", reset_carry_on_done: bool = True, intervention=None):
        """`intervention` (analysis.intervene.Intervention; its window / dose: one value, or one per env): the decoder runs with its edit, one more
        launch of the "layers" list; step counts the control steps since reset() for its gate.  path="fused" then raises (the fused launches have
        no seam) and path="auto" takes "layers"."""
        from ..agent.checkpoint import DecoderPolicy, LSTMDecoderPolicy
        if path not in ("auto", "fused", "layers"):
            raise ValueError(f"HighLevelWrapper: path must be 'auto', 'fused' or 'layers', not {path!r}")
        if intervention is not None:
            if path == "fused":
                raise ValueError("HighLevelWrapper: path='fused' cannot run an intervention: the fused decoder launch has no seam between its layers; "
                                 "use path='layers' (or 'auto', which takes it)")
            if not isinstance(decoder_inference_fn, (DecoderPolicy, LSTMDecoderPolicy)):
                raise ValueError("HighLevelWrapper: an intervention needs a DecoderPolicy / LSTMDecoderPolicy (the launch-list path)")
            path = "layers"
        self._intervention, self._t = intervention, 0
        if not callable(decoder_inference_fn):
            raise TypeError("HighLevelWrapper: decoder_inference_fn must be a DecoderPolicy or a callable fn(x) -> (action, extras)")
        self.env, self._fn, self._ref = env, decoder_inference_fn, int(reference_obs_size)
        W = int(env.observation_size)
        if not 0 <= self._ref <= W:
            raise ValueError(f"HighLevelWrapper: reference_obs_size {self._ref} outside the observation's {W} columns")
        self._step = self._state = None
        self.path = "callable"
        self._lstm = isinstance(decoder_inference_fn, LSTMDecoderPolicy)
        self.reset_carry_on_done = bool(reset_carry_on_done)
        self._h = self._c = None              # the callable path's carry (the device paths keep theirs in the launch list's buffers)
        if isinstance(decoder_inference_fn, (DecoderPolicy, LSTMDecoderPolicy)):
            dp = decoder_inference_fn
            if dp.reference_obs_size != self._ref:
                raise ValueError(f"HighLevelWrapper: reference_obs_size={self._ref}, but the decoder policy was built for {dp.reference_obs_size}")
            if dp.proprioceptive_obs_size != W - self._ref:
                raise ValueError(f"HighLevelWrapper: the env has {W - self._ref} proprioceptive columns, the decoder policy takes {dp.proprioceptive_obs_size}")
            if dp.action_size != int(env.action_size):
                raise ValueError(f"HighLevelWrapper: the decoder policy acts on {dp.action_size} controls, the env takes {int(env.action_size)}")
            self._Z = dp.latent_size
            import torch
            if hasattr(env, "obs_buf") and dp.device.type == "cuda" and _same_device(env.device, dp.device):
                why = decoder_act_why_not(dp, W, int(env.num_envs))
                if self._lstm:
                    shape, prefers = f"LSTM decoder (L = {dp.hidden_layer_num}, H = {dp.hidden_state_size})", self.AUTO_PREFERS_FUSED_LSTM
                else:
                    shape, prefers = f"decoder {list(dp.decoder_layer_sizes)}", self.AUTO_PREFERS_FUSED
                if path == "fused" and why is not None:
                    raise ValueError(f"HighLevelWrapper: path='fused' does not run this {shape}: {why}")
                self.path = "fused" if path == "fused" or (path == "auto" and why is None and prefers) else "layers"
            elif path != "auto":
                raise ValueError(f"HighLevelWrapper: path={path!r} needs the decoder policy on the env's device ({getattr(env, 'device', None)}), it is on {dp.device}")
        else:
            if path != "auto":
                raise ValueError(f"HighLevelWrapper: path={path!r} needs a DecoderPolicy (agent.checkpoint.make_decoder_policy_fn); a generic callable runs "
                                 "through torch")
            self._Z = None

    def __getattr__(self, name):
        return getattr(self.env, name)

    @property
    def action_size(self) -> int:
        if self._Z is None:
            raise AttributeError("HighLevelWrapper.action_size: a generic callable does not say its latent width")
        return self._Z

    @property
    def observation_size(self) -> int:
        return int(self.env.observation_size)

    def reset(self, *a, **kw):
        self._state = None
        self._h = self._c = None
        self._t = 0
        if self._lstm and self._step is not None:
            self._step.h.zero_(); self._step.c.zero_()
        return self.env.reset(*a, **kw)

    def _carry(self):
        if not self._lstm:
            raise TypeError("HighLevelWrapper: only an LSTMDecoderPolicy carries a hidden state")
        if self.path == "callable":
            if self._h is None:
                self._h, self._c = self._fn.zero_carry(int(self.env.num_envs), getattr(self.env, "device", None))
            return self._h, self._c
        if self._step is None:
            self._make_step()
        return self._step.h, self._step.c

    @property
    def hidden_state(self):
        """(h, c) [n, L, H] of the LSTM decoder: views of the buffers the next step reads and overwrites."""
        return self._carry()

    def set_hidden_state(self, h, c) -> None:
        hh, cc = self._carry()
        if tuple(h.shape) != tuple(hh.shape) or tuple(c.shape) != tuple(cc.shape):
            raise ValueError(f"HighLevelWrapper.set_hidden_state: h and c must be {tuple(hh.shape)}")
        hh.copy_(h); cc.copy_(c)

    def _make_step(self) -> None:
        import torch
        env, n = self.env, int(self.env.num_envs)
        with torch.cuda.device(env.device):
            iv = self._intervention
            self._step = _DecoderStep(self._fn, n, env.obs_buf, self.path, env.done_buf if self._lstm and self.reset_carry_on_done else None,
                                      intervention=iv, gates=None if iv is None else iv.per_clip(n))
        p = lambda t: t.data_ptr()      # noqa: E731
        self._env_args = (env._handle, p(env.state_buf), p(env.istate_buf), p(self._step.action_t), p(env.obs_buf), p(env.reward_buf), p(env.done_buf),
                          p(env.trunc_buf), p(env.metrics_buf), p(env.workspace), n)

    def _check_latents(self, latents):
        n = int(self.env.num_envs)
        if latents.dim() != 2 or latents.shape[0] != n:
            raise ValueError(f"HighLevelWrapper.step: latents must be [{n}, Z] (one row per env), got {tuple(latents.shape)}")
        if self._Z is not None and latents.shape[1] != self._Z:
            raise ValueError(f"HighLevelWrapper.step: latents have {latents.shape[1]} columns, the decoder's intention size is {self._Z}")

    def step(self, state, latents, t: int | None = None):
        """`t`: the control-step index an intervention's gate sees (default: the steps taken since reset())."""
        self._check_latents(latents)
        if t is not None:
            self._t = int(t)
        env = self.env
        if self.path == "callable":
            import torch
            x = torch.cat([latents.to(state.obs.device), state.obs[..., self._ref:]], dim=-1)
            if self._lstm:
                done = getattr(state, "done", None) if self.reset_carry_on_done else None
                action, _, (self._h, self._c) = self._fn(x, hidden_state=self._carry(), reset=done)
            else:
                action, _ = self._fn(x)
            return env.step(state, action)
        import torch
        if latents.device.type != "cuda" or (latents.device.index is not None and self._fn.device.index is not None
                                             and latents.device.index != self._fn.device.index):
            raise ValueError(f"HighLevelWrapper.step: latents are on {latents.device}, the env and its decoder on {self._fn.device}")
        if latents.dtype != torch.float32 or latents.stride(1) != 1 or latents.stride(0) < latents.shape[1] or latents.data_ptr() % 4:
            latents = latents.to(torch.float32).contiguous()
        n = int(env.num_envs)
        if self._step is None:
            self._make_step()
        if self._state is None:
            self._state = env._state()
        if getattr(env, "_physics_events", None) is not None:
            raise RuntimeError("HighLevelWrapper: the K2-bracketing measurement mode steps the plain env")
        with torch.cuda.device(env.device):
            stream = C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
            self._step.launch(latents.data_ptr(), latents.stride(0), stream, self._t)
            self._step.ll.hip.check(self._step.ll.L.tmjx_step(*self._env_args, stream), "tmjx_step")
        self._t += 1
        self._keep_lat = latents
        return self._state

    @property
    def intervention_projection(self):
        """[n, K] view of the pre-edit coordinates of the last device-path step under a subspace intervention (else None)."""
        return None if self._step is None or self._step.iv is None else self._step.iv.proj

    @property
    def last_ctrl(self):
        """[n, A] view of the controls the decoder produced in the last device-path step (None before it)."""
        return None if self._step is None else self._step.ctrl
