#!/usr/bin/env python3
"""Times the decoder policy of a high-level env step (environment/wrappers.py: HighLevelWrapper): the fused launch (tmjx_decoder_act) against the
layer-by-layer launch list it replaces — tmjx_latent_concat_det -> per block tmjx_linear_nolds + tmjx_silu_ln_fwd -> head (tmjx_linear_nolds) ->
tmjx_action_mode, the decoder half of the roll-out's policy step.

Decoder [256, 256], Z = 60, proprioception 226 of 696 observation columns, A = 38; n = 4 096 and 8 192 envs.  Device events around `iters` back-to-back
decoder steps, after a warm-up; `repeats` alternating repeats (layered, fused, layered, fused, ...) per size; one process.

    python tools/decoder_act_bench.py [--sizes 4096,8192] [--iters 200] [--warmup 50] [--repeats 5] [--out profiles/decoder_act_bench.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from track_mjx_amd import hip  # noqa: E402

Z, W, REF, A, WIDTHS = 60, 696, 470, 38, (256, 256)


def build(n: int, dev: str):
    """(layered launch list, fused descriptor, buffers to keep alive, (action_t layered, action_t fused))."""
    g = torch.Generator().manual_seed(n)
    f32 = dict(dtype=torch.float32, device=dev)
    r = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).to(dev)      # noqa: E731
    p = lambda t: None if t is None else t.data_ptr()                           # noqa: E731
    K1 = Z + W - REF
    K1p = (K1 + 3) // 4 * 4
    lat2 = r(n, 2 * Z)                      # the latents in the front of an [n][2Z] buffer: tmjx_latent_concat_det insists on ldf >= 2Z
    obs = (r(W, n, scale=2.0) + 0.5).contiguous()
    mean, std = r(W, scale=0.3), (0.4 + torch.rand(W, generator=g) * 1.5).to(dev)
    keep = [lat2, obs, mean, std]
    x = torch.zeros((n, K1p), **f32)
    calls = [("tmjx_latent_concat_det", (p(lat2), 2 * Z, p(obs), 1, n, p(mean), p(std), p(x), K1p, None, 0, n, Z, W, REF))]
    e = hip.DecoderAct()
    e.latents, e.ldz, e.obs, e.obs_s0, e.obs_s1, e.mean, e.std = p(lat2), 2 * Z, p(obs), 1, n, p(mean), p(std)
    e.n, e.Z, e.obs_w, e.ref_w, e.n_blocks = n, Z, W, REF, len(WIDTHS)
    h, K = x, K1
    for l, N in enumerate(WIDTHS):
        w = torch.zeros((N, (K + 3) // 4 * 4), **f32)
        w[:, :K] = r(N, K, scale=K ** -0.5)
        b, ga, be = r(N, scale=0.05), 1 + r(N, scale=0.05), r(N, scale=0.05)
        z, y, st = torch.empty((n, N), **f32), torch.empty((n, N), **f32), torch.empty((n, 2), **f32)
        keep += [w, b, ga, be, z, y, st]
        calls.append(("tmjx_linear_nolds", (p(h), h.shape[1], 1, p(w), None, p(z), n, N, w.shape[1])))
        calls.append(("tmjx_silu_ln_fwd", (p(z), p(b), p(ga), p(be), p(y), p(st), n, N, 1e-6)))
        blk = e.block[l]
        blk.W, blk.bias, blk.gamma, blk.beta, blk.width, blk.ldw = p(w), p(b), p(ga), p(be), N, w.shape[1]
        h, K = y, N
    wf, bf = r(2 * A, K, scale=0.1 * K ** -0.5), r(2 * A, scale=0.05)
    logits, ctrl, act_l, act_f, ctrl_f = (torch.empty(s, **f32) for s in ((n, 2 * A), (n, A), (A, n), (A, n), (n, A)))
    keep += [x, wf, bf, logits, ctrl, ctrl_f]
    calls.append(("tmjx_linear_nolds", (p(h), h.shape[1], 1, p(wf), p(bf), p(logits), n, 2 * A, K)))
    calls.append(("tmjx_action_mode", (p(logits), 2 * A, p(ctrl), p(act_l), n, A)))
    e.Wf, e.bf, e.ldwf, e.A, e.eps = p(wf), p(bf), K, A, 1e-6
    e.action_t, e.ctrl, e.logits, e.ldl = p(act_f), p(ctrl_f), None, 0          # what the wrapper asks for: the action rows and ctrl
    return calls, e, keep, (act_l, act_f)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("--repeats must be >= 3")
    dev = "cuda:0"
    L = hip.lib()
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines = [f"decoder step, decoder {list(WIDTHS)}, Z = {Z}, prop = {W - REF}, A = {A}; build {hip.build_id()}; {a.iters} steps per timing, "
             f"{a.warmup} warm-up, {a.repeats} alternating repeats; us per decoder step"]
    for n in (int(v) for v in a.sizes.split(",")):
        calls, e, keep, (act_l, act_f) = build(n, dev)
        if L.tmjx_decoder_act_ok(C.byref(e)) != 1:
            raise SystemExit("tmjx_decoder_act_ok refused the benchmark's decoder")

        def layered():
            for name, args in calls:
                hip.check(getattr(L, name)(*args, s), name)

        def fused():
            hip.check(L.tmjx_decoder_act(C.byref(e), s), "tmjx_decoder_act")

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.iters

        for fn in (layered, fused):
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        worst = float((act_l - act_f).abs().max())
        tl, tf = [], []
        for _ in range(a.repeats):
            tl.append(timed(layered)); tf.append(timed(fused))
        med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
        lines.append(f"n = {n:5d}  layered ({len(calls)} launches): median {med(tl):7.1f}  [{min(tl):7.1f} .. {max(tl):7.1f}]   fused (1 launch): median {med(tf):7.1f}  "
                     f"[{min(tf):7.1f} .. {max(tf):7.1f}]   layered / fused {med(tl) / med(tf):5.2f}   max |action difference| {worst:.2e}")
        lines.append("           layered repeats: " + " ".join(f"{v:.1f}" for v in tl) + "   fused repeats: " + " ".join(f"{v:.1f}" for v in tf))
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
