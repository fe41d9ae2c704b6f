#!/usr/bin/env python3
"""Times the LSTM decoder policy of a high-level env step (environment/wrappers.py: HighLevelWrapper with an LSTMDecoderPolicy): the fused launch
(tmjx_lstm_decoder_act) against the layer-by-layer launch list it replaces — tmjx_decoder_input -> per layer tmjx_linear_nolds + tmjx_lstm_seq_fwd
(T = 1) -> projection (tmjx_linear_nolds) -> tmjx_action_mode, the decoder half of the roll-out's LSTM policy step.

H = 128, L = 2, Z = 60, proprioception 226 of 696 observation columns, A = 38; n = 4 096 and 8 192 envs, each carrying its own (h, c) from step to
step.  Device events around `iters` back-to-back decoder steps, after a warm-up; `repeats` alternating repeats (layered, fused, layered, fused, ...)
per size.  Every size runs in a child process of its own under a time limit; the first failure ends the run.  Run it on an otherwise idle device.

    python tools/lstm_decoder_act_bench.py [--sizes 4096,8192] [--iters 200] [--warmup 50] [--repeats 5] [--out profiles/lstm_decoder_act_bench.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

Z, W, REF, A, H, LAYERS = 60, 696, 470, 38, 128, 2


def build(n: int, dev: str):
    """(layered launch list, fused descriptor, buffers to keep alive, (action_t layered, action_t fused))."""
    import torch
    from track_mjx_amd import hip
    g = torch.Generator().manual_seed(n)
    f32 = dict(dtype=torch.float32, device=dev)
    r = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).to(dev)      # noqa: E731
    p = lambda t: None if t is None else t.data_ptr()                           # noqa: E731
    K1 = Z + W - REF
    K1p = (K1 + 3) // 4 * 4
    lat = r(n, Z)
    obs = (r(W, n, scale=2.0) + 0.5).contiguous()
    mean, std = r(W, scale=0.3), (0.4 + torch.rand(W, generator=g) * 1.5).to(dev)
    x, xg = torch.zeros((n, K1p), **f32), torch.empty((n, 4 * H), **f32)
    hl, cl, hf, cf = (torch.zeros((n, LAYERS, H), **f32) for _ in range(4))
    keep = [lat, obs, mean, std, x, xg, hl, cl, hf, cf]
    calls = [("tmjx_decoder_input", (p(lat), Z, p(obs), 1, n, p(mean), p(std), p(x), K1p, n, Z, W, REF))]
    e = hip.LstmDecoderAct()
    e.latents, e.ldz, e.obs, e.obs_s0, e.obs_s1, e.mean, e.std, e.reset = p(lat), Z, p(obs), 1, n, p(mean), p(std), None
    e.n, e.Z, e.obs_w, e.ref_w, e.L, e.H = n, Z, W, REF, LAYERS, H
    a, lda, K = x, K1p, K1
    for k in range(LAYERS):
        wi = torch.zeros((4 * H, (K + 3) // 4 * 4), **f32)
        wi[:, :K] = r(4 * H, K, scale=K ** -0.5)
        wh, bh = r(4 * H, H, scale=H ** -0.5), r(4 * H, scale=0.1)
        hk, ck = hl[:, k], cl[:, k]
        args = hip.LstmFwd(p(xg), 4 * H, p(wh), H, p(bh), p(hk), p(ck), LAYERS * H, None, n, p(hk), p(ck), LAYERS * H, None, None, 1, n, H)
        keep += [wi, wh, bh, args]
        calls.append(("tmjx_linear_nolds", (p(a), lda, 1, p(wi), None, p(xg), n, 4 * H, wi.shape[1])))
        calls.append(("tmjx_lstm_seq_fwd", (C.byref(args),)))
        y = e.layer[k]
        y.Wi, y.Wh, y.bh, y.ldwi, y.ldwh = p(wi), p(wh), p(bh), wi.shape[1], H
        a, lda, K = hk, LAYERS * H, H
    wp, bp = r(2 * A, H, scale=0.1 * H ** -0.5), r(2 * A, scale=0.05)
    logits, ctrl, act_l, act_f, ctrl_f = (torch.empty(s, **f32) for s in ((n, 2 * A), (n, A), (A, n), (A, n), (n, A)))
    keep += [wp, bp, logits, ctrl, ctrl_f]
    calls.append(("tmjx_linear_nolds", (p(a), lda, 1, p(wp), p(bp), p(logits), n, 2 * A, H)))
    calls.append(("tmjx_action_mode", (p(logits), 2 * A, p(ctrl), p(act_l), n, A)))
    e.Wp, e.bp, e.ldwp, e.A = p(wp), p(bp), H, A
    e.h, e.c, e.ld = p(hf), p(cf), LAYERS * H
    e.action_t, e.ctrl, e.logits, e.ldl = p(act_f), p(ctrl_f), None, 0          # what the wrapper asks for: the action rows and ctrl
    return calls, e, keep, (act_l, act_f)


def one(n: int, a) -> int:
    import torch
    from track_mjx_amd import hip
    dev = "cuda:0"
    L = hip.lib()
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    calls, e, keep, (act_l, act_f) = build(n, dev)
    if L.tmjx_lstm_decoder_act_ok(C.byref(e)) != 1:
        raise SystemExit("tmjx_lstm_decoder_act_ok refused the benchmark's decoder")

    def layered():
        for name, args in calls:
            hip.check(getattr(L, name)(*args, s), name)

    def fused():
        hip.check(L.tmjx_lstm_decoder_act(C.byref(e), s), "tmjx_lstm_decoder_act")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    layered(); fused()
    torch.cuda.synchronize()
    worst = float((act_l - act_f).abs().max())          # (after one step from the same zero carry)
    for fn in (layered, fused):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    tl, tf = [], []
    for _ in range(a.repeats):
        tl.append(timed(layered)); tf.append(timed(fused))
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    print(f"n = {n:5d}  layered ({len(calls)} launches): median {med(tl):7.1f}  [{min(tl):7.1f} .. {max(tl):7.1f}]   fused (1 launch): median {med(tf):7.1f}  "
          f"[{min(tf):7.1f} .. {max(tf):7.1f}]   layered / fused {med(tl) / med(tf):5.2f}   max |action difference| {worst:.2e}")
    print("           layered repeats: " + " ".join(f"{v:.1f}" for v in tl) + "   fused repeats: " + " ".join(f"{v:.1f}" for v in tf))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each size's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("--repeats must be >= 3")
    if a.one is not None:
        return one(a.one, a)
    from track_mjx_amd import hip
    lines = [f"LSTM decoder step, H = {H}, L = {LAYERS}, Z = {Z}, prop = {W - REF}, A = {A}; build {hip.build_id()}; {a.iters} steps per timing, "
             f"{a.warmup} warm-up, {a.repeats} alternating repeats; us per decoder step"]
    rc = 0
    for n in (int(v) for v in a.sizes.split(",")):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--one", str(n), "--iters", str(a.iters), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"n = {n:5d}  no result within {a.step_timeout} s: stopped here")
            rc = 1
            break
        if res.returncode != 0:
            lines.append(f"n = {n:5d}  failed with exit status {res.returncode}: stopped here\n{res.stderr[-2000:]}")
            rc = 1
            break
        lines.append(res.stdout.rstrip())
    text = "\n".join(lines)
    print(text)
    if a.out and rc == 0:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
