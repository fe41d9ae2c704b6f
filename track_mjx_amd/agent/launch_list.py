"""The launch list of a policy step: preallocated buffers and the C-ABI calls that run on them, in launch order.

analysis.rollout._PolicyStep (encoder + decoder of a roll-out's policy step) and environment.wrappers._DecoderStep (the decoder inside a
HighLevelWrapper env) build their layer-by-layer paths here, so a decoder fed recorded latents issues the very calls of the roll-out that
recorded them: the same entry points with the same operand layouts, hence the same bits.

Every dense layer is the matrix-core variant of tmjx_linear_nolds (row-major operands with 16-byte aligned rows, K padded to a multiple of 4):
its per-row arithmetic does not depend on the number of rows.
"""
from __future__ import annotations

import ctypes as C


def ceil4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


class LaunchList:
    """`calls`: [entry point, argument list] in launch order (lists: a caller may patch an argument between runs); `keep`: everything the raw
    pointers in them name, alive as long as the list."""

    def __init__(self, n: int, device):
        from .. import hip
        self.hip, self.L = hip, hip.lib()
        self.n, self.device = int(n), device
        self.calls, self.keep = [], []
        self._padded = {}

    def buf(self, *shape, zero: bool = False):
        import torch
        t = (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=self.device)
        self.keep.append(t)
        return t

    def call(self, name: str, *args) -> None:
        self.calls.append([name, list(args)])

    def pad(self, w):
        """A [N][ceil4(K)] fp32 copy of a weight (zero pad columns), one per weight."""
        if id(w) not in self._padded:
            N, K = w.shape
            buf = self.buf(N, ceil4(K), zero=True)
            buf[:, :K].copy_(w.detach())
            self.keep.append(w)              # (the cache is keyed by id: the weight must not be freed and its id reused)
            self._padded[id(w)] = buf
        return self._padded[id(w)]

    def linear(self, a, lda: int, weight, bias=None, out=None):
        """out [n][N] = a [n][lda] weight^T (+ bias)."""
        w = self.pad(weight)
        N = weight.shape[0]
        out = self.buf(self.n, N) if out is None else out
        self.call("tmjx_linear_nolds", ptr(a), lda, 1, ptr(w), ptr(bias), ptr(out), self.n, N, w.shape[1])
        return out

    def linear_norm(self, a, lda: int, weight, fold_mean, fold_inv):
        """linear without a bias on (a - fold_mean) * fold_inv, the normaliser folded into the operand load."""
        w = self.pad(weight)
        N = weight.shape[0]
        out = self.buf(self.n, N)
        self.call("tmjx_linear_nolds_norm", ptr(a), lda, 1, ptr(w), None, ptr(out), self.n, N, w.shape[1], ptr(fold_mean), ptr(fold_inv))
        return out

    def intervene(self, buf, c0: int, w: int, ld: int, spec_buffers):
        """Append tmjx_intervene on columns [c0, c0 + w) of buf [n][ld] (the edit of analysis.intervene.InterventionBuffers `spec_buffers`, which
        must hold one gate per row of this list) and return its entry of `calls`: [name, [descriptor, t]] — the step loop writes the control-step
        index into entry[1][1] before each run."""
        sb = spec_buffers
        if sb.n != self.n:
            raise ValueError(f"intervention buffers for {sb.n} rows in a launch list of {self.n}")
        if sb.w != int(w):
            raise ValueError(f"the intervention is {sb.w} wide, the target buffer {int(w)}")
        d = self.hip.Intervene(buf.data_ptr() + 4 * int(c0), int(ld), int(w), self.n, sb.mode, ptr(sb.dirs), sb.K, sb.ldv, ptr(sb.center), ptr(sb.gain),
                               ptr(sb.offset), ptr(sb.dose), ptr(sb.t_on), ptr(sb.t_off), ptr(sb.proj), sb.ldp, 0)
        if not self.L.tmjx_intervene_ok(C.byref(d)):
            raise ValueError(self.L.tmjx_last_error().decode())
        self.keep += [buf, sb, d]
        self.call("tmjx_intervene", C.byref(d), 0)
        return self.calls[-1]

    def place_intervention(self, intervention, window, dose, x, Z: int, layers: dict, h=None):
        """Insert the tmjx_intervene call of `intervention` (analysis.intervene.Intervention; window [n, 2], dose [n]) into the finished list,
        directly behind the call that produces its target, and return (the call's entry, its buffers).  x [n][ldx]: the decoder's input, whose
        columns [0, Z) are the intention; layers: {"encoder/layer_0": y, ..} the Dense -> SiLU -> LayerNorm outputs; h [n][L][H]: the LSTM carry."""
        target = intervention.target
        supported = ["intention", *layers] + ([f"hidden_state/h:{k}" for k in range(h.shape[1])] if h is not None else [])

        def index(pred, nth=0):
            return [i for i, (name, args) in enumerate(self.calls) if pred(name, args)][nth]
        if target == "intention":
            at, buf, c0, w, ld = index(lambda nm, a: nm in ("tmjx_latent_concat_det", "tmjx_decoder_input")), x, 0, int(Z), x.shape[1]
        elif target in layers:
            y = layers[target]
            at, buf, c0, w, ld = index(lambda nm, a: nm == "tmjx_silu_ln_fwd" and a[4] == y.data_ptr()), y, 0, y.shape[1], y.shape[1]
        elif h is not None and target in supported:
            k = int(target.rpartition(":")[2])
            at, buf, c0, w, ld = index(lambda nm, a: nm == "tmjx_lstm_seq_fwd", k), h[:, k], 0, h.shape[2], h.shape[1] * h.shape[2]
        else:
            raise ValueError(f"intervention target {target!r} does not exist in this policy step; it has: {', '.join(supported)}")
        sb = intervention.buffers(self.n, w, self.device, window, dose)
        entry = self.intervene(buf, c0, w, ld, sb)
        self.calls.insert(at + 1, self.calls.pop())
        return entry, sb

    def block(self, a, lda: int, blk, fold=None):
        """Dense -> SiLU -> LayerNorm: y [n][N]; `fold` = (fold_mean, fold_inv) takes linear_norm for the dense layer."""
        z = self.linear(a, lda, blk.dense.weight) if fold is None else self.linear_norm(a, lda, blk.dense.weight, *fold)
        N = z.shape[1]
        y, stats = self.buf(self.n, N), self.buf(self.n, 2)
        self.call("tmjx_silu_ln_fwd", ptr(z), ptr(blk.dense.bias), ptr(blk.norm.weight), ptr(blk.norm.bias), ptr(y), ptr(stats), self.n, N, float(blk.norm.eps))
        return y

    def lstm_layers(self, a, lda: int, w_ih, w_hh, b_hh, h, c, reset):
        """One step (T = 1) of the stacked cells on the carry h, c [n][L][H] in place, rows with reset != 0 from a zero carry; returns the top
        layer's h and its leading dimension."""
        Lk, H = h.shape[1], h.shape[2]
        xg = self.buf(self.n, 4 * H)
        self.keep.append(reset)
        for k in range(Lk):
            self.linear(a, lda, w_ih[k], out=xg)
            hk, ck = h[:, k], c[:, k]
            wh = w_hh[k].detach().contiguous()
            args = self.hip.LstmFwd(ptr(xg), 4 * H, ptr(wh), H, ptr(b_hh[k]), ptr(hk), ptr(ck), Lk * H, ptr(reset), self.n, ptr(hk), ptr(ck), Lk * H,
                                    None, None, 1, self.n, H)
            self.keep += [wh, args]
            self.call("tmjx_lstm_seq_fwd", C.byref(args))
            a, lda = hk, Lk * H
        return a, lda

    def action_mode(self, logits):
        """(ctrl [n][A], action_t [A][n]) = tanh of the first half of logits [n][2A]."""
        A = logits.shape[1] // 2
        ctrl, action_t = self.buf(self.n, A), self.buf(A, self.n)
        self.call("tmjx_action_mode", ptr(logits), logits.shape[1], ptr(ctrl), ptr(action_t), self.n, A)
        return ctrl, action_t

    def decoder(self, x, blocks, head_w, head_b, lstm=None):
        """The decoder half on its input x [n][ceil4(Z + prop)]: LSTM layers (`lstm` = lstm_layers' arguments behind the input) or Dense -> SiLU ->
        LayerNorm `blocks`, the head / projection, the action.  Returns (the blocks' outputs, logits, ctrl, action_t)."""
        a, lda, ys = x, x.shape[1], []
        if lstm is not None:
            a, lda = self.lstm_layers(a, lda, *lstm)
        for blk in blocks:
            a = self.block(a, lda, blk)
            lda = a.shape[1]
            ys.append(a)
        logits = self.linear(a, lda, head_w, head_b)
        return (ys, logits, *self.action_mode(logits))

    def run(self, stream) -> None:
        """The launches on `stream` (ctypes calls only: no torch operation)."""
        L, check = self.L, self.hip.check
        for name, args in self.calls:
            check(getattr(L, name)(*args, stream), name)
