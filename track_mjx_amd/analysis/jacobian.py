"""The decoder's Jacobian at recorded steps on the GPU (csrc/tmjx_jacobian.hip; DESIGN.md "Decoder Jacobian"): sensitivity.  At every recorded
step the decoder's input row [intention | normalised proprioception] is in the roll-out; this tool recomputes the decoder there and differentiates
ctrl = tanh(loc) (or loc) with respect to the intention (or any 128 columns of the input): how strongly each latent dimension drives each
actuator, which latent directions matter for action and which are slack, and how much of the stochastic encoder's noise reaches the muscles.

    python -m track_mjx_amd.analysis.jacobian checkpoint=<run dir | step dir> rollouts=<dir of clip_<i>.h5> [wrt=intention | input:a:b] [mode=ctrl|loc]
                                              [max_rows=0] [seed=0] [labels=<clusters.h5>] [store=false] [features_out=<dir>] out=<jacobian.h5>

writes gain/clip_<i> [T-1] (the squared Frobenius norm of J), latent_sensitivity/clip_<i> [T-1, Z] (sum over actuators of J_aj^2),
actuator_sensitivity/clip_<i> [T-1, A] (sum over inputs) and, where the roll-out recorded encoder/logvar and the differentiated columns are
intention columns, action_var/clip_<i> [T-1, A] (sum_j J_aj^2 exp(logvar_j): the variance the encoder's noise puts on each actuator, to first
order); mean_jacobian [A, Z], gram_in [Z, Z] (the mean of J^T J) and gram_out [A, A] (of J J^T); the eigen-decomposition of gram_in as `feature`,
`mean`, `components` [Z, Z], `explained_variance`, `explained_variance_ratio`, the layout of analysis.pca, so that `python -m
track_mjx_amd.analysis.rollout ... intervene_pca=<jacobian.h5> intervene_components=0:3` projects out the latent directions the decoder listens to
most (the trailing components are the slack ones); forward_mismatch, the largest |recomputed ctrl - recorded ctrl| (a warning above 1e-3: a
checkpoint that did not make these roll-outs differs at O(0.1), and so does an intervention downstream of the intention); rows, wrt, mode, clips.
max_rows= evaluates a sorted random sample (the other rows of the per-clip series are NaN); labels= (a clusters.h5, hmm.h5, arhmm.h5 or map.h5)
adds motif_mean_jacobian [K, A, Z], motif_gram_in [K, Z, Z], motif_gain [K] and motif_rows [K]; store=true adds jacobian/clip_<i> [T-1, A, Z]
(refused above 2^31 bytes); features_out= writes a directory of clip_<i>.h5 with activations/latent_sensitivity, activations/actuator_sensitivity,
activations/jacobian_gain [T-1, 1] and the clip's meta, which analysis.cluster, hmm, pca, readout, spectrogram and embed take like a roll-out
directory.

A use_lstm checkpoint (the stacked-LSTM decoder; csrc/tmjx_lstm_jacobian.hip, DESIGN.md "LSTM decoder Jacobian") is taken the same way, on roll-outs
made with `analysis.rollout ... log_activations=true log_decoder_input=true` (an LSTM roll-out records egocentric_obs only with that option; a
replay_latents= directory records neither the carry nor the input and is refused).  The step is linearised at its recorded input row AND at the carry
(h, c) entering it: the recorded hidden_state of row t - 1, zeros at t = 0 and behind a step whose `aligned` flag is set (the roll-out zeroes the
carry of a re-aligned env).  Beyond the above it writes memory_sensitivity/clip_<i> [T-1, 2 L] (the squared Frobenius norm of d ctrl / d h_k, then
of d ctrl / d c_k, per layer, each carry column scaled by its standard deviation over the evaluated rows: how much of the action comes from memory
rather than from the current input, comparable with action_var), carry_std [2 L H] (that scale), mean_carry_jacobian [A, 2 L H] (the h blocks of
every layer, then the c blocks), with labels= motif_mean_carry_jacobian [K, A, 2 L H] and motif_memory_sensitivity [K, 2 L], with store=true
carry_jacobian/clip_<i> [T-1, A, 2 L H], with features_out= activations/memory_sensitivity, and hidden_state_size, hidden_layer_num; `model` says
which decoder (mlp | lstm) the file is of.

Limits: the MLP decoder up to 8 blocks of up to 1024 units, the LSTM decoder up to 4 layers of 32, 64, 128 or 256 units behind up to 1024 inputs; 64
actuators, 128 differentiated columns a call; one time step (the Jacobian of the new carry with respect to the old one, followed through time, is
analysis.dynamics)."""
from __future__ import annotations

import os
import sys
from typing import NamedTuple

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import resolve
from .recorded import aligned_of, feature_of, labels_for_rows, meta_of, rollout_features, scatter_per_clip

CLI_OPTIONS = ("checkpoint", "rollouts", "wrt", "mode", "max_rows", "seed", "labels", "store", "out", "features_out")
USAGE = ("usage: python -m track_mjx_amd.analysis.jacobian checkpoint=<run dir | step dir> rollouts=<dir of clip_<i>.h5> [wrt=intention | input:a:b] "
         "[mode=ctrl|loc] [max_rows=0] [seed=0] [labels=<clusters.h5>] [store=false] [features_out=<dir>] out=<jacobian.h5>")
MODES = {"ctrl": _hip.JACOBIAN_CTRL, "loc": _hip.JACOBIAN_LOC}
MISMATCH_WARN = 1e-3
STORE_MAX_BYTES = 2 ** 31
LSTM_REFUSAL = ("the checkpoint holds an LSTM decoder (train_config.use_lstm): decoder_weights reads the MLP decoder (Dense -> SiLU -> LayerNorm blocks); "
                "the LSTM decoder's weights come from lstm_decoder_weights")
LSTM_NO_CARRY = ("the checkpoint holds an LSTM decoder and {where} has no activations/hidden_state: the recorded carry is missing; roll the LSTM checkpoint out "
                 "with `analysis.rollout ... log_activations=true log_decoder_input=true`")
LSTM_NO_INPUT = ("{where} has no activations/egocentric_obs: an LSTM roll-out records the decoder's input only with `analysis.rollout ... "
                 "log_decoder_input=true`")
LSTM_REPLAY = ("{where} is a replay_latents= roll-out: it records neither the LSTM decoder's carry nor its input, so the Jacobian cannot be placed at its "
               "steps; use the roll-out the latents came from")


def decoder_weights(source):
    """-> (layers [(W [H, K], b, gamma, beta)], (Wh [2A, H_L], bh, A), eps) as float32 numpy.  `source`: a checkpoint (a run directory, a step directory
    or a .npz: loaded as the decoder policy loads it, agent/checkpoint.py), or a module with `.decoder` blocks and a `.head` (DecoderNet,
    IntentionPolicy), or a DecoderPolicy (its `.net`)."""
    if isinstance(source, (str, os.PathLike)):
        from ..agent import checkpoint as ckpt
        try:
            source = ckpt.make_decoder_policy_fn(source, device="cpu")
        except NotImplementedError:
            raise ValueError(LSTM_REFUSAL) from None
    net = getattr(source, "net", source)
    if not hasattr(net, "decoder") or not hasattr(net, "head") or hasattr(net, "hidden_layer_num"):
        raise ValueError(LSTM_REFUSAL if hasattr(net, "hidden_layer_num") or hasattr(net, "w_hh") else
                         f"{type(net).__name__} has no decoder blocks and head: expected a DecoderNet, an IntentionPolicy or a checkpoint of one")
    num = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), np.float32)      # noqa: E731
    blocks = list(net.decoder)
    if not blocks:
        raise ValueError("the decoder has no hidden block")
    eps = {float(b.norm.eps) for b in blocks}
    if len(eps) != 1:
        raise ValueError(f"the decoder's LayerNorms have different eps: {sorted(eps)}")
    layers = [(num(b.dense.weight), num(b.dense.bias), num(b.norm.weight), num(b.norm.bias)) for b in blocks]
    wh, bh = num(net.head.weight), num(net.head.bias)
    return layers, (wh, bh, wh.shape[0] // 2), eps.pop()


def is_lstm_decoder(source) -> bool:
    net = getattr(source, "net", source)
    return hasattr(net, "w_hh") and hasattr(net, "w_ih")


def lstm_decoder_weights(source):
    """-> (layers [(W_ih [4H, in_k], W_hh [4H, H], b_hh [4H])], (Wp [2A, H], bp, A)) as float32 numpy.  `source`: a use_lstm checkpoint (loaded as
    agent.checkpoint.make_lstm_decoder_policy_fn loads it), an LSTMDecoderPolicy or an LSTMIntentionPolicy."""
    if isinstance(source, (str, os.PathLike)):
        from ..agent import checkpoint as ckpt
        source = ckpt.make_lstm_decoder_policy_fn(source, device="cpu")
    if not is_lstm_decoder(source):
        raise ValueError(f"{type(source).__name__} has no LSTM decoder (w_ih, w_hh, b_hh and a projection)")
    num = lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), np.float32)      # noqa: E731
    wp, bp = (source.w_p, source.b_p) if hasattr(source, "w_p") else (source.projection.weight, source.projection.bias)
    layers = [(num(a), num(b), num(c)) for a, b, c in zip(source.w_ih, source.w_hh, source.b_hh)]
    if not layers:
        raise ValueError("the LSTM decoder has no layer")
    wp = num(wp)
    return layers, (wp, num(bp), wp.shape[0] // 2)


def load_decoder(source):
    """-> ("mlp", layers, head, eps) as decoder_weights gives them, or ("lstm", layers, head, None) as lstm_decoder_weights does: whichever decoder
    the checkpoint (or the module, or the policy object) holds."""
    if isinstance(source, (str, os.PathLike)):
        from ..agent import checkpoint as ckpt
        try:
            source = ckpt.make_decoder_policy_fn(source, device="cpu")
        except NotImplementedError:
            source = ckpt.make_lstm_decoder_policy_fn(source, device="cpu")
    if is_lstm_decoder(source):
        return ("lstm", *lstm_decoder_weights(source), None)
    return ("mlp", *decoder_weights(source))


def _carry_of(r, where):
    """(h, c) [T-1, L, H] of a roll-out's activations/hidden_state (written as the pair (h, c): members 0 and 1; a group h, c is taken too), or None."""
    try:
        node = r["activations"]["hidden_state"]
    except (KeyError, IndexError, TypeError):
        return None
    out = []
    for names in (("h", "0", 0), ("c", "1", 1)):
        for k in names:
            try:
                v = node[k]
            except (KeyError, IndexError, TypeError):
                continue
            out.append(np.asarray(v if isinstance(v, np.ndarray) else v[()], np.float32))
            break
    if len(out) != 2 or out[0].ndim != 3 or out[0].shape != out[1].shape:
        raise ValueError(f"{where}: activations/hidden_state is not the pair (h, c) of [T-1, L, H] arrays")
    return out[0], out[1]


class Clip(NamedTuple):
    """What the decoder tools read of one roll-out.  The last four are an LSTM roll-out's."""
    x: np.ndarray                  # [T-1, d_in]: the decoder's input rows [intention | egocentric_obs]
    Z: int                         # the width of the intention
    logvar: np.ndarray | None      # encoder/logvar [T-1, Z], where recorded
    ctrl: np.ndarray | None        # the recorded ctrl [T-1, A], where recorded
    meta: dict | None              # the roll-out's meta tree
    h_in: np.ndarray | None = None       # [T-1, L H]: the carry ENTERING every step: the recorded one of the row before, zeros at t = 0 and behind a
    c_in: np.ndarray | None = None       # step whose `aligned` flag is set
    shape: tuple | None = None           # (L, H) of the recorded carry
    aligned: np.ndarray | None = None    # bool [T-1]: the step ended with a re-alignment (the roll-out zeroed the carry behind it)


def read_clip(r, clip, where) -> Clip:
    z, prop = feature_of(r, "intention", where), feature_of(r, "egocentric_obs", where)
    if z.shape[0] != prop.shape[0]:
        raise ValueError(f"{where}: intention has {z.shape[0]} rows, egocentric_obs {prop.shape[0]}")
    try:
        logvar = feature_of(r, "encoder/logvar", where)
    except KeyError:
        logvar = None
    try:
        ctrl = feature_of(r, "ctrl", where)[:z.shape[0]]
    except KeyError:
        ctrl = None
    return Clip(np.concatenate([z, prop], 1), z.shape[1], logvar, ctrl, meta_of(r))


def read_lstm_clip(r, clip, where) -> Clip:
    """read_clip for an LSTM roll-out, with the carry placed at every step; a roll-out without the carry or the input, or a replay, is refused by name."""
    meta = meta_of(r)
    if meta is not None and "replay_latents" in meta:
        raise ValueError(LSTM_REPLAY.format(where=where))
    carry = _carry_of(r, where)
    if carry is None:
        raise ValueError(LSTM_NO_CARRY.format(where=where))
    try:
        feature_of(r, "egocentric_obs", where)
    except KeyError:
        raise ValueError(LSTM_NO_INPUT.format(where=where)) from None
    one = read_clip(r, clip, where)
    h, c = carry
    T1, L, H = h.shape
    if T1 != one.x.shape[0]:
        raise ValueError(f"{where}: hidden_state has {T1} rows, intention {one.x.shape[0]}")
    aligned = aligned_of(r, T1, where)
    aligned = np.zeros(T1, bool) if aligned is None else aligned
    keep = np.ones(T1, bool)
    keep[0] = False
    keep[1:] &= ~aligned[:-1]
    h_in, c_in = np.zeros((T1, L * H), np.float32), np.zeros((T1, L * H), np.float32)
    h_in[1:], c_in[1:] = h.reshape(T1, -1)[:-1], c.reshape(T1, -1)[:-1]
    h_in[~keep], c_in[~keep] = 0.0, 0.0
    return one._replace(h_in=h_in, c_in=c_in, shape=(L, H), aligned=aligned)


def read_clips(rollouts, layers, lstm: bool, verb: str):
    """-> (clip numbers, the Clip of every roll-out), read for the decoder `layers` belong to; roll-outs another checkpoint made are refused."""
    d_in = layers[0][0].shape[1]
    ids, clips = rollout_features(rollouts, read_lstm_clip if lstm else read_clip, "the decoder's input", verb)
    width = clips[0].x.shape[1]
    if width != d_in:
        raise ValueError(f"the roll-outs' decoder input [intention | egocentric_obs] is {width} wide, the checkpoint's decoder takes {d_in}: "
                         "this checkpoint did not make these roll-outs")
    Lk, H = (len(layers), layers[0][1].shape[1]) if lstm else (0, 0)
    if lstm and any(c.shape != (Lk, H) for c in clips):
        raise ValueError(f"the roll-outs' hidden_state is [T-1, L, H] with (L, H) = {sorted({c.shape for c in clips})}, the checkpoint's decoder has "
                         f"{Lk} layers of {H} units: this checkpoint did not make these roll-outs")
    return ids, clips


def forward_mismatch(ctrl, clips, A: int, rows) -> np.float64:
    """The largest |recomputed ctrl - recorded ctrl| over the evaluated `rows`; NaN where a roll-out did not record ctrl [T-1, A]."""
    if not all(c.ctrl is not None and c.ctrl.shape[1] == A for c in clips):
        return np.float64(np.nan)
    return np.float64(np.abs(ctrl.astype(np.float64) - np.concatenate([c.ctrl for c in clips], 0)[rows]).max())


def warn_mismatch(tool: str, mismatch: float) -> None:
    if mismatch > MISMATCH_WARN:
        print(f"[{tool}] warning: the recomputed ctrl differs from the recorded one by up to {mismatch:.3g} (> {MISMATCH_WARN}): did this checkpoint make "
              "these roll-outs, and without an intervention downstream of the intention?", file=sys.stderr)


def feature_trees(ids, clips, series: dict) -> dict:
    """What features_out= writes, {clip: tree}: activations/<name> of every per-clip series {name: {clip_<c>: [T-1, ...]}} and the clip's meta."""
    return {c: {"activations": {name: per[f"clip_{c}"] for name, per in series.items()}, **({} if clip.meta is None else {"meta": clip.meta})}
            for c, clip in zip(ids, clips)}


def _parse_wrt(wrt: str, Z: int, d_in: int) -> tuple:
    if wrt == "intention":
        a, b = 0, Z
    else:
        parts = str(wrt).split(":")
        if len(parts) != 3 or parts[0] != "input":
            raise ValueError(f"wrt = {wrt!r}: expected intention or input:a:b")
        try:
            a, b = int(parts[1]), int(parts[2])
        except ValueError:
            raise ValueError(f"wrt = {wrt!r}: expected intention or input:a:b with integers a < b") from None
    if not 0 <= a < b <= d_in:
        raise ValueError(f"wrt = {wrt}: the columns {a}:{b} do not lie inside the decoder's {d_in} inputs")
    if b - a > _hip.JACOBIAN_MAX_WRT:
        raise ValueError(f"wrt = {wrt}: {b - a} columns exceed the {_hip.JACOBIAN_MAX_WRT} one call differentiates; pick a range with wrt=input:a:b")
    return a, b - a


def eigen(gram, backend):
    """The eigen-decomposition of a symmetric positive semi-definite [Z, Z] float64 matrix by the backend's one-sided Jacobi kernel (its singular
    values are the eigenvalues): -> (values [Z] descending, vectors [Z, Z] rows, the largest-magnitude coefficient of each positive)."""
    sigma, _, v, _ = backend.compare_svd(np.ascontiguousarray(gram, np.float64))
    v = np.array(v, np.float64)
    lead = np.abs(v).argmax(1)
    v *= np.where(v[np.arange(v.shape[0]), lead] < 0.0, -1.0, 1.0)[:, None]
    return np.array(sigma, np.float64), v


def jacobian_rollouts(checkpoint, rollouts, wrt="intention", mode="ctrl", max_rows=0, seed=0, labels=None, store=False, features=False, device="cuda",
                      backend=None) -> dict:
    """The tool as a function (the module's text says what the result holds): `checkpoint` as decoder_weights takes it, `rollouts` a directory of
    clip_<i>.h5 or a list of roll-out dicts, `labels` a file or {clip: int labels}.  features=True adds "features": per clip the tree features_out=
    writes.  -> the dict the command line writes."""
    if mode not in MODES:
        raise ValueError(f"mode = {mode!r}: ctrl (through the tanh) or loc")
    model, layers, head, eps = load_decoder(checkpoint)
    lstm = model == "lstm"
    d_in, A = layers[0][0].shape[1], head[2]
    ids, clips = read_clips(rollouts, layers, lstm, "differentiate")
    Z = clips[0].Z
    Lk, H = (len(layers), layers[0][1].shape[1]) if lstm else (0, 0)
    W = 2 * Lk * H
    col0, cols = _parse_wrt(wrt, Z, d_in)
    lens = [c.x.shape[0] for c in clips]
    n = int(sum(lens))
    if n < 1:
        raise ValueError("the roll-outs hold no recorded step")
    x = np.ascontiguousarray(np.concatenate([c.x for c in clips], 0), np.float32)
    scale = None
    if all(c.logvar is not None for c in clips) and col0 + cols <= Z:
        lv = np.concatenate([c.logvar for c in clips], 0)[:, col0:col0 + cols]
        scale = np.ascontiguousarray(np.exp(0.5 * lv.astype(np.float64)), np.float32)
    max_rows = int(max_rows)
    if max_rows < 0:
        raise ValueError(f"max_rows must be >= 0 (got {max_rows})")
    # a row that is not finite (a roll-out whose physics diverged is recorded to its end) is never evaluated: its series stay NaN
    carry = np.ascontiguousarray(np.concatenate([np.concatenate([c.h_in, c.c_in], 1) for c in clips], 0), np.float32) if lstm else None      # [n, h | c]
    finite = np.flatnonzero(np.isfinite(x).all(1) & (np.isfinite(scale).all(1) if scale is not None else True) & (np.isfinite(carry).all(1) if lstm else True))
    if finite.shape[0] < 1:
        raise ValueError("no recorded step has a finite decoder input")
    sampled = 0 < max_rows < finite.shape[0]
    if sampled and features:
        raise ValueError("features_out= needs every row: drop max_rows=")
    index = None
    if sampled:
        index = np.sort(np.random.default_rng(int(seed)).choice(finite, size=max_rows, replace=False)).astype(np.int32)
    elif finite.shape[0] < n:
        index = finite.astype(np.int32)
    m = n if index is None else int(index.shape[0])
    if store and m * A * cols * 4 > STORE_MAX_BYTES:
        raise ValueError(f"store=true: {m} rows x {A} x {cols} float32 exceed 2^31 bytes; sample with max_rows= or differentiate fewer columns")
    if store and lstm and m * A * W * 4 > STORE_MAX_BYTES:
        raise ValueError(f"store=true: {m} rows x {A} x {W} float32 of the carry Jacobian exceed 2^31 bytes; sample with max_rows=")
    bk = resolve(backend, device)
    xa, sa = bk.asarray(x), None if scale is None else bk.asarray(scale)
    want = ("ctrl", "gain", "col2", "row2") + (("jac",) if store else ())
    rows = np.arange(n) if index is None else index.astype(np.int64)
    if lstm:
        # the scale of the memory's sensitivity: the standard deviation of every carry column over the evaluated rows
        carry_std = carry[rows].astype(np.float64).std(0).astype(np.float32)
        ha, ca = bk.asarray(carry[:, :W // 2]), bk.asarray(carry[:, W // 2:])
        want = want + ("carry_gain",) + (("carry_jac",) if store else ())

        def evaluate(idx, sc, wanted):
            return bk.lstm_decoder_jacobian(xa, ha, ca, layers, head, (col0, cols), idx, sc, carry_std, MODES[mode], wanted)
    else:
        def evaluate(idx, sc, wanted):
            return bk.decoder_jacobian(xa, layers, head, (col0, cols), eps, idx, sc, MODES[mode], wanted)
    try:
        res = evaluate(index, sa, want)
    except _hip.TmjxError as e:
        raise ValueError(str(e)) from None

    def per_clip(a):
        return scatter_per_clip(a, rows, n, ids, lens)
    out = {"gain": per_clip(res["gain"]), "latent_sensitivity": per_clip(res["col2"]), "actuator_sensitivity": per_clip(res["row2"])}
    if "action_var" in res:
        out["action_var"] = per_clip(res["action_var"])
    if store:
        out["jacobian"] = per_clip(res["jac"])
    if lstm:
        out.update({"memory_sensitivity": per_clip(res["carry_gain"]), "carry_std": carry_std, "mean_carry_jacobian": res["carry_sum"] / m,
                    "hidden_state_size": np.int64(H), "hidden_layer_num": np.int64(Lk)})
        if store:
            out["carry_jacobian"] = per_clip(res["carry_jac"])
    gram_in = res["gram_in"] / m
    values, vectors = eigen(gram_in, bk)
    total = float(values.sum())
    out.update({"mean_jacobian": res["mean_sum"] / m, "gram_in": gram_in, "gram_out": res["gram_out"] / m,
                "feature": "intention" if (col0, cols) == (0, Z) else f"input:{col0}:{col0 + cols}",
                "mean": x[rows, col0:col0 + cols].astype(np.float64).mean(0).astype(np.float32), "components": vectors.astype(np.float32),
                "explained_variance": values.astype(np.float32),
                "explained_variance_ratio": (values / total if total > 0.0 else np.zeros_like(values)).astype(np.float32),
                "forward_mismatch": forward_mismatch(res["ctrl"], clips, A, rows), "rows": np.int64(m), "wrt": f"{col0}:{col0 + cols}", "mode": mode, "clips": np.asarray(ids, np.int64), "model": model})
    if index is not None:
        out["row_index"] = index.astype(np.int64)
    if labels is not None:
        flat = labels_for_rows(labels, ids, lens)
        K = int(flat.max()) + 1
        picked = np.zeros(n, bool)
        picked[rows] = True
        mj, mg, gain, count = np.full((K, A, cols), np.nan), np.full((K, cols, cols), np.nan), np.full(K, np.nan), np.zeros(K, np.int64)
        mcj, mms = np.full((K, A, W), np.nan), np.full((K, 2 * Lk), np.nan)
        for k in range(K):
            mine = np.flatnonzero((flat == k) & picked).astype(np.int32)
            count[k] = mine.shape[0]
            if mine.shape[0]:
                r = evaluate(mine, None, ("gain", "carry_gain") if lstm else ("gain",))
                mj[k], mg[k], gain[k] = r["mean_sum"] / mine.shape[0], r["gram_in"] / mine.shape[0], float(r["gain"].astype(np.float64).mean())
                if lstm:
                    mcj[k], mms[k] = r["carry_sum"] / mine.shape[0], r["carry_gain"].astype(np.float64).mean(0)
        out.update({"motif_mean_jacobian": mj, "motif_gram_in": mg, "motif_gain": gain, "motif_rows": count})
        if lstm:
            out.update({"motif_mean_carry_jacobian": mcj, "motif_memory_sensitivity": mms})
    if features:
        series = {"latent_sensitivity": out["latent_sensitivity"], "actuator_sensitivity": out["actuator_sensitivity"],
                  "jacobian_gain": {key: v.reshape(-1, 1) for key, v in out["gain"].items()}}
        if lstm:
            series["memory_sensitivity"] = out["memory_sensitivity"]
        out["features"] = feature_trees(ids, clips, series)
    return out


def main(argv=None, backend=None, policy=None) -> int:
    """The command line; `policy`: a module or policy object in place of checkpoint= (DecoderNet, IntentionPolicy, DecoderPolicy; LSTMIntentionPolicy,
    LSTMDecoderPolicy), `backend`: a stand-in for HipBackend."""
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out"), USAGE, lambda o: "checkpoint" in o or policy is not None)
    if opts is None:
        return 2
    try:
        res = jacobian_rollouts(opts["checkpoint"] if policy is None else policy, opts["rollouts"], opts.get("wrt", "intention"), opts.get("mode", "ctrl"),
                                int(opts.get("max_rows", 0)), int(opts.get("seed", 0)), opts.get("labels"), cli.flag(opts, "store"), "features_out" in opts,
                                backend=backend)
    except (KeyError, ValueError, OSError) as e:
        return cli.report("jacobian", e)
    feats = res.pop("features", None)
    cli.write(opts["out"], res)
    if feats is not None:
        cli.write_clips(opts["features_out"], feats)
    mismatch = float(res["forward_mismatch"])
    warn_mismatch("jacobian", mismatch)
    ratio = ", ".join(f"{100 * r:.1f}%" for r in res["explained_variance_ratio"][:4])
    print(f"[jacobian] d {res['mode']} / d input[{res['wrt']}]: {int(res['rows'])} rows of {len(res['clips'])} clips, {res['mean_jacobian'].shape[0]} actuators; "
          f"mean gain {float(np.trace(res['gram_in'])):.4g}, the leading sensitive directions carry {ratio}; forward mismatch {mismatch:.3g}; wrote {opts['out']}",
          flush=True)
    if res["model"] == "lstm":
        mem = np.nanmean(np.concatenate(list(res["memory_sensitivity"].values()), 0), 0)
        L = int(res["hidden_layer_num"])
        print(f"[jacobian] LSTM decoder, {L} layers of {int(res['hidden_state_size'])} units: mean memory sensitivity per layer, d ctrl / d h "
              f"{', '.join(f'{v:.4g}' for v in mem[:L])}; d ctrl / d c {', '.join(f'{v:.4g}' for v in mem[L:])} (carry columns scaled by carry_std)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
