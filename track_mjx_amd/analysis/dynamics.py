"""The LSTM decoder's recurrent dynamics at recorded steps on the GPU (csrc/tmjx_lstm_tangent.hip; DESIGN.md "LSTM decoder dynamics"): how long the
decoder remembers.  analysis.jacobian linearises one step; this tool follows the carry through time.  Along every recorded sequence K tangent
vectors of the carry (h, c) are pushed through the carry-to-carry map J_t = d (h', c') / d (h, c) step after step, re-orthonormalised at every
step, and the logarithms of their stretch factors are averaged: the Lyapunov spectrum.  A negative leading exponent says a perturbation of the
memory dies out, and at what rate; the number of exponents near zero is the number of slow directions the memory has; the energy says which
layer, and which of h or c, holds them.

What this is, plainly: the CONDITIONAL exponents of the decoder driven by its recorded input.  The input row of every step (intention and
proprioception) is held as recorded; the loop through the body, by which a perturbed action changes the next observation, is not closed.

    python -m track_mjx_amd.analysis.dynamics checkpoint=<use_lstm run dir | step dir> rollouts=<dir of clip_<i>.h5> [k=16] [warmup=25] [rate=<Hz>]
                                              [seed=0] [labels=<clusters.h5>] [store=false] [features_out=<dir>] out=<dynamics.h5>

takes roll-outs made with `analysis.rollout ... log_activations=true log_decoder_input=true`, read as analysis.jacobian reads them and refused by
name for the same reasons: an MLP checkpoint (it has no carry), no recorded carry, no recorded egocentric_obs, a replay_latents= directory.  A
clip is one sequence, except that the step behind a set `aligned` flag starts a NEW sequence (the roll-out zeroed the carry there, so the product
of Jacobians is broken), and so does the step behind a row that is not finite (such rows are left out; their series are NaN).  Every sequence
starts from the same basis: the orthonormalised first k columns of a numpy.random.default_rng(seed) Gaussian [W, k], W = 2 L H (the h blocks of
every layer, then the c blocks).  The first `warmup` rows of a sequence are propagated and not counted: the basis needs them to turn into the
leading directions.

writes exponents [k] (per step: the sums over all sequences divided by the counted rows, descending for a converged basis), with rate=
exponents_per_second; exponents_per_clip/clip_<i> [k] (NaN for a clip without a counted row); local_exponents/clip_<i> [T-1, k] (log R_jj at
every row); energy [k, 2 L] (the mean over the counted rows of the squared norm of each basis vector inside each layer's h block, then c block:
every row sums to 1), with store=true energy_per_clip/clip_<i> [T-1, k, 2 L]; memory_halflife_steps = ln 2 / -exponents[0] (inf if it is not
negative) and, with rate=, memory_halflife_seconds; kaplan_yorke_dimension (of the k exponents computed: k itself where their sum stays
non-negative); n_positive; final_basis/clip_<i> [k, W] (behind the clip's last row); sequences [S, 3] (clip, first row, rows) and status [S] (1:
a tangent collapsed to zero, its exponents are -inf from there on) and sequence_counted_rows [S] (a sequence with no row past warmup counts
nothing and is named in one warning line); rows, counted_rows, clips, k, warmup, seed, model, hidden_state_size, hidden_layer_num; forward_mismatch, as analysis.jacobian computes it and with its warning.  labels= (a clusters.h5, hmm.h5, arhmm.h5 or map.h5)
adds motif_local_exponents [n_motifs, k] (the mean of the local exponents over each motif's counted rows) and motif_rows; features_out= writes a
directory of clip_<i>.h5 with activations/local_exponents and the clip's meta, which analysis.cluster, hmm, pca, readout, spectrogram and embed
take like a roll-out directory.

Limits: up to 4 layers of 32, 64, 128 or 256 units behind up to 1024 inputs, 1 <= k <= 32, up to 65536 sequences."""
from __future__ import annotations

import os
import sys

import numpy as np

from .. import hip as _hip
from . import jacobian as _jac
from . import pca as _pca
from .utils import rollout_features

CLI_OPTIONS = ("checkpoint", "rollouts", "k", "warmup", "rate", "seed", "labels", "store", "out", "features_out")
USAGE = ("usage: python -m track_mjx_amd.analysis.dynamics checkpoint=<use_lstm run dir | step dir> rollouts=<dir of clip_<i>.h5> [k=16] [warmup=25] [rate=<Hz>] "
         "[seed=0] [labels=<clusters.h5>] [store=false] [features_out=<dir>] out=<dynamics.h5>")
MLP_REFUSAL = ("the checkpoint holds an MLP decoder (Dense -> SiLU -> LayerNorm blocks): it has no carry, so there are no recurrent dynamics to follow; "
               "analysis.dynamics takes a train_config.use_lstm checkpoint")


def _read_clip(r, clip, where):
    """jacobian._read_lstm_clip, plus the rows at which a new sequence starts: row 0 and every row behind a set `aligned` flag (bool [T-1])."""
    x, Z, logvar, ctrl, meta, h_in, c_in, shape = _jac._read_lstm_clip(r, clip, where)
    first = np.zeros(x.shape[0], bool)
    first[:1] = True
    try:
        node = r["aligned"]
        aligned = np.asarray(node if isinstance(node, np.ndarray) else node[()]).reshape(-1) != 0
        first[1:] |= aligned[:x.shape[0] - 1]
    except (KeyError, IndexError, TypeError):
        pass
    return x, Z, logvar, ctrl, meta, h_in, c_in, shape, first


def first_basis(W: int, k: int, seed: int) -> np.ndarray:
    """[k, W] float32: the orthonormalised first k columns of a default_rng(seed) Gaussian [W, k], as rows."""
    q, _ = np.linalg.qr(np.random.default_rng(int(seed)).standard_normal((W, k)))
    return np.ascontiguousarray(q.T, np.float32)


def kaplan_yorke(exponents) -> float:
    """The Kaplan-Yorke dimension of the exponents given: j + (lambda_1 + .. + lambda_j) / |lambda_(j+1)| with j the last index at which the sum
    of the j largest is non-negative; 0 where the largest is negative, their number where the sum never turns negative."""
    lam = np.sort(np.asarray(exponents, np.float64))[::-1]
    total = np.cumsum(lam)
    if lam.shape[0] == 0 or not lam[0] >= 0.0:
        return 0.0
    below = np.flatnonzero(~(total >= 0.0))
    if below.shape[0] == 0:
        return float(lam.shape[0])
    j = int(below[0])
    return float(j + total[j - 1] / abs(lam[j]))


def dynamics_rollouts(checkpoint, rollouts, k=16, warmup=25, rate=None, seed=0, labels=None, store=False, features=False, device="cuda", backend=None) -> dict:
    """The tool as a function (the module's text says what the result holds): `checkpoint` as jacobian.load_decoder takes it, `rollouts` a directory
    of clip_<i>.h5 or a list of roll-out dicts, `labels` a file or {clip: int labels}.  features=True adds "features": per clip the tree
    features_out= writes.  -> the dict the command line writes."""
    model, layers, head, _ = _jac.load_decoder(checkpoint)
    if model != "lstm":
        raise ValueError(MLP_REFUSAL)
    k, warmup = int(k), int(warmup)
    d_in, A, Lk, H = layers[0][0].shape[1], head[2], len(layers), layers[0][1].shape[1]
    W = 2 * Lk * H
    if not 1 <= k <= min(_hip.LSTM_TANGENT_MAX_K, W):
        raise ValueError(f"k = {k}: 1 to {min(_hip.LSTM_TANGENT_MAX_K, W)} tangents (the carry has {W} columns)")
    if warmup < 0:
        raise ValueError(f"warmup must be >= 0 (got {warmup})")
    if rate is not None and not float(rate) > 0.0:
        raise ValueError(f"rate must be > 0 (got {rate})")
    ids, items = rollout_features(rollouts, _read_clip, "the decoder's input", "follow")
    width = items[0][0].shape[1]
    if width != d_in:
        raise ValueError(f"the roll-outs' decoder input [intention | egocentric_obs] is {width} wide, the checkpoint's decoder takes {d_in}: "
                         "this checkpoint did not make these roll-outs")
    if any(it[7] != (Lk, H) for it in items):
        raise ValueError(f"the roll-outs' hidden_state is [T-1, L, H] with (L, H) = {sorted({it[7] for it in items})}, the checkpoint's decoder has "
                         f"{Lk} layers of {H} units: this checkpoint did not make these roll-outs")
    lens = [it[0].shape[0] for it in items]
    total = int(sum(lens))
    if total < 1:
        raise ValueError("the roll-outs hold no recorded step")
    x_all = np.concatenate([it[0] for it in items], 0)
    carry_all = np.concatenate([np.concatenate([it[5], it[6]], 1) for it in items], 0)      # [rows, h | c]
    first = np.concatenate([it[8] for it in items], 0)
    finite = np.isfinite(x_all).all(1) & np.isfinite(carry_all).all(1)
    first[1:] |= ~finite[:-1]      # (the carry behind a row that is not finite is not the product's)
    rows = np.flatnonzero(finite)
    if rows.shape[0] < 1:
        raise ValueError("no recorded step has a finite decoder input and carry")
    n = int(rows.shape[0])
    starts = np.flatnonzero(first[rows])      # positions in the kept rows (a kept row behind a dropped one is a first row)
    seq_start = np.concatenate([starts, [n]]).astype(np.int32)
    clip_of_row = np.repeat(np.arange(len(ids)), lens)[rows]
    ends = np.cumsum(lens)
    t_in = np.arange(n) - np.repeat(starts, np.diff(seq_start))      # the row's index inside its sequence
    counted = t_in >= warmup
    x = np.ascontiguousarray(x_all[rows], np.float32)
    carry = np.ascontiguousarray(carry_all[rows], np.float32)
    bk = _pca.HipBackend(device) if backend is None else backend
    xa, ha, ca = bk.asarray(x), bk.asarray(carry[:, :W // 2]), bk.asarray(carry[:, W // 2:])
    q0 = first_basis(W, k, seed)
    try:
        res = bk.lstm_lyapunov(xa, ha, ca, layers, seq_start, q0, warmup, ("local", "energy", "q_out", "status"))
        ctrl = bk.lstm_decoder_jacobian(xa, ha, ca, layers, head, (0, 1), want=("ctrl",))["ctrl"]
    except _hip.TmjxError as e:
        raise ValueError(str(e)) from None
    recorded = np.concatenate([it[3] for it in items], 0)[rows] if all(it[3] is not None and it[3].shape[1] == A for it in items) else None

    def per_clip(a):
        full = np.full((total, *a.shape[1:]), np.nan, np.float32)
        full[rows] = a
        return {f"clip_{c}": full[e - t:e] for c, e, t in zip(ids, ends, lens)}
    seq_clip = clip_of_row[starts]
    seq_counted = np.array([int(counted[a:b].sum()) for a, b in zip(seq_start[:-1], seq_start[1:])], np.int64)
    n_counted = int(seq_counted.sum())
    sums = res["sums"].astype(np.float64)
    nan = np.full(k, np.nan)
    with np.errstate(invalid="ignore"):      # (-inf sums of collapsed tangents stay -inf)
        exponents = sums.sum(0) / n_counted if n_counted else nan
        by_clip = {f"clip_{c}": (sums[seq_clip == j].sum(0) / seq_counted[seq_clip == j].sum() if seq_counted[seq_clip == j].sum() else nan)
                   for j, c in enumerate(ids)}
    energy = res["energy"][counted].astype(np.float64).mean(0) if n_counted else np.full((k, 2 * Lk), np.nan)
    lead = float(exponents[0])
    half = float(np.log(2.0) / -lead) if lead < 0.0 else float("inf")
    last_seq = {j: int(np.flatnonzero(seq_clip == j)[-1]) for j in range(len(ids)) if (seq_clip == j).any()}
    first_in_clip = rows[starts] - (ends - lens)[seq_clip]
    out = {"exponents": exponents, "exponents_per_clip": by_clip, "local_exponents": per_clip(res["local"]), "energy": energy,
           "memory_halflife_steps": np.float64(half), "kaplan_yorke_dimension": np.float64(kaplan_yorke(exponents) if n_counted else np.nan),
           "n_positive": np.int64((exponents > 0.0).sum()), "final_basis": {f"clip_{ids[j]}": res["q_out"][s] for j, s in last_seq.items()},
           "sequences": np.stack([np.asarray(ids, np.int64)[seq_clip], first_in_clip.astype(np.int64), np.diff(seq_start).astype(np.int64)], 1),
           "status": res["status"].astype(np.int32), "rows": np.int64(n), "counted_rows": np.int64(n_counted), "clips": np.asarray(ids, np.int64), "k": np.int64(k),
           "warmup": np.int64(warmup), "seed": np.int64(seed), "model": model, "hidden_state_size": np.int64(H), "hidden_layer_num": np.int64(Lk),
           "forward_mismatch": np.float64(np.abs(ctrl.astype(np.float64) - recorded).max()) if recorded is not None else np.float64(np.nan)}
    if rate is not None:
        out.update({"rate": np.float64(rate), "exponents_per_second": exponents * float(rate), "memory_halflife_seconds": np.float64(half / float(rate))})
    if store:
        out["energy_per_clip"] = per_clip(res["energy"])
    out["sequence_counted_rows"] = seq_counted      # (0: no row past warmup)
    if labels is not None:
        lab = _jac._labels_file(labels) if isinstance(labels, (str, os.PathLike)) else {int(c): np.asarray(v).reshape(-1) for c, v in dict(labels).items()}
        flat = np.full(total, -1, np.int64)
        for c, e, t in zip(ids, ends, lens):
            if c not in lab:
                raise KeyError(f"the labels file has no clip_{c}")
            if lab[c].shape[0] < t:
                raise ValueError(f"the labels of clip_{c} hold {lab[c].shape[0]} rows, the roll-out {t}")
            flat[e - t:e] = lab[c][:t]
        flat = flat[rows]
        M = int(flat.max()) + 1
        motif, count = np.full((M, k), np.nan), np.zeros(M, np.int64)
        local64 = res["local"].astype(np.float64)
        for m in range(M):
            mine = (flat == m) & counted
            count[m] = int(mine.sum())
            if count[m]:
                with np.errstate(invalid="ignore"):
                    motif[m] = local64[mine].sum(0) / count[m]
        out.update({"motif_local_exponents": motif, "motif_rows": count})
    if features:
        out["features"] = {}
        for j, c in enumerate(ids):
            tree = {"activations": {"local_exponents": out["local_exponents"][f"clip_{c}"]}}
            if items[j][4] is not None:
                tree["meta"] = items[j][4]
            out["features"][c] = tree
    return out


def main(argv=None, backend=None, policy=None) -> int:
    """The command line; `policy`: an LSTMDecoderPolicy or LSTMIntentionPolicy in place of checkpoint=, `backend`: a stand-in for HipBackend."""
    from .. import h5lite
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = dict(a.split("=", 1) for a in argv if "=" in a and a.split("=", 1)[0] in CLI_OPTIONS)
    if ("checkpoint" not in opts and policy is None) or "rollouts" not in opts or "out" not in opts or len(opts) != len(argv):
        print(USAGE, file=sys.stderr)
        return 2
    try:
        res = dynamics_rollouts(opts["checkpoint"] if policy is None else policy, opts["rollouts"], int(opts.get("k", 16)), int(opts.get("warmup", 25)),
                                float(opts["rate"]) if "rate" in opts else None, int(opts.get("seed", 0)), opts.get("labels"), _jac._flag(opts, "store"),
                                "features_out" in opts, backend=backend)
    except (KeyError, ValueError, OSError) as e:
        print(f"[dynamics] {e.args[0] if e.args else e}", file=sys.stderr)
        return 2
    feats = res.pop("features", None)
    os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
    h5lite.write_tree(opts["out"], res)
    if feats is not None:
        os.makedirs(opts["features_out"], exist_ok=True)
        for c, tree in feats.items():
            h5lite.write_tree(os.path.join(opts["features_out"], f"clip_{c}.h5"), tree)
    idle = [f"clip_{c} rows {a}:{a + t}" for (c, a, t), rows in zip(res["sequences"], res["sequence_counted_rows"]) if rows == 0]
    if idle:
        print(f"[dynamics] warning: {len(idle)} sequence(s) have no row past warmup={int(res['warmup'])} and count nothing: {', '.join(idle)}", file=sys.stderr)
    mismatch = float(res["forward_mismatch"])
    if mismatch > _jac.MISMATCH_WARN:
        print(f"[dynamics] warning: the recomputed ctrl differs from the recorded one by up to {mismatch:.3g} (> {_jac.MISMATCH_WARN}): did this checkpoint make "
              "these roll-outs, and without an intervention downstream of the intention?", file=sys.stderr)
    if int(np.asarray(res["status"]).sum()):
        print(f"[dynamics] warning: a tangent collapsed to zero in {int(np.asarray(res['status']).sum())} sequence(s): its exponents are -inf", file=sys.stderr)
    lam = ", ".join(f"{v:.4g}" for v in res["exponents"][:6])
    per_s = f" ({float(res['memory_halflife_seconds']):.4g} s)" if "rate" in res else ""
    print(f"[dynamics] conditional Lyapunov spectrum of the LSTM decoder ({int(res['hidden_layer_num'])} layers of {int(res['hidden_state_size'])} units) driven by "
          f"its recorded input: {int(res['counted_rows'])} counted of {int(res['rows'])} rows in {len(res['status'])} sequences of {len(res['clips'])} clips; leading "
          f"exponents per step {lam}; memory half-life {float(res['memory_halflife_steps']):.4g} steps{per_s}; {int(res['n_positive'])} positive, Kaplan-Yorke "
          f"dimension {float(res['kaplan_yorke_dimension']):.4g} of {int(res['k'])}; forward mismatch {mismatch:.3g}; wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
