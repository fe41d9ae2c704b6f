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

import sys

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import resolve
from .jacobian import feature_trees, forward_mismatch, load_decoder, read_clips, warn_mismatch
from .recorded import by_clip, labels_for_rows, scatter_per_clip

CLI_OPTIONS = ("checkpoint", "rollouts", "k", "warmup", "rate", "seed", "labels", "store", "out", "features_out")
USAGE = ("usage: python -m track_mjx_amd.analysis.dynamics checkpoint=<use_lstm run dir | step dir> rollouts=<dir of clip_<i>.h5> [k=16] [warmup=25] [rate=<Hz>] "
         "[seed=0] [labels=<clusters.h5>] [store=false] [features_out=<dir>] out=<dynamics.h5>")
MLP_REFUSAL = ("the checkpoint holds an MLP decoder (Dense -> SiLU -> LayerNorm blocks): it has no carry, so there are no recurrent dynamics to follow; "
               "analysis.dynamics takes a train_config.use_lstm checkpoint")


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
    model, layers, head, _ = load_decoder(checkpoint)
    if model != "lstm":
        raise ValueError(MLP_REFUSAL)
    k, warmup = int(k), int(warmup)
    A, Lk, H = head[2], len(layers), layers[0][1].shape[1]
    W = 2 * Lk * H
    if not 1 <= k <= min(_hip.LSTM_TANGENT_MAX_K, W):
        raise ValueError(f"k = {k}: 1 to {min(_hip.LSTM_TANGENT_MAX_K, W)} tangents (the carry has {W} columns)")
    if warmup < 0:
        raise ValueError(f"warmup must be >= 0 (got {warmup})")
    if rate is not None and not float(rate) > 0.0:
        raise ValueError(f"rate must be > 0 (got {rate})")
    ids, clips = read_clips(rollouts, layers, True, "follow")
    lens = [c.x.shape[0] for c in clips]
    total = int(sum(lens))
    if total < 1:
        raise ValueError("the roll-outs hold no recorded step")
    x_all = np.concatenate([c.x for c in clips], 0)
    carry_all = np.concatenate([np.concatenate([c.h_in, c.c_in], 1) for c in clips], 0)      # [rows, h | c]
    # a new sequence starts at row 0 of a clip and at every row behind a set `aligned` flag
    first = np.concatenate([np.concatenate([[True], c.aligned[:-1]]) for c in clips], 0)
    finite = np.isfinite(x_all).all(1) & np.isfinite(carry_all).all(1)
    first[1:] |= ~finite[:-1]      # (the carry behind a row that is not finite is not the product's)
    rows = np.flatnonzero(finite)
    if rows.shape[0] < 1:
        raise ValueError("no recorded step has a finite decoder input and carry")
    n = int(rows.shape[0])
    starts = np.flatnonzero(first[rows])      # positions in the kept rows (a kept row behind a dropped one is a first row)
    seq_start = np.concatenate([starts, [n]]).astype(np.int32)
    clip_of_row = np.repeat(np.arange(len(ids)), lens)[rows]
    t_in = np.arange(n) - np.repeat(starts, np.diff(seq_start))      # the row's index inside its sequence
    counted = t_in >= warmup
    x = np.ascontiguousarray(x_all[rows], np.float32)
    carry = np.ascontiguousarray(carry_all[rows], np.float32)
    bk = resolve(backend, device)
    xa, ha, ca = bk.asarray(x), bk.asarray(carry[:, :W // 2]), bk.asarray(carry[:, W // 2:])
    q0 = first_basis(W, k, seed)
    try:
        res = bk.lstm_lyapunov(xa, ha, ca, layers, seq_start, q0, warmup, ("local", "energy", "q_out", "status"))
        ctrl = bk.lstm_decoder_jacobian(xa, ha, ca, layers, head, (0, 1), want=("ctrl",))["ctrl"]
    except _hip.TmjxError as e:
        raise ValueError(str(e)) from None

    def per_clip(a):
        return scatter_per_clip(a, rows, total, ids, lens)
    seq_clip = clip_of_row[starts]
    seq_counted = np.array([int(counted[a:b].sum()) for a, b in zip(seq_start[:-1], seq_start[1:])], np.int64)
    n_counted = int(seq_counted.sum())
    sums = res["sums"].astype(np.float64)
    nan = np.full(k, np.nan)
    with np.errstate(invalid="ignore"):      # (-inf sums of collapsed tangents stay -inf)
        exponents = sums.sum(0) / n_counted if n_counted else nan
        per_clip_exponents = by_clip(ids, [sums[seq_clip == j].sum(0) / seq_counted[seq_clip == j].sum() if seq_counted[seq_clip == j].sum() else nan
                                           for j in range(len(ids))])
    energy = res["energy"][counted].astype(np.float64).mean(0) if n_counted else np.full((k, 2 * Lk), np.nan)
    lead = float(exponents[0])
    half = float(np.log(2.0) / -lead) if lead < 0.0 else float("inf")
    last_seq = {j: int(np.flatnonzero(seq_clip == j)[-1]) for j in range(len(ids)) if (seq_clip == j).any()}
    first_in_clip = rows[starts] - (np.cumsum(lens) - lens)[seq_clip]
    out = {"exponents": exponents, "exponents_per_clip": per_clip_exponents, "local_exponents": per_clip(res["local"]), "energy": energy,
           "memory_halflife_steps": np.float64(half), "kaplan_yorke_dimension": np.float64(kaplan_yorke(exponents) if n_counted else np.nan),
           "n_positive": np.int64((exponents > 0.0).sum()), "final_basis": {f"clip_{ids[j]}": res["q_out"][s] for j, s in last_seq.items()},
           "sequences": np.stack([np.asarray(ids, np.int64)[seq_clip], first_in_clip.astype(np.int64), np.diff(seq_start).astype(np.int64)], 1),
           "status": res["status"].astype(np.int32), "rows": np.int64(n), "counted_rows": np.int64(n_counted), "clips": np.asarray(ids, np.int64), "k": np.int64(k),
           "warmup": np.int64(warmup), "seed": np.int64(seed), "model": model, "hidden_state_size": np.int64(H), "hidden_layer_num": np.int64(Lk),
           "forward_mismatch": forward_mismatch(ctrl, clips, A, rows)}
    if rate is not None:
        out.update({"rate": np.float64(rate), "exponents_per_second": exponents * float(rate), "memory_halflife_seconds": np.float64(half / float(rate))})
    if store:
        out["energy_per_clip"] = per_clip(res["energy"])
    out["sequence_counted_rows"] = seq_counted      # (0: no row past warmup)
    if labels is not None:
        flat = labels_for_rows(labels, ids, lens)[rows]
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
        out["features"] = feature_trees(ids, clips, {"local_exponents": out["local_exponents"]})
    return out


def main(argv=None, backend=None, policy=None) -> int:
    """The command line; `policy`: an LSTMDecoderPolicy or LSTMIntentionPolicy in place of checkpoint=, `backend`: a stand-in for HipBackend."""
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out"), USAGE, lambda o: "checkpoint" in o or policy is not None)
    if opts is None:
        return 2
    try:
        res = dynamics_rollouts(opts["checkpoint"] if policy is None else policy, opts["rollouts"], int(opts.get("k", 16)), int(opts.get("warmup", 25)),
                                float(opts["rate"]) if "rate" in opts else None, int(opts.get("seed", 0)), opts.get("labels"), cli.flag(opts, "store"),
                                "features_out" in opts, backend=backend)
    except (KeyError, ValueError, OSError) as e:
        return cli.report("dynamics", e)
    feats = res.pop("features", None)
    cli.write(opts["out"], res)
    if feats is not None:
        cli.write_clips(opts["features_out"], feats)
    idle = [f"clip_{c} rows {a}:{a + t}" for (c, a, t), rows in zip(res["sequences"], res["sequence_counted_rows"]) if rows == 0]
    if idle:
        print(f"[dynamics] warning: {len(idle)} sequence(s) have no row past warmup={int(res['warmup'])} and count nothing: {', '.join(idle)}", file=sys.stderr)
    mismatch = float(res["forward_mismatch"])
    warn_mismatch("dynamics", mismatch)
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
