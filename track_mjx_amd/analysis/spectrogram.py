"""Morlet wavelet spectrograms of recorded signals on the GPU (csrc/tmjx_spectrogram.hip; DESIGN.md "Spectrogram"): rhythm as a feature.  Every
channel of a recorded series (the animal's joint angles, forces, sensors, or a layer's activations) is filtered with a bank of complex wavelets, and
the time-frequency amplitudes become the rows that analysis.cluster, analysis.hmm, analysis.pca and analysis.readout work on: a limb that swings at
2 Hz and one that swings at 6 Hz differ in no single time step, and in every row of the spectrogram.

    python -m track_mjx_amd.analysis.spectrogram rollouts=<dir of clip_<i>.h5> source=qposes_rollout rate=50 [cols=7:] [f_min=1] [f_max=rate/2]
                                                 [n_freqs=25] [omega0=5] [support=4] [detrend=true] [output=amplitude|log] [floor=1e-3]
                                                 [projections=<pca.h5>] out=<dir>

writes <out>/clip_<i>.h5 for every input clip: activations/spectrogram [T_src, F C] (column j C + c: frequency j, channel c), spectrogram_coverage
[T_src, F] (the share of each wavelet's window that lay inside the clip: mask edge rows with it), frequencies [F], spectrogram_meta (source, cols,
rate, omega0, support, detrend, output, floor, n_channels) and the input's meta group, so that `python -m track_mjx_amd.analysis.cluster
rollouts=<out> feature=spectrogram k=..` (and analysis.hmm, analysis.pca, analysis.readout) take the directory as they take a roll-out directory.
T_src is the row count of the source: qposes_rollout and qposes_ref hold one row per frame, one more than ctrl, the forces, the sensors and the
activations, which hold one per step.  source is one of ctrl, qposes_rollout, qposes_ref, joint_forces, sensor_readings, state_rewards,
rollout_metrics/<name> or activations/<path>; with projections=<pca.h5> the signals are that file's projections/clip_<i> instead (the leading
components of a wide layer).  rate is the control rate of the roll-out in Hz and has no default: the two shipped configurations step at 50 Hz
(rodent-full-clips: 10 physics steps of 2 ms) and 100 Hz (rodent-sps-per-actor: 5).  The tool refuses F C > 1024, the width the tools it feeds stop at.
"""
from __future__ import annotations

import os
import sys

import numpy as np

from .. import hip as _hip
from . import cli
from .backend import resolve
from .recorded import seq_start, signals, split

CLI_OPTIONS = ("rollouts", "out", "source", "cols", "rate", "f_min", "f_max", "n_freqs", "omega0", "support", "detrend", "output", "floor", "projections")
MAX_TOOL_WIDTH = 1024      # analysis.cluster, analysis.hmm and the wide PCA stop here
USAGE = ("usage: python -m track_mjx_amd.analysis.spectrogram rollouts=<dir of clip_<i>.h5> source=<series> rate=<Hz> [cols=a:b] [f_min=1] [f_max=rate/2] "
         "[n_freqs=25] [omega0=5] [support=4] [detrend=true] [output=amplitude|log] [floor=1e-3] [projections=<pca.h5>] out=<dir>")


def dyadic_frequencies(f_min: float, f_max: float, n: int) -> np.ndarray:
    """f_min (f_max / f_min)^(i / (n - 1)), i = 0 .. n - 1: equal steps in log frequency (n = 1: f_min)."""
    f_min, f_max, n = float(f_min), float(f_max), int(n)
    if n < 1 or not 0.0 < f_min <= f_max:
        raise ValueError(f"expected n >= 1 and 0 < f_min <= f_max (got n = {n}, f_min = {f_min}, f_max = {f_max})")
    if n == 1:
        return np.array([f_min])
    return f_min * (f_max / f_min) ** (np.arange(n) / (n - 1))


class Spectrogram:
    """The Morlet wavelet amplitudes of [n, C] rows in sequences of `lengths`, C <= 1024, up to 64 frequencies: `transform(x, lengths)` ->
    (features [n, F C], coverage [n, F]); attributes `frequencies_` [F] (Hz), `radius_` [F] (samples on either side), `columns_` [F C, 2]
    ((frequency index, channel) of every column), `n_freqs_`.  `frequencies` overrides the dyadic grid of n_freqs from f_min to f_max (f_max:
    rate / 2 by default).  No tap crosses a sequence boundary; near an edge the amplitude is renormalised by the part of the envelope inside
    (coverage), so a steady oscillation keeps its amplitude there.  output = "log" gives ln(max(A, floor)).  Inputs: numpy arrays, or torch
    device tensors (a row stride is fine), which stay on the device: a tensor in, tensors out.  Every run gives the same bits."""

    def __init__(self, rate: float, frequencies=None, f_min: float = 1.0, f_max: float | None = None, n_freqs: int = 25, omega0: float = 5.0,
                 support: float = 4.0, detrend: bool = True, output: str = "amplitude", floor: float = 1e-3, device="cuda", backend=None):
        rate = float(rate)
        if not rate > 0.0:
            raise ValueError(f"rate must be > 0 (got {rate})")
        if output not in ("amplitude", "log"):
            raise ValueError(f"output must be amplitude or log (got {output})")
        if not float(omega0) > 0.0 or not float(support) > 0.0 or not float(floor) > 0.0:
            raise ValueError(f"omega0, support and floor must be > 0 (got {omega0}, {support}, {floor})")
        freqs = dyadic_frequencies(f_min, 0.5 * rate if f_max is None else f_max, n_freqs) if frequencies is None else np.asarray(frequencies, np.float64).reshape(-1)
        if not 1 <= freqs.shape[0] <= _hip.SPECTROGRAM_MAX_F:
            raise ValueError(f"{freqs.shape[0]} frequencies: the spectrogram takes 1 .. {_hip.SPECTROGRAM_MAX_F}")
        if not ((freqs > 0.0) & (freqs <= 0.5 * rate * (1 + 1e-12))).all():
            raise ValueError(f"every frequency must lie in (0, rate / 2 = {0.5 * rate}] (got {freqs.min():.6g} .. {freqs.max():.6g})")
        freqs = np.minimum(freqs, 0.5 * rate)      # (the last step of a dyadic grid may exceed f_max by a rounding)
        self.rate, self.omega0, self.support, self.detrend, self.output, self.floor = rate, float(omega0), float(support), bool(detrend), output, float(floor)
        self._b = resolve(backend, device)
        try:
            self._bank, self._offset, self.radius_ = self._b.wavelet_bank(rate, freqs, self.omega0, self.support)
        except _hip.TmjxError as e:
            raise ValueError(str(e)) from None
        self.frequencies_, self.n_freqs_ = freqs, int(freqs.shape[0])

    def columns(self, n_channels: int) -> np.ndarray:
        """(frequency index, channel) of every output column for a signal of n_channels."""
        return np.stack(np.divmod(np.arange(self.n_freqs_ * int(n_channels)), int(n_channels)), 1)

    def transform(self, x, lengths):
        xa = self._b.asarray(x)
        n, C = (int(v) for v in xa.shape)
        if C > _hip.SPECTROGRAM_MAX_C:
            raise ValueError(f"{C} channels: the spectrogram takes up to {_hip.SPECTROGRAM_MAX_C}")
        seq = seq_start(lengths, n)
        out, cov = self._b.spectrogram(xa, seq, self._bank, self._offset, self.radius_, self.detrend, self.output == "log", self.floor)
        self.columns_ = self.columns(C)
        if isinstance(x, np.ndarray):
            return self._b.to_numpy(out), self._b.to_numpy(cov)
        return out, cov


def transform_rollouts(rollouts, source: str, cols=None, projections=None, rate: float = 50.0, device="cuda", backend=None, max_width=None, **spectrogram_args):
    """The spectrogram of `source` (see the module's text; `cols` = "a:b" picks columns) of every roll-out, each clip one sequence.  `rollouts`: a
    directory of clip_<i>.h5, or a list of roll-out dicts; `projections`: a pca.h5 whose projections/clip_<i> are the signals instead.
    -> (spec, features, coverage): features[j] float32 [T_j, F C] and coverage[j] [T_j, F] of roll-out j; spec.clips_ are the clip numbers (the
    list positions for dicts), spec.source_, spec.cols_, spec.n_channels_, spec.metas_ (the roll-outs' meta trees).  max_width: refuse more columns
    than this (the command line's 1024)."""
    ids, sigs, metas = signals(rollouts, source, cols, projections)
    spec = Spectrogram(rate, device=device, backend=backend, **spectrogram_args)
    width = spec.n_freqs_ * sigs[0].shape[1]
    if max_width is not None and width > max_width:
        raise ValueError(f"{spec.n_freqs_} frequencies x {sigs[0].shape[1]} channels = {width} columns exceed the {max_width} the clustering, HMM and PCA tools "
                         f"take: pick fewer channels with cols=, fewer frequencies with n_freqs=, or transform the leading components of the layer with "
                         f"projections=<pca.h5>")
    lens = [s.shape[0] for s in sigs]
    feats, cov = spec.transform(np.concatenate(sigs, 0), lens)
    spec.clips_, spec.source_, spec.cols_, spec.n_channels_, spec.metas_ = ids, source, "" if cols is None else str(cols), sigs[0].shape[1], metas
    return spec, split(feats, lens), split(cov, lens)


def main(argv=None, backend=None) -> int:
    opts = cli.parse(argv, CLI_OPTIONS, ("rollouts", "out", "rate"), USAGE, lambda o: "source" in o or "projections" in o)
    if opts is None:
        return 2
    source = opts.get("source", "projections")
    try:
        rate, n_freqs = float(opts["rate"]), int(opts.get("n_freqs", 25))
        args = dict(f_min=float(opts.get("f_min", 1.0)), f_max=float(opts["f_max"]) if "f_max" in opts else None, n_freqs=n_freqs,
                    omega0=float(opts.get("omega0", 5.0)), support=float(opts.get("support", 4.0)), detrend=cli.flag(opts, "detrend", "true"),
                    output=opts.get("output", "amplitude"), floor=float(opts.get("floor", 1e-3)))
        if args["f_max"] is not None and args["f_max"] > 0.5 * rate:
            raise ValueError(f"f_max = {args['f_max']} exceeds rate / 2 = {0.5 * rate}")
        spec, feats, cov = transform_rollouts(opts["rollouts"], source, opts.get("cols"), opts.get("projections"), rate, backend=backend, max_width=MAX_TOOL_WIDTH, **args)
    except (KeyError, ValueError, OSError) as e:
        return cli.report("spectrogram", e)
    meta = {"source": spec.source_, "cols": spec.cols_, "rate": np.float64(rate), "omega0": np.float64(spec.omega0), "support": np.float64(spec.support),
            "detrend": np.int64(spec.detrend), "output": spec.output, "floor": np.float64(spec.floor), "n_channels": np.int64(spec.n_channels_)}
    if "projections" in opts:
        meta["projections"] = os.path.basename(opts["projections"])
    cli.write_clips(opts["out"], {c: {"activations": {"spectrogram": np.ascontiguousarray(f, np.float32)}, "spectrogram_coverage": np.ascontiguousarray(cv, np.float32),
                                      "frequencies": np.asarray(spec.frequencies_, np.float64), "spectrogram_meta": meta, **({} if m is None else {"meta": m})}
                                  for c, f, cv, m in zip(spec.clips_, feats, cov, spec.metas_)})
    print(f"[spectrogram] {source}{'[' + spec.cols_ + ']' if spec.cols_ else ''}: {sum(f.shape[0] for f in feats)} rows x {spec.n_channels_} channels from "
          f"{len(feats)} clips at {spec.n_freqs_} frequencies {spec.frequencies_[0]:.3g} .. {spec.frequencies_[-1]:.3g} Hz (radii {int(spec.radius_.max())} .. "
          f"{int(spec.radius_.min())} samples, output {spec.output}) -> {spec.n_freqs_ * spec.n_channels_} columns; wrote {opts['out']}/clip_<i>.h5", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
