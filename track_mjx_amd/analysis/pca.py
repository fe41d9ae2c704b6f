"""PCA of recorded activations on the GPU (csrc/tmjx_pca.hip; DESIGN.md "PCA").

Reference: track_mjx/analysis/render.py fits sklearn's PCA on a recorded feature (the intention, ctrl or a layer) over many clips and plots the
first components of one clip against the timestep.  Here the fit is two passes over the rows and, for features up to 128 wide, one workgroup of
Jacobi rotations; wider features (the 256- to 1024-wide layers, the LSTM carry), up to 1024, go through block Jacobi on the covariance in global
memory (csrc/tmjx_pca_wide.hip), whose inner solver is that same workgroup.

    python -m track_mjx_amd.analysis.pca rollouts=<dir of clip_<i>.h5> [feature=intention] [n_components=4] out=<pca.h5>

writes mean, components, explained_variance, explained_variance_ratio, feature, n_samples, clips and projections/clip_<i> [T - 1, K];
`python -m track_mjx_amd.analysis.render ... pca=<pca.h5>` draws them beside the frames.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import sys

import numpy as np

from .. import hip as _hip

CLI_OPTIONS = ("rollouts", "out", "feature", "n_components")
# the first eight of matplotlib's default colour cycle (what the reference's curves get), then background, axes, "terminated" line
STRIP_COLOURS = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194), (127, 127, 127))


def strip_style(width: int, height: int, line_half_width: float = 1.0, marker_radius: float = 3.0, colours=STRIP_COLOURS, background=(255, 255, 255),
                axes=(0, 0, 0), terminated=(255, 0, 0), margins=None) -> _hip.StripStyle:
    """tmjx_strip_style_t: `margins` (left, right, top, bottom) in pixels, by default a sixteenth of the panel on every side (at least 2)."""
    st = _hip.StripStyle()
    mx, my = max(int(width) // 16, 2), max(int(height) // 16, 2)
    st.margin_left, st.margin_right, st.margin_top, st.margin_bottom = (mx, mx, my, my) if margins is None else (int(v) for v in margins)
    st.line_half_width, st.marker_radius = float(line_half_width), float(marker_radius)
    for c in range(8):
        st.colour[c][:] = [*colours[c % len(colours)], 255]
    st.background[:], st.axes[:], st.terminated[:] = [*background, 255], [*axes, 255], [*terminated, 255]
    return st


class HipBackend:
    """The PCA and panel entry points on torch device tensors.  A stand-in with the same methods (the CPU tests pass the host emulation's) is
    accepted wherever a `backend` is; one without `fit_wide` / `transform_wide` serves features up to 128 wide only.  The `readout_*` methods are
    analysis.readout's (tmjx_readout_*), the `kmeans_*` methods analysis.cluster's (tmjx_kmeans_*), the `hmm_*` methods analysis.hmm's (tmjx_hmm_*), `wavelet_bank` and
    `spectrogram` analysis.spectrogram's (tmjx_wavelet_bank, tmjx_spectrogram)."""

    def __init__(self, device="cuda", lib=None):
        import torch
        self.device = torch.device(device)
        self._L = _hip.lib() if lib is None else lib

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def asarray(self, x):
        """A 2-D float32 device tensor whose columns are contiguous; a row stride (a column slice of a wider buffer) is kept."""
        import torch
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=np.float32, order="C"))      # (a copy: read-only arrays are fine)
        if t.dim() != 2:
            raise ValueError(f"expected a 2-D array [n, d], got shape {tuple(t.shape)}")
        t = t.to(device=self.device, dtype=torch.float32)
        return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()

    @staticmethod
    def to_numpy(t):
        return t.cpu().numpy()

    def fit(self, x):
        """x from asarray -> (mean [d], components [d, d], variance [d]) float32 numpy, and the call's hip.PcaInfo."""
        return self._fit(x, "tmjx_pca_workspace", "tmjx_pca_fit")

    def _fit(self, x, workspace_entry, fit_entry):
        import torch
        n, d = x.shape
        floats, info = C.c_int64(0), _hip.PcaInfo()
        _hip.check(getattr(self._L, workspace_entry)(n, d, C.byref(floats)), workspace_entry)
        ws = torch.empty(int(floats.value), dtype=torch.float32, device=self.device)
        mean, comp, var = (torch.empty(s, dtype=torch.float32, device=self.device) for s in ((d,), (d, d), (d,)))
        with torch.cuda.device(self.device):
            _hip.check(getattr(self._L, fit_entry)(x.data_ptr(), n, d, x.stride(0), mean.data_ptr(), comp.data_ptr(), var.data_ptr(), ws.data_ptr(),
                                                   C.byref(info), self._stream()), fit_entry)
        return mean.cpu().numpy(), comp.cpu().numpy(), var.cpu().numpy(), info

    def transform(self, x, mean, components):
        """(x - mean) . components^T as a device tensor [n, k]; mean [d] and components [k, d] numpy."""
        return self._transform(x, mean, components, "tmjx_pca_transform")

    def _transform(self, x, mean, components, entry):
        import torch
        n, d = x.shape
        k = components.shape[0]
        m = torch.as_tensor(np.ascontiguousarray(mean, np.float32), device=self.device)
        c = torch.as_tensor(np.ascontiguousarray(components, np.float32), device=self.device)
        out = torch.empty((n, k), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(getattr(self._L, entry)(x.data_ptr(), n, d, x.stride(0), m.data_ptr(), c.data_ptr(), k, out.data_ptr(), k, self._stream()), entry)
        return out

    def fit_wide(self, x):
        """`fit` for d <= 1024 (tmjx_pca_fit_wide: block Jacobi above 128 features, the narrow fit's bits up to 128); info.sweeps: block sweeps."""
        return self._fit(x, "tmjx_pca_wide_workspace", "tmjx_pca_fit_wide")

    def transform_wide(self, x, mean, components):
        """`transform` for d <= 1024 (tmjx_pca_transform_wide)."""
        return self._transform(x, mean, components, "tmjx_pca_transform_wide")

    # the linear readout (analysis/readout.py; tmjx_readout_*): x and y from asarray, everything else float32 numpy
    def _dev(self, a):
        import torch
        return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=self.device)

    def _readout_workspace(self, n, d, m, n_lambda):
        import torch
        floats = C.c_int64(0)
        _hip.check(self._L.tmjx_readout_workspace(n, d, m, n_lambda, C.byref(floats)), "tmjx_readout_workspace")
        return torch.empty(int(floats.value), dtype=torch.float32, device=self.device)

    def readout_fit(self, x, y):
        """-> (mean_x [d], components [d, d], variance [d], mean_y [m], z [d, m]) float32 numpy and the PCA part's hip.PcaInfo (tmjx_readout_fit)."""
        import torch
        (n, d), m = x.shape, y.shape[1]
        ws, info = self._readout_workspace(n, d, m, 1), _hip.PcaInfo()
        mean_x, comp, var, mean_y, z = (torch.empty(s, dtype=torch.float32, device=self.device) for s in ((d,), (d, d), (d,), (m,), (d, m)))
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_readout_fit(x.data_ptr(), n, d, x.stride(0), y.data_ptr(), m, y.stride(0), mean_x.data_ptr(), comp.data_ptr(), var.data_ptr(),
                                                mean_y.data_ptr(), z.data_ptr(), ws.data_ptr(), C.byref(info), self._stream()), "tmjx_readout_fit")
        return (*(t.cpu().numpy() for t in (mean_x, comp, var, mean_y, z)), info)

    def readout_weights(self, components, variance, z, lambdas):
        """lambdas: absolute penalties [L] -> w [L, d, m] float32 numpy (tmjx_readout_weights)."""
        import torch
        d, m = z.shape
        lam = np.ascontiguousarray(lambdas, np.float64)
        comp, var, zz = self._dev(components), self._dev(variance), self._dev(z)
        w = torch.empty((max(lam.shape[0], 1), d, m), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_readout_weights(comp.data_ptr(), var.data_ptr(), zz.data_ptr(), d, m, lam.ctypes.data_as(C.POINTER(C.c_double)), lam.shape[0],
                                                    w.data_ptr(), self._stream()), "tmjx_readout_weights")
        return w.cpu().numpy()

    def readout_predict(self, x, mean_x, w, mean_y):
        """w [d, m] -> (x - mean_x) w + mean_y as a device tensor [n, m] (tmjx_readout_predict)."""
        import torch
        (n, d), m = x.shape, w.shape[1]
        mx, ww, my = self._dev(mean_x), self._dev(w), self._dev(mean_y)
        out = torch.empty((n, m), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_readout_predict(x.data_ptr(), n, d, x.stride(0), mx.data_ptr(), ww.data_ptr(), my.data_ptr(), m, out.data_ptr(), m,
                                                    self._stream()), "tmjx_readout_predict")
        return out

    def readout_score(self, x, y, mean_x, w, mean_y):
        """w [L, d, m] -> (sse [L, m], sst [m]) float64 numpy over the rows given (tmjx_readout_score)."""
        import torch
        (n, d), (L, _, m) = x.shape, w.shape
        mx, ww, my = self._dev(mean_x), self._dev(w), self._dev(mean_y)
        ws = self._readout_workspace(n, d, m, L)
        sse, sst = torch.empty((L, m), dtype=torch.float64, device=self.device), torch.empty((m,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_readout_score(x.data_ptr(), n, d, x.stride(0), y.data_ptr(), m, y.stride(0), mx.data_ptr(), ww.data_ptr(), my.data_ptr(), L,
                                                  sse.data_ptr(), sst.data_ptr(), ws.data_ptr(), self._stream()), "tmjx_readout_score")
        return sse.cpu().numpy(), sst.cpu().numpy()

    # k-means (analysis/cluster.py; tmjx_kmeans_*): x from asarray, centroids float32 numpy [k, d], labels int32 numpy
    def _kmeans_workspace(self, n, d, k):
        import torch
        floats = C.c_int64(0)
        _hip.check(self._L.tmjx_kmeans_workspace(n, d, k, C.byref(floats)), "tmjx_kmeans_workspace")
        return torch.empty(int(floats.value), dtype=torch.float32, device=self.device)

    def _labels(self, labels):
        import torch
        return torch.as_tensor(np.array(labels, dtype=np.int32), device=self.device)      # (a copy: read-only arrays are fine)

    def kmeans_seed(self, x, k, u):
        """k-means++ with the uniforms u [k] -> (centroids [k, d] float32, index [k] int32: the rows chosen) numpy (tmjx_kmeans_seed)."""
        import torch
        n, d = x.shape
        uu = np.ascontiguousarray(u, np.float64)
        if uu.shape != (k,):
            raise ValueError(f"expected {k} uniforms, got shape {uu.shape}")
        ws, index = self._kmeans_workspace(n, d, k), np.zeros(k, np.int32)
        cen = torch.empty((k, d), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_kmeans_seed(x.data_ptr(), n, d, x.stride(0), k, uu.ctypes.data_as(C.POINTER(C.c_double)), cen.data_ptr(),
                                                index.ctypes.data_as(C.POINTER(C.c_int32)), ws.data_ptr(), self._stream()), "tmjx_kmeans_seed")
        return cen.cpu().numpy(), index

    def kmeans_assign(self, x, centroids, labels_prev=None):
        """-> (labels [n] int32, dist2 [n] float32, inertia float, changed int: the rows whose label differs from labels_prev, n without one)
        (tmjx_kmeans_assign)."""
        import torch
        (n, d), k = x.shape, centroids.shape[0]
        cen, ws = self._dev(np.array(centroids, dtype=np.float32)), self._kmeans_workspace(n, d, k)
        prev = None if labels_prev is None else self._labels(labels_prev)
        labels, dist2 = torch.empty(n, dtype=torch.int32, device=self.device), torch.empty(n, dtype=torch.float32, device=self.device)
        inertia, changed = torch.zeros(1, dtype=torch.float64, device=self.device), torch.zeros(1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_kmeans_assign(x.data_ptr(), n, d, x.stride(0), cen.data_ptr(), k, None if prev is None else prev.data_ptr(), labels.data_ptr(),
                                                  dist2.data_ptr(), inertia.data_ptr(), changed.data_ptr(), ws.data_ptr(), self._stream()), "tmjx_kmeans_assign")
        return labels.cpu().numpy(), dist2.cpu().numpy(), float(inertia.item()), int(changed.item())

    def kmeans_update(self, x, labels, centroids):
        """-> (centroids [k, d] float32: the mean of each cluster's rows, an empty cluster's row as given; counts [k] int32) (tmjx_kmeans_update)."""
        import torch
        (n, d), k = x.shape, centroids.shape[0]
        cen, lab, ws = self._dev(np.array(centroids, dtype=np.float32)), self._labels(labels), self._kmeans_workspace(n, d, k)
        counts = torch.empty(k, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_kmeans_update(x.data_ptr(), n, d, x.stride(0), lab.data_ptr(), k, cen.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                                  self._stream()), "tmjx_kmeans_update")
        return cen.cpu().numpy(), counts.cpu().numpy()

    def kmeans_fit(self, x, centroids, max_iter=100, tol=1e-4):
        """Lloyd's iteration from `centroids` -> (centroids, labels int32 [n], dist2 float32 [n]) numpy and the call's hip.KMeansInfo (tmjx_kmeans_fit)."""
        import torch
        (n, d), k = x.shape, centroids.shape[0]
        cen, ws, info = self._dev(np.array(centroids, dtype=np.float32)), self._kmeans_workspace(n, d, k), _hip.KMeansInfo()
        labels, dist2 = torch.empty(n, dtype=torch.int32, device=self.device), torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_kmeans_fit(x.data_ptr(), n, d, x.stride(0), k, cen.data_ptr(), labels.data_ptr(), dist2.data_ptr(), int(max_iter), float(tol),
                                               C.byref(info), ws.data_ptr(), self._stream()), "tmjx_kmeans_fit")
        return cen.cpu().numpy(), labels.cpu().numpy(), dist2.cpu().numpy(), info

    # the hidden Markov model (analysis/hmm.py; tmjx_hmm_*): x from asarray; logb, gamma and the parameters float32 numpy; seq_start int32 [S + 1]
    def _hmm_workspace(self, n, d, k, S):
        import torch
        floats = C.c_int64(0)
        _hip.check(self._L.tmjx_hmm_workspace(n, d, k, S, C.byref(floats)), "tmjx_hmm_workspace")
        return torch.empty(int(floats.value), dtype=torch.float32, device=self.device)

    @staticmethod
    def _seq(seq_start):
        seq = np.ascontiguousarray(seq_start, np.int32)
        return seq, seq.ctypes.data_as(C.POINTER(C.c_int32)), seq.shape[0] - 1

    def _devc(self, a):
        return self._dev(np.array(a, dtype=np.float32))      # (a copy: read-only arrays are fine)

    def _f64(self, shape):
        import torch
        return torch.empty(shape, dtype=torch.float64, device=self.device)

    def hmm_emission(self, x, means, vars):
        """-> logb [n, k] float32: the log density of every row under every state's diagonal Gaussian (tmjx_hmm_emission)."""
        import torch
        (n, d), k = x.shape, means.shape[0]
        mu, var, ws = self._devc(means), self._devc(vars), self._hmm_workspace(n, d, k, 1)
        logb = torch.empty((n, k), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_hmm_emission(x.data_ptr(), n, d, x.stride(0), mu.data_ptr(), var.data_ptr(), k, logb.data_ptr(), ws.data_ptr(), self._stream()),
                       "tmjx_hmm_emission")
        return logb.cpu().numpy()

    def hmm_forward_backward(self, logb, seq_start, transmat, startprob):
        """-> (gamma [n, k] float32, xi [k, k] float64, start [k] float64, loglik [S] float64, their total) (tmjx_hmm_forward_backward)."""
        import torch
        n, k = logb.shape
        seq, seq_p, S = self._seq(seq_start)
        lb, A, pi, ws = self._devc(logb), self._devc(transmat), self._devc(startprob), self._hmm_workspace(n, 1, k, S)
        gamma = torch.empty((n, k), dtype=torch.float32, device=self.device)
        xi, start, loglik, total = self._f64((k, k)), self._f64((k,)), self._f64((S,)), self._f64((1,))
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_hmm_forward_backward(lb.data_ptr(), n, k, seq_p, S, A.data_ptr(), pi.data_ptr(), gamma.data_ptr(), xi.data_ptr(), start.data_ptr(),
                                                         loglik.data_ptr(), total.data_ptr(), ws.data_ptr(), self._stream()), "tmjx_hmm_forward_backward")
        return gamma.cpu().numpy(), xi.cpu().numpy(), start.cpu().numpy(), loglik.cpu().numpy(), float(total.item())

    def hmm_mstep(self, x, gamma, means, vars, min_var=0.0, min_weight=0.0):
        """-> (means, vars [k, d] float32, weight [k] float64): the weighted moments of every state; one below min_weight as given (tmjx_hmm_mstep)."""
        (n, d), k = x.shape, means.shape[0]
        g, mu, var, ws, weight = self._devc(gamma), self._devc(means), self._devc(vars), self._hmm_workspace(n, d, k, 1), self._f64((k,))
        import torch
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_hmm_mstep(x.data_ptr(), n, d, x.stride(0), g.data_ptr(), k, float(min_var), float(min_weight), mu.data_ptr(), var.data_ptr(),
                                              weight.data_ptr(), ws.data_ptr(), self._stream()), "tmjx_hmm_mstep")
        return mu.cpu().numpy(), var.cpu().numpy(), weight.cpu().numpy()

    def hmm_transitions(self, xi, start, prior, kappa, transmat, startprob):
        """-> (transmat [k, k], startprob [k]) float32 from expected counts and Dirichlet pseudo-counts; a row without mass as given (tmjx_hmm_transitions)."""
        import torch
        k = len(start)
        xx = torch.as_tensor(np.ascontiguousarray(xi, np.float64), device=self.device)
        st = torch.as_tensor(np.ascontiguousarray(start, np.float64), device=self.device)
        A, pi = self._devc(transmat), self._devc(startprob)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_hmm_transitions(xx.data_ptr(), st.data_ptr(), k, float(prior), float(kappa), A.data_ptr(), pi.data_ptr(), self._stream()),
                       "tmjx_hmm_transitions")
        return A.cpu().numpy(), pi.cpu().numpy()

    def hmm_viterbi(self, logb, seq_start, transmat, startprob, logspace=False):
        """-> (labels [n] int32: the best path of every sequence, path_logprob [S] float64); logspace: the parameters hold logarithms (tmjx_hmm_viterbi)."""
        import torch
        n, k = logb.shape
        seq, seq_p, S = self._seq(seq_start)
        lb, A, pi, ws = self._devc(logb), self._devc(transmat), self._devc(startprob), self._hmm_workspace(n, 1, k, S)
        labels, path = torch.empty(n, dtype=torch.int32, device=self.device), self._f64((S,))
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_hmm_viterbi(lb.data_ptr(), n, k, seq_p, S, A.data_ptr(), pi.data_ptr(), int(bool(logspace)), labels.data_ptr(), path.data_ptr(),
                                                ws.data_ptr(), self._stream()), "tmjx_hmm_viterbi")
        return labels.cpu().numpy(), path.cpu().numpy()

    def hmm_fit(self, x, seq_start, means, vars, transmat, startprob, max_iter=50, tol=1e-4, prior=0.0, kappa=0.0, min_var=0.0, min_weight=0.0):
        """EM from the parameters given -> (means, vars, transmat, startprob, gamma [n, k], labels [n] int32) numpy and the call's hip.HmmInfo
        (tmjx_hmm_fit)."""
        import torch
        (n, d), k = x.shape, means.shape[0]
        seq, seq_p, S = self._seq(seq_start)
        mu, var, A, pi = (self._devc(a) for a in (means, vars, transmat, startprob))
        ws, info = self._hmm_workspace(n, d, k, S), _hip.HmmInfo()
        gamma, labels = torch.empty((n, k), dtype=torch.float32, device=self.device), torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_hmm_fit(x.data_ptr(), n, d, x.stride(0), seq_p, S, k, mu.data_ptr(), var.data_ptr(), A.data_ptr(), pi.data_ptr(), gamma.data_ptr(),
                                            labels.data_ptr(), int(max_iter), float(tol), float(prior), float(kappa), float(min_var), float(min_weight),
                                            C.byref(info), ws.data_ptr(), self._stream()), "tmjx_hmm_fit")
        return (*(t.cpu().numpy() for t in (mu, var, A, pi, gamma, labels)), info)

    # the wavelet spectrogram (analysis/spectrogram.py; tmjx_wavelet_bank*, tmjx_spectrogram*): x from asarray, the bank as wavelet_bank returns it
    def wavelet_bank(self, rate, freqs, omega0=5.0, support=4.0):
        """-> (bank float32, offset int32 [F + 1], radius int32 [F]) numpy: the Morlet tables of every frequency (tmjx_wavelet_bank, a host function)."""
        fr = np.ascontiguousarray(freqs, np.float64).reshape(-1)
        F, floats, dp = fr.shape[0], C.c_int64(0), fr.ctypes.data_as(C.POINTER(C.c_double))
        _hip.check(self._L.tmjx_wavelet_bank_size(float(rate), dp, F, float(omega0), float(support), C.byref(floats)), "tmjx_wavelet_bank_size")
        bank, offset, radius = np.zeros(int(floats.value), np.float32), np.zeros(F + 1, np.int32), np.zeros(F, np.int32)
        _hip.check(self._L.tmjx_wavelet_bank(float(rate), dp, F, float(omega0), float(support), bank.ctypes.data, offset.ctypes.data_as(C.POINTER(C.c_int32)),
                                             radius.ctypes.data_as(C.POINTER(C.c_int32))), "tmjx_wavelet_bank")
        return bank, offset, radius

    def spectrogram(self, x, seq_start, bank, offset, radius, detrend=True, log=False, floor=1e-3, out=None):
        """-> (out [n, F C], coverage [n, F]) device tensors: the amplitude (or its logarithm) of every channel at every frequency, column j C + c,
        and the share of each window inside its sequence (tmjx_spectrogram).  `out`: a device tensor [n, F C] to write into (a row stride is fine)."""
        import torch
        n, Cn = x.shape
        seq, seq_p, S = self._seq(seq_start)
        off, rad = np.ascontiguousarray(offset, np.int32), np.ascontiguousarray(radius, np.int32)
        F, i32p = rad.shape[0], C.POINTER(C.c_int32)
        bk, floats = self._dev(bank), C.c_int64(0)
        _hip.check(self._L.tmjx_spectrogram_workspace(n, Cn, F, S, C.byref(floats)), "tmjx_spectrogram_workspace")
        ws = torch.empty(int(floats.value), dtype=torch.float32, device=self.device)
        if out is None:
            out = torch.empty((n, F * Cn), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (n, F * Cn) or out.dtype != torch.float32 or out.stride(1) != 1:
            raise ValueError(f"out must be a float32 device tensor [{n}, {F * Cn}] with contiguous columns")
        cov = torch.empty((n, F), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_spectrogram(x.data_ptr(), n, Cn, x.stride(0), seq_p, S, bk.data_ptr(), off.ctypes.data_as(i32p), rad.ctypes.data_as(i32p), F,
                                                int(bool(detrend)), _hip.SPECTROGRAM_LOG if log else _hip.SPECTROGRAM_AMPLITUDE, float(floor), out.data_ptr(),
                                                out.stride(0), cov.data_ptr(), ws.data_ptr(), self._stream()), "tmjx_spectrogram")
            torch.cuda.current_stream(self.device).synchronize()      # (the host offsets must outlive the queued copies)
        return out, cov

    def strips(self, proj, k, frame_idx, flags, ymin, ymax, window, style, width, height):
        """One tmjx_plot_strips call: proj from asarray, frame_idx / flags numpy -> rgba uint8 numpy [F, H, W, 4]."""
        import torch
        fi = torch.as_tensor(np.ascontiguousarray(frame_idx, np.int32), device=self.device)
        fl = torch.as_tensor(np.ascontiguousarray(flags, np.uint8), device=self.device)
        F = fi.shape[0]
        out = torch.empty((F, max(height, 0), max(width, 0), 4), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self._L.tmjx_plot_strips(proj.data_ptr(), proj.shape[0], k, proj.stride(0), fi.data_ptr(), fl.data_ptr(), F, ymin, ymax, window,
                                                C.byref(style), width, height, out.data_ptr(), self._stream()), "tmjx_plot_strips")
        return out.cpu().numpy()


class PCA:
    """Principal components of [n, d] rows, d <= 1024: `fit`, `transform`, `fit_transform`, and after a fit `mean_` [D], `components_` [K, D] (unit rows,
    descending variance, the largest-magnitude coefficient of each positive), `explained_variance_` [K], `explained_variance_ratio_` [K] (zeros when
    the total variance is 0), `n_samples_`, `n_sweeps_` (Jacobi sweeps; above 128 features the block sweeps, also in `n_block_sweeps_`, which is 0
    for a narrow fit).  Features wider than 128 go through the backend's `fit_wide` / `transform_wide` where it has them.  Inputs: numpy arrays, or torch device tensors (a row stride is fine: activations are
    stored as column slices of wider buffers).  `transform` returns numpy for numpy, a device tensor for a tensor."""

    def __init__(self, n_components: int | None = None, device="cuda", backend=None):
        if n_components is not None and int(n_components) < 1:
            raise ValueError(f"n_components must be >= 1 (got {n_components})")
        self.n_components = None if n_components is None else int(n_components)
        self._b = HipBackend(device) if backend is None else backend

    def fit(self, x):
        xa = self._b.asarray(x)
        n, d = (int(v) for v in xa.shape)
        k = min(n, d) if self.n_components is None else self.n_components
        if k > d:
            raise ValueError(f"n_components = {k} exceeds the {d} features")
        wide = d > _hip.PCA_MAX_D and hasattr(self._b, "fit_wide")
        mean, comp, var, info = self._b.fit_wide(xa) if wide else self._b.fit(xa)
        total = float(var.astype(np.float64).sum())
        self.mean_, self.components_, self.explained_variance_ = mean, np.ascontiguousarray(comp[:k]), var[:k].copy()
        self.explained_variance_ratio_ = (var[:k].astype(np.float64) / total).astype(np.float32) if total > 0.0 else np.zeros(k, np.float32)
        self.n_samples_, self.n_features_, self.n_sweeps_, self.off_rel_ = n, d, int(info.sweeps), float(info.off_rel)
        self.moments_ms_, self.jacobi_ms_, self.n_block_sweeps_ = float(info.moments_ms), float(info.jacobi_ms), int(info.sweeps) if wide else 0
        return self

    def transform(self, x):
        if not hasattr(self, "components_"):
            raise ValueError("this PCA is not fitted")
        xa = self._b.asarray(x)
        if xa.shape[1] != self.n_features_:
            raise ValueError(f"expected {self.n_features_} features, got {xa.shape[1]}")
        wide = self.n_features_ > _hip.PCA_MAX_D and hasattr(self._b, "transform_wide")
        out = self._b.transform_wide(xa, self.mean_, self.components_) if wide else self._b.transform(xa, self.mean_, self.components_)
        return self._b.to_numpy(out) if isinstance(x, np.ndarray) else out

    def fit_transform(self, x):
        return self.fit(x).transform(x)


def _feature_of(rollout, feature: str, where: str) -> np.ndarray:
    """The recorded feature of one roll-out as [T, D]: `ctrl`, or a path under activations/ (intention, decoder/layer_0, hidden_state/h, ...)."""
    node, path = rollout, ([feature] if feature == "ctrl" else ["activations", *[p for p in feature.split("/") if p]])
    for part in path:
        try:
            node = node[part]
        except (KeyError, IndexError, TypeError):
            raise KeyError(f"{where} has no {'/'.join(path)}" + (" (roll it out with log_activations=true)" if feature != "ctrl" else "")) from None
    if hasattr(node, "keys"):
        raise KeyError(f"{where}: {'/'.join(path)} is a group ({', '.join(node.keys())}), not a recorded array")
    a = np.asarray(node if isinstance(node, (np.ndarray, list, tuple)) else node[()], np.float32)      # (an h5lite dataset reads with [()])
    if a.ndim < 2:
        raise ValueError(f"{where}: {'/'.join(path)} has shape {a.shape}, expected [T, D]")
    return a.reshape(-1, a.shape[-1])


def fit_rollouts(rollouts, feature: str = "intention", n_components: int | None = None, device="cuda", backend=None):
    """Fit one PCA on `feature` (up to 1024 wide) over every roll-out and project each.  `rollouts`: a directory of clip_<i>.h5, or a list of roll-out dicts.
    -> (pca, projections): projections[j] float32 [T_j, K] of roll-out j; pca.clips_ are the clip numbers (the list positions for dicts)."""
    if isinstance(rollouts, (str, os.PathLike)):
        from .. import h5lite
        ids = sorted(int(m.group(1)) for m in (re.fullmatch(r"clip_(\d+)\.h5", f) for f in os.listdir(rollouts)) if m)
        if not ids:
            raise ValueError(f"no clip_<i>.h5 in {rollouts}")
        feats = []
        for c in ids:
            with h5lite.File(os.path.join(rollouts, f"clip_{c}.h5")) as h:
                feats.append(_feature_of(h, feature, f"clip_{c}.h5"))
    else:
        ids = list(range(len(rollouts)))
        if not ids:
            raise ValueError("no roll-outs to fit")
        feats = [_feature_of(r, feature, f"roll-out {j}") for j, r in enumerate(rollouts)]
    widths = {f.shape[1] for f in feats}
    if len(widths) != 1:
        raise ValueError(f"{feature} has different widths across roll-outs: {sorted(widths)}")
    pca = PCA(n_components, device=device, backend=backend)
    x = pca._b.asarray(np.concatenate(feats, 0))
    proj = pca._b.to_numpy(pca.fit(x).transform(x))
    pca.clips_, pca.feature_ = ids, feature
    ends = np.cumsum([f.shape[0] for f in feats])
    return pca, [proj[e - f.shape[0]:e] for e, f in zip(ends, feats)]


def main(argv=None, backend=None) -> int:
    from .. import h5lite
    argv = list(sys.argv[1:] if argv is None else argv)
    opts = dict(a.split("=", 1) for a in argv if "=" in a and a.split("=", 1)[0] in CLI_OPTIONS)
    if "rollouts" not in opts or "out" not in opts or len(opts) != len(argv):
        print("usage: python -m track_mjx_amd.analysis.pca rollouts=<dir of clip_<i>.h5> [feature=intention] [n_components=4] out=<pca.h5>", file=sys.stderr)
        return 2
    feature = opts.get("feature", "intention")
    try:
        pca, proj = fit_rollouts(opts["rollouts"], feature, int(opts.get("n_components", 4)), backend=backend)
    except (KeyError, ValueError) as e:
        print(f"[pca] {e.args[0] if e.args else e}", file=sys.stderr)
        return 2
    os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
    h5lite.write_tree(opts["out"], {"mean": pca.mean_, "components": pca.components_, "explained_variance": pca.explained_variance_,
                                    "explained_variance_ratio": pca.explained_variance_ratio_, "feature": feature, "n_samples": np.int64(pca.n_samples_),
                                    "clips": np.asarray(pca.clips_, np.int64), "projections": {f"clip_{c}": p for c, p in zip(pca.clips_, proj)}})
    ratio = ", ".join(f"{100 * r:.1f}%" for r in pca.explained_variance_ratio_)
    print(f"[pca] {feature}: {pca.n_samples_} samples x {pca.n_features_} features from {len(proj)} clips, {pca.n_sweeps_} sweeps; explained variance "
          f"{ratio}; wrote {opts['out']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
