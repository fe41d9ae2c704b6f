"""The analysis entry points of the C-ABI (include/tmjx.h: tmjx_pca_*, tmjx_plot_strips, tmjx_readout_*, tmjx_kmeans_*, tmjx_hmm_*, tmjx_arhmm_*,
tmjx_wavelet_bank*, tmjx_spectrogram*, tmjx_knn, tmjx_tsne_*, tmjx_cka_linear, tmjx_rdm_corr, tmjx_cca, tmjx_compare_svd, tmjx_decoder_jacobian, tmjx_lstm_decoder_jacobian, tmjx_lstm_tangent_step, tmjx_lstm_lyapunov) as methods on
arrays.

`Backend` marshals every call once, against a small provider of arrays: what differs between the device and a host is how an array is uploaded,
allocated, addressed and read back, not which arguments go where.  `HipBackend` is the backend on torch device tensors (`TorchArrays`), the one
the product uses; the CPU tests run the same methods on numpy arrays against the host emulation of the kernels (tests/hostemu/), so the
marshalling below is executed without a GPU.

A provider has: `lib` (the library handle), `check(rc, what)` (raises on a non-zero return code), `rows(x)` (a 2-D float32 array whose columns are
contiguous, a row stride kept), `upload(a, dtype, copy=False)`, `empty(shape, dtype, zero=False)`, `host_empty(shape, dtype)` (for what a host
function fills), `workspace(floats)`, `ptr(a)`, `ld(a)` (the row stride in elements), `dense_columns(a)`, `stream()`, `guard()` (a context manager
around a launch), `to_numpy(a)` and `sync()`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import hip as _hip

_I32P, _F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
f32, f64, i32 = np.float32, np.float64, np.int32


class Backend:
    """x (and y, proj) come from `asarray`; every other input is a numpy array.  Which outputs are numpy and which stay the provider's arrays is
    said per method."""

    def __init__(self, arrays):
        self._p = arrays

    def _call(self, name, *args):
        with self._p.guard():
            self._p.check(getattr(self._p.lib, name)(*args), name)

    def _workspace(self, name, *dims):
        """The workspace `name` (a tmjx_*_workspace entry) reports for `dims`."""
        floats = C.c_int64(0)
        self._p.check(getattr(self._p.lib, name)(*dims, C.byref(floats)), name)
        return self._p.workspace(int(floats.value))

    def asarray(self, x):
        """A 2-D float32 array of the provider whose columns are contiguous; a row stride (a column slice of a wider buffer) is kept."""
        shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
        if len(shape) != 2:
            raise ValueError(f"expected a 2-D array [n, d], got shape {shape}")
        return self._p.rows(x)

    def to_numpy(self, t):
        return self._p.to_numpy(t)

    # PCA (analysis/pca.py; tmjx_pca_*)
    def fit(self, x):
        """x from asarray -> (mean [d], components [d, d], variance [d]) float32 numpy, and the call's hip.PcaInfo."""
        return self._fit(x, "tmjx_pca_workspace", "tmjx_pca_fit")

    def _fit(self, x, workspace_entry, fit_entry):
        p = self._p
        n, d = x.shape
        ws, info = self._workspace(workspace_entry, n, d), _hip.PcaInfo()
        mean, comp, var = (p.empty(s, f32) for s in ((d,), (d, d), (d,)))
        self._call(fit_entry, p.ptr(x), n, d, p.ld(x), p.ptr(mean), p.ptr(comp), p.ptr(var), p.ptr(ws), C.byref(info), p.stream())
        return p.to_numpy(mean), p.to_numpy(comp), p.to_numpy(var), info

    def transform(self, x, mean, components):
        """(x - mean) . components^T as the provider's array [n, k]; mean [d] and components [k, d] numpy."""
        return self._transform(x, mean, components, "tmjx_pca_transform")

    def _transform(self, x, mean, components, entry):
        p = self._p
        n, d = x.shape
        k = components.shape[0]
        m, c = p.upload(mean, f32), p.upload(components, f32)
        out = p.empty((n, k), f32)
        self._call(entry, p.ptr(x), n, d, p.ld(x), p.ptr(m), p.ptr(c), k, p.ptr(out), k, p.stream())
        return out

    def fit_wide(self, x):
        """`fit` for d <= 1024 (tmjx_pca_fit_wide: block Jacobi above 128 features, the narrow fit's bits up to 128); info.sweeps: block sweeps."""
        return self._fit(x, "tmjx_pca_wide_workspace", "tmjx_pca_fit_wide")

    def transform_wide(self, x, mean, components):
        """`transform` for d <= 1024 (tmjx_pca_transform_wide)."""
        return self._transform(x, mean, components, "tmjx_pca_transform_wide")

    # the linear readout (analysis/readout.py; tmjx_readout_*): x and y from asarray, everything else float32 numpy
    def readout_fit(self, x, y):
        """-> (mean_x [d], components [d, d], variance [d], mean_y [m], z [d, m]) float32 numpy and the PCA part's hip.PcaInfo (tmjx_readout_fit)."""
        p = self._p
        (n, d), m = x.shape, y.shape[1]
        ws, info = self._workspace("tmjx_readout_workspace", n, d, m, 1), _hip.PcaInfo()
        mean_x, comp, var, mean_y, z = (p.empty(s, f32) for s in ((d,), (d, d), (d,), (m,), (d, m)))
        self._call("tmjx_readout_fit", p.ptr(x), n, d, p.ld(x), p.ptr(y), m, p.ld(y), p.ptr(mean_x), p.ptr(comp), p.ptr(var), p.ptr(mean_y), p.ptr(z),
                   p.ptr(ws), C.byref(info), p.stream())
        return (*(p.to_numpy(t) for t in (mean_x, comp, var, mean_y, z)), info)

    def readout_weights(self, components, variance, z, lambdas):
        """lambdas: absolute penalties [L] -> w [L, d, m] float32 numpy (tmjx_readout_weights)."""
        p = self._p
        d, m = z.shape
        lam = np.ascontiguousarray(lambdas, f64)
        comp, var, zz = p.upload(components, f32), p.upload(variance, f32), p.upload(z, f32)
        w = p.empty((max(lam.shape[0], 1), d, m), f32)
        self._call("tmjx_readout_weights", p.ptr(comp), p.ptr(var), p.ptr(zz), d, m, lam.ctypes.data_as(_F64P), lam.shape[0], p.ptr(w), p.stream())
        return p.to_numpy(w)

    def readout_predict(self, x, mean_x, w, mean_y):
        """w [d, m] -> (x - mean_x) w + mean_y as the provider's array [n, m] (tmjx_readout_predict)."""
        p = self._p
        (n, d), m = x.shape, w.shape[1]
        mx, ww, my = p.upload(mean_x, f32), p.upload(w, f32), p.upload(mean_y, f32)
        out = p.empty((n, m), f32)
        self._call("tmjx_readout_predict", p.ptr(x), n, d, p.ld(x), p.ptr(mx), p.ptr(ww), p.ptr(my), m, p.ptr(out), m, p.stream())
        return out

    def readout_score(self, x, y, mean_x, w, mean_y):
        """w [L, d, m] -> (sse [L, m], sst [m]) float64 numpy over the rows given (tmjx_readout_score)."""
        p = self._p
        (n, d), (L, _, m) = x.shape, w.shape
        mx, ww, my = p.upload(mean_x, f32), p.upload(w, f32), p.upload(mean_y, f32)
        ws = self._workspace("tmjx_readout_workspace", n, d, m, L)
        sse, sst = p.empty((L, m), f64), p.empty((m,), f64)
        self._call("tmjx_readout_score", p.ptr(x), n, d, p.ld(x), p.ptr(y), m, p.ld(y), p.ptr(mx), p.ptr(ww), p.ptr(my), L, p.ptr(sse), p.ptr(sst),
                   p.ptr(ws), p.stream())
        return p.to_numpy(sse), p.to_numpy(sst)

    # k-means (analysis/cluster.py; tmjx_kmeans_*): x from asarray, centroids float32 numpy [k, d], labels int32 numpy (copied: read-only is fine)
    def kmeans_seed(self, x, k, u):
        """k-means++ with the uniforms u [k] -> (centroids [k, d] float32, index [k] int32: the rows chosen) numpy (tmjx_kmeans_seed)."""
        p = self._p
        n, d = x.shape
        uu = np.ascontiguousarray(u, f64)
        if uu.shape != (k,):
            raise ValueError(f"expected {k} uniforms, got shape {uu.shape}")
        ws, index = self._workspace("tmjx_kmeans_workspace", n, d, k), p.host_empty((k,), i32)
        cen = p.empty((k, d), f32)
        self._call("tmjx_kmeans_seed", p.ptr(x), n, d, p.ld(x), k, uu.ctypes.data_as(_F64P), p.ptr(cen), index.ctypes.data_as(_I32P), p.ptr(ws), p.stream())
        return p.to_numpy(cen), index

    def kmeans_assign(self, x, centroids, labels_prev=None):
        """-> (labels [n] int32, dist2 [n] float32, inertia float, changed int: the rows whose label differs from labels_prev, n without one)
        (tmjx_kmeans_assign)."""
        p = self._p
        (n, d), k = x.shape, centroids.shape[0]
        cen, ws = p.upload(centroids, f32, copy=True), self._workspace("tmjx_kmeans_workspace", n, d, k)
        prev = None if labels_prev is None else p.upload(labels_prev, i32, copy=True)
        labels, dist2 = p.empty((n,), i32), p.empty((n,), f32)
        inertia, changed = p.empty((1,), f64, zero=True), p.empty((1,), i32, zero=True)
        self._call("tmjx_kmeans_assign", p.ptr(x), n, d, p.ld(x), p.ptr(cen), k, None if prev is None else p.ptr(prev), p.ptr(labels), p.ptr(dist2),
                   p.ptr(inertia), p.ptr(changed), p.ptr(ws), p.stream())
        return p.to_numpy(labels), p.to_numpy(dist2), float(inertia.item()), int(changed.item())

    def kmeans_update(self, x, labels, centroids):
        """-> (centroids [k, d] float32: the mean of each cluster's rows, an empty cluster's row as given; counts [k] int32) (tmjx_kmeans_update)."""
        p = self._p
        (n, d), k = x.shape, centroids.shape[0]
        cen, lab, ws = p.upload(centroids, f32, copy=True), p.upload(labels, i32, copy=True), self._workspace("tmjx_kmeans_workspace", n, d, k)
        counts = p.empty((k,), i32)
        self._call("tmjx_kmeans_update", p.ptr(x), n, d, p.ld(x), p.ptr(lab), k, p.ptr(cen), p.ptr(counts), p.ptr(ws), p.stream())
        return p.to_numpy(cen), p.to_numpy(counts)

    def kmeans_fit(self, x, centroids, max_iter=100, tol=1e-4):
        """Lloyd's iteration from `centroids` -> (centroids, labels int32 [n], dist2 float32 [n]) numpy and the call's hip.KMeansInfo (tmjx_kmeans_fit)."""
        p = self._p
        (n, d), k = x.shape, centroids.shape[0]
        cen, ws, info = p.upload(centroids, f32, copy=True), self._workspace("tmjx_kmeans_workspace", n, d, k), _hip.KMeansInfo()
        labels, dist2 = p.empty((n,), i32), p.empty((n,), f32)
        self._call("tmjx_kmeans_fit", p.ptr(x), n, d, p.ld(x), k, p.ptr(cen), p.ptr(labels), p.ptr(dist2), int(max_iter), float(tol), C.byref(info),
                   p.ptr(ws), p.stream())
        return p.to_numpy(cen), p.to_numpy(labels), p.to_numpy(dist2), info

    # the hidden Markov model (analysis/hmm.py; tmjx_hmm_*): x from asarray; logb, gamma and the parameters float32 numpy (copied: read-only is
    # fine, and the in-place entry points never touch the caller's); seq_start int32 [S + 1]
    @staticmethod
    def _seq(seq_start):
        seq = np.ascontiguousarray(seq_start, i32)
        return seq, seq.ctypes.data_as(_I32P), seq.shape[0] - 1

    def hmm_emission(self, x, means, vars):
        """-> logb [n, k] float32: the log density of every row under every state's diagonal Gaussian (tmjx_hmm_emission)."""
        p = self._p
        (n, d), k = x.shape, means.shape[0]
        mu, var, ws = p.upload(means, f32, copy=True), p.upload(vars, f32, copy=True), self._workspace("tmjx_hmm_workspace", n, d, k, 1)
        logb = p.empty((n, k), f32)
        self._call("tmjx_hmm_emission", p.ptr(x), n, d, p.ld(x), p.ptr(mu), p.ptr(var), k, p.ptr(logb), p.ptr(ws), p.stream())
        return p.to_numpy(logb)

    def hmm_forward_backward(self, logb, seq_start, transmat, startprob):
        """-> (gamma [n, k] float32, xi [k, k] float64, start [k] float64, loglik [S] float64, their total) (tmjx_hmm_forward_backward)."""
        p = self._p
        n, k = logb.shape
        seq, seq_p, S = self._seq(seq_start)
        lb, A, pi = (p.upload(a, f32, copy=True) for a in (logb, transmat, startprob))
        ws = self._workspace("tmjx_hmm_workspace", n, 1, k, S)
        gamma = p.empty((n, k), f32)
        xi, start, loglik, total = p.empty((k, k), f64), p.empty((k,), f64), p.empty((S,), f64), p.empty((1,), f64)
        self._call("tmjx_hmm_forward_backward", p.ptr(lb), n, k, seq_p, S, p.ptr(A), p.ptr(pi), p.ptr(gamma), p.ptr(xi), p.ptr(start), p.ptr(loglik),
                   p.ptr(total), p.ptr(ws), p.stream())
        return p.to_numpy(gamma), p.to_numpy(xi), p.to_numpy(start), p.to_numpy(loglik), float(total.item())

    def hmm_mstep(self, x, gamma, means, vars, min_var=0.0, min_weight=0.0):
        """-> (means, vars [k, d] float32, weight [k] float64): the weighted moments of every state; one below min_weight as given (tmjx_hmm_mstep)."""
        p = self._p
        (n, d), k = x.shape, means.shape[0]
        g, mu, var = (p.upload(a, f32, copy=True) for a in (gamma, means, vars))
        ws, weight = self._workspace("tmjx_hmm_workspace", n, d, k, 1), p.empty((k,), f64)
        self._call("tmjx_hmm_mstep", p.ptr(x), n, d, p.ld(x), p.ptr(g), k, float(min_var), float(min_weight), p.ptr(mu), p.ptr(var), p.ptr(weight),
                   p.ptr(ws), p.stream())
        return p.to_numpy(mu), p.to_numpy(var), p.to_numpy(weight)

    def hmm_transitions(self, xi, start, prior, kappa, transmat, startprob):
        """-> (transmat [k, k], startprob [k]) float32 from expected counts and Dirichlet pseudo-counts; a row without mass as given (tmjx_hmm_transitions)."""
        p = self._p
        k = len(start)
        xx, st = p.upload(xi, f64), p.upload(start, f64)
        A, pi = p.upload(transmat, f32, copy=True), p.upload(startprob, f32, copy=True)
        self._call("tmjx_hmm_transitions", p.ptr(xx), p.ptr(st), k, float(prior), float(kappa), p.ptr(A), p.ptr(pi), p.stream())
        return p.to_numpy(A), p.to_numpy(pi)

    def hmm_viterbi(self, logb, seq_start, transmat, startprob, logspace=False):
        """-> (labels [n] int32: the best path of every sequence, path_logprob [S] float64); logspace: the parameters hold logarithms (tmjx_hmm_viterbi)."""
        p = self._p
        n, k = logb.shape
        seq, seq_p, S = self._seq(seq_start)
        lb, A, pi = (p.upload(a, f32, copy=True) for a in (logb, transmat, startprob))
        ws = self._workspace("tmjx_hmm_workspace", n, 1, k, S)
        labels, path = p.empty((n,), i32), p.empty((S,), f64)
        self._call("tmjx_hmm_viterbi", p.ptr(lb), n, k, seq_p, S, p.ptr(A), p.ptr(pi), int(bool(logspace)), p.ptr(labels), p.ptr(path), p.ptr(ws),
                   p.stream())
        return p.to_numpy(labels), p.to_numpy(path)

    def hmm_fit(self, x, seq_start, means, vars, transmat, startprob, max_iter=50, tol=1e-4, prior=0.0, kappa=0.0, min_var=0.0, min_weight=0.0):
        """EM from the parameters given -> (means, vars, transmat, startprob, gamma [n, k], labels [n] int32) numpy and the call's hip.HmmInfo
        (tmjx_hmm_fit)."""
        p = self._p
        (n, d), k = x.shape, means.shape[0]
        seq, seq_p, S = self._seq(seq_start)
        mu, var, A, pi = (p.upload(a, f32, copy=True) for a in (means, vars, transmat, startprob))
        ws, info = self._workspace("tmjx_hmm_workspace", n, d, k, S), _hip.HmmInfo()
        gamma, labels = p.empty((n, k), f32), p.empty((n,), i32)
        self._call("tmjx_hmm_fit", p.ptr(x), n, d, p.ld(x), seq_p, S, k, p.ptr(mu), p.ptr(var), p.ptr(A), p.ptr(pi), p.ptr(gamma), p.ptr(labels),
                   int(max_iter), float(tol), float(prior), float(kappa), float(min_var), float(min_weight), C.byref(info), p.ptr(ws), p.stream())
        return (*(p.to_numpy(t) for t in (mu, var, A, pi, gamma, labels)), info)

    # the autoregressive HMM (analysis/arhmm.py; tmjx_arhmm_*): x from asarray; center [d], weights [k, d, p], vars [k, d] float32 numpy (copied);
    # center=None is the null pointer (zeros)
    def arhmm_emission(self, x, seq_start, lags, warmup, center, weights, vars):
        """-> logb [n, k] float32: the log density of every scored row under every state's linear law, 0 in the unscored rows (tmjx_arhmm_emission)."""
        p = self._p
        (n, d), k = x.shape, vars.shape[0]
        seq, seq_p, S = self._seq(seq_start)
        cen = None if center is None else p.upload(center, f32, copy=True)
        W, var = p.upload(weights, f32, copy=True), p.upload(vars, f32, copy=True)
        ws, logb = self._workspace("tmjx_arhmm_workspace", n, d, int(lags), k, S), p.empty((n, k), f32)
        with p.guard():
            p.check(p.lib.tmjx_arhmm_emission(p.ptr(x), n, d, p.ld(x), seq_p, S, int(lags), int(warmup), None if cen is None else p.ptr(cen), p.ptr(W), p.ptr(var),
                                              k, p.ptr(logb), p.ptr(ws), p.stream()), "tmjx_arhmm_emission")
            p.sync()      # (the host offsets must outlive the queued copy)
        return p.to_numpy(logb)

    def arhmm_moments(self, x, seq_start, lags, warmup, center, gamma):
        """-> (moments [k, q, q], weight [k]) float64: the weighted Gram matrices of psi = [phi; xc] over the scored rows (tmjx_arhmm_moments)."""
        p = self._p
        (n, d), k = x.shape, gamma.shape[1]
        seq, seq_p, S = self._seq(seq_start)
        q = (int(lags) + 1) * d + 1
        cen = None if center is None else p.upload(center, f32, copy=True)
        g, ws = p.upload(gamma, f32, copy=True), self._workspace("tmjx_arhmm_workspace", n, d, int(lags), k, S)
        moments, weight = p.empty((k, q, q), f64), p.empty((k,), f64)
        with p.guard():
            p.check(p.lib.tmjx_arhmm_moments(p.ptr(x), n, d, p.ld(x), seq_p, S, int(lags), int(warmup), None if cen is None else p.ptr(cen), p.ptr(g), k,
                                             p.ptr(moments), p.ptr(weight), p.ptr(ws), p.stream()), "tmjx_arhmm_moments")
            p.sync()
        return p.to_numpy(moments), p.to_numpy(weight)

    def arhmm_solve(self, moments, weight, d, lags, center, weights, vars, ridge=0.0, min_var=0.0, min_weight=0.0, means=None):
        """-> (weights [k, d, p], vars [k, d], means [k, d] float32, status [k] int32): every state's ridge regression from its moments; a light
        (status 1) or singular (2) state as given, its row of `means` (zeros without one) too (tmjx_arhmm_solve)."""
        p = self._p
        k = vars.shape[0]
        cen = None if center is None else p.upload(center, f32, copy=True)
        M, w = p.upload(moments, f64), p.upload(weight, f64)
        W, var = p.upload(weights, f32, copy=True), p.upload(vars, f32, copy=True)
        mu = p.upload(np.zeros((k, d), f32) if means is None else means, f32, copy=True)
        status, ws = p.empty((k,), i32), self._workspace("tmjx_arhmm_workspace", 1, d, int(lags), k, 1)
        self._call("tmjx_arhmm_solve", p.ptr(M), p.ptr(w), k, d, int(lags), None if cen is None else p.ptr(cen), float(ridge), float(min_var), float(min_weight),
                   p.ptr(W), p.ptr(var), p.ptr(mu), p.ptr(status), p.ptr(ws), p.stream())
        return p.to_numpy(W), p.to_numpy(var), p.to_numpy(mu), p.to_numpy(status)

    def arhmm_fit(self, x, seq_start, lags, warmup, center, weights, vars, transmat, startprob, max_iter=50, tol=1e-4, prior=0.0, kappa=0.0, ridge=0.0,
                  min_var=0.0, min_weight=0.0):
        """EM from the parameters given -> (weights, vars, transmat, startprob, gamma [n, k], labels [n] int32, status [k] int32) numpy and the call's
        hip.ArhmmInfo (tmjx_arhmm_fit)."""
        p = self._p
        (n, d), k = x.shape, vars.shape[0]
        seq, seq_p, S = self._seq(seq_start)
        cen = None if center is None else p.upload(center, f32, copy=True)
        W, var, A, pi = (p.upload(a, f32, copy=True) for a in (weights, vars, transmat, startprob))
        ws, info = self._workspace("tmjx_arhmm_workspace", n, d, int(lags), k, S), _hip.ArhmmInfo()
        gamma, labels, status = p.empty((n, k), f32), p.empty((n,), i32), p.empty((k,), i32)
        self._call("tmjx_arhmm_fit", p.ptr(x), n, d, p.ld(x), seq_p, S, int(lags), int(warmup), None if cen is None else p.ptr(cen), k, p.ptr(W), p.ptr(var),
                   p.ptr(A), p.ptr(pi), p.ptr(gamma), p.ptr(labels), p.ptr(status), int(max_iter), float(tol), float(prior), float(kappa), float(ridge),
                   float(min_var), float(min_weight), C.byref(info), p.ptr(ws), p.stream())
        return (*(p.to_numpy(t) for t in (W, var, A, pi, gamma, labels, status)), info)

    # the behaviour map (analysis/embed.py; tmjx_knn, tmjx_tsne_*): x and q from asarray; idx int32 / dist2, p float32 numpy [m, k]; the CSR of P as
    # (row_ptr int32 [n + 1], col int32 [nnz], val float32 [nnz]) numpy; y, velocity, gains float32 numpy [n, 2] (copied: the caller's stay)
    def knn(self, x, q=None, k=1, exclude_self=False):
        """-> (idx [m, k] int32, dist2 [m, k] float32): the k nearest rows of x to every row of q, sorted by (dist2, index).  q=None searches x
        against itself; exclude_self then leaves row i out of query i's list (tmjx_knn)."""
        p = self._p
        q = x if q is None else q
        (n, d), m = x.shape, q.shape[0]
        if q.shape[1] != d:
            raise ValueError(f"queries of {q.shape[1]} features against references of {d}")
        ws = self._workspace("tmjx_tsne_workspace", n, m, d, int(k))
        idx, dist2 = p.empty((m, max(int(k), 1)), i32), p.empty((m, max(int(k), 1)), f32)
        self._call("tmjx_knn", p.ptr(x), n, d, p.ld(x), p.ptr(q), m, p.ld(q), int(bool(exclude_self)), int(k), p.ptr(idx), p.ptr(dist2), p.ptr(ws), p.stream())
        return p.to_numpy(idx), p.to_numpy(dist2)

    def tsne_affinities(self, dist2, perplexity):
        """-> (p [m, k] float32: every row's conditional probabilities at the beta whose entropy is log(perplexity); beta [m] float32)
        (tmjx_tsne_affinities)."""
        p = self._p
        m, k = dist2.shape
        dd = p.upload(dist2, f32, copy=True)
        out, beta = p.empty((m, k), f32), p.empty((m,), f32)
        self._call("tmjx_tsne_affinities", p.ptr(dd), m, k, float(perplexity), p.ptr(out), p.ptr(beta), p.stream())
        return p.to_numpy(out), p.to_numpy(beta)

    def _csr(self, csr):
        p = self._p
        row_ptr, col, val = np.ascontiguousarray(csr[0], i32), p.upload(csr[1], i32, copy=True), p.upload(csr[2], f32, copy=True)
        return row_ptr, row_ptr.ctypes.data_as(_I32P), col, val, int(np.shape(csr[1])[0])

    def tsne_gradient(self, y, csr, exaggeration=1.0):
        """-> (grad [n, 2] float32, Z, kl): one gradient of the t-SNE objective at y for the symmetric P = csr (tmjx_tsne_gradient)."""
        p = self._p
        n = y.shape[0]
        row_ptr, rp, col, val, nnz = self._csr(csr)
        yy, ws = p.upload(y, f32, copy=True), self._workspace("tmjx_tsne_workspace", n, 1, 1, 1)
        grad, z, kl = p.empty((n, 2), f32), p.empty((1,), f64), p.empty((1,), f64)
        with p.guard():
            p.check(p.lib.tmjx_tsne_gradient(p.ptr(yy), n, rp, p.ptr(col), p.ptr(val), nnz, float(exaggeration), p.ptr(grad), p.ptr(z), p.ptr(kl), p.ptr(ws),
                                             p.stream()), "tmjx_tsne_gradient")
            p.sync()      # (the host offsets must outlive the queued copy)
        return p.to_numpy(grad), float(z.item()), float(kl.item())

    def tsne_update(self, y, grad, velocity, gains, momentum, eta, min_gain=0.01):
        """-> (y, velocity, gains) [n, 2] float32: one delta-bar-delta step, y recentred (tmjx_tsne_update)."""
        p = self._p
        n = y.shape[0]
        yy, g, v, ga = (p.upload(a, f32, copy=True) for a in (y, grad, velocity, gains))
        ws = self._workspace("tmjx_tsne_workspace", n, 1, 1, 1)
        self._call("tmjx_tsne_update", p.ptr(yy), p.ptr(g), p.ptr(v), p.ptr(ga), n, float(momentum), float(eta), float(min_gain), p.ptr(ws), p.stream())
        return p.to_numpy(yy), p.to_numpy(v), p.to_numpy(ga)

    def tsne_fit(self, y, csr, n_iter, exaggeration, exaggeration_iters, momentum_early, momentum_late, eta, min_gain=0.01, velocity=None, gains=None):
        """The schedule from y (velocity zeros, gains ones unless given) -> (y, velocity, gains) [n, 2] float32 numpy and the call's hip.TsneInfo
        (tmjx_tsne_fit)."""
        p = self._p
        n = y.shape[0]
        row_ptr, rp, col, val, nnz = self._csr(csr)
        yy = p.upload(y, f32, copy=True)
        v = p.upload(np.zeros((n, 2), f32) if velocity is None else velocity, f32, copy=True)
        ga = p.upload(np.ones((n, 2), f32) if gains is None else gains, f32, copy=True)
        ws, info = self._workspace("tmjx_tsne_workspace", n, 1, 1, 1), _hip.TsneInfo()
        self._call("tmjx_tsne_fit", p.ptr(yy), n, rp, p.ptr(col), p.ptr(val), nnz, int(n_iter), float(exaggeration), int(exaggeration_iters), float(momentum_early),
                   float(momentum_late), float(eta), float(min_gain), p.ptr(v), p.ptr(ga), C.byref(info), p.ptr(ws), p.stream())
        return p.to_numpy(yy), p.to_numpy(v), p.to_numpy(ga), info

    def tsne_place(self, idx, p_rows, y_train):
        """-> y_out [m, 2] float32: every query at the p-weighted mean of its neighbours' positions (tmjx_tsne_place)."""
        p = self._p
        (m, k), n = idx.shape, y_train.shape[0]
        ii, pp, yt = p.upload(idx, i32, copy=True), p.upload(p_rows, f32, copy=True), p.upload(y_train, f32, copy=True)
        out = p.empty((m, 2), f32)
        self._call("tmjx_tsne_place", p.ptr(ii), p.ptr(pp), m, k, p.ptr(yt), n, p.ptr(out), p.stream())
        return p.to_numpy(out)

    # representation comparison (analysis/compare.py; tmjx_cka_linear, tmjx_rdm_corr, tmjx_cca, tmjx_compare_svd): x and y from asarray, the same rows
    def _pair(self, x, y):
        (n, d1), (ny, d2) = x.shape, y.shape
        if ny != n:
            raise ValueError(f"the two sides have {n} and {ny} rows: they must be the same time steps")
        return n, d1, d2

    def cka_linear(self, x, y):
        """-> float64 numpy [3]: ||Cxy||_F^2, ||Cxx||_F^2, ||Cyy||_F^2 of the centred covariances (tmjx_cka_linear)."""
        p = self._p
        n, d1, d2 = self._pair(x, y)
        ws, out = self._workspace("tmjx_compare_workspace", n, d1, d2), p.empty((3,), f64)
        self._call("tmjx_cka_linear", p.ptr(x), n, d1, p.ld(x), p.ptr(y), d2, p.ld(y), p.ptr(out), p.ptr(ws), p.stream())
        return p.to_numpy(out)

    def rdm_corr(self, x, metric_x, y, metric_y):
        """-> float64 numpy [5]: sum Dx, sum Dy, sum Dx^2, sum Dy^2, sum Dx Dy over the pairs i < j of rows (tmjx_rdm_corr); the metrics are
        hip.COMPARE_SQEUCLIDEAN, _EUCLIDEAN, _CORRELATION, _LABEL."""
        p = self._p
        n, d1, d2 = self._pair(x, y)
        ws, sums = self._workspace("tmjx_compare_workspace", n, d1, d2), p.empty((5,), f64)
        self._call("tmjx_rdm_corr", p.ptr(x), n, d1, p.ld(x), int(metric_x), p.ptr(y), d2, p.ld(y), int(metric_y), p.ptr(sums), p.ptr(ws), p.stream())
        return p.to_numpy(sums)

    def cca(self, x, y, var_keep=0.99, max_rank=_hip.COMPARE_MAX_RANK):
        """-> (rho [r], a [r, d1], b [r, d2]) float32 numpy and the call's hip.CcaInfo: the canonical correlations, descending, and the directions in
        feature space (tmjx_cca)."""
        p = self._p
        n, d1, d2 = self._pair(x, y)
        ws, info = self._workspace("tmjx_compare_workspace", n, d1, d2), _hip.CcaInfo()
        cap = max(1, min(int(max_rank), d1, d2, _hip.COMPARE_MAX_RANK))
        rho, a, b = p.empty((cap,), f32), p.empty((cap, d1), f32), p.empty((cap, d2), f32)
        self._call("tmjx_cca", p.ptr(x), n, d1, p.ld(x), p.ptr(y), d2, p.ld(y), float(var_keep), int(max_rank), p.ptr(rho), p.ptr(a), p.ptr(b), C.byref(info),
                   p.ptr(ws), p.stream())
        r = min(info.kx, info.ky)
        return p.to_numpy(rho)[:r], p.to_numpy(a)[:r], p.to_numpy(b)[:r], info

    def compare_svd(self, m):
        """m float64 numpy [rows, cols], both <= 128 -> (sigma [r] descending, u [r, rows], v [r, cols]) float64 numpy and the sweeps run: the kernel
        behind tmjx_cca on its own (tmjx_compare_svd)."""
        p = self._p
        m = np.ascontiguousarray(m, f64)
        rows, cols = m.shape
        r, sweeps = max(min(rows, cols), 1), C.c_int32(0)
        a, ws = p.upload(m, f64), p.workspace(2 * r * r + 4)
        sigma, u, v = p.empty((r,), f64), p.empty((r, rows), f64), p.empty((r, cols), f64)
        self._call("tmjx_compare_svd", p.ptr(a), rows, cols, cols, p.ptr(sigma), p.ptr(u), p.ptr(v), C.byref(sweeps), p.ptr(ws), p.stream())
        return p.to_numpy(sigma), p.to_numpy(u), p.to_numpy(v), int(sweeps.value)

    # the decoder's Jacobian (analysis/jacobian.py; tmjx_jacobian_workspace, tmjx_decoder_jacobian): x from asarray, the weights float32 numpy
    def decoder_jacobian(self, x, layers, head, wrt, eps=1e-6, row_index=None, scale=None, mode=0, want=("ctrl", "jac", "gain", "col2", "row2")):
        """The Jacobian of ctrl = tanh(loc) (mode 0) or of loc (mode 1) with respect to the columns wrt = (col0, cols) of the rows of x [n, d_in].
        layers: [(W [H, K], b, gamma, beta)] of the Dense -> SiLU -> LayerNorm blocks; head: (Wh [>= A, H_L], bh, A); row_index: int32 [m], the rows to
        evaluate in that order (None: every row); scale: from asarray [n, cols], the standard deviation of each differentiated input (adds
        action_var).  -> a dict of numpy arrays: those of `want` (ctrl [m, A], jac [m, A, cols], gain [m], col2 [m, cols], row2 [m, A]),
        action_var [m, A] with a scale, and the float64 sums over the rows mean_sum [A, cols], gram_in [cols, cols], gram_out [A, A]."""
        p = self._p
        n, d_in = x.shape
        (col0, cols), (wh, bh, A) = (int(v) for v in wrt), head
        desc, keep = _hip.JacobianDesc(), []

        def up(a):
            keep.append(p.upload(a, f32))
            return keep[-1]
        desc.L, desc.d_in, desc.eps, desc.A, desc.wrt_col0, desc.wrt_cols = len(layers), d_in, float(eps), int(A), col0, cols
        if len(layers) > _hip.JACOBIAN_MAX_LAYERS:
            raise ValueError(f"{len(layers)} decoder blocks: the Jacobian takes up to {_hip.JACOBIAN_MAX_LAYERS}")
        for slot, (W, b, gamma, beta) in zip(desc.layer, layers):
            w = up(W)
            slot.W, slot.b, slot.gamma, slot.beta, slot.width, slot.ldw = p.ptr(w), p.ptr(up(b)), p.ptr(up(gamma)), p.ptr(up(beta)), w.shape[0], p.ld(w)
        w = up(wh)
        desc.Wh, desc.bh, desc.ldwh = p.ptr(w), p.ptr(up(bh)), p.ld(w)
        idx = None if row_index is None else p.upload(row_index, i32, copy=True)
        m = n if idx is None else int(idx.shape[0])
        ws = self._workspace("tmjx_jacobian_workspace", C.byref(desc), m)
        shapes = {"ctrl": (m, A), "jac": (m, A, cols), "gain": (m,), "col2": (m, cols), "row2": (m, A)}
        out = {k: p.empty(shapes[k], f32) for k in shapes if k in want}
        if scale is not None:
            out["action_var"] = p.empty((m, A), f32)
        sums = p.empty((A * cols + cols * cols + A * A,), f64)
        arg = lambda k: p.ptr(out[k]) if k in out else None      # noqa: E731
        self._call("tmjx_decoder_jacobian", C.byref(desc), p.ptr(x), n, p.ld(x), None if idx is None else p.ptr(idx), m, None if scale is None else p.ptr(scale),
                   0 if scale is None else p.ld(scale), int(mode), arg("ctrl"), arg("jac"), arg("gain"), arg("col2"), arg("row2"), arg("action_var"), p.ptr(sums),
                   p.ptr(ws), p.stream())
        res = {k: p.to_numpy(v) for k, v in out.items()}
        s = p.to_numpy(sums)
        res["mean_sum"], res["gram_in"], res["gram_out"] = s[:A * cols].reshape(A, cols), s[A * cols:A * cols + cols * cols].reshape(cols, cols), s[A * cols + cols * cols:].reshape(A, A)
        return res

    # the LSTM decoder's Jacobian (analysis/jacobian.py; tmjx_lstm_jacobian_workspace, tmjx_lstm_decoder_jacobian): x, h_in, c_in from asarray
    def lstm_decoder_jacobian(self, x, h_in, c_in, layers, head, wrt, row_index=None, scale=None, carry_scale=None, mode=0,
                              want=("ctrl", "jac", "gain", "col2", "row2", "carry_jac", "carry_gain")):
        """The Jacobian of one step of the stacked-LSTM decoder, ctrl = tanh(loc) (mode 0) or loc (mode 1), with respect to the columns wrt = (col0, cols)
        of the rows of x [n, d_in] and to the carry h_in, c_in [n, L H] entering the step (layer k in the columns [k H, (k + 1) H)).  layers:
        [(W_ih [4H, in_k], W_hh [4H, H], b_hh [4H])]; head: (Wp [>= A, H], bp, A); row_index, scale, mode as in decoder_jacobian; carry_scale: numpy
        [2 L H], one factor per carry column (h then c) for carry_gain.  -> the dict of decoder_jacobian plus those of `want` among carry_jac
        [m, A, 2 L H] (the h blocks of every layer, then the c blocks) and carry_gain [m, 2 L], and the float64 carry_sum [A, 2 L H]."""
        p = self._p
        n, d_in = x.shape
        (col0, cols), (wp, bp, A) = (int(v) for v in wrt), head
        L, H = len(layers), int(layers[0][1].shape[1]) if len(layers) else 0
        if not 1 <= L <= _hip.LSTM_JACOBIAN_MAX_LAYERS:
            raise ValueError(f"{L} LSTM layers: the Jacobian takes 1 to {_hip.LSTM_JACOBIAN_MAX_LAYERS}")
        for name, a in (("h_in", h_in), ("c_in", c_in)):
            if tuple(a.shape) != (n, L * H):
                raise ValueError(f"{name} has shape {tuple(a.shape)}: expected the carry entering every row of x, [{n}, {L * H}]")
        if p.ld(h_in) != p.ld(c_in):
            raise ValueError(f"h_in and c_in have the row strides {p.ld(h_in)} and {p.ld(c_in)}: the call takes one")
        desc, keep = _hip.LstmJacobianDesc(), []

        def up(a):
            keep.append(p.upload(a, f32))
            return keep[-1]
        desc.L, desc.H, desc.d_in, desc.A, desc.wrt_col0, desc.wrt_cols = L, H, d_in, int(A), col0, cols
        self._lstm_cells(desc, layers, up)
        w = up(wp)
        desc.Wp, desc.bp, desc.ldwp = p.ptr(w), p.ptr(up(bp)), p.ld(w)
        idx = None if row_index is None else p.upload(row_index, i32, copy=True)
        cs = None if carry_scale is None else up(np.asarray(carry_scale).reshape(-1))
        if cs is not None and cs.shape[0] != 2 * L * H:
            raise ValueError(f"carry_scale holds {cs.shape[0]} factors: expected one per carry column, {2 * L * H}")
        m = n if idx is None else int(idx.shape[0])
        ws = self._workspace("tmjx_lstm_jacobian_workspace", C.byref(desc), m)
        W = 2 * L * H
        shapes = {"ctrl": (m, A), "jac": (m, A, cols), "gain": (m,), "col2": (m, cols), "row2": (m, A), "carry_jac": (m, A, W), "carry_gain": (m, 2 * L)}
        out = {k: p.empty(shapes[k], f32) for k in shapes if k in want}
        if scale is not None:
            out["action_var"] = p.empty((m, A), f32)
        E = A * cols + cols * cols + A * A
        sums = p.empty((E + A * W,), f64)
        arg = lambda k: p.ptr(out[k]) if k in out else None      # noqa: E731
        self._call("tmjx_lstm_decoder_jacobian", C.byref(desc), p.ptr(x), n, p.ld(x), p.ptr(h_in), p.ptr(c_in), p.ld(h_in), None if idx is None else p.ptr(idx), m,
                   None if scale is None else p.ptr(scale), 0 if scale is None else p.ld(scale), None if cs is None else p.ptr(cs), int(mode), arg("ctrl"), arg("jac"),
                   arg("gain"), arg("col2"), arg("row2"), arg("action_var"), arg("carry_jac"), arg("carry_gain"), p.ptr(sums), p.ptr(ws), p.stream())
        res = {k: p.to_numpy(v) for k, v in out.items()}
        s = p.to_numpy(sums)
        res["mean_sum"], res["gram_in"], res["gram_out"] = s[:A * cols].reshape(A, cols), s[A * cols:A * cols + cols * cols].reshape(cols, cols), s[A * cols + cols * cols:E].reshape(A, A)
        res["carry_sum"] = s[E:].reshape(A, W)
        return res

    def _lstm_cells(self, desc, layers, up):
        """The cells of a tmjx_lstm_jacobian_desc_t (L, H, d_in set) from layers [(W_ih, W_hh, b_hh)], uploaded through `up`."""
        p, H, d_in = self._p, desc.H, desc.d_in
        for k, (slot, (w_ih, w_hh, b_hh)) in enumerate(zip(desc.layer, layers)):
            if tuple(w_hh.shape) != (4 * H, H) or tuple(w_ih.shape) != (4 * H, d_in if k == 0 else H) or tuple(b_hh.shape) != (4 * H,):
                raise ValueError(f"LSTM layer {k}: W_ih {tuple(w_ih.shape)}, W_hh {tuple(w_hh.shape)}, b_hh {tuple(b_hh.shape)} are not those of {H} units behind "
                                 f"{d_in if k == 0 else H} inputs")
            wi, wh = up(w_ih), up(w_hh)
            slot.W_ih, slot.W_hh, slot.b_hh, slot.ldwi, slot.ldwh = p.ptr(wi), p.ptr(wh), p.ptr(up(b_hh)), p.ld(wi), p.ld(wh)

    # the LSTM decoder's recurrent dynamics (analysis/dynamics.py; tmjx_lstm_tangent_workspace, tmjx_lstm_tangent_step, tmjx_lstm_lyapunov): x, h_in,
    # c_in from asarray, the weights and the tangents float32 numpy.  The carry space has W = 2 L H columns: the h blocks of every layer, then the c blocks
    def _lstm_dynamics(self, x, h_in, c_in, layers):
        """-> (desc, keep, n, L, H, W) of a dynamics call: the descriptor's cells (no projection, no wrt columns) and the checks on the carry."""
        p = self._p
        n, d_in = x.shape
        L, H = len(layers), int(layers[0][1].shape[1]) if len(layers) else 0
        if not 1 <= L <= _hip.LSTM_JACOBIAN_MAX_LAYERS:
            raise ValueError(f"{L} LSTM layers: the dynamics take 1 to {_hip.LSTM_JACOBIAN_MAX_LAYERS}")
        for name, a in (("h_in", h_in), ("c_in", c_in)):
            if tuple(a.shape) != (n, L * H):
                raise ValueError(f"{name} has shape {tuple(a.shape)}: expected the carry entering every row of x, [{n}, {L * H}]")
        if p.ld(h_in) != p.ld(c_in):
            raise ValueError(f"h_in and c_in have the row strides {p.ld(h_in)} and {p.ld(c_in)}: the call takes one")
        desc, keep = _hip.LstmJacobianDesc(), []

        def up(a):
            keep.append(p.upload(a, f32))
            return keep[-1]
        desc.L, desc.H, desc.d_in = L, H, d_in
        self._lstm_cells(desc, layers, up)
        return desc, keep, n, L, H, 2 * L * H

    def lstm_tangent_step(self, x, h_in, c_in, layers, v):
        """v [n, K, W] -> J_row v [n, K, W] float32 numpy: K tangents of the carry pushed through the carry-to-carry map d (h', c') / d (h, c) of one step
        of the stacked-LSTM decoder at every row of x [n, d_in] with the carry h_in, c_in [n, L H] entering it; the input row is held as recorded
        (tmjx_lstm_tangent_step)."""
        p = self._p
        desc, keep, n, L, H, W = self._lstm_dynamics(x, h_in, c_in, layers)
        if np.ndim(v) != 3 or np.shape(v)[0] != n or np.shape(v)[2] != W:
            raise ValueError(f"v has shape {tuple(np.shape(v))}: expected K tangents of the {W} carry columns for every row, [{n}, K, {W}]")
        K = int(np.shape(v)[1])
        vv, out = p.upload(v, f32, copy=True), p.empty((n, max(K, 1), W), f32)
        ws = self._workspace("tmjx_lstm_tangent_workspace", C.byref(desc), min(n, _hip.JACOBIAN_CHUNK), K)
        self._call("tmjx_lstm_tangent_step", C.byref(desc), p.ptr(x), n, p.ld(x), p.ptr(h_in), p.ptr(c_in), p.ld(h_in), p.ptr(vv), K, p.ptr(out), p.ptr(ws), p.stream())
        return p.to_numpy(out)

    def lstm_lyapunov(self, x, h_in, c_in, layers, seq_start, q0, warmup=0, want=("local", "energy", "q_out", "status")):
        """The Lyapunov spectrum of the carry-to-carry map along the sequences seq_start int32 [S + 1] of the rows of x: per sequence Q = q0 ([K, W]: one
        basis for all, or [S, K, W]), then at every row V = J_t Q, V = Q' R by modified Gram-Schmidt twice, Q = Q'.  -> a dict of numpy arrays: those of
        `want` among local [n, K] (log R_jj at that row), energy [n, K, 2 L] (the squared norm of each column of Q' in each layer's h block, then c
        block), q_out [S, K, W] (the basis behind each sequence's last row), status int32 [S] (1: a column died), and sums float64 [S, K]: the sum of
        local over each sequence's rows from `warmup` on (tmjx_lstm_lyapunov)."""
        p = self._p
        desc, keep, n, L, H, W = self._lstm_dynamics(x, h_in, c_in, layers)
        seq, seq_p, S = self._seq(seq_start)
        q0 = np.asarray(q0)
        if q0.ndim not in (2, 3) or q0.shape[-1] != W or (q0.ndim == 3 and q0.shape[0] != S):
            raise ValueError(f"q0 has shape {tuple(q0.shape)}: expected one basis [K, {W}] or one a sequence [{S}, K, {W}]")
        K = int(q0.shape[-2])
        qq = p.upload(q0, f32, copy=True)
        ws = self._workspace("tmjx_lstm_tangent_workspace", C.byref(desc), S, K)
        shapes = {"local": ((n, K), f32), "energy": ((n, K, 2 * L), f32), "q_out": ((S, K, W), f32), "status": ((S,), i32)}
        out = {k: p.empty(*shapes[k]) for k in shapes if k in want}
        sums = p.empty((S, max(K, 1)), f64)
        arg = lambda k: p.ptr(out[k]) if k in out else None      # noqa: E731
        with p.guard():
            p.check(p.lib.tmjx_lstm_lyapunov(C.byref(desc), p.ptr(x), n, p.ld(x), p.ptr(h_in), p.ptr(c_in), p.ld(h_in), seq_p, S, p.ptr(qq), int(q0.ndim == 3), K,
                                             int(warmup), arg("local"), arg("energy"), arg("q_out"), arg("status"), p.ptr(sums), p.ptr(ws), p.stream()),
                    "tmjx_lstm_lyapunov")
            p.sync()      # (the host offsets must outlive the queued copy)
        res = {k: p.to_numpy(v) for k, v in out.items()}
        res["sums"] = p.to_numpy(sums)
        return res

    # the wavelet spectrogram (analysis/spectrogram.py; tmjx_wavelet_bank*, tmjx_spectrogram*): x from asarray, the bank as wavelet_bank returns it
    def wavelet_bank(self, rate, freqs, omega0=5.0, support=4.0):
        """-> (bank float32, offset int32 [F + 1], radius int32 [F]) numpy: the Morlet tables of every frequency (tmjx_wavelet_bank, a host function)."""
        p = self._p
        fr = np.ascontiguousarray(freqs, f64).reshape(-1)
        F, floats, dp = fr.shape[0], C.c_int64(0), fr.ctypes.data_as(_F64P)
        p.check(p.lib.tmjx_wavelet_bank_size(float(rate), dp, F, float(omega0), float(support), C.byref(floats)), "tmjx_wavelet_bank_size")
        bank, offset, radius = p.host_empty((int(floats.value),), f32), p.host_empty((F + 1,), i32), p.host_empty((F,), i32)
        p.check(p.lib.tmjx_wavelet_bank(float(rate), dp, F, float(omega0), float(support), bank.ctypes.data, offset.ctypes.data_as(_I32P),
                                        radius.ctypes.data_as(_I32P)), "tmjx_wavelet_bank")
        return bank, offset, radius

    def spectrogram(self, x, seq_start, bank, offset, radius, detrend=True, log=False, floor=1e-3, out=None):
        """-> (out [n, F C], coverage [n, F]) arrays of the provider: the amplitude (or its logarithm) of every channel at every frequency, column
        j C + c, and the share of each window inside its sequence (tmjx_spectrogram).  `out`: an array of the provider [n, F C] to write into (a row
        stride is fine)."""
        p = self._p
        n, Cn = x.shape
        seq, seq_p, S = self._seq(seq_start)
        off, rad = np.ascontiguousarray(offset, i32), np.ascontiguousarray(radius, i32)
        F = rad.shape[0]
        bk, ws = p.upload(bank, f32), self._workspace("tmjx_spectrogram_workspace", n, Cn, F, S)
        if out is None:
            out = p.empty((n, F * Cn), f32)
        elif tuple(out.shape) != (n, F * Cn) or not p.dense_columns(out):
            raise ValueError(f"out must be a float32 device tensor [{n}, {F * Cn}] with contiguous columns")
        cov = p.empty((n, F), f32)
        with p.guard():
            p.check(p.lib.tmjx_spectrogram(p.ptr(x), n, Cn, p.ld(x), seq_p, S, p.ptr(bk), off.ctypes.data_as(_I32P), rad.ctypes.data_as(_I32P), F,
                                           int(bool(detrend)), _hip.SPECTROGRAM_LOG if log else _hip.SPECTROGRAM_AMPLITUDE, float(floor), p.ptr(out), p.ld(out),
                                           p.ptr(cov), p.ptr(ws), p.stream()), "tmjx_spectrogram")
            p.sync()      # (the host offsets must outlive the queued copies)
        return out, cov

    def strips(self, proj, k, frame_idx, flags, ymin, ymax, window, style, width, height):
        """One tmjx_plot_strips call: proj from asarray, frame_idx / flags numpy -> rgba uint8 numpy [F, H, W, 4]."""
        p = self._p
        fi, fl = p.upload(frame_idx, i32), p.upload(flags, np.uint8)
        F = fi.shape[0]
        out = p.empty((F, max(height, 0), max(width, 0), 4), np.uint8)
        self._call("tmjx_plot_strips", p.ptr(proj), proj.shape[0], k, p.ld(proj), p.ptr(fi), p.ptr(fl), F, ymin, ymax, window, C.byref(style), width, height,
                   p.ptr(out), p.stream())
        return p.to_numpy(out)


class TorchArrays:
    """The provider of torch tensors on one device, for the product library."""

    def __init__(self, device="cuda", lib=None):
        import torch
        self._t, self.device = torch, torch.device(device)
        self.lib = _hip.lib() if lib is None else lib
        self.check = _hip.check

    def rows(self, x):
        t = x if isinstance(x, self._t.Tensor) else self._t.from_numpy(np.array(x, dtype=np.float32, order="C"))      # (a copy: read-only arrays are fine)
        t = t.to(device=self.device, dtype=self._t.float32)
        return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()

    def upload(self, a, dtype, copy=False):
        return self._t.as_tensor(np.ascontiguousarray(np.array(a, dtype=dtype) if copy else a, dtype), device=self.device)

    def empty(self, shape, dtype, zero=False):
        return (self._t.zeros if zero else self._t.empty)(shape, dtype=getattr(self._t, np.dtype(dtype).name), device=self.device)

    @staticmethod
    def host_empty(shape, dtype):
        return np.zeros(shape, dtype)

    def workspace(self, floats):
        return self._t.empty(floats, dtype=self._t.float32, device=self.device)

    @staticmethod
    def ptr(t):
        return t.data_ptr()

    @staticmethod
    def ld(t):
        return t.stride(0)

    def dense_columns(self, t):
        return t.dtype == self._t.float32 and t.stride(1) == 1

    def stream(self):
        return C.c_void_p(self._t.cuda.current_stream(self.device).cuda_stream)

    def guard(self):
        return self._t.cuda.device(self.device)

    @staticmethod
    def to_numpy(t):
        return t.cpu().numpy()

    def sync(self):
        self._t.cuda.current_stream(self.device).synchronize()


class HipBackend(Backend):
    """The analysis entry points on torch device tensors.  A stand-in with the same methods is accepted wherever a `backend` is; one without
    `fit_wide` / `transform_wide` serves features up to 128 wide only."""

    def __init__(self, device="cuda", lib=None):
        super().__init__(TorchArrays(device, lib))
        self.device = self._p.device


def resolve(backend=None, device="cuda"):
    """The backend a tool runs on: the stand-in it was handed, or the HIP library on `device`."""
    return HipBackend(device) if backend is None else backend
