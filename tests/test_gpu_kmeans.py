"""The k-means kernels (csrc/tmjx_kmeans.hip) through the C-ABI against the float64 reference (tests/kmeans_ref.py): assign, update, the
teacher-forced seeding and the fit at the five blob cases, the integer grids where every output is exact, the bit-level properties (repeatability,
row strides, predict on the training rows, the best of several restarts), the refusals, `KMeans` on device tensors and the command-line tool.
tests/test_kmeans_cpu.py runs the same checks on the host emulation of the same kernel bodies."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import kmeans_ref as K
from track_mjx_amd import hip
from track_mjx_amd.analysis import cluster as CL
from track_mjx_amd.analysis import pca as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(None)
def backend():
    return P.HipBackend(DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


@functools.lru_cache(None)
def prev_of(case):
    return np.random.default_rng(3).integers(0, case[2], case[0]).astype(np.int32)


@functools.lru_cache(None)
def assigned(case):
    x, c, _ = K.case_data(case)
    return backend().kmeans_assign(backend().asarray(x), c, prev_of(case))


@pytest.mark.parametrize("case", K.CASES)
def test_assign_against_float64(case):
    x, c, _ = K.case_data(case)
    labels, dist2, inertia, changed = assigned(case)
    K.check_assign(x, c, K.case_dist(case), labels, dist2, inertia, changed, prev_of(case), "kernel")


@pytest.mark.parametrize("case", K.CASES)
def test_update_against_float64(case):
    x, c, _ = K.case_data(case)
    labels = K.case_dist(case).argmin(1).astype(np.int32)
    out, counts = backend().kmeans_update(backend().asarray(x), labels, c)
    K.check_update(x, labels, c, out, counts, "kernel")


def test_update_leaves_empty_clusters_alone():
    x, c, _ = K.case_data(K.MID)
    labels = K.case_dist(K.MID).argmin(1).astype(np.int32)
    labels[labels == 2] = 0
    labels[labels == 5] = 6
    out, counts = backend().kmeans_update(backend().asarray(x), labels, c)
    assert counts[2] == 0 and counts[5] == 0
    K.check_update(x, labels, c, out, counts, "kernel, two empty")


@pytest.mark.parametrize("case", K.CASES)
def test_seed_teacher_forced(case):
    x, _, u = K.case_data(case)
    cen, index = backend().kmeans_seed(backend().asarray(x), case[2], u)
    assert K.check_seed(x, u, cen, index, "kernel") == 0


def test_seed_with_fewer_distinct_rows_than_centres():
    rows = np.float32(np.random.default_rng(2).standard_normal((5, 9)) + 3)
    x = np.ascontiguousarray(rows[np.random.default_rng(4).integers(0, 5, 300)])
    u = np.random.default_rng(7).random(8)
    cen, index = backend().kmeans_seed(backend().asarray(x), 8, u)
    assert K.check_seed(x, u, cen, index, "kernel, 5 distinct rows") == 3


@pytest.mark.parametrize("case", K.CASES)
def test_fit_matches_float64_lloyd(case):
    K.check_fit(case, backend(), "kernel")


def test_exact_on_the_grids_and_ties_go_to_the_lowest_index():
    x, c = K.grid_small()
    assert K.check_exact(x, c, backend(), min_ties=0.1) >= 0.1
    u = np.random.default_rng(7).random(12)
    np.testing.assert_array_equal(backend().kmeans_seed(backend().asarray(x), 12, u)[1], K.seed64(x, u))
    x, c = K.grid_large()
    K.check_exact(x, c, backend())
    u = np.random.default_rng(7).random(16)
    np.testing.assert_array_equal(backend().kmeans_seed(backend().asarray(x), 16, u)[1], K.seed64(x, u))


def strided(a, pad_left, pad_right):
    buf = torch.full((a.shape[0], a.shape[1] + pad_left + pad_right), 1e6, dtype=torch.float32, device=DEV)
    buf[:, pad_left:pad_left + a.shape[1]] = torch.from_numpy(np.array(a))
    return buf[:, pad_left:pad_left + a.shape[1]]


def test_two_calls_and_strided_rows_give_the_same_bits():
    b = backend()
    case = K.CASES[3]
    x, c, u = K.case_data(case)
    xa, xs = b.asarray(x), strided(x, 3, 2)
    assert b.asarray(xs).data_ptr() == xs.data_ptr() and xs.stride(0) == case[1] + 5      # no copy
    labels = K.case_dist(case).argmin(1).astype(np.int32)
    c0, index = b.kmeans_seed(xa, case[2], u)
    want = (assigned(case), b.kmeans_update(xa, labels, c), (c0, index), b.kmeans_fit(xa, c0, 100, 0.0)[:3])
    for rows in (xa, xs):
        got = (b.kmeans_assign(rows, c, prev_of(case)), b.kmeans_update(rows, labels, c), b.kmeans_seed(rows, case[2], u), b.kmeans_fit(rows, c0, 100, 0.0)[:3])
        for g, w in zip(got, want):
            for u_, v_ in zip(g, w):
                np.testing.assert_array_equal(bits(np.asarray(u_)), bits(np.asarray(v_)))


def test_kmeans_class_on_device_tensors():
    x, _, _ = K.case_data(K.MID)
    xs = strided(x, 2, 3)
    km = CL.KMeans(7, n_init=3, seed=0, device=DEV).fit(xs)
    assert km.cluster_centers_.shape == (7, 60) and km.labels_.dtype == np.int32 and (np.diff(km.counts_) <= 0).all()
    np.testing.assert_array_equal(np.bincount(km.labels_, minlength=7), km.counts_)
    np.testing.assert_array_equal(km.predict(xs), km.labels_)
    np.testing.assert_array_equal(km.predict(x), km.labels_)
    b, u = backend(), np.random.default_rng(0).random((3, 7))
    inertias = [float(b.kmeans_fit(xs, b.kmeans_seed(xs, 7, u[r])[0], 100, 1e-4)[3].inertia) for r in range(3)]
    assert km.inertia_ == min(inertias) and km.best_init_ == int(np.argmin(inertias))


def test_refusals_launch_nothing():
    L = hip.lib()
    x = torch.zeros((300, 8), dtype=torch.float32, device=DEV)
    c = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
    lab = torch.full((300,), -5, dtype=torch.int32, device=DEV)
    cnt = torch.full((4,), -5, dtype=torch.int32, device=DEV)
    inertia = torch.full((1,), -5.0, dtype=torch.float64, device=DEV)
    floats = C.c_int64(0)
    assert L.tmjx_kmeans_workspace(300, 8, 4, C.byref(floats)) == 0 and floats.value > 0
    ws = torch.zeros(int(floats.value) + 4, dtype=torch.float32, device=DEV)
    X, Cn, Lb, In, W = x.data_ptr(), c.data_ptr(), lab.data_ptr(), inertia.data_ptr(), ws.data_ptr()

    def assign(n=300, d=8, ldx=8, k=4, x=X, cen=Cn, labels=Lb, inertia=In, ws=W):
        return L.tmjx_kmeans_assign(x, n, d, ldx, cen, k, None, labels, None, inertia, None, ws, None)
    for kw, word in ((dict(n=3), b"k <= n"), (dict(k=0), b"k must be >= 1"), (dict(k=257), b"limit of 256"), (dict(d=1025, ldx=1025), b"limit of 1024"),
                     (dict(n=0), b"n must be >= 1"), (dict(ldx=7), b"ldx = 7"), (dict(labels=None), b"null"), (dict(inertia=None), b"null"),
                     (dict(x=None), b"null"), (dict(ws=W + 4), b"16-byte")):
        assert assign(**kw) == -22 and word in L.tmjx_last_error(), (kw, L.tmjx_last_error())
    assert L.tmjx_kmeans_update(X, 300, 8, 8, Lb, 4, Cn, None, W, None) == -22 and b"null" in L.tmjx_last_error()
    u = (C.c_double * 4)(0.1, 0.2, 1.0, 0.4)
    index = (C.c_int32 * 4)()
    assert L.tmjx_kmeans_seed(X, 300, 8, 8, 4, u, Cn, index, W, None) == -22 and b"uniform" in L.tmjx_last_error()
    assert L.tmjx_kmeans_seed(X, 300, 8, 8, 4, u, Cn, None, W, None) == -22
    info = hip.KMeansInfo()
    assert L.tmjx_kmeans_fit(X, 300, 8, 8, 4, Cn, Lb, None, 0, 0.0, C.byref(info), W, None) == -22 and b"max_iter" in L.tmjx_last_error()
    assert L.tmjx_kmeans_fit(X, 300, 8, 8, 4, Cn, Lb, None, 10, 0.0, None, W, None) == -22
    assert L.tmjx_kmeans_workspace(300, 8, 301, C.byref(floats)) == -22 and L.tmjx_kmeans_workspace(300, 8, 4, None) == -22
    torch.cuda.synchronize()
    assert (lab == -5).all() and (cnt == -5).all() and float(inertia.item()) == -5.0 and float(ws.abs().sum().item()) == 0.0


def test_cli_round_trip(tmp_path, capsys):
    K.check_cli(tmp_path, backend(), capsys)
