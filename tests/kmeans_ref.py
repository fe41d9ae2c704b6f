"""The float64 reference of the k-means kernels, the case generator and the checkers that tests/test_kmeans_cpu.py (the host emulation) and
tests/test_gpu_kmeans.py (the C-ABI) share.  A `backend` is analysis.pca.HipBackend or tests/hostemu/analysis_emu.B.

Blob cases (n, d, k): one row; one row past a 256-row block; the intention's width; odd tile edges; both limits.  The assign bounds are the
worst-case error of comparing two d-term float32 FMA chains on data centred at the column mean mu:
    tau_i = 2 (d + 4) 2^-24 (||x_i - mu|| + max_j ||c_j - mu||)^2
a row whose float64 margin (second best minus best) exceeds tau_i must carry the float64 label, any other a label within tau_i of the best."""
from __future__ import annotations

import functools

import numpy as np

CASES = ((1, 1, 1), (257, 3, 2), (1000, 60, 7), (4099, 129, 33), (2050, 1024, 256))
MID = CASES[2]
U24 = 2.0 ** -24


@functools.lru_cache(None)
def case_data(case):
    """-> (x float32 [n, d], centroids float32 [k, d], seeding uniforms float64 [k]); read-only."""
    n, d, k = case
    r = np.random.default_rng(1234 + n)
    ctr = 2.0 * r.standard_normal((k, d))
    lab = r.integers(0, k, n)
    x = np.float32(ctr[lab] + r.standard_normal((n, d))) + np.float32(3)
    c = np.float32(ctr + 3 + 0.25 * r.standard_normal((k, d)))
    u = np.random.default_rng(7).random(k)
    for a in (x, c, u):
        a.setflags(write=False)
    assert x.dtype == np.float32 and c.dtype == np.float32
    return x, c, u


def dist64(x, c):
    """Float64 squared distances [n, k], formed on data centred at the column mean (its own rounding, 2^-53 of the norms, is far below every bound
    here; on the integer grids every term is an integer and the result is exact)."""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    mu = x64.mean(0)
    xc, cc = x64 - mu, c64 - mu
    return (xc * xc).sum(1)[:, None] + (cc * cc).sum(1)[None, :] - 2.0 * (xc @ cc.T)


@functools.lru_cache(None)
def case_dist(case):
    x, c, _ = case_data(case)
    D = dist64(x, c)
    D.setflags(write=False)
    return D


def norms(x, c):
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    mu = x64.mean(0)
    return np.sqrt(((x64 - mu) ** 2).sum(1)), np.sqrt(((c64 - mu) ** 2).sum(1))


def margins(D):
    """(best label, best distance, second best minus best: inf with one centroid)"""
    ref = D.argmin(1)
    best = D[np.arange(D.shape[0]), ref]
    if D.shape[1] == 1:
        return ref, best, np.full(D.shape[0], np.inf)
    two = np.partition(D, 1, axis=1)[:, :2]
    return ref, best, two[:, 1] - two[:, 0]


def input_condition(x, c, D):
    """The share of rows whose float64 margin is within tau: a property of the inputs alone."""
    xn, cn = norms(x, c)
    tau = 2 * (x.shape[1] + 4) * U24 * (xn + cn.max()) ** 2
    return float((margins(D)[2] <= tau).mean())


def check_assign(x, c, D, labels, dist2, inertia, changed, labels_prev, what=""):
    n, d = x.shape
    xn, cn = norms(x, c)
    tau = 2 * (d + 4) * U24 * (xn + cn.max()) ** 2
    ref, best, margin = margins(D)
    sure = margin > tau
    assert labels.dtype == np.int32 and labels.shape == (n,) and labels.min() >= 0 and labels.max() < c.shape[0]
    mine = D[np.arange(n), labels]
    wrong = int((labels[sure] != ref[sure]).sum())
    excess = float(((mine - best) / np.maximum(tau, 1e-300)).max())
    err = np.abs(dist2.astype(np.float64) - mine)
    bound = (d + 4) * U24 * (xn + cn[labels]) ** 2
    worst = float((err / np.maximum(bound, 1e-300)).max())
    total = float(dist2.astype(np.float64).sum())
    print(f"[kmeans {what}] assign {n} x {d} vs {c.shape[0]}: {int((~sure).sum())} rows within tau, {wrong} sure rows wrong, worst excess over the best "
          f"{excess:.3g} tau, dist2 error {worst:.3g} of its bound, inertia rel {abs(inertia - total) / max(total, 1e-300):.3g}")
    assert (~sure).mean() <= 0.01
    assert wrong == 0
    assert (mine - best <= tau).all()
    assert dist2.dtype == np.float32 and (dist2 >= 0).all()
    assert (err <= bound).all()
    assert abs(inertia - total) <= 1e-12 * total
    assert changed == (n if labels_prev is None else int((labels != labels_prev).sum()))


def update64(x, labels, c):
    """-> (float64 means [k, d], an empty cluster's row as given; counts)"""
    out, counts = np.asarray(c, np.float64).copy(), np.bincount(labels, minlength=c.shape[0])
    x64 = np.asarray(x, np.float64)
    for j in np.nonzero(counts)[0]:
        out[j] = x64[labels == j].mean(0)
    return out, counts


def check_update(x, labels, c_in, c_out, counts, what=""):
    ref, cnt = update64(x, labels, c_in)
    assert counts.dtype == np.int32
    np.testing.assert_array_equal(counts, cnt)
    absx = np.abs(np.asarray(x, np.float64))
    worst = 0.0
    for j in range(c_in.shape[0]):
        if cnt[j] == 0:
            np.testing.assert_array_equal(c_out[j].view(np.uint32), c_in[j].view(np.uint32))
            continue
        bound = 2.0 ** -23 * np.maximum(np.abs(ref[j]), absx[labels == j].mean(0))
        err = np.abs(c_out[j].astype(np.float64) - ref[j])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), j
    print(f"[kmeans {what}] update {x.shape[0]} x {x.shape[1]} into {c_in.shape[0]}: worst error {worst:.3g} of its bound, {int((cnt == 0).sum())} empty")


def fallback(u, n):
    return min(int(np.floor(u * n)), n - 1)


def check_seed(x, u, centroids, index, what=""):
    """Teacher-forced: the reference follows the kernel's own earlier picks.  A pick i at step j passes when u_j total lies in
    [cum[i - 1] (1 - rho), cum[i] (1 + rho)], rho = (d + 2) 2^-23, cum the float64 prefix sum of the float64 weights; a row of zero weight is never
    picked while the total is positive; with a total of 0 the pick is min(floor(u_j n), n - 1)."""
    n, d = x.shape
    k = len(u)
    x64, rho = np.asarray(x, np.float64), (d + 2) * 2.0 ** -23
    assert index.dtype == np.int32 and index.shape == (k,) and index.min() >= 0 and index.max() < n
    np.testing.assert_array_equal(centroids.view(np.uint32), x[index].view(np.uint32))
    assert index[0] == fallback(u[0], n)
    d2, zero_total = np.full(n, np.inf), 0
    for j in range(1, k):
        d2 = np.minimum(d2, ((x64 - x64[index[j - 1]]) ** 2).sum(1))
        cum = np.cumsum(d2)
        i = int(index[j])
        if cum[-1] == 0.0:
            zero_total += 1
            assert i == fallback(u[j], n), (j, i)
            continue
        assert d2[i] > 0.0, (j, i)
        lo = cum[i - 1] * (1 - rho) if i > 0 else 0.0
        assert lo <= u[j] * cum[-1] <= cum[i] * (1 + rho), (j, i, lo, u[j] * cum[-1], cum[i])
    print(f"[kmeans {what}] seed {n} x {d} into {k}: every pick inside its interval, {zero_total} picks with a total of 0")
    return zero_total


def seed64(x, u):
    """The free-running float64 k-means++ (what the kernel must pick exactly where its float32 weights are exact: the integer grids)."""
    n, x64 = x.shape[0], np.asarray(x, np.float64)
    index, d2 = [fallback(u[0], n)], np.full(n, np.inf)
    for j in range(1, len(u)):
        d2 = np.minimum(d2, ((x64 - x64[index[-1]]) ** 2).sum(1))
        cum = np.cumsum(d2)
        index.append(fallback(u[j], n) if cum[-1] == 0.0 else int(np.argmax(cum > u[j] * cum[-1])))
    return np.asarray(index, np.int32)


def lloyd64(x, c0, max_iter=100, tol=0.0):
    """Float64 Lloyd with the loop of tmjx_kmeans_fit -> (centroids, labels against them, n_iter: the assigns of the loop)."""
    c, n = np.asarray(c0, np.float64).copy(), x.shape[0]
    prev_labels, prev_inertia, n_iter = None, 0.0, 0
    for it in range(max_iter):
        D = dist64(x, c)
        labels = D.argmin(1)
        inertia = float(D[np.arange(n), labels].sum())
        changed = n if prev_labels is None else int((labels != prev_labels).sum())
        n_iter = it + 1
        if changed == 0 or (it > 0 and prev_inertia - inertia <= tol * prev_inertia):
            break
        prev_labels, prev_inertia = labels, inertia
        c = update64(x, labels, c)[0]
    return c, dist64(x, c).argmin(1), n_iter


def check_fit(case, backend, what=""):
    """Seed with the case's uniforms, fit with tol = 0: the labels and n_iter of float64 Lloyd from the same seeds; then the same fit step by
    step: the inertia never rises by more than relative 1e-6, and the steps reproduce the fit's centroids and labels to the bit."""
    x, _, u = case_data(case)
    xa = backend.asarray(x)
    c0, index = backend.kmeans_seed(xa, case[2], u)
    assert len(set(index.tolist())) == case[2]
    cen, labels, dist2, info = backend.kmeans_fit(xa, c0, 100, 0.0)
    ref_c, ref_labels, ref_iter = lloyd64(x, c0)
    print(f"[kmeans {what}] fit {case}: {info.n_iter} iterations (float64: {ref_iter}), inertia {info.inertia:.9g}, "
          f"{int((labels != ref_labels).sum())} labels differ from float64 Lloyd")
    np.testing.assert_array_equal(labels, ref_labels)
    assert info.n_iter == ref_iter
    assert info.changed == 0 and abs(info.inertia - dist2.astype(np.float64).sum()) <= 1e-12 * info.inertia
    c, prev, trace = c0, None, []
    for it in range(info.n_iter):
        lab, _, inertia, changed = backend.kmeans_assign(xa, c, prev)
        trace.append(inertia)
        if it < info.n_iter - 1:
            c, prev = backend.kmeans_update(xa, lab, c)[0], lab
    for a, b in zip(trace, trace[1:]):
        assert b <= a * (1 + 1e-6), trace
    np.testing.assert_array_equal(c.view(np.uint32), cen.view(np.uint32))
    np.testing.assert_array_equal(lab, labels)
    assert trace[-1] == info.inertia


@functools.lru_cache(None)
def grid_large():
    """Symmetric integer grid at both limits: the column mean is exactly 0 and every product and sum an integer below 2^24."""
    r = np.random.default_rng(99)
    g = r.integers(-8, 9, (1500, 1024))
    x, c = np.float32(np.concatenate([g, -g], 0)), np.float32(r.integers(-8, 9, (256, 1024)))
    x.setflags(write=False), c.setflags(write=False)
    return x, c


@functools.lru_cache(None)
def grid_small():
    """Values -2 .. 2, d = 5, k = 40 with two centroids duplicated: about a quarter of the rows have exact ties."""
    r = np.random.default_rng(5)
    g = r.integers(-2, 3, (300, 5))
    x, c = np.float32(np.concatenate([g, -g], 0)), np.float32(r.integers(-2, 3, (40, 5)))
    c[17], c[30] = c[3], c[8]
    x.setflags(write=False), c.setflags(write=False)
    return x, c


def check_exact(x, c, backend, min_ties=0.0):
    D = dist64(x, c)
    assert (x.astype(np.float64).mean(0) == 0).all() and (D == np.rint(D)).all() and D.max() < 2 ** 24
    ref = D.argmin(1)      # (the first of equal minima: the lowest index)
    best = D[np.arange(x.shape[0]), ref]
    ties = float(((D == best[:, None]).sum(1) > 1).mean())
    assert ties >= min_ties, ties
    labels, dist2, inertia, changed = backend.kmeans_assign(backend.asarray(x), c)
    np.testing.assert_array_equal(labels, ref)
    np.testing.assert_array_equal(dist2.astype(np.float64), best)
    assert inertia == best.sum() and changed == x.shape[0]
    return ties


def clip_files(tmp_path, widths=(40, 25, 33), d=6, k=3):
    """A directory of three small synthetic clip_<i>.h5 with activations/intention [T, d] in k well separated blobs -> (directory, features)."""
    from track_mjx_amd import h5lite
    r = np.random.default_rng(11)
    ctr = 6.0 * r.standard_normal((k, d))
    feats = {}
    for clip, T in zip((0, 2, 5), widths):
        lab = np.repeat(r.integers(0, k, T // 4 + 1), 4)[:T]
        feats[clip] = np.float32(ctr[lab] + 0.3 * r.standard_normal((T, d)))
        h5lite.write_tree(str(tmp_path / f"clip_{clip}.h5"), {"activations": {"intention": feats[clip]}, "ctrl": np.zeros((T, 2), np.float32)})
    return str(tmp_path), feats


def check_cli(tmp_path, backend, capsys):
    """The command-line round trip: keys, shapes and dtypes, labels numbered by count, the clips' labels concatenated = KMeans.labels_, usage
    errors and a missing feature return 2."""
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import cluster as CL
    (tmp_path / "clips").mkdir()
    rollouts, feats = clip_files(tmp_path / "clips")
    out = str(tmp_path / "out" / "clusters.h5")
    assert CL.main([f"rollouts={rollouts}", "k=3", f"out={out}", "seed=1", "n_init=2"], backend=backend) == 0
    assert "[cluster] intention: 98 samples x 6 features from 3 clips into 3 motifs" in capsys.readouterr().out
    with h5lite.File(out) as h:
        got = {key: np.asarray(h[key][()]) for key in ("centroids", "counts", "transitions", "dwell_mean", "inertia", "n_iter", "clips", "seed")}
        feature = bytes(h["feature"][()])
        labels = {c: np.asarray(h["labels"][f"clip_{c}"][()]) for c in feats}
        dists = {c: np.asarray(h["distances"][f"clip_{c}"][()]) for c in feats}
    assert feature.decode() == "intention"
    assert got["centroids"].shape == (3, 6) and got["centroids"].dtype == np.float32
    assert got["counts"].shape == (3,) and got["counts"].dtype == np.int64 and got["counts"].sum() == 98
    assert got["transitions"].shape == (3, 3) and got["transitions"].dtype == np.int64 and got["transitions"].sum() == 98 - 3
    assert got["dwell_mean"].shape == (3,) and got["dwell_mean"].dtype == np.float64
    assert list(got["clips"]) == [0, 2, 5] and int(got["seed"]) == 1 and int(got["n_iter"]) >= 1 and float(got["inertia"]) > 0
    assert (np.diff(got["counts"]) <= 0).all()
    for c, f in feats.items():
        assert labels[c].dtype == np.int32 and labels[c].shape == (f.shape[0],)
        assert dists[c].dtype == np.float32 and dists[c].shape == (f.shape[0],)
    km = CL.KMeans(3, n_init=2, seed=1, backend=backend).fit(np.concatenate([feats[c] for c in (0, 2, 5)], 0))
    np.testing.assert_array_equal(np.concatenate([labels[c] for c in (0, 2, 5)]), km.labels_)
    np.testing.assert_array_equal(got["counts"], km.counts_)
    np.testing.assert_array_equal(got["centroids"].view(np.uint32), km.cluster_centers_.view(np.uint32))
    assert CL.main([f"rollouts={rollouts}", "k=3"], backend=backend) == 2                                   # no out=
    assert CL.main([f"rollouts={rollouts}", "k=3", f"out={out}", "colour=red"], backend=backend) == 2       # an unknown option
    assert "usage:" in capsys.readouterr().err
    assert CL.main([f"rollouts={rollouts}", "k=3", f"out={out}", "feature=decoder/layer_9"], backend=backend) == 2
    assert "decoder/layer_9" in capsys.readouterr().err
