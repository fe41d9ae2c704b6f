"""CPU: the k-means kernel bodies (csrc/kmeans_core.h) compiled into the host emulation (tests/hostemu/kmeans_emu.cpp),
called through the shared analysis backend (tests/hostemu/analysis_emu.py), against the float64
reference (tests/kmeans_ref.py): assign, update, the teacher-forced seeding and the fit at the five blob cases, the integer grids where every
output is exact, the refusals, `KMeans`, `segment_summary`, the command-line tool, and the emulation as a stand-alone program under
AddressSanitizer and UBSan.  tests/test_gpu_kmeans.py runs the same checks through the C-ABI."""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

from tests import kmeans_ref as K
from tests.hostemu import analysis_emu as E
from track_mjx_amd import hip
from track_mjx_amd.analysis import cluster as CL

B = E.B


def test_limits_are_exported_and_the_entry_points_declared():
    assert (hip.KMEANS_MAX_D, hip.KMEANS_MAX_K) == (1024, 256)
    for name in ("tmjx_kmeans_workspace", "tmjx_kmeans_assign", "tmjx_kmeans_update", "tmjx_kmeans_seed", "tmjx_kmeans_fit"):
        assert name in hip.EXPORTS
    assert [f[0] for f in hip.KMeansInfo._fields_] == ["n_iter", "changed", "inertia", "assign_ms", "update_ms"]


@pytest.mark.parametrize("case", K.CASES)
def test_inputs_have_clear_margins(case):
    x, c, _ = K.case_data(case)
    assert K.input_condition(x, c, K.case_dist(case)) <= 0.01


@pytest.mark.parametrize("case", K.CASES)
def test_assign_against_float64(case):
    x, c, _ = K.case_data(case)
    prev = np.random.default_rng(3).integers(0, case[2], case[0]).astype(np.int32)
    labels, dist2, inertia, changed = B.kmeans_assign(x, c, prev)
    K.check_assign(x, c, K.case_dist(case), labels, dist2, inertia, changed, prev, "emulation")
    if case == K.MID:
        again = B.kmeans_assign(x, c, None)
        np.testing.assert_array_equal(again[0], labels)
        assert again[3] == case[0] and again[2] == inertia


@pytest.mark.parametrize("case", K.CASES)
def test_update_against_float64(case):
    x, c, _ = K.case_data(case)
    labels = K.case_dist(case).argmin(1).astype(np.int32)
    out, counts = B.kmeans_update(x, labels, c)
    K.check_update(x, labels, c, out, counts, "emulation")


def test_update_leaves_empty_clusters_alone():
    x, c, _ = K.case_data(K.MID)
    labels = K.case_dist(K.MID).argmin(1).astype(np.int32)
    labels[labels == 2] = 0
    labels[labels == 5] = 6
    out, counts = B.kmeans_update(x, labels, c)
    assert counts[2] == 0 and counts[5] == 0
    K.check_update(x, labels, c, out, counts, "emulation, two empty")


@pytest.mark.parametrize("case", K.CASES)
def test_seed_teacher_forced(case):
    x, _, u = K.case_data(case)
    cen, index = B.kmeans_seed(x, case[2], u)
    assert K.check_seed(x, u, cen, index, "emulation") == 0


def test_seed_with_fewer_distinct_rows_than_centres():
    rows = np.float32(np.random.default_rng(2).standard_normal((5, 9)) + 3)
    x = np.ascontiguousarray(rows[np.random.default_rng(4).integers(0, 5, 300)])
    u = np.random.default_rng(7).random(8)
    cen, index = B.kmeans_seed(x, 8, u)
    assert K.check_seed(x, u, cen, index, "emulation, 5 distinct rows") == 3
    assert len({x[i].tobytes() for i in index[:5]}) == 5


@pytest.mark.parametrize("case", K.CASES[:4])      # (nine emulated passes at 2050 x 1024 x 256 take 15 s: that fit runs on the GPU only)
def test_fit_matches_float64_lloyd(case):
    K.check_fit(case, B, "emulation")


def test_exact_on_the_small_grid_and_ties_go_to_the_lowest_index():
    x, c = K.grid_small()
    assert K.check_exact(x, c, B, min_ties=0.1) >= 0.1
    u = np.random.default_rng(7).random(12)
    np.testing.assert_array_equal(B.kmeans_seed(x, 12, u)[1], K.seed64(x, u))


def test_exact_on_the_large_grid():
    x, c = K.grid_large()
    K.check_exact(x[::6], c, B)      # (every sixth row and its mirror image: 250 + 250 rows keep the mean at exactly 0)


def test_strided_rows_give_the_dense_bits():
    x, c, u = K.case_data(K.MID)
    buf = np.full((x.shape[0], x.shape[1] + 7), 1e6, np.float32)
    buf[:, 3:3 + x.shape[1]] = x
    xs = buf[:, 3:3 + x.shape[1]]
    assert B.asarray(xs) is xs
    for a, b in zip(B.kmeans_assign(xs, c), B.kmeans_assign(x, c)):
        np.testing.assert_array_equal(a, b)
    labels = K.case_dist(K.MID).argmin(1)
    for a, b in zip(B.kmeans_update(xs, labels, c), B.kmeans_update(x, labels, c)):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(B.kmeans_seed(xs, 7, u), B.kmeans_seed(x, 7, u)):
        np.testing.assert_array_equal(a, b)


def test_refusals():
    x, c, u = K.case_data(K.CASES[1])
    for kw, word in ((dict(n=100, k=101), "k <= n"), (dict(k=0), "k must be >= 1"), (dict(n=400, k=257), "limit of 256"), (dict(d=1025, ldx=2000), "limit of 1024"),
                     (dict(n=0), "n must be >= 1"), (dict(ldx=2), "ldx = 2"), (dict(labels=None), "null"), (dict(inertia=None), "null"),
                     (dict(misalign=True), "16-byte")):
        with pytest.raises(ValueError, match=word):
            E.over("tmjx_kmeans_assign", **kw).kmeans_assign(x, c)
    with pytest.raises(ValueError, match="null"):
        E.over("tmjx_kmeans_update", counts=None).kmeans_update(x, np.zeros(257, np.int32), c)
    with pytest.raises(ValueError, match="k <= n"):
        E.over("tmjx_kmeans_seed", n=1).kmeans_seed(x, 2, u[:2])
    with pytest.raises(ValueError, match="uniform"):
        B.kmeans_seed(x, 2, [0.5, 1.0])
    with pytest.raises(ValueError, match="max_iter"):
        B.kmeans_fit(x, c, 0, 0.0)
    with pytest.raises(ValueError, match="limit of 256"):
        E.workspace("tmjx_kmeans_workspace", 1000, 4, 257)
    labels, dist2, _, changed = E.over("tmjx_kmeans_assign", dist2=None, changed=None).kmeans_assign(x, c)      # the two optional outputs
    assert (dist2 == E.sentinel(np.float32)).all() and changed == E.sentinel(np.int32) and (labels >= 0).all()


def test_workspace_does_not_scale_with_n_k_d():
    """The update's partial sums are capped at 2^23 doubles (or 32 parts); beyond them there are the per-chunk column sums [n / 256][d] float64 and a
    few per-row and per-block arrays."""
    for n in (8192, 210000, 4000000):
        chunks = -(-n // 256)
        for d, k in ((1024, 256), (60, 16), (512, 64)):
            assert E.workspace("tmjx_kmeans_workspace", n, d, k) <= 2 * max(2 ** 23, 32 * k * d) + 2 * chunks * d + 6 * n + 1024 * k + 8 * d + 4096, (n, d, k)


def test_kmeans_class():
    x, _, _ = K.case_data(K.MID)
    km = CL.KMeans(7, n_init=3, seed=0, backend=B).fit(x)
    assert km.cluster_centers_.shape == (7, 60) and km.labels_.dtype == np.int32 and km.counts_.sum() == 1000
    assert (np.diff(km.counts_) <= 0).all()
    np.testing.assert_array_equal(np.bincount(km.labels_, minlength=7), km.counts_)
    np.testing.assert_array_equal(km.predict(x), km.labels_)
    # the restart with the lowest inertia, the earlier one on a tie
    u = np.random.default_rng(0).random((3, 7))
    inertias = [float(B.kmeans_fit(x, B.kmeans_seed(x, 7, u[r])[0], 100, 1e-4)[3].inertia) for r in range(3)]
    assert km.inertia_ == min(inertias) and km.best_init_ == int(np.argmin(inertias))
    np.testing.assert_array_equal(CL.KMeans(7, n_init=3, seed=0, backend=B).fit_predict(x), km.labels_)
    with pytest.raises(ValueError, match="exceeds the 3 rows"):
        CL.KMeans(4, backend=B).fit(x[:3])
    with pytest.raises(ValueError, match="n_clusters must be in 1 .. 256"):
        CL.KMeans(257, backend=B)
    with pytest.raises(ValueError, match="not fitted"):
        CL.KMeans(4, backend=B).predict(x)


def test_equal_counts_keep_their_order():
    x = np.float32([[0, 0], [10, 10], [0, 0.5], [10, 10.5], [20, 20]])
    km = CL.KMeans(3, n_init=1, seed=3, backend=B).fit(x)
    np.testing.assert_array_equal(km.counts_, [2, 2, 1])
    assert km.labels_[4] == 2


def test_segment_summary():
    counts, trans, dwell = CL.segment_summary([[0, 0, 1, 1, 1, 0], [3], [1, 3, 3]], 4)      # motif 2 never occurs; a clip of length 1
    np.testing.assert_array_equal(counts, [3, 4, 0, 3])
    want = np.zeros((4, 4), np.int64)
    want[0, 0], want[0, 1], want[1, 1], want[1, 0], want[1, 3], want[3, 3] = 1, 1, 2, 1, 1, 1
    np.testing.assert_array_equal(trans, want)
    assert trans.dtype == np.int64 and counts.dtype == np.int64
    np.testing.assert_allclose(dwell, [3 / 2, 4 / 2, 0.0, 3 / 2])
    with pytest.raises(ValueError, match="outside"):
        CL.segment_summary([[0, 4]], 4)


def test_intervene_centroids_makes_the_intervention_of_the_same_directions(tmp_path):
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import intervene as IV
    cen = np.float32(np.random.default_rng(8).standard_normal((6, 9)) + 2)
    mean = cen.astype(np.float64).mean(0)
    h5lite.write_tree(str(tmp_path / "clusters.h5"), {"centroids": cen, "feature": "intention"})
    h5lite.write_tree(str(tmp_path / "readout.h5"), {"coef": np.ascontiguousarray((cen.astype(np.float64) - mean).T), "mean_x": mean.astype(np.float32),
                                                     "feature": "intention"})
    common = {"intervene_columns": "1:4", "intervene_gain": "1", "intervene_offset": "2", "intervene_window": "10:50", "intervene_dose": "0.5"}
    a = IV.from_cli({"intervene_centroids": str(tmp_path / "clusters.h5"), **common})
    b = IV.from_cli({"intervene_readout": str(tmp_path / "readout.h5"), **common})
    assert a.target == b.target == "intention" and a.mode == b.mode == "subspace" and a.directions.shape == (3, 9)
    for name in ("directions", "center", "gain", "offset"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))
    assert a.window == b.window and a.dose == b.dose
    assert "intervene_centroids" in IV.CLI_OPTIONS
    with pytest.raises(ValueError, match="exactly one of"):
        IV.from_cli({"intervene_centroids": "a.h5", "intervene_readout": "b.h5"})
    with pytest.raises(ValueError, match="intervene_centroids: "):
        IV.from_cli({"intervene_centroids": str(tmp_path / "missing.h5")})


def test_cli_round_trip(tmp_path, capsys):
    K.check_cli(tmp_path, B, capsys)


def test_emulation_runs_clean_under_sanitizers(tmp_path):
    exe = E.build_main("kmeans", tmp_path / "kmeans_emu_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for args in ((), ("4099", "129", "33")):
        res = subprocess.run([str(exe), *args], capture_output=True, text=True)
        assert res.returncode == 0 and "checksum" in res.stdout and not res.stderr, res.stdout + res.stderr
