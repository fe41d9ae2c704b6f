"""The two modules every analysis tool starts from, alone: analysis/cli.py (arguments, flags, reports, files) and analysis/recorded.py (what a tool
reads from roll-outs, labels, rows back into clips).  Host numpy, no backend."""
from __future__ import annotations

import numpy as np
import pytest

from track_mjx_amd import h5lite
from track_mjx_amd.analysis import cli
from track_mjx_amd.analysis import recorded as R

OPTIONS, REQUIRED, USAGE = ("rollouts", "out", "k", "store"), ("rollouts", "out"), "usage: tool rollouts=<dir> [k=3] [store=false] out=<file>"


# ---------------------------------------------------------------------------------------------------------------- cli
def test_parse_accepts_known_keys(capsys):
    assert cli.parse(["rollouts=a", "out=b=c", "k=3"], OPTIONS, REQUIRED, USAGE) == {"rollouts": "a", "out": "b=c", "k": "3"}
    assert cli.parse(["out=b", "rollouts=a"], OPTIONS, REQUIRED, USAGE, extra_ok=lambda o: "k" not in o) == {"rollouts": "a", "out": "b"}
    assert capsys.readouterr().err == ""


@pytest.mark.parametrize("argv", [["rollouts=a", "out=b", "verbose"],            # an argument without =
                                  ["rollouts=a", "out=b", "colour=red"],         # an unknown key
                                  ["rollouts=a", "k=3"],                         # a missing required key
                                  ["rollouts=a", "out=b", "rollouts=c"],         # a repeated key
                                  []])
def test_parse_prints_the_usage(argv, capsys):
    assert cli.parse(argv, OPTIONS, REQUIRED, USAGE) is None
    assert capsys.readouterr().err == USAGE + "\n"


def test_parse_extra_condition_and_split(capsys):
    assert cli.parse(["rollouts=a", "out=b", "k=3"], OPTIONS, REQUIRED, USAGE, extra_ok=lambda o: "k" not in o) is None
    assert capsys.readouterr().err == USAGE + "\n"
    # the roll-out's rule: what is no option of the tool is kept, in order, as a config override; a repeated option keeps its last value
    assert cli.split(["out=b", "env.mocap_hz=50", "k=1", "verbose", "k=2"], OPTIONS) == ({"out": "b", "k": "2"}, ["env.mocap_hz=50", "verbose"])


def test_flag():
    assert cli.flag({}, "store") is False and cli.flag({}, "detrend", "true") is True
    assert cli.flag({"store": "TRUE"}, "store") is True and cli.flag({"store": "False"}, "store", "true") is False
    with pytest.raises(ValueError, match=r"^store must be true or false \(got maybe\)$"):
        cli.flag({"store": "maybe"}, "store")


def test_report_and_write(tmp_path, capsys):
    assert cli.report("tool", KeyError("clip_3.h5 has no ctrl")) == 2 and cli.report("tool", ValueError()) == 2
    assert capsys.readouterr().err == "[tool] clip_3.h5 has no ctrl\n[tool] \n"
    cli.write(str(tmp_path / "deep" / "er" / "out.h5"), {"a": np.arange(3)})
    cli.write_clips(str(tmp_path / "clips"), {4: {"a": np.arange(2)}, 0: {"b": {"c": np.zeros(1)}}})
    with h5lite.File(str(tmp_path / "deep" / "er" / "out.h5")) as h:
        assert h["a"][()].tolist() == [0, 1, 2]
    assert sorted(p.name for p in (tmp_path / "clips").iterdir()) == ["clip_0.h5", "clip_4.h5"]
    assert R.rollout_features(str(tmp_path / "clips"), lambda r, c, where: (c, where, sorted(r.keys())))[1] == [(0, "clip_0.h5", ["b"]), (4, "clip_4.h5", ["a"])]


# ---------------------------------------------------------------------------------------------------------------- numbering and splitting
def test_number_by_count():
    labels = np.array([1, 0, 1, 2, 1, 0, 2, 1, 0, 2, 1])      # counts 3, 5, 3, 0
    order, rank, counts = R.number_by_count(labels, 4)
    assert order.tolist() == [1, 0, 2, 3] and counts.tolist() == [5, 3, 3, 0] and counts.dtype == np.int64      # ties stable, the empty motif kept
    assert rank[order].tolist() == [0, 1, 2, 3] and order[rank].tolist() == [0, 1, 2, 3]
    assert np.bincount(rank[labels], minlength=4).tolist() == counts.tolist()


def test_split_and_scatter_per_clip():
    lens, rows = [1, 3, 2], np.array([0, 2, 5])
    a = np.arange(6 * 2 * 3, dtype=np.float32).reshape(6, 2, 3)
    parts = R.split(a, lens)
    assert [p.shape for p in parts] == [(1, 2, 3), (3, 2, 3), (2, 2, 3)] and np.array_equal(np.concatenate(parts), a)
    per = R.scatter_per_clip(a[rows], rows, 6, [7, 8, 11], lens)
    assert list(per) == ["clip_7", "clip_8", "clip_11"] and [v.shape for v in per.values()] == [(1, 2, 3), (3, 2, 3), (2, 2, 3)]
    full = np.concatenate(list(per.values()))
    assert full.dtype == np.float32 and np.array_equal(full[rows], a[rows]) and np.isnan(full[[1, 3, 4]]).all()
    flat = R.scatter_per_clip(np.ones(3, np.float32), rows, 6, [0, 1, 2], lens)      # no trailing dimension
    assert np.isnan(np.concatenate(list(flat.values()))).tolist() == [False, True, False, True, True, False]
    group = R.by_clip([3, 5], [np.arange(2), np.arange(3)], np.int32)
    assert list(group) == ["clip_3", "clip_5"] and all(v.dtype == np.int32 for v in group.values()) and R.by_clip([1], [a])["clip_1"] is a


def test_seq_start():
    assert R.seq_start([2, 3, 1], 6).tolist() == [0, 2, 5, 6] and R.seq_start([2, 3, 1], 6).dtype == np.int32
    for lengths, n in (([], 0), ([2, 0, 4], 6), ([2, 3], 6)):      # empty, a zero length, a sum that is not n
        with pytest.raises(ValueError, match="lengths must be positive and sum to"):
            R.seq_start(lengths, n)


# ---------------------------------------------------------------------------------------------------------------- labels
def test_labels_for_rows(tmp_path):
    labels = {0: np.array([0, 1, 1]), 4: np.array([[2], [2], [0], [1], [1]]), 9: np.array([5])}      # (clip 4: longer than the clip, and [T, 1])
    path = str(tmp_path / "clusters.h5")
    h5lite.write_tree(path, {"labels": {f"clip_{c}": np.asarray(v, np.int32) for c, v in labels.items()}, "feature": "intention"})
    from_dict, from_file = R.labels_for_rows(labels, [0, 4], [3, 4]), R.labels_for_rows(path, [0, 4], [3, 4])
    assert from_dict.tolist() == from_file.tolist() == [0, 1, 1, 2, 2, 0, 1] and from_dict.dtype == from_file.dtype == np.int64
    assert {c: v.tolist() for c, v in R.labels_file(path).items()} == {0: [0, 1, 1], 4: [2, 2, 0, 1, 1], 9: [5]}
    with pytest.raises(KeyError, match="the labels file has no clip_2"):
        R.labels_for_rows(path, [0, 2], [3, 1])
    with pytest.raises(ValueError, match="the labels of clip_0 hold 3 rows, the roll-out 4"):
        R.labels_for_rows(labels, [0], [4])
    h5lite.write_tree(str(tmp_path / "pca.h5"), {"feature": "intention"})
    with pytest.raises(KeyError, match="has no labels group"):
        R.labels_file(str(tmp_path / "pca.h5"))


# ---------------------------------------------------------------------------------------------------------------- a dict and a file
def test_meta_feature_target_and_aligned_on_a_dict_and_a_file(tmp_path):
    rng = np.random.default_rng(0)
    rollout = {"ctrl": rng.standard_normal((5, 2)).astype(np.float32), "qposes_rollout": rng.standard_normal((6, 4)).astype(np.float32),
               "joint_forces": rng.standard_normal((5, 3, 6)).astype(np.float32), "aligned": np.array([0, 0, 1, 0, 0], bool),
               "activations": {"intention": rng.standard_normal((5, 3)).astype(np.float32), "decoder": {"layer_0": rng.standard_normal((5, 1, 4)).astype(np.float32)}},
               "meta": {"clip_idx": np.int64(4), "model": "mlp", "nested": {"seed": np.int64(7)}}}
    h5lite.write_tree(str(tmp_path / "clip_4.h5"), rollout)
    with h5lite.File(str(tmp_path / "clip_4.h5")) as h:
        for r in (rollout, h):
            assert np.array_equal(R.feature_of(r, "intention", "w"), rollout["activations"]["intention"])
            assert np.array_equal(R.feature_of(r, "decoder/layer_0", "w"), rollout["activations"]["decoder"]["layer_0"].reshape(5, 4))
            assert np.array_equal(R.feature_of(r, "ctrl", "w"), rollout["ctrl"]) and np.array_equal(R.target_of(r, "activations/intention", "w"), R.feature_of(r, "intention", "w"))
            assert R.target_of(r, "joint_forces", "w").shape == (5, 18) and R.target_of(r, "qposes_rollout", "w").shape == (6, 4)
            assert R.aligned_of(r, 5, "w").tolist() == [False, False, True, False, False]
            with pytest.raises(KeyError, match=r"w has no activations/encoder/layer_7 \(roll it out with log_activations=true\)"):
                R.feature_of(r, "encoder/layer_7", "w")
            with pytest.raises(KeyError, match="w: activations/decoder is a group"):
                R.feature_of(r, "decoder", "w")
            with pytest.raises(KeyError, match="unknown target 'velocity'"):
                R.target_of(r, "velocity", "w")
            with pytest.raises(ValueError, match="w: aligned has 5 rows, intention 4"):
                R.aligned_of(r, 4, "w")
        meta = R.meta_of(h)
        assert int(meta["clip_idx"]) == 4 and bytes(meta["model"]) == b"mlp" and int(meta["nested"]["seed"]) == 7 and R.meta_of(rollout) is rollout["meta"]
    del rollout["meta"], rollout["aligned"]
    h5lite.write_tree(str(tmp_path / "clip_5.h5"), rollout)
    with h5lite.File(str(tmp_path / "clip_5.h5")) as h:
        assert R.meta_of(h) is None and R.meta_of(rollout) is None and R.aligned_of(h, 5, "w") is None and R.aligned_of(rollout, 5, "w") is None
    assert R.columns(None, 4) == slice(0, 4) and R.columns("1:", 4) == slice(1, None)
    with pytest.raises(ValueError, match=r"^cols = 9: selects no column of 4$"):
        R.columns("9:", 4, "cols")
    ids, sigs, metas = R.signals(str(tmp_path), "qposes_rollout", "2:", None)
    assert ids == [4, 5] and np.array_equal(sigs[0], rollout["qposes_rollout"][:, 2:]) and int(metas[0]["clip_idx"]) == 4 and metas[1] is None
