"""CPU: the checkpoint roll-out's host side — the nested HDF5 writer and save_to_h5py / load_from_h5py, the reset key derivation of
generate_rollout, argument validation of the recorder / deterministic-policy exports without a GPU, and the generator's refusals."""
import ctypes as C

import numpy as np
import pytest

from track_mjx_amd import h5lite, hip
from track_mjx_amd import jax_random as jr


def _tree():
    rng = np.random.default_rng(0)
    return {
        "qposes_rollout": rng.standard_normal((7, 74)).astype(np.float32),
        "ctrl": rng.standard_normal((6, 38)),
        "state_rewards": np.arange(7, dtype=np.int32),
        "big": np.arange(12, dtype=np.int64).reshape(3, 4),
        "scalar_f": 2.5, "scalar_i": 7, "np_scalar": np.float32(-1.25), "name": b"rodent", "text": "meta",
        "activations": {"encoder": {f"layer_{i}": rng.standard_normal((3, 5 + i)).astype(np.float32) for i in range(12)},
                        "decoder": {"layer_0": np.zeros((3, 4), np.float32)}, "intention": np.ones((3, 60), np.float32)},
        "many": {f"g{i:02d}": {"v": np.full(2, i, np.float64)} for i in range(40)},
        "hidden_state": (np.ones((2, 2, 3), np.float32), np.zeros((2, 2, 3), np.float32)),
        "skipped": None,
        "lst": [np.float64(1.0), {"a": np.int32(3)}, [b"x", b"yz"]],
    }


def _eq(a, b):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), (a.keys() if isinstance(a, dict) else a, b.keys() if isinstance(b, dict) else b)
        for k in a:
            _eq(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, list) and len(a) == len(b)
        for x, y in zip(a, b):
            _eq(x, y)
    elif isinstance(a, str):
        assert bytes(b) == a.encode()
    elif isinstance(a, (bytes, np.bytes_)):
        assert bytes(b) == bytes(a)
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.shape == y.shape and np.array_equal(x, y), (x, y)
        if isinstance(a, np.ndarray) or isinstance(a, np.generic):
            assert x.dtype == y.dtype


def test_save_load_h5py_round_trip(tmp_path):
    from track_mjx_amd.analysis.utils import load_from_h5py, save_to_h5py
    t = _tree()
    p = tmp_path / "r.h5"
    save_to_h5py(p, t)
    back = load_from_h5py(p)
    expect = {k: v for k, v in t.items() if v is not None}
    _eq(expect, back)
    f = h5lite.File(p)                                 # the same file through the pinned reader's h5py-style API
    assert sorted(f["activations/encoder"].keys()) == sorted(f"layer_{i}" for i in range(12))
    assert len(f["many"].keys()) == 40 and f["many/g39/v"][()].tolist() == [39.0, 39.0]
    assert f["qposes_rollout"].dtype == np.float32 and f["big"].dtype == np.int64 and f["state_rewards"].dtype == np.int32
    assert f["scalar_i"][()] == 7 and f["scalar_f"].shape == ()
    _eq(t["activations"], load_from_h5py(p, "/activations"))
    p2 = tmp_path / "g.h5"
    save_to_h5py(p2, {"x": np.ones(3)}, group_path="/rollout/clip_3")
    _eq({"x": np.ones(3)}, load_from_h5py(p2, "rollout/clip_3"))


@pytest.mark.parametrize("n", [0, 1, 8, 9, 256, 257, 700])
def test_write_tree_group_sizes(tmp_path, n):
    """Symbol-table nodes of 8 links, B-tree nodes of 32 children: 257 and 700 links need a second B-tree level (the 270-link group of
    tests/golden/refclip_small.h5 is laid out the same way by libhdf5)."""
    t = {"g": {f"k{i:04d}": np.int32(i) for i in range(n)}, "z": np.zeros(1)}
    p = tmp_path / "n.h5"
    h5lite.write_tree(p, t)
    f = h5lite.File(p)
    assert sorted(f["g"].keys()) == sorted(t["g"])
    assert all(int(f["g"][k][()]) == v for k, v in t["g"].items())
    raw = p.read_bytes()
    if n > 256:
        i = raw.index(b"TREE")
        levels = set()
        while i >= 0:
            levels.add(raw[i + 5]); i = raw.find(b"TREE", i + 1)
        assert 1 in levels


def test_write_tree_matches_the_pinned_reader_on_real_file_layout():
    """The reader walks libhdf5's own two-level group B-tree (refclip_small.h5: 270 links); the writer emits the same node kinds."""
    from pathlib import Path
    p = Path(__file__).resolve().parent / "golden" / "refclip_small.h5"
    raw = p.read_bytes()
    assert raw.count(b"TREE") >= 2 and b"SNOD" in raw


def test_reset_draws_compose_the_pinned_threefry():
    from track_mjx_amd.analysis.rollout import reset_inputs
    for seed in (0, 42, 12345):
        key = jr.PRNGKey(seed)
        _, reset_rng, _act_rng = jr.split(key, 3)
        _, clip_rng, rng = jr.split(reset_rng, 3)
        _, rng1, _ = jr.split(rng, 3)
        c, qn, vn = reset_inputs(seed, 850, 74, 73, 1e-3, clip_idx=5)
        assert c == 5
        assert np.array_equal(qn, jr.uniform(rng1, (74,), -1e-3, 1e-3)) and np.array_equal(vn, jr.uniform(rng1, (73,), -1e-3, 1e-3))
        assert np.array_equal(vn, qn[:73])            # both from rng1 (the reference's own re-use)
        assert qn.dtype == np.float32 and np.abs(qn).max() <= 1e-3
        c2, qn2, _ = reset_inputs(seed, 850, 74, 73, 1e-3, clip_idx=None)
        assert c2 == int(jr.randint(clip_rng, (), 0, 850)) and np.array_equal(qn2, qn)


def _stream(**kw):
    buf = kw.pop("_buf")
    a = dict(src=buf, dst=buf + 4096, layout=hip.RECORD_ROWMAJOR, ld=64, w=32, src_extent=64, T=10, t0=0, n_idx=0)
    a.update(kw)
    s = hip.RecordStream(*[a[k] for k in ("src", "dst", "layout", "ld", "w", "src_extent", "T", "t0", "n_idx")])
    for i, v in enumerate(kw.get("idx", ())):
        s.idx[i] = v
    return s


@pytest.mark.parametrize("bad", [dict(src=None), dict(dst=None), dict(src=0x10002), dict(w=0), dict(w=5000), dict(w=65), dict(layout=3),
                                 dict(layout=hip.RECORD_SOA, ld=4), dict(ld=16), dict(n_idx=3), dict(n_idx=32, w=32, idx=[70] * 32),
                                 dict(T=5), dict(t0=3)])
def test_record_check_refuses_bad_streams_without_gpu(bad):
    L = hip.lib()
    good = (hip.RecordStream * 1)(_stream(_buf=0x10000))
    assert L.tmjx_record_check(good, 1, 8, 10) == 0
    tab = (hip.RecordStream * 2)(_stream(_buf=0x10000), _stream(_buf=0x20000, **bad))
    assert L.tmjx_record_check(tab, 2, 8, 10) == -22
    assert b"tmjx_record_check: stream 1" in L.tmjx_last_error()


def test_record_step_refuses_bad_arguments_without_gpu():
    L = hip.lib()
    assert L.tmjx_record_check(None, 1, 8, 10) == -22
    tab = (hip.RecordStream * 1)(_stream(_buf=0x10000))
    assert L.tmjx_record_check(tab, 0, 8, 10) == -22 and L.tmjx_record_check(tab, 1, 0, 10) == -22
    assert L.tmjx_record_step(None, 1, 8, 0, 10, None) == -22
    assert L.tmjx_record_step(0x10008, 1, 8, 0, 10, None) == -22             # device table not 16-byte aligned
    for t, T in ((10, 10), (11, 10), (-1, 10)):
        assert L.tmjx_record_step(0x10000, 1, 8, t, T, None) == -22
        assert b"0 <= t < T" in L.tmjx_last_error()
    assert L.tmjx_record_step(0x10000, 0, 8, 0, 10, None) == -22
    assert L.tmjx_record_step(0x10000, 65, 8, 0, 10, None) == -22
    assert C.sizeof(hip.RecordStream) == 176


def test_deterministic_policy_kernels_refuse_bad_arguments_without_gpu():
    L = hip.lib()
    a = 0x10000
    ok = dict(fc2=a, ldf=120, obs=a, s0=696, s1=1, mean=a, std=a, x=a, ldx=288, traj=a, ldt=472, n=4, Z=60, W=696, ref=470)
    for bad in (dict(fc2=None), dict(obs=None), dict(x=None), dict(mean=None), dict(ldf=100), dict(ldx=200), dict(ldt=400), dict(n=0),
                dict(ref=696), dict(x=a + 2), dict(obs=a + 1)):
        v = dict(ok, **bad)
        assert L.tmjx_latent_concat_det(*v.values(), None) == -22, bad
        assert b"tmjx_latent_concat_det" in L.tmjx_last_error()
    for args in ((None, 76, a, a, 4, 38), (a, 76, None, a, 4, 38), (a, 76, a, None, 4, 38), (a, 70, a, a, 4, 38), (a, 76, a, a, 0, 38),
                 (a, 76, a, a, 4, 0), (a + 2, 76, a, a, 4, 38)):
        assert L.tmjx_action_mode(*args, None) == -22, args
        assert b"tmjx_action_mode" in L.tmjx_last_error()


def test_generator_refusals():
    from track_mjx_amd import config as _config
    from track_mjx_amd.analysis.rollout import create_rollout_generator
    cfg = _config.load_config(None, [])
    with pytest.raises(NotImplementedError, match="cfrc_ext and sensordata are not computed by the physics kernel"):
        create_rollout_generator(cfg, None, lambda obs, key: obs, log_sensor_data=True)
    with pytest.raises(TypeError, match="load_inference_fn"):
        create_rollout_generator(cfg, None, lambda obs, key: obs)


def test_cli_clip_spec():
    from track_mjx_amd.analysis.rollout import _parse_clips
    assert _parse_clips("all", 5) == [0, 1, 2, 3, 4]
    assert _parse_clips("1:3", 5) == [1, 2] and _parse_clips("3:", 5) == [3, 4]
    assert _parse_clips("4,0,2", 5) == [4, 0, 2]
