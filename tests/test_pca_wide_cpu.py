"""Wide PCA (129 <= d <= 1024, block Jacobi) on the CPU: the host emulation of the kernel bodies (tests/hostemu/pca_wide_emu.cpp),
called through the shared analysis backend (tests/hostemu/analysis_emu.py), under the
checks tests/test_gpu_pca_wide.py applies to the kernels at the same shapes, the product library's refusals (no GPU is touched), forwarding of
d <= 128 to the narrow path, repeatability, degenerate inputs, analysis.pca and both command-line tools on wide features, and the emulation as a
stand-alone program under the sanitizers."""
from __future__ import annotations

import ctypes as C
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

from tests import pca_ref as R
from tests.hostemu import analysis_emu as E
from track_mjx_amd import hip
from track_mjx_amd.analysis import pca as P

ROOT = Path(__file__).resolve().parents[1]
# (n, d, offset, seed): the first wide size (a 1-column block and a bye); n < d (3 blocks and a bye); an uneven last block with a bye; an odd
# count of full blocks; the offset-100 case a one-pass variance fails
CASES = ((300, 129, 3.0, 0), (130, 192, 3.0, 0), (513, 257, 3.0, 0), (700, 320, 3.0, 0), (1500, 512, 100.0, 0))
B = E.B


@pytest.mark.parametrize("case", CASES)
def test_emu_fit_and_transform(case):
    x = R.case_data(*case)
    mean, comp, var, info = B.fit_wide(x)
    print(case, f"{info.sweeps} block sweeps, off / norm {info.off_rel:.2e}")
    assert info.converged == 1 and 1 <= info.sweeps <= 15
    R.check_fit(x, mean, comp, var, B.transform_wide(x, mean, comp[:R.top_k(*x.shape)]), case, "emulation")


def test_emu_transform_many_components_and_row_stride():
    """k > 16 takes the 64-component tiles; a row stride at a column offset gives the dense input's bits; ldo > k leaves the rest unwritten."""
    case = CASES[1]
    n, d = case[:2]
    x = R.case_data(*case)
    wide = np.full((n, d + 5), 1e6, np.float32)
    wide[:, 3:3 + d] = x
    view = wide[:, 3:3 + d]
    assert view.strides[0] == 4 * (d + 5)
    a, b = B.fit_wide(view), B.fit_wide(x)
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
    for k in (4, 16, 17, 70, d):
        got = B.transform_wide(view, a[0], a[1][:k])
        np.testing.assert_array_equal(got, B.transform_wide(x, a[0], a[1][:k]))
        want = R.transform(x, a[0], a[1][:k])
        assert np.abs(got - want).max() <= R.bound(d) * np.abs(want).max()
    out = np.full((n, 9), -5.0, np.float32)
    m, c = a[0], np.ascontiguousarray(a[1][:4])
    E.over("tmjx_pca_transform_wide", out=out, ldo=9).transform_wide(x, m, c)
    np.testing.assert_array_equal(out[:, :4], B.transform_wide(x, m, c))
    assert (out[:, 4:] == -5.0).all()


def test_library_refuses_before_any_launch():
    """The product library's own checks (no GPU is touched: the dummy pointers are never dereferenced)."""
    L = hip.lib()
    one, info, floats = C.c_void_p(1 << 20), hip.PcaInfo(), C.c_int64(0)
    for args, word in (((one, 10, 1025, 1025), b"d = 1025 exceeds the wide PCA limit of 1024"), ((one, 1, 300, 300), b"n >= 2"), ((one, 10, 300, 299), b"ldx = 299"),
                       ((one, 10, 0, 4), b"d must be >= 1")):
        assert L.tmjx_pca_fit_wide(*args, one, one, one, one, C.byref(info), None) == -22 and word in L.tmjx_last_error(), L.tmjx_last_error()
    assert L.tmjx_pca_fit_wide(None, 10, 300, 300, one, one, one, one, C.byref(info), None) == -22 and b"null argument" in L.tmjx_last_error()
    assert L.tmjx_pca_fit_wide(one, 10, 300, 300, one, one, one, one, None, None) == -22 and b"null argument" in L.tmjx_last_error()
    assert L.tmjx_pca_fit_wide(one, 10, 300, 300, one, one, one, C.c_void_p((1 << 20) + 4), C.byref(info), None) == -22 and b"aligned" in L.tmjx_last_error()
    assert L.tmjx_pca_transform_wide(one, 10, 300, 300, one, one, 301, one, 301, None) == -22 and b"k = 301 components asked of d = 300" in L.tmjx_last_error()
    assert L.tmjx_pca_transform_wide(one, 10, 300, 300, one, one, 0, one, 4, None) == -22 and b"k = 0" in L.tmjx_last_error()
    assert L.tmjx_pca_transform_wide(one, 10, 300, 299, one, one, 2, one, 2, None) == -22 and b"ldx = 299" in L.tmjx_last_error()
    assert L.tmjx_pca_transform_wide(one, 10, 300, 300, one, one, 4, one, 3, None) == -22 and b"ldo = 3 is smaller than k = 4" in L.tmjx_last_error()
    assert L.tmjx_pca_transform_wide(one, 10, 1025, 1025, one, one, 4, one, 4, None) == -22 and b"exceeds the wide PCA limit of 1024" in L.tmjx_last_error()
    assert L.tmjx_pca_transform_wide(one, 10, 300, 300, None, one, 4, one, 4, None) == -22 and b"null argument" in L.tmjx_last_error()
    assert L.tmjx_pca_wide_workspace(1, 300, C.byref(floats)) == -22 and L.tmjx_pca_wide_workspace(10, 1025, C.byref(floats)) == -22
    assert L.tmjx_pca_wide_workspace(10, 300, None) == -22
    # the narrow entry points refuse what they refused
    assert L.tmjx_pca_fit(one, 10, 129, 129, one, one, one, one, C.byref(info), None) == -22 and b"d = 129 exceeds the PCA limit of 128" in L.tmjx_last_error()
    assert L.tmjx_pca_workspace(10, 129, C.byref(floats)) == -22 and b"d = 129 exceeds the PCA limit of 128" in L.tmjx_last_error()
    assert L.tmjx_pca_transform(one, 10, 129, 129, one, one, 4, one, 4, None) == -22 and b"d = 129 exceeds the PCA limit of 128" in L.tmjx_last_error()


def test_workspace_grows_with_d_squared_only():
    L, floats = hip.lib(), C.c_int64(0)
    assert L.tmjx_pca_wide_workspace(210_000, 1024, C.byref(floats)) == 0
    big = floats.value
    print(f"workspace of 210 000 x 1024: {4 * big / 2 ** 20:.1f} MiB")
    assert 4 * big <= 256 * 2 ** 20 and big == E.workspace("tmjx_pca_wide_workspace", 210_000, 1024)
    for n in (16 * hip.PCA_ROWS_PER_WG, 420_000, 2 ** 30):                 # the row count does not enter once there are 16 super-chunks
        assert L.tmjx_pca_wide_workspace(n, 1024, C.byref(floats)) == 0 and floats.value == big
    assert L.tmjx_pca_wide_workspace(210_000, 512, C.byref(floats)) == 0 and 3.9 < big / floats.value < 4.1
    for n, d in ((2, 129), (300, 129), (130, 192), (4097, 257)):
        assert L.tmjx_pca_wide_workspace(n, d, C.byref(floats)) == 0 and floats.value == E.workspace("tmjx_pca_wide_workspace", n, d)
    assert L.tmjx_pca_wide_workspace(600, 128, C.byref(floats)) == 0 and floats.value == E.workspace("tmjx_pca_workspace", 600, 128)      # d <= 128: the narrow layout


def test_emu_refusals():
    x = R.make_data(8, 130)
    with pytest.raises(ValueError, match="d = 1025 exceeds the wide PCA limit of 1024"):
        B.fit_wide(np.zeros((4, 1025), np.float32))
    with pytest.raises(ValueError, match="n >= 2 rows .got 1."):
        B.fit_wide(x[:1])
    with pytest.raises(ValueError, match="ldx = 129 is smaller than d = 130"):
        E.over("tmjx_pca_fit_wide", ldx=129).fit_wide(x)
    mean = np.zeros(130, np.float32)
    with pytest.raises(ValueError, match="k = 131 components asked of d = 130"):
        B.transform_wide(x, mean, np.zeros((131, 130), np.float32))
    with pytest.raises(ValueError, match="ldo = 1 is smaller than k = 2"):
        E.over("tmjx_pca_transform_wide", ldo=1).transform_wide(x, mean, np.zeros((2, 130), np.float32))
    with pytest.raises(ValueError, match="d = 1025"):
        E.workspace("tmjx_pca_wide_workspace", 10, 1025)


def test_narrow_forwarding_gives_the_narrow_bits():
    case = (129, 65, 3.0, 0)
    x = R.case_data(*case)
    a, b = B.fit_wide(x), B.fit(x)
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
    assert a[3].sweeps == b[3].sweeps and E.workspace("tmjx_pca_wide_workspace", 129, 65) == E.workspace("tmjx_pca_workspace", 129, 65)
    np.testing.assert_array_equal(B.transform_wide(x, a[0], a[1][:4]).view(np.uint32), B.transform(x, b[0], b[1][:4]).view(np.uint32))


def test_two_calls_give_the_same_bits():
    x = R.case_data(*CASES[2])
    a, b = B.fit_wide(x), B.fit_wide(x.copy())
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
    assert a[3].sweeps == b[3].sweeps
    p = [B.transform_wide(x, a[0], a[1][:4]) for _ in range(2)]
    np.testing.assert_array_equal(p[0].view(np.uint32), p[1].view(np.uint32))


def test_degenerate_inputs():
    d = 130
    row = np.linspace(-3.0, 7.0, d).astype(np.float32)
    x = np.tile(row, (10, 1))
    mean, comp, var, info = B.fit_wide(x)
    np.testing.assert_array_equal(var, 0)
    np.testing.assert_array_equal(comp, np.eye(d, dtype=np.float32))
    np.testing.assert_array_equal(mean, row)
    assert info.converged == 1 and info.sweeps == 0
    assert np.isfinite(B.transform_wide(x, mean, comp)).all()
    p = P.PCA(2, backend=B).fit(x)
    np.testing.assert_array_equal(p.explained_variance_ratio_, 0)
    bad = R.make_data(40, d).copy()
    bad[3, 77] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        B.fit_wide(bad)
    bad[3, 77] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        B.fit_wide(bad)


# ------------------------------------------------------------------------------------------------------------------ Python and the tools
def test_pca_class_on_a_strided_wide_slice():
    n, d = 200, 160
    x = R.make_data(n, d, 3.0, 1)
    buf = np.full((n, d + 40), 1e6, np.float32)
    buf[:, 17:17 + d] = x
    view = buf[:, 17:17 + d]
    assert B.asarray(view) is view                                   # no copy: ldx = d + 40
    p = P.PCA(4, backend=B).fit(view)
    m64, c64, l64 = R.fit(x)
    assert p.components_.shape == (4, d) and p.n_samples_ == n and p.n_features_ == d
    assert 1 <= p.n_block_sweeps_ <= 15 and p.n_sweeps_ == p.n_block_sweeps_
    np.testing.assert_allclose(p.explained_variance_, l64[:4], rtol=1e-5)
    np.testing.assert_allclose(p.explained_variance_ratio_, l64[:4] / l64.sum(), rtol=1e-5)
    proj = p.transform(view)
    assert isinstance(proj, np.ndarray) and proj.shape == (n, 4)
    np.testing.assert_array_equal(proj, P.PCA(4, backend=B).fit_transform(x))
    assert R.projection_error(x, proj, 4) <= R.bound(d) / R.eigengap(l64, 4)
    narrow = P.PCA(4, backend=B).fit(x[:, :60])
    assert narrow.n_block_sweeps_ == 0 and narrow.n_sweeps_ >= 1     # d <= 128: the narrow fit
    with pytest.raises(ValueError, match="expected 160 features, got 159"):
        p.transform(x[:, :159])
    with pytest.raises(ValueError, match="d = 1025 exceeds the wide PCA limit of 1024"):
        P.PCA(backend=B).fit(np.zeros((4, 1025), np.float32))


def test_a_backend_without_the_wide_methods_behaves_as_before():
    old = types.SimpleNamespace(asarray=B.asarray, to_numpy=B.to_numpy, fit=B.fit, transform=B.transform)
    assert not hasattr(old, "fit_wide")
    with pytest.raises(ValueError, match="d = 129 exceeds the PCA limit of 128"):
        P.PCA(backend=old).fit(np.zeros((4, 129), np.float32))
    assert P.PCA(2, backend=old).fit(R.make_data(20, 8)).n_block_sweeps_ == 0


def _rollouts(n_clips=3, T=9, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n_clips):
        lat = R.make_data(T - 1, 6, 0.5, seed + c)
        out.append({"ctrl": rng.standard_normal((T - 1, 5)).astype(np.float32),
                    "activations": {"intention": lat, "decoder": {"layer_0": np.tanh(lat @ rng.standard_normal((6, 160))).astype(np.float32)},
                                    "hidden_state": {"h": np.tanh(lat @ rng.standard_normal((6, 256))).astype(np.float32)}}})
    return out


def test_fit_rollouts_and_both_tools_on_wide_features(tmp_path, capsys):
    from tests import render_scenes as S
    from tests.test_pca_cpu import EmuRenderer
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import render as Rn
    rolls = _rollouts()
    for feature, width in (("decoder/layer_0", 160), ("hidden_state/h", 256)):
        pca, proj = P.fit_rollouts(rolls, feature, 3, backend=B)
        allx = np.concatenate([r["activations"][feature.split("/")[0]][feature.split("/")[1]] for r in rolls])
        want = P.PCA(3, backend=B).fit(allx)
        assert pca.components_.shape == (3, width) and pca.n_samples_ == 24 and pca.n_block_sweeps_ >= 1
        np.testing.assert_array_equal(pca.components_, want.components_)
        np.testing.assert_array_equal(np.concatenate(proj), want.transform(allx))
        m64, c64, l64 = R.fit(allx)
        np.testing.assert_allclose(pca.explained_variance_, l64[:3], rtol=1e-4)
    w, m, qpos = S.walker_setup()
    (tmp_path / "in").mkdir()
    for c, r in zip((0, 3), rolls[:2]):
        h5lite.write_tree(tmp_path / "in" / f"clip_{c}.h5", dict(r, qposes_rollout=qpos[0, c:c + 9], qposes_ref=qpos[1, c:c + 9]))
    for feature, width in (("decoder/layer_0", 160), ("hidden_state/h", 256)):
        out = tmp_path / "fit" / f"pca_{width}.h5"
        assert P.main([f"rollouts={tmp_path / 'in'}", f"out={out}", "n_components=3", f"feature={feature}"], backend=B) == 0
        assert f"16 samples x {width} features from 2 clips" in capsys.readouterr().out
        pca, proj = P.fit_rollouts(tmp_path / "in", feature, 3, backend=B)
        with h5lite.File(out) as h:
            np.testing.assert_array_equal(h["components"][()], pca.components_)
            np.testing.assert_array_equal(h["projections/clip_3"][()], proj[1])
            assert bytes(h["feature"][()]).decode() == feature and h["mean"][()].shape == (width,)
    common = [f"rollouts={tmp_path / 'in'}", "size=24x18", "camera=side"]
    assert Rn.main(common + [f"out={tmp_path / 'wide'}", f"pca={tmp_path / 'fit' / 'pca_160.h5'}", "pca_window=4"], renderer_cls=EmuRenderer, pca_backend=B) == 0
    with h5lite.File(tmp_path / "wide" / "clip_3.frames.h5") as h:
        assert bytes(h["pca_feature"][()]).decode() == "decoder/layer_0" and h["frames"][()].shape[2] == 24 + 640
        np.testing.assert_array_equal(h["pca_explained_variance_ratio"][()], P.fit_rollouts(tmp_path / "in", "decoder/layer_0", 3, backend=B)[0].explained_variance_ratio_)


def test_abi_declares_the_wide_entry_points():
    names = ("tmjx_pca_wide_workspace", "tmjx_pca_fit_wide", "tmjx_pca_transform_wide")
    assert set(names) <= set(hip.EXPORTS)
    header = (ROOT / "include" / "tmjx.h").read_text()
    for name in names + ("#define PCA_WIDE_MAX_D 1024",):
        assert name in header
    assert any(p.name == "tmjx_pca_wide.hip" for p in hip.SOURCES)
    core = (ROOT / "track_mjx_amd" / "csrc" / "pca_wide_core.h").read_text()
    assert f"#define PCA_WIDE_MAX_D {hip.PCA_WIDE_MAX_D}" in core and f"#define PCA_WIDE_BLOCK {hip.PCA_WIDE_BLOCK}" in core
    assert f"#define PCA_WIDE_MAX_SUPER {hip.PCA_WIDE_MAX_SUPER}" in (ROOT / "track_mjx_amd" / "csrc" / "moments_core.h").read_text()      # (with the split)
    for name in ("fit_wide", "transform_wide"):
        assert callable(getattr(P.HipBackend, name))


def test_emulation_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """The emulation's own main, built with AddressSanitizer and UBSan (a host program: no preload, no Python), runs clean at 130 x 192."""
    exe = E.build_main("pca_wide", tmp_path / "pca_wide_emu", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    out = subprocess.run([str(exe), "130", "192"], capture_output=True, text=True)
    assert out.returncode == 0 and "checksum" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr
    assert "130 x 192" in out.stdout and "block sweeps" in out.stdout
