"""PCA and the progression panel on the CPU: the float64 reference's own preconditions (eigengaps, the share of panel pixels it excludes), the host
emulation of the kernel bodies (tests/hostemu/pca_emu.cpp),
called through the shared analysis backend (tests/hostemu/analysis_emu.py), under the checks tests/test_gpu_pca.py applies to the kernels at the same shapes, every
refusal, analysis.pca / analysis.render on the emulation, both command-line tools on synthetic clip_<i>.h5 files, and sklearn where it imports."""
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
CASES = R.fit_cases(hip.PCA_ROWS_PER_WG)
B = E.B


# ------------------------------------------------------------------------------------------------------------------ 1. the reference alone
@pytest.mark.parametrize("case", CASES)
def test_generator_eigengaps(case):
    gap = R.case_reference(*case)[2]
    print(case, f"top-{R.top_k(case[0], case[1]) + 1} relative eigengap {gap:.3f}")
    assert gap >= 0.05


@pytest.mark.parametrize("size", R.PANEL_SIZES)
def test_reference_panel_excludes_under_a_thousandth(size):
    for k in R.PANEL_KS:
        for window in R.PANEL_WINDOWS:
            ref, near = R.panel_reference(size, k, window)
            share = near.reshape(near.shape[0], -1).mean(1)
            print(size, k, window, f"excluded share per frame: {np.round(100 * share, 4)} %")
            assert share.max() <= 1e-3 and (ref[..., 3] == 255).all()
            colours = {tuple(c) for c in ref[-1].reshape(-1, 4)[:, :3]}
            st = R.style_dict(R.panel_style(*size))
            assert {st["background"], st["axes"], st["terminated"], st["colour"][0]} <= colours      # a picture: every layer is visible in the last frame
            assert (ref[0] == ref[0][0, 0]).all(-1).sum() > 0 and {tuple(c) for c in ref[0].reshape(-1, 4)[:, :3]} == {st["background"], st["axes"]}      # i = 0: empty


def test_one_pass_variance_fails_the_offset_case():
    """The check has teeth: float32 E[x^2] - E[x]^2 misses the bound of the offset-100 case by orders of magnitude."""
    case = CASES[-1]
    x = R.case_data(*case)
    n = x.shape[0]
    mean = x.mean(0, dtype=np.float32)
    cov = ((x.T @ x) / np.float32(n) - np.outer(mean, mean)) * np.float32(n / (n - 1))
    lam, vec = np.linalg.eigh(cov.astype(np.float32))
    order = np.argsort(-lam)
    m = R.fit_metrics(x, mean, R.sign_rows(vec.T[order]), np.maximum(lam[order], 0))
    print(m, R.bound(case[1]))
    assert m["eig"] > 100 * R.bound(case[1])


# ------------------------------------------------------------------------------------------------------------------ 2. the emulation: fit / transform
@pytest.mark.parametrize("case", CASES)
def test_emu_fit_and_transform(case):
    x = R.case_data(*case)
    mean, comp, var, info = B.fit(x)
    assert info.converged == 1 and info.sweeps <= 15
    R.check_fit(x, mean, comp, var, B.transform(x, mean, comp[:R.top_k(*x.shape)]), case, "emulation")


def test_emu_row_stride():
    case = (129, 65, 3.0, 0)
    x = R.case_data(*case)
    wide = np.full((129, 65 + 5), 1e6, np.float32)
    wide[:, 3:68] = x
    view = wide[:, 3:68]
    assert view.strides[0] == 4 * (65 + 5)
    a, b = B.fit(view), B.fit(x)
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(B.transform(view, a[0], a[1][:4]), B.transform(x, b[0], b[1][:4]))


def test_emu_degenerate_and_repeatable():
    x = np.tile(np.float32([1.5, -2.0, 7.0]), (10, 1))
    mean, comp, var, info = B.fit(x)
    np.testing.assert_array_equal(var, 0)
    np.testing.assert_array_equal(comp, np.eye(3, dtype=np.float32))
    np.testing.assert_array_equal(mean, x[0])
    assert np.isfinite(B.transform(x, mean, comp)).all()
    n, d = 5, 9                                        # n < d: d - n + 1 variances vanish
    x = R.make_data(n, d, 3.0, 2)
    a, b = B.fit(x), B.fit(x.copy())
    assert (a[2][n - 1:] <= R.bound(d) * a[2][0]).all() and a[2][n - 2] > 1e-3 * a[2][0]
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
    bad = R.make_data(20, 4).copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="did not converge"):
        B.fit(bad)


def test_emu_refusals():
    x = R.make_data(8, 4)
    with pytest.raises(ValueError, match="d = 129 exceeds the PCA limit of 128"):
        B.fit(np.zeros((4, 129), np.float32))
    with pytest.raises(ValueError, match="n >= 2 rows .got 1."):
        B.fit(x[:1])
    with pytest.raises(ValueError, match="ldx = 3 is smaller than d = 4"):
        E.over("tmjx_pca_fit", ldx=3).fit(x)
    mean, comp, _, _ = B.fit(x)
    with pytest.raises(ValueError, match="k = 5 components asked of d = 4"):
        B.transform(x, mean, np.zeros((5, 4), np.float32))
    with pytest.raises(ValueError, match="ldo = 1 is smaller than k = 2"):
        E.over("tmjx_pca_transform", ldo=1).transform(x, mean, comp[:2])
    with pytest.raises(ValueError, match="d = 129"):
        E.workspace("tmjx_pca_workspace", 10, 129)
    p, st = R.panel_projections(), R.panel_style(96, 64)
    ok = dict(proj=p, k=3, frame_idx=[1], flags=[0], ymin=-1.0, ymax=1.0, window=5, style=st, width=96, height=64)
    assert B.strips(**ok).shape == (1, 64, 96, 4)
    for over, word in ((dict(k=9), "k = 9 curves"), (dict(k=0), "k = 0 curves"), (dict(ldp=2), "ldp = 2"), (dict(window=0), "window must be >= 1"),
                       (dict(ymax=-1.0), "ymax > ymin"), (dict(ymax=float("inf")), "finite"), (dict(width=0), "W and H"), (dict(T=0), "T must be >= 1"),
                       (dict(frame_idx=[]), "F must be >= 1"), (dict(width=12), "smaller than 3 x 3")):
        args = {k: over.pop(k) for k in list(over) if k in ("ldp", "T")}      # (not arguments of the method: substituted in tmjx_plot_strips)
        with pytest.raises(ValueError, match=word):
            E.over("tmjx_plot_strips", **args).strips(**dict(ok, **over))
    thin = P.strip_style(96, 64, line_half_width=0.0)
    with pytest.raises(ValueError, match="line_half_width"):
        B.strips(**dict(ok, style=thin))


def test_library_refuses_before_any_launch():
    """The product library's own checks (no GPU is touched: the dummy pointers are never dereferenced)."""
    L = hip.lib()
    one, info, floats = C.c_void_p(1 << 20), hip.PcaInfo(), C.c_int64(0)
    for args, word in (((one, 10, 129, 129), b"d = 129 exceeds the PCA limit of 128"), ((one, 1, 4, 4), b"n >= 2"), ((one, 10, 4, 3), b"ldx = 3")):
        assert L.tmjx_pca_fit(*args, one, one, one, one, C.byref(info), None) == -22 and word in L.tmjx_last_error(), L.tmjx_last_error()
    assert L.tmjx_pca_fit(one, 10, 4, 4, one, one, one, C.c_void_p((1 << 20) + 4), C.byref(info), None) == -22 and b"aligned" in L.tmjx_last_error()
    assert L.tmjx_pca_transform(one, 10, 4, 4, one, one, 5, one, 5, None) == -22 and b"k = 5" in L.tmjx_last_error()
    assert L.tmjx_pca_transform(one, 10, 4, 3, one, one, 2, one, 2, None) == -22 and b"ldx = 3" in L.tmjx_last_error()
    assert L.tmjx_pca_workspace(1, 4, C.byref(floats)) == -22 and L.tmjx_pca_workspace(10, 129, C.byref(floats)) == -22
    assert L.tmjx_pca_workspace(2 * hip.PCA_ROWS_PER_WG + 1, 128, C.byref(floats)) == 0 and floats.value == E.workspace("tmjx_pca_workspace", 2 * hip.PCA_ROWS_PER_WG + 1, 128)
    st = R.panel_style(96, 64)
    assert L.tmjx_plot_strips(one, 12, 9, 9, one, one, 1, -1.0, 1.0, 5, C.byref(st), 96, 64, one, None) == -22 and b"k = 9" in L.tmjx_last_error()
    assert L.tmjx_plot_strips(one, 12, 3, 3, one, one, 1, 1.0, 1.0, 5, C.byref(st), 96, 64, one, None) == -22 and b"ymax > ymin" in L.tmjx_last_error()


def test_abi_declares_pca():
    names = ("tmjx_pca_workspace", "tmjx_pca_fit", "tmjx_pca_transform", "tmjx_plot_strips")
    assert set(names) <= set(hip.EXPORTS)
    header = (ROOT / "include" / "tmjx.h").read_text()
    for name in names + ("tmjx_pca_info_t", "tmjx_strip_style_t", "TMJX_ENOCONV"):
        assert name in header
    assert any(p.name == "tmjx_pca.hip" for p in hip.SOURCES) and "tmjx_pca.hip" not in hip.SOURCE_FLAGS
    assert C.sizeof(hip.PcaInfo) == 20 and C.sizeof(hip.StripStyle) == 68
    core = (ROOT / "track_mjx_amd" / "csrc" / "pca_core.h").read_text()
    wg = (ROOT / "track_mjx_amd" / "csrc" / "wg_core.h").read_text()      # (the fixed row split is the discipline's)
    assert f"#define PCA_ROWS_PER_WG {hip.PCA_ROWS_PER_WG}" in wg and f"#define PCA_MAX_D {hip.PCA_MAX_D}" in core and f"#define PCA_MAX_K {hip.PCA_MAX_K}" in core


# ------------------------------------------------------------------------------------------------------------------ 3. the emulation: the panel
@pytest.mark.parametrize("window", R.PANEL_WINDOWS)
@pytest.mark.parametrize("k", R.PANEL_KS)
@pytest.mark.parametrize("size", R.PANEL_SIZES)
def test_emu_panel(size, k, window):
    flags = np.zeros(len(R.PANEL_FRAMES), np.uint8)
    flags[-1] = 1
    got = B.strips(R.panel_projections(), k, R.PANEL_FRAMES, flags, *R.PANEL_YLIM, window, R.panel_style(*size), *size)
    R.check_panel(got, size, k, window, "emulation")


# ------------------------------------------------------------------------------------------------------------------ 4. Python and the tools
def test_pca_class_on_the_emulation():
    x = R.case_data(*CASES[3])
    p = P.PCA(4, backend=B).fit(x)
    m64, c64, l64 = R.fit(x)
    assert p.components_.shape == (4, 60) and p.mean_.shape == (60,) and p.n_samples_ == 63 and 1 <= p.n_sweeps_ <= 15
    np.testing.assert_allclose(p.explained_variance_, l64[:4], rtol=1e-5)
    np.testing.assert_allclose(p.explained_variance_ratio_, l64[:4] / l64.sum(), rtol=1e-5)
    proj = p.transform(x)
    assert isinstance(proj, np.ndarray) and proj.shape == (63, 4)
    np.testing.assert_array_equal(proj, P.PCA(4, backend=B).fit_transform(x))
    full = P.PCA(backend=B).fit(x)
    assert full.components_.shape == (60, 60)                     # n_components=None: min(n, d)
    assert P.PCA(backend=B).fit(x[:7]).components_.shape == (7, 60)
    flat = P.PCA(2, backend=B).fit(np.ones((5, 3), np.float32))
    np.testing.assert_array_equal(flat.explained_variance_ratio_, 0)
    with pytest.raises(ValueError, match="n_components = 61 exceeds the 60 features"):
        P.PCA(61, backend=B).fit(x)
    with pytest.raises(ValueError, match="n_components must be >= 1"):
        P.PCA(0, backend=B)
    with pytest.raises(ValueError, match="not fitted"):
        P.PCA(2, backend=B).transform(x)
    with pytest.raises(ValueError, match="expected 60 features, got 59"):
        p.transform(x[:, :59])
    with pytest.raises(ValueError, match="2-D"):
        p.fit(x[0])
    narrow = types.SimpleNamespace(asarray=B.asarray, to_numpy=B.to_numpy, fit=B.fit, transform=B.transform)      # a backend without the wide methods
    with pytest.raises(ValueError, match="d = 129"):
        P.PCA(backend=narrow).fit(np.zeros((4, 129), np.float32))


def _rollouts(n_clips=3, T=9, Z=6, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n_clips):
        lat = R.make_data(T - 1, Z, 0.5, seed + c)
        out.append({"ctrl": rng.standard_normal((T - 1, 5)).astype(np.float32),
                    "activations": {"intention": lat, "decoder": {"layer_0": np.tanh(lat @ rng.standard_normal((Z, 12))).astype(np.float32)}}})
    return out


def test_fit_rollouts_on_the_emulation(tmp_path):
    from track_mjx_amd import h5lite
    rolls = _rollouts()
    pca, proj = P.fit_rollouts(rolls, "intention", 3, backend=B)
    allx = np.concatenate([r["activations"]["intention"] for r in rolls])
    want = P.PCA(3, backend=B).fit(allx)
    np.testing.assert_array_equal(pca.components_, want.components_)
    assert pca.clips_ == [0, 1, 2] and [p.shape for p in proj] == [(8, 3)] * 3 and pca.n_samples_ == 24
    np.testing.assert_array_equal(np.concatenate(proj), want.transform(allx))
    assert P.fit_rollouts(rolls, "decoder/layer_0", 2, backend=B)[0].components_.shape == (2, 12)
    assert P.fit_rollouts(rolls, "ctrl", 2, backend=B)[0].components_.shape == (2, 5)
    with pytest.raises(KeyError, match="no activations/encoder/layer_9"):
        P.fit_rollouts(rolls, "encoder/layer_9", backend=B)
    with pytest.raises(KeyError, match="is a group"):
        P.fit_rollouts(rolls, "decoder", backend=B)
    for c, r in zip((4, 11, 2), rolls):                            # a directory: clips in numeric order
        h5lite.write_tree(tmp_path / f"clip_{c}.h5", r)
    pca2, proj2 = P.fit_rollouts(tmp_path, "intention", 3, backend=B)
    assert pca2.clips_ == [2, 4, 11]
    np.testing.assert_array_equal(proj2[1], P.fit_rollouts([rolls[2], rolls[0], rolls[1]], "intention", 3, backend=B)[1][1])
    with pytest.raises(ValueError, match="no clip_<i>.h5"):
        P.fit_rollouts(tmp_path / "nothing_here" if (tmp_path / "nothing_here").mkdir() is None else None, backend=B)


class EmuRenderer:
    """analysis.render.Renderer's constructor and .render on the renderer's host emulation."""

    def __init__(self, walker, device, height=480, width=640, camera="close_profile", render_ghost=True):
        from tests.hostemu import render_emu
        from track_mjx_amd import blob as _blob
        self.em, self.h, self.w, self.ghost = render_emu.RenderEmu(_blob.pack(walker.model)), height, width, render_ghost
        self.cam = self.em.camera(camera)

    def render(self, q, g=None):
        return self.em.render(q, g if self.ghost else None, self.cam, self.w, self.h)[0][..., :3]


def test_progression_functions_on_the_emulation():
    from tests import render_scenes as S
    from track_mjx_amd import config as _config
    from track_mjx_amd.analysis import render as Rn
    proj = R.panel_projections()
    idx = np.arange(70) % 13
    term = idx == 12
    panel = Rn.plot_pca_progression(proj, idx, n_components=3, window_size=5, size=(48, 32), terminated=term, backend=B)
    assert panel.shape == (70, 32, 48, 3) and panel.dtype == np.uint8 and Rn.MAX_FRAMES_PER_CALL == 64
    lo, hi = np.nanmin(proj[:, :3]) - 0.2, np.nanmax(proj[:, :3]) + 0.2      # the reference's y limits
    one = B.strips(proj, 3, idx[60:], term[60:].astype(np.uint8), float(lo), float(hi), 5, P.strip_style(48, 32), 48, 32)[..., :3]
    np.testing.assert_array_equal(panel[60:], one)
    np.testing.assert_array_equal(panel[13:26], panel[:13])
    with pytest.raises(ValueError, match="n_components = 9"):
        Rn.plot_pca_progression(proj, idx, n_components=9, backend=B)
    with pytest.raises(ValueError, match=r"frame_idx must lie in \[0, 12\]"):
        Rn.plot_pca_progression(proj, [13], backend=B)
    w, m, qpos = S.walker_setup()
    cfg = _config.default_config()
    roll = {"qposes_rollout": qpos[0, :7], "qposes_ref": qpos[1, :7]}
    frames, fps = Rn.render_with_pca_progression(cfg, roll, proj[:6], n_components=2, hold=3, window_size=4, panel_width=30, backend=B, height=18, width=24,
                                                 every=2, renderer_cls=EmuRenderer)
    base, fps0 = Rn.render_rollout(cfg, roll, height=18, width=24, every=2, renderer_cls=EmuRenderer)
    assert frames.shape == (4 + 3, 18, 24 + 30, 3) and fps == fps0
    np.testing.assert_array_equal(frames[:4, :, :24], base)
    want = Rn.plot_pca_progression(proj[:6], [0, 2, 4, 6, 6], 2, 4, (30, 18), [0, 0, 0, 0, 1], backend=B)
    np.testing.assert_array_equal(frames[:4, :, 24:], want[:4])
    for f in frames[4:]:
        np.testing.assert_array_equal(f, np.concatenate([base[-1], want[4]], 1))
    assert (want[4] != want[3]).any()                              # the terminated line


def test_both_tools_end_to_end(tmp_path, capsys):
    from tests import render_scenes as S
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import render as Rn
    w, m, qpos = S.walker_setup()
    rolls = _rollouts(2, T=7)
    (tmp_path / "in").mkdir()
    for c, r in zip((0, 3), rolls):
        h5lite.write_tree(tmp_path / "in" / f"clip_{c}.h5", dict(r, qposes_rollout=qpos[0, c:c + 7], qposes_ref=qpos[1, c:c + 7]))
    out = tmp_path / "fit" / "pca.h5"
    assert P.main([f"rollouts={tmp_path / 'in'}", f"out={out}", "n_components=3"], backend=B) == 0
    assert "12 samples x 6 features from 2 clips" in capsys.readouterr().out
    pca, proj = P.fit_rollouts(tmp_path / "in", "intention", 3, backend=B)
    with h5lite.File(out) as h:
        assert sorted(h.keys()) == ["clips", "components", "explained_variance", "explained_variance_ratio", "feature", "mean", "n_samples", "projections"]
        np.testing.assert_array_equal(h["components"][()], pca.components_)
        np.testing.assert_array_equal(h["mean"][()], pca.mean_)
        np.testing.assert_array_equal(h["explained_variance_ratio"][()], pca.explained_variance_ratio_)
        assert bytes(h["feature"][()]).decode() == "intention" and int(h["n_samples"][()]) == 12 and list(h["clips"][()]) == [0, 3]
        np.testing.assert_array_equal(h["projections/clip_3"][()], proj[1])
        assert h["projections/clip_0"][()].shape == (6, 3)
    assert P.main([f"rollouts={tmp_path / 'in'}"], backend=B) == 2 and "usage" in capsys.readouterr().err
    assert P.main([f"rollouts={tmp_path / 'in'}", f"out={out}", "feature=encoder/layer_7"], backend=B) == 2 and "no activations/encoder/layer_7" in capsys.readouterr().err
    # the render tool: without pca= what it wrote before, with pca= the wide frames and the legend as data
    common = [f"rollouts={tmp_path / 'in'}", "size=24x18", "camera=side"]
    assert Rn.main(common + [f"out={tmp_path / 'plain'}"], renderer_cls=EmuRenderer) == 0
    assert Rn.main(common + [f"out={tmp_path / 'wide'}", f"pca={out}", "pca_window=4"], renderer_cls=EmuRenderer, pca_backend=B) == 0
    with h5lite.File(tmp_path / "plain" / "clip_3.frames.h5") as h:
        assert sorted(h.keys()) == ["camera", "fps", "frames"]
        plain = h["frames"][()]
    with h5lite.File(tmp_path / "wide" / "clip_3.frames.h5") as h:
        wide, ratio, colours = h["frames"][()], h["pca_explained_variance_ratio"][()], h["pca_colors"][()]
        assert bytes(h["pca_feature"][()]).decode() == "intention" and float(h["fps"][()]) == pytest.approx(50.0)
    assert plain.shape == (7, 18, 24, 3) and wide.shape == (7 + 50, 18, 24 + 640, 3)
    np.testing.assert_array_equal(wide[:7, :, :24], plain)
    np.testing.assert_array_equal(ratio, pca.explained_variance_ratio_)
    np.testing.assert_array_equal(colours, np.asarray(P.STRIP_COLOURS[:3], np.uint8))
    np.testing.assert_array_equal(wide[:7, :, 24:], Rn.plot_pca_progression(proj[1], np.minimum(np.arange(7), 6), 3, 4, (640, 18), backend=B))
    (tmp_path / "in" / "clip_5.h5").write_bytes((tmp_path / "in" / "clip_3.h5").read_bytes())
    assert Rn.main(common + [f"out={tmp_path / 'wide'}", f"pca={out}"], renderer_cls=EmuRenderer, pca_backend=B) == 2
    assert "no projections/clip_5" in capsys.readouterr().err


def test_against_sklearn():
    sk = pytest.importorskip("sklearn.decomposition")
    for case in (CASES[3], CASES[5], CASES[8]):
        x = R.case_data(*case)
        ref = sk.PCA(n_components=4, svd_solver="full").fit(x.astype(np.float64))
        p = P.PCA(4, backend=B).fit(x)
        gap = R.case_reference(*case)[2]
        tol = R.bound(case[1]) / gap
        assert np.abs(p.components_ - ref.components_).max() <= tol                      # signs included
        assert np.abs(p.explained_variance_ratio_ - ref.explained_variance_ratio_).max() <= R.bound(case[1])
        want = ref.transform(x.astype(np.float64))
        assert np.abs(p.transform(x) - want).max() / np.abs(want).max() <= tol


def test_emulation_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """The emulation's own main, built with AddressSanitizer and UBSan (a host program: no preload, no Python), runs clean."""
    exe = E.build_main("pca", tmp_path / "pca_emu", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "checksum" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr
    assert out.stdout.count("sweeps") == 6
