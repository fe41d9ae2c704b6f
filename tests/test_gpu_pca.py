"""The PCA kernels and the progression panel (csrc/tmjx_pca.hip) against the float64 reference (tests/pca_ref.py): every fit metric under
max(d, 8) 2^-23, the projections under that over the eigengap, the panel pixel for pixel; bit-for-bit repeatability, the refusals, and
analysis.pca / analysis.render on top.  The measured values are in DESIGN.md "PCA"."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests import pca_ref as R
from track_mjx_amd import hip
from track_mjx_amd.analysis import pca as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = R.fit_cases(hip.PCA_ROWS_PER_WG)


def backend():
    return P.HipBackend(DEV)


def fit_dev(x):
    b = backend()
    return b.fit(b.asarray(x))


@pytest.mark.parametrize("case", CASES)
def test_fit_and_transform(case):
    x = R.case_data(*case)
    b = backend()
    xd = b.asarray(x)
    mean, comp, var, info = b.fit(xd)
    assert info.converged == 1 and info.sweeps <= 15
    proj = b.transform(xd, mean, comp[:R.top_k(*x.shape)]).cpu().numpy()
    R.check_fit(x, mean, comp, var, proj, case, "kernel")


def test_row_stride_at_a_column_offset():
    case = (129, 65, 3.0, 0)
    x = R.case_data(*case)
    wide = torch.full((129, 65 + 5), 1e6, dtype=torch.float32, device=DEV)
    wide[:, 3:68] = torch.from_numpy(x.copy())
    view = wide[:, 3:68]
    b = backend()
    assert b.asarray(view).data_ptr() == view.data_ptr() and view.stride(0) == 65 + 5      # no copy: ldx = d + 5
    got, dense = b.fit(view), b.fit(b.asarray(x))
    for u, v in zip(got[:3], dense[:3]):
        np.testing.assert_array_equal(u, v)
    proj = b.transform(view, got[0], got[1][:4]).cpu().numpy()
    R.check_fit(x, *got[:3], proj, case, "kernel, ldx = d + 5")
    out = torch.full((129, 7), -5.0, dtype=torch.float32, device=DEV)                       # ldo > k: the other columns are not written
    m, c = torch.as_tensor(got[0], device=DEV), torch.as_tensor(got[1][:4].copy(), device=DEV)
    hip.check(hip.lib().tmjx_pca_transform(view.data_ptr(), 129, 65, 70, m.data_ptr(), c.data_ptr(), 4, out.data_ptr(), 7, None), "tmjx_pca_transform")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[:, :4].cpu().numpy(), proj)
    assert (out[:, 4:] == -5.0).all()


def test_degenerate_inputs():
    x = np.tile(np.float32([1.5, -2.0, 7.0]), (10, 1))
    mean, comp, var, info = fit_dev(x)
    np.testing.assert_array_equal(var, 0)
    np.testing.assert_array_equal(comp, np.eye(3, dtype=np.float32))
    np.testing.assert_array_equal(mean, x[0])
    p = P.PCA(2, device=DEV).fit(x)
    np.testing.assert_array_equal(p.explained_variance_ratio_, 0)
    assert np.isfinite(p.transform(x)).all()
    n, d = 5, 9                                        # n < d: d - n + 1 variances vanish
    mean, comp, var, info = fit_dev(R.make_data(n, d, 3.0, 2))
    print("n < d variances / largest:", var / var[0])
    assert (var[n - 1:] <= R.bound(d) * var[0]).all() and var[n - 2] > 1e-3 * var[0] and np.isfinite(comp).all()
    bad = R.make_data(20, 4).copy()
    bad[3, 1] = np.nan
    with pytest.raises(hip.TmjxError, match="did not converge"):
        fit_dev(bad)


def test_two_calls_give_the_same_bits():
    x = R.case_data(*CASES[7])                         # several row chunks: the reduction order is fixed
    b = backend()
    xd = b.asarray(x)
    first, second = b.fit(xd), b.fit(xd)
    for u, v in zip(first[:3], second[:3]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
    p1, p2 = (b.transform(xd, first[0], first[1][:4]).cpu().numpy() for _ in range(2))
    np.testing.assert_array_equal(p1.view(np.uint32), p2.view(np.uint32))


def test_refusals_launch_nothing():
    L, b = hip.lib(), backend()
    x = b.asarray(R.make_data(8, 4))
    with pytest.raises(hip.TmjxError, match="d = 129 exceeds the PCA limit of 128"):
        b.fit(torch.zeros((4, 129), dtype=torch.float32, device=DEV))
    with pytest.raises(hip.TmjxError, match="n >= 2 rows .got 1."):
        b.fit(x[:1])
    mean, comp, var, _ = b.fit(x)
    info, ws, outs = hip.PcaInfo(), torch.zeros(4096, device=DEV), [torch.full((16,), 7.0, device=DEV) for _ in range(3)]
    assert L.tmjx_pca_fit(x.data_ptr(), 8, 4, 3, *[o.data_ptr() for o in outs], ws.data_ptr(), C.byref(info), None) == -22       # ldx < d
    assert b"ldx = 3 is smaller than d = 4" in L.tmjx_last_error()
    with pytest.raises(hip.TmjxError, match="k = 5 components asked of d = 4"):
        b.transform(x, mean, np.zeros((5, 4), np.float32))
    with pytest.raises(ValueError, match="n_components = 5 exceeds the 4 features"):
        P.PCA(5, device=DEV).fit(x)
    torch.cuda.synchronize()
    assert all((o == 7.0).all() for o in outs) and (ws == 0).all()      # nothing was written


@pytest.mark.parametrize("window", R.PANEL_WINDOWS)
@pytest.mark.parametrize("k", R.PANEL_KS)
@pytest.mark.parametrize("size", R.PANEL_SIZES)
def test_panel(size, k, window):
    b = backend()
    flags = np.zeros(len(R.PANEL_FRAMES), np.uint8)
    flags[-1] = 1
    got = b.strips(b.asarray(R.panel_projections()), k, R.PANEL_FRAMES, flags, *R.PANEL_YLIM, window, R.panel_style(*size), *size)
    R.check_panel(got, size, k, window, "kernel")


def test_plot_pca_progression_batches():
    from track_mjx_amd.analysis import render as Rn
    proj = R.panel_projections()
    idx = np.arange(65) % 13
    term = idx == 12
    assert Rn.MAX_FRAMES_PER_CALL == 64
    panel = Rn.plot_pca_progression(proj, idx, n_components=3, window_size=5, size=(48, 32), terminated=term, device=DEV)
    assert panel.shape == (65, 32, 48, 3) and panel.dtype == np.uint8
    b, lo, hi = backend(), float(np.nanmin(proj[:, :3])) - 0.2, float(np.nanmax(proj[:, :3])) + 0.2
    two = [b.strips(b.asarray(proj), 3, idx[s], term[s].astype(np.uint8), lo, hi, 5, P.strip_style(48, 32), 48, 32)[..., :3] for s in (slice(0, 64), slice(64, 65))]
    np.testing.assert_array_equal(panel, np.concatenate(two))
    assert len(np.unique(panel[11].reshape(-1, 3), axis=0)) >= 5       # background, axes and three curves


def _synthetic_rollouts():
    from tests import render_scenes as S
    w, m, qpos = S.walker_setup()
    rolls = []
    for c in range(3):
        lat = R.make_data(6, 8, 0.5, 10 + c)
        rolls.append({"qposes_rollout": qpos[0, c:c + 7], "qposes_ref": qpos[1, c:c + 7], "ctrl": lat[:, :5].copy(), "activations": {"intention": lat}})
    return rolls


def test_render_with_pca_progression():
    from track_mjx_amd import config as _config
    from track_mjx_amd.analysis import render as Rn
    rolls = _synthetic_rollouts()
    pca, proj = P.fit_rollouts(rolls, "intention", 4, device=DEV)
    assert pca.n_samples_ == 18 and [p.shape for p in proj] == [(6, 4)] * 3
    cfg = _config.default_config()
    kw = dict(height=30, width=40, every=2, camera="side", device=DEV)
    frames, fps = Rn.render_with_pca_progression(cfg, rolls[1], proj[1], n_components=4, feature_name="intention", hold=5, window_size=4, panel_width=56, **kw)
    base, fps0 = Rn.render_rollout(cfg, rolls[1], **kw)
    assert frames.shape == (4 + 5, 30, 40 + 56, 3) and fps == fps0
    np.testing.assert_array_equal(frames[:4, :, :40], base)                                  # the left W columns: render_rollout's frames, bit for bit
    want = Rn.plot_pca_progression(proj[1], [0, 2, 4, 6, 6], 4, 4, (56, 30), [0, 0, 0, 0, 1], device=DEV)
    np.testing.assert_array_equal(frames[:4, :, 40:], want[:4])                              # the right Wp: plot_pca_progression
    for f in frames[4:]:                                                                     # hold: the last frame with the terminated line
        np.testing.assert_array_equal(f, np.concatenate([base[-1], want[4]], 1))
    assert (want[4] != want[3]).any()


def test_tools_and_the_unchanged_render_cli(tmp_path):
    from track_mjx_amd import config as _config
    from track_mjx_amd import h5lite
    from track_mjx_amd.analysis import render as Rn
    rolls = _synthetic_rollouts()
    (tmp_path / "in").mkdir()
    for c, r in enumerate(rolls):
        h5lite.write_tree(tmp_path / "in" / f"clip_{c}.h5", r)
    common = [f"rollouts={tmp_path / 'in'}", "size=40x30", "camera=side"]
    assert Rn.main(common + [f"out={tmp_path / 'plain'}"]) == 0
    with h5lite.File(tmp_path / "plain" / "clip_2.frames.h5") as h:                          # without pca=: what the tool wrote before
        assert sorted(h.keys()) == ["camera", "fps", "frames"]
        plain, fps = h["frames"][()], float(h["fps"][()])
    want, _ = Rn.render_rollout(_config.default_config(), rolls[2], height=30, width=40, camera="side", device=DEV)
    np.testing.assert_array_equal(plain, want)
    assert fps == pytest.approx(50.0)
    again = tmp_path / "again"
    assert Rn.main(common + [f"out={again}"]) == 0
    assert (again / "clip_2.frames.h5").read_bytes() == (tmp_path / "plain" / "clip_2.frames.h5").read_bytes()
    assert P.main([f"rollouts={tmp_path / 'in'}", f"out={tmp_path / 'pca.h5'}", "n_components=3"]) == 0
    assert Rn.main(common + [f"out={tmp_path / 'wide'}", f"pca={tmp_path / 'pca.h5'}", "pca_window=4"]) == 0
    with h5lite.File(tmp_path / "wide" / "clip_2.frames.h5") as h:
        wide, ratio = h["frames"][()], h["pca_explained_variance_ratio"][()]
        assert bytes(h["pca_feature"][()]).decode() == "intention" and h["pca_colors"][()].shape == (3, 3)
    assert wide.shape == (7 + 50, 30, 40 + 640, 3) and ratio.shape == (3,) and 0.5 < ratio.sum() <= 1.0 + 1e-6
    np.testing.assert_array_equal(wide[:7, :, :40], plain)
