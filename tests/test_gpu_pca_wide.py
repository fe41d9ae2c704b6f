"""The wide PCA kernels (csrc/tmjx_pca_wide.hip: 129 <= d <= 1024, block Jacobi) against the float64 reference (tests/pca_ref.py): every fit
metric under max(d, 8) 2^-23, the projections under that over the eigengap, at most 15 block sweeps; a row stride, bit-for-bit repeatability, the
refusals, and analysis.pca on top.  The measured values are in DESIGN.md "PCA"."""
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
# the cases of tests/test_pca_wide_cpu.py, and the size limit: 16 blocks, 8 concurrent pairs
CASES = ((300, 129, 3.0, 0), (130, 192, 3.0, 0), (513, 257, 3.0, 0), (700, 320, 3.0, 0), (1500, 512, 100.0, 0), (2100, 1024, 3.0, 0))


def backend():
    return P.HipBackend(DEV)


@pytest.mark.parametrize("case", CASES)
def test_fit_and_transform(case):
    x = R.case_data(*case)
    b = backend()
    xd = b.asarray(x)
    mean, comp, var, info = b.fit_wide(xd)
    print(case, f"{info.sweeps} block sweeps, off / norm {info.off_rel:.2e}, moments {info.moments_ms:.3f} ms, block iteration {info.jacobi_ms:.3f} ms")
    assert info.converged == 1 and 1 <= info.sweeps <= 15
    proj = b.transform_wide(xd, mean, comp[:R.top_k(*x.shape)]).cpu().numpy()
    R.check_fit(x, mean, comp, var, proj, case, "kernel")


def test_row_stride_at_a_column_offset():
    case = CASES[2]
    n, d = case[:2]
    x = R.case_data(*case)
    wide = torch.full((n, d + 5), 1e6, dtype=torch.float32, device=DEV)
    wide[:, 3:3 + d] = torch.from_numpy(x.copy())
    view = wide[:, 3:3 + d]
    b = backend()
    assert b.asarray(view).data_ptr() == view.data_ptr() and view.stride(0) == d + 5      # no copy: ldx = d + 5
    got, dense = b.fit_wide(view), b.fit_wide(b.asarray(x))
    for u, v in zip(got[:3], dense[:3]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
    proj = b.transform_wide(view, got[0], got[1][:4]).cpu().numpy()
    np.testing.assert_array_equal(proj, b.transform_wide(b.asarray(x), got[0], got[1][:4]).cpu().numpy())
    R.check_fit(x, *got[:3], proj, case, "kernel, ldx = d + 5")
    many = b.transform_wide(view, got[0], got[1][:70]).cpu().numpy()                       # k > 16: the 64-component tiles
    want = R.transform(x, got[0], got[1][:70])
    np.testing.assert_array_equal(many[:, :4], proj)
    assert np.abs(many - want).max() <= R.bound(d) * np.abs(want).max()
    out = torch.full((n, 7), -5.0, dtype=torch.float32, device=DEV)                         # ldo > k: the other columns are not written
    m, c = torch.as_tensor(got[0], device=DEV), torch.as_tensor(got[1][:4].copy(), device=DEV)
    hip.check(hip.lib().tmjx_pca_transform_wide(view.data_ptr(), n, d, d + 5, m.data_ptr(), c.data_ptr(), 4, out.data_ptr(), 7, None), "tmjx_pca_transform_wide")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[:, :4].cpu().numpy(), proj)
    assert (out[:, 4:] == -5.0).all()


def test_two_calls_give_the_same_bits():
    x = R.case_data(*CASES[3])
    b = backend()
    xd = b.asarray(x)
    first, second = b.fit_wide(xd), b.fit_wide(xd)
    for u, v in zip(first[:3], second[:3]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
    assert first[3].sweeps == second[3].sweeps
    p1, p2 = (b.transform_wide(xd, first[0], first[1][:4]).cpu().numpy() for _ in range(2))
    np.testing.assert_array_equal(p1.view(np.uint32), p2.view(np.uint32))


def test_narrow_forwarding_and_degenerate_inputs():
    b = backend()
    x = b.asarray(R.case_data(129, 65, 3.0, 0))
    wide, narrow = b.fit_wide(x), b.fit(x)
    for u, v in zip(wide[:3], narrow[:3]):
        np.testing.assert_array_equal(u.view(np.uint32), v.view(np.uint32))
    np.testing.assert_array_equal(b.transform_wide(x, wide[0], wide[1][:4]).cpu().numpy(), b.transform(x, narrow[0], narrow[1][:4]).cpu().numpy())
    d = 130
    row = np.linspace(-3.0, 7.0, d).astype(np.float32)
    const = np.tile(row, (10, 1))
    mean, comp, var, info = b.fit_wide(b.asarray(const))
    np.testing.assert_array_equal(var, 0)
    np.testing.assert_array_equal(comp, np.eye(d, dtype=np.float32))
    np.testing.assert_array_equal(mean, row)
    assert info.converged == 1 and info.sweeps == 0
    assert np.isfinite(b.transform_wide(b.asarray(const), mean, comp).cpu().numpy()).all()
    bad = R.make_data(40, d).copy()
    bad[3, 77] = np.nan
    with pytest.raises(hip.TmjxError, match="non-finite"):
        b.fit_wide(b.asarray(bad))


def test_refusals_launch_nothing():
    L, b = hip.lib(), backend()
    x = b.asarray(R.make_data(8, 130))
    with pytest.raises(hip.TmjxError, match="d = 1025 exceeds the wide PCA limit of 1024"):
        b.fit_wide(torch.zeros((4, 1025), dtype=torch.float32, device=DEV))
    with pytest.raises(hip.TmjxError, match="n >= 2 rows .got 1."):
        b.fit_wide(x[:1])
    with pytest.raises(hip.TmjxError, match="d = 129 exceeds the PCA limit of 128"):      # the narrow entry point keeps its limit
        b.fit(torch.zeros((4, 129), dtype=torch.float32, device=DEV))
    floats = C.c_int64(0)
    hip.check(L.tmjx_pca_wide_workspace(8, 130, C.byref(floats)), "tmjx_pca_wide_workspace")
    info, ws = hip.PcaInfo(), torch.full((int(floats.value),), 3.0, device=DEV)
    outs = [torch.full((130 * 130,), 7.0, device=DEV) for _ in range(3)]
    ptrs = [o.data_ptr() for o in outs]
    assert L.tmjx_pca_fit_wide(x.data_ptr(), 8, 130, 129, *ptrs, ws.data_ptr(), C.byref(info), None) == -22 and b"ldx = 129 is smaller than d = 130" in L.tmjx_last_error()
    assert L.tmjx_pca_fit_wide(x.data_ptr(), 8, 130, 130, ptrs[0], None, ptrs[2], ws.data_ptr(), C.byref(info), None) == -22 and b"null argument" in L.tmjx_last_error()
    assert L.tmjx_pca_fit_wide(x.data_ptr(), 8, 130, 130, *ptrs, ws.data_ptr() + 4, C.byref(info), None) == -22 and b"aligned" in L.tmjx_last_error()
    assert L.tmjx_pca_transform_wide(x.data_ptr(), 8, 130, 130, ptrs[0], ptrs[1], 131, ptrs[2], 131, None) == -22 and b"k = 131 components asked of d = 130" in L.tmjx_last_error()
    assert L.tmjx_pca_transform_wide(x.data_ptr(), 8, 130, 130, ptrs[0], ptrs[1], 4, ptrs[2], 3, None) == -22 and b"ldo = 3 is smaller than k = 4" in L.tmjx_last_error()
    with pytest.raises(ValueError, match="n_components = 131 exceeds the 130 features"):
        P.PCA(131, device=DEV).fit(x)
    torch.cuda.synchronize()
    assert all((o == 7.0).all() for o in outs) and (ws == 3.0).all()      # nothing was written


def test_pca_class_end_to_end():
    n, d = 400, 256
    x = R.make_data(n, d, 3.0, 1)
    xt = torch.from_numpy(x).to(DEV)
    p = P.PCA(4, device=DEV).fit(xt)
    m64, c64, l64 = R.fit(x)
    assert p.components_.shape == (4, d) and p.n_samples_ == n and 1 <= p.n_block_sweeps_ <= 15 and p.n_sweeps_ == p.n_block_sweeps_
    np.testing.assert_allclose(p.explained_variance_, l64[:4], rtol=1e-5)
    np.testing.assert_allclose(p.explained_variance_ratio_, l64[:4] / l64.sum(), rtol=1e-5)
    proj = p.transform(xt)
    assert isinstance(proj, torch.Tensor) and proj.shape == (n, 4)
    gap = R.eigengap(l64, 4)
    assert gap >= 0.05 and R.projection_error(x, proj.cpu().numpy(), 4) <= R.bound(d) / gap
    np.testing.assert_array_equal(p.transform(x), proj.cpu().numpy())                       # numpy in, numpy out
    assert P.PCA(4, device=DEV).fit(xt[:, :60].contiguous()).n_block_sweeps_ == 0


def test_tool_on_a_wide_feature(tmp_path, capsys):
    from track_mjx_amd import h5lite
    rng = np.random.default_rng(3)
    (tmp_path / "in").mkdir()
    feats = []
    for c in range(3):
        lat = R.make_data(8, 6, 0.5, 10 + c)
        feats.append(np.tanh(lat @ rng.standard_normal((6, 160))).astype(np.float32))
        h5lite.write_tree(tmp_path / "in" / f"clip_{c}.h5", {"activations": {"intention": lat, "decoder": {"layer_0": feats[-1]}}})
    out = tmp_path / "pca.h5"
    assert P.main([f"rollouts={tmp_path / 'in'}", f"out={out}", "n_components=3", "feature=decoder/layer_0"]) == 0
    assert "24 samples x 160 features from 3 clips" in capsys.readouterr().out
    pca, proj = P.fit_rollouts(tmp_path / "in", "decoder/layer_0", 3, device=DEV)
    with h5lite.File(out) as h:
        np.testing.assert_array_equal(h["components"][()], pca.components_)
        np.testing.assert_array_equal(h["projections/clip_2"][()], proj[2])
        assert h["projections/clip_0"][()].shape == (8, 3) and h["mean"][()].shape == (160,)
        ratio = h["explained_variance_ratio"][()]
    l64 = R.fit(np.concatenate(feats))[2]
    np.testing.assert_allclose(ratio, l64[:3] / l64.sum(), rtol=1e-4)                       # the float64 reference's ratios
