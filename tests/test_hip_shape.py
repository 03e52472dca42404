"""GPU tests of the shape descriptors (mivp_amd.regions.region_shape, csrc/region_shape.hip) against the restatement
tests/shape_ref.py: moment2, faces, cells and euler bit for bit on the label map that region_stats wrote; the covariance
within 2 ulp of the float64 value formed from the exact integer numerator; eigenvalues, residuals and orthonormality
within 1e-12 * lambda_0; repeatability and graph capture.  The kernel's brick is 8 x 8 x 64 voxels with 32 LDS slots."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_FIELDS = ("moment2", "faces", "cells", "euler")
ALL_FIELDS = INT_FIELDS + ("covariance_mm2", "eigenvalues", "axes", "major_axis_length", "minor_axis_length",
                           "least_axis_length", "elongation", "flatness", "surface_area_mm2", "surface_to_volume",
                           "sphericity")
SPACING = (0.7, 0.7, 2.5)
_observed = {"eig": 0.0, "res": 0.0, "orth": 0.0}          # largest errors relative to lambda_0, printed by the axes test


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _blobs(shape, seed, density=0.35):
    """smoothed noise above a quantile: blobs of every size that cross brick faces, edges and corners"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal(shape)
    for axis in range(3):                                   # a 3-tap box filter per axis, twice (no scipy needed)
        for _ in range(2):
            p = np.pad(f, [(1, 1) if a == axis else (0, 0) for a in range(3)], mode="edge")
            f = sum(np.take(p, range(k, k + shape[axis]), axis=axis) for k in range(3))
    return (f > np.quantile(f, 1 - density)).astype(np.uint8)


def _run(x, conn=26, spacing=(1.0, 1.0, 1.0), max_regions=4096):
    """(RegionTable, RegionShape, restatement on the table's own label map)"""
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import region_shape, region_stats
    tab = region_stats(_gpu(x), 2, spacing=spacing, connectivity=conn, max_regions=max_regions)
    shp = region_shape(tab)
    want = S.shape_stats(tab.labels.cpu().numpy(), int(tab.n), spacing, capacity=max_regions)
    return tab, shp, want


def _same_integers(got, want):
    assert got["n"] == want["n"]
    for k in INT_FIELDS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _check_axes(got, want, tab_host):
    """covariance within 2 ulp of the value formed from the exact numerator (one conversion and one division, each correctly
    rounded; exact zeros stay exact); eigenvalues against eigvalsh, residuals and orthonormality within 1e-12 * lambda_0"""
    cov, lam, ax = got["covariance_mm2"], got["eigenvalues"], got["axes"]
    assert cov.dtype == lam.dtype == ax.dtype == np.float64
    assert np.all(S.ulp_distance(cov, want["covariance_mm2"]) <= 2)
    assert np.array_equal(cov == 0.0, want["covariance_mm2"] == 0.0)
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1)))
    for r in range(want["n"]):
        a, l0 = cov[r], lam[r, 0]
        assert np.all(np.diff(lam[r]) <= 0) and np.all(lam[r] >= 0)
        ref = np.linalg.eigvalsh(a)[::-1]
        e_eig = np.abs(lam[r] - np.maximum(ref, 0.0)).max()
        e_res = np.abs(a @ ax[r].T - ax[r].T * lam[r][None, :]).max()
        e_orth = np.abs(ax[r] @ ax[r].T - np.eye(3)).max()
        assert e_eig <= 1e-12 * l0 and e_res <= 1e-12 * l0 and e_orth <= 1e-12 * l0, (r, e_eig, e_res, e_orth, l0)
        if l0 > 0:
            for k, e in (("eig", e_eig), ("res", e_res), ("orth", e_orth)):
                _observed[k] = max(_observed[k], e / l0)
        for i in range(3):                                  # the sign rule: the first largest-magnitude component is positive
            assert ax[r, i, int(np.argmax(np.abs(ax[r, i])))] > 0
    print("shape axes, largest errors / lambda_0 so far (eigenvalues, residual, orthonormality):", _observed)
    size = tab_host["size"].astype(np.float64)
    sp = tab_host["_spacing"]
    area = got["faces"][:, 0] * (sp[1] * sp[2]) + got["faces"][:, 1] * (sp[0] * sp[2]) + got["faces"][:, 2] * (sp[0] * sp[1])
    vol = size * (sp[0] * sp[1] * sp[2])
    np.testing.assert_allclose(got["surface_area_mm2"], area, rtol=1e-14)
    np.testing.assert_allclose(got["surface_to_volume"], area / vol, rtol=1e-14)
    np.testing.assert_allclose(got["sphericity"], np.cbrt(36 * np.pi * vol * vol) / area, rtol=1e-14)
    for k, i in (("major_axis_length", 0), ("minor_axis_length", 1), ("least_axis_length", 2)):
        np.testing.assert_allclose(got[k], 4 * np.sqrt(lam[:, i]), rtol=1e-15)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_allclose(got["elongation"], np.where(lam[:, 0] > 0, np.sqrt(lam[:, 1] / lam[:, 0]), np.nan),
                                   rtol=1e-15, equal_nan=True)
        np.testing.assert_allclose(got["flatness"], np.where(lam[:, 0] > 0, np.sqrt(lam[:, 2] / lam[:, 0]), np.nan),
                                   rtol=1e-15, equal_nan=True)


def _host_table(tab, spacing):
    t = tab.cpu()
    t["_spacing"] = spacing
    return t


# ------------------------------------------------------------------------------------------- 1. random blobs
@pytest.mark.parametrize("shape", [(19, 21, 37), (11, 13, 75)])
@pytest.mark.parametrize("conn", [6, 26])
def test_random_blobs_equal_reference(conn, shape):
    """No dimension is a multiple of the brick; regions cross brick faces, edges and corners and touch every border of the
    volume.  19 x 21 x 37 has several bricks along h and w and the four waves' segments along d; 11 x 13 x 75 also has two
    bricks along d.  Also the axes of these regions, under anisotropic spacing."""
    x = _blobs(shape, 3)
    tab, shp, want = _run(x, conn, SPACING)
    lab = tab.labels.cpu().numpy()
    assert want["n"] > 3 and x[0].any() and x[-1].any() and x[:, 0].any() and x[:, -1].any() and x[:, :, 0].any() \
        and x[:, :, -1].any()
    big = np.nonzero(lab == np.bincount(lab.ravel())[1:].argmax() + 1)
    assert np.ptp(big[0] // 8) >= 1 and np.ptp(big[1] // 8) >= 1 and np.ptp(big[2] // 16) >= 1     # across bricks and waves
    assert shape[2] < 64 or np.ptp(big[2] // 64) == 1
    got = shp.cpu()
    _same_integers(got, want)
    assert np.array_equal(tab.cpu()["size"], want["size"]) and np.array_equal(tab.cpu()["coord_sum"], want["coord_sum"])
    _check_axes(got, want, _host_table(tab, SPACING))


# ------------------------------------------------------------------------------------------- 2. more regions than slots
def test_checkerboard_surplus_and_capacity():
    """12 x 12 x 40 at 6-connectivity: every other voxel is its own region, 1280 per brick against 32 LDS slots."""
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import region_shape, region_stats
    shape = (12, 12, 40)
    h, w, d = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    x = ((h + w + d) % 2).astype(np.uint8)
    n = int(x.sum())
    tab, shp, want = _run(x, 6, max_regions=4096)
    got = shp.cpu()
    assert got["n"] == n == 2880
    _same_integers(got, want)
    assert np.array_equal(got["faces"], np.full((n, 3), 2)) and np.array_equal(got["cells"], np.tile([8, 12], (n, 1)))
    assert np.array_equal(got["euler"], np.ones(n, dtype=np.int64))
    assert not got["covariance_mm2"].any() and not got["eigenvalues"].any()            # single voxels: exactly zero
    assert np.isnan(got["elongation"]).all() and np.isnan(got["flatness"]).all()
    small_tab = region_stats(_gpu(x), 2, connectivity=6, max_regions=50)
    small = region_shape(small_tab)
    with pytest.raises(RuntimeError, match=r"2880 components, capacity 50"):
        small.cpu()
    for k in ("moment2", "faces", "cells", "euler"):                                  # labels above 50 are skipped
        assert np.array_equal(getattr(small, k).cpu().numpy(), want[k][:50]), k
    assert small.moment2.shape == (50, 6) and small.axes.shape == (50, 3, 3)


# ------------------------------------------------------------------------------------------- 3. full and empty volumes
def test_one_region_filling_the_volume_and_an_empty_one():
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import region_shape, region_stats
    H, W, D = 16, 16, 64
    tab, shp, want = _run(np.ones((H, W, D), dtype=np.uint8), 26)
    got = shp.cpu()
    _same_integers(got, want)
    assert got["faces"].tolist() == [[2 * W * D, 2 * H * D, 2 * H * W]] and got["euler"].tolist() == [1]
    assert got["cells"].tolist() == [[(H + 1) * (W + 1) * (D + 1),
                                      H * (W + 1) * (D + 1) + (H + 1) * W * (D + 1) + (H + 1) * (W + 1) * D]]
    _check_axes(got, want, _host_table(tab, (1.0, 1.0, 1.0)))
    np.testing.assert_allclose(got["eigenvalues"][0], [(D * D - 1) / 12, (H * H - 1) / 12, (W * W - 1) / 12], rtol=1e-14)
    empty = region_shape(region_stats(torch.zeros((H, W, D), dtype=torch.uint8, device=DEV), 2, max_regions=64))
    for k in ("moment2", "faces", "cells", "covariance_mm2", "eigenvalues", "axes", "euler"):
        t = getattr(empty, k)
        assert t.shape[0] == 64 and not t.cpu().numpy().any(), k
    assert empty.cpu()["n"] == 0


# ------------------------------------------------------------------------------------------- 4. topology at a brick corner
@pytest.mark.parametrize("make,chi", [(S.square_ring, 0), (S.hollow_cube, 2), (S.vertex_pair, 1)])
def test_topology_across_a_brick_corner(make, chi):
    x = S.place(make(), (19, 21, 75), (8, 8, 64)).astype(np.uint8)
    tab, shp, want = _run(x, 26)
    got = shp.cpu()
    assert got["n"] == 1
    _same_integers(got, want)
    assert got["euler"].tolist() == [chi] == want["euler"].tolist()
    idx = np.nonzero(x)
    assert all(i.min() < c <= i.max() for i, c in zip(idx[1:], (8, 64)))               # it does straddle the corner


# ------------------------------------------------------------------------------------------- 5. the largest coordinate
def test_moments_at_the_largest_coordinate():
    D = 65535
    x = np.zeros((2, 2, D), dtype=np.uint8)
    x[0, 0, 0:3] = 1
    x[1, :, D - 5:D] = 1
    tab, shp, want = _run(x, 6)
    got = shp.cpu()
    assert got["n"] == 2
    _same_integers(got, want)
    ds = range(D - 5, D)
    assert got["moment2"][1].tolist() == [10, 5, 2 * sum(d * d for d in ds), 5, 2 * sum(ds), sum(ds)]
    assert got["moment2"][1, 2] > 2 ** 35 and got["euler"].tolist() == [1, 1]
    _check_axes(got, want, _host_table(tab, (1.0, 1.0, 1.0)))


# ------------------------------------------------------------------------------------------- 6. axes on boxes
@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), SPACING])
def test_axes_of_boxes(spacing):
    """the boxes of the CPU test in one volume (another class would not separate them: they are kept apart); a cube has a
    triple eigenvalue and the 5 x 1 x 1 bar a double zero: those eigenvectors are tested by residual and orthonormality"""
    boxes = [((2, 3, 4), (1, 1, 1)), ((5, 1, 1), (5, 2, 10)), ((1, 4, 6), (11, 10, 30)), ((3, 3, 3), (12, 14, 60)),
             ((1, 1, 1), (17, 19, 70))]
    x = np.zeros((19, 21, 75), dtype=np.uint8)
    for (a, b, c), (h, w, d) in boxes:
        x[h:h + a, w:w + b, d:d + c] = 1
    tab, shp, want = _run(x, 26, spacing)
    got = shp.cpu()
    assert got["n"] == len(boxes)
    _same_integers(got, want)
    _check_axes(got, want, _host_table(tab, spacing))
    for r, ((a, b, c), _) in enumerate(boxes):              # raster order of first voxels = the order above
        var = sorted(((k * k - 1) / 12 * s * s for k, s in zip((a, b, c), spacing)), reverse=True)
        np.testing.assert_allclose(got["eigenvalues"][r], var, rtol=1e-14, atol=0)
        cov = got["covariance_mm2"][r]
        assert not (cov - np.diag(np.diag(cov))).any()      # no cross terms: exact zeros
        for k, flat in enumerate((a, b, c)):
            if flat == 1:
                assert not cov[k].any() and not cov[:, k].any()
    assert not got["covariance_mm2"][4].any() and not got["eigenvalues"][4].any()
    assert np.array_equal(got["axes"][4], np.eye(3))
    bar = got["axes"][1]                                    # the 5 x 1 x 1 bar: its major axis is h
    assert np.array_equal(bar[0], [1.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------- 7. reproducible, recordable
def test_repeatable_and_recordable_in_a_graph(monkeypatch):
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib as L
    from mivp_amd.regions import region_shape, region_stats
    shape = (19, 21, 37)
    maps = [_blobs(shape, 11), _blobs(shape, 12, 0.2)]

    def eager(x):
        return region_shape(region_stats(_gpu(x), 2, spacing=SPACING, max_regions=256)).cpu()

    a, b = eager(maps[0]), eager(maps[0])
    for k in ALL_FIELDS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    buf = _gpu(maps[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        region_shape(region_stats(buf, 2, spacing=SPACING, max_regions=256))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    streams = []
    plain = L.call
    monkeypatch.setattr(L, "call", lambda name, *args: (streams.append((name, args[-1])), plain(name, *args))[1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        capture = L.stream()
        tab = region_stats(buf, 2, spacing=SPACING, max_regions=256)
        shp = region_shape(tab)
    monkeypatch.undo()
    # a serial chain, no parallel branches: every entry point of the recording got the one capture stream
    assert [n for n, _ in streams] == ["mivp_region_stats", "mivp_region_shape", "mivp_region_axes"]
    assert {s for _, s in streams} == {capture}
    for x in (maps[1], maps[0]):
        buf.copy_(_gpu(x))
        g.replay()
        torch.cuda.synchronize()
        got, want = shp.cpu(), eager(x)
        assert got["n"] == want["n"] > 1
        for k in ALL_FIELDS:
            assert got[k].tobytes() == want[k].tobytes(), k
