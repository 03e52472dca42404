"""CPU: the host side of the elastic deformation of the batch filler (mivp_amd.batches: draw_elastic, ElasticDraws), the
C-ABI declaration, and the restatement the GPU tests compare against (tests/elastic_crops_ref.py), pinned to scipy's
B-spline basis and -- through a lattice whose spline is an affine function -- to the existing affine restatement
(tests/spatial_crops_ref.py), which test_spatial_crops_host.py pins to ``grid_sample``."""
import os
import re

import numpy as np
import pytest
from scipy.interpolate import BSpline

from conftest import ROOT

import mivp_amd  # noqa: F401
from mivp_amd import batches as BT

import elastic_cases as EC
import elastic_crops_ref as ER
import spatial_crops_ref as SR


# ---------------------------------------------------------------------------------------------- the basis
def test_basis_is_a_partition_of_unity_and_scipys_cubic_bspline():
    f = np.concatenate([np.linspace(0.0, 1.0, 257), np.random.RandomState(0).uniform(0, 1, 64)])
    B = ER.basis(f)
    assert B.shape == (4, f.size) and (B >= 0).all()
    assert np.abs(B.sum(axis=0) - 1).max() < 1e-15
    N = BSpline.basis_element(np.arange(5.0), extrapolate=False)    # the uniform cubic B-spline on the knots 0..4
    for a in range(4):
        want = np.nan_to_num(N(f + 3 - a))                          # (the open end of the support evaluates to nan)
        assert np.abs(B[a] - want).max() < 1e-15, a
    i, fr = ER.knots(20, 7)
    x = (np.arange(20) + 0.5) * 4 / 20
    assert np.array_equal(i, np.floor(x).astype(int)) and i.max() == 3 and np.allclose(i + fr, x) and (fr >= 0).all() and (fr < 1).all()


# ---------------------------------------------------------------------------------------------- linear precision
DYADIC = [[[0.5, 0.125, 0], [0, 1.25, 0], [0, 0, 1]], [[1, 0, 0.125], [0, -0.5, 0], [0.25, 0, 1.25]]]
DYADIC_SHIFT = [[0.125, -0.375, 0.5], [0.5, 0.25, -0.125]]


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_a_linear_lattice_is_the_composed_affine_map_of_the_existing_restatement(rot):
    """P[c][j] = alpha_c j_c gives d_c = alpha_c (x_c + 1), affine in u.  roi (12, 10, 20) with nodes (6, 8, 8) makes
    (n - 3) / roi = (1/4, 1/2, 1/4); with dyadic alpha and A the composed words are exact in fp32, which
    ``spatial_crops_ref.positions`` demands, and the two restatements must then agree to float64 rounding."""
    images, labels = EC.bank_arrays(2, integer=False)
    lut = BT.label_table(EC.ACTIVE)
    roi, nodes, alpha = EC.ROI, (6, 8, 8), (0.5, -0.25, 0.25)
    affine = np.zeros((2, 12), np.float32)
    affine[:, :9], affine[:, 9:] = np.asarray(DYADIC).reshape(2, 9), DYADIC_SHIFT
    P = ER.linear_lattice(alpha, nodes).astype(np.float32)
    assert np.array_equal(P.astype(np.float64), ER.linear_lattice(alpha, nodes))
    d = ER.displacement(P, roi)
    for c in range(3):                                              # the spline itself: alpha (x + 1), along its own axis only
        x = (np.arange(roi[c]) + 0.5) * (nodes[c] - 3) / roi[c]
        shape = [1, 1, 1]
        shape[c] = roi[c]
        assert np.abs(d[c] - (alpha[c] * (x + 1)).reshape(shape)).max() < 1e-14
    composed = np.stack([ER.composed_affine(a, alpha, nodes, roi) for a in affine])
    assert np.array_equal(composed.astype(np.float32).astype(np.float64), composed)
    volume, origin = [0, 1], [EC.GENERAL_ORIGINS[rot], (1, 2, 3)]
    got = ER.teacher_batch(images, labels, lut, volume, [rot, rot], origin, roi, affine, [1, 1], [P, P])
    want = SR.teacher_batch(images, labels, lut, volume, [rot, rot], origin, roi, composed.astype(np.float32))
    assert np.abs(got[3] - want[3]).max() < 1e-12
    assert np.abs(got[0] - want[0]).max() < 1e-11 and np.abs(got[2] - want[2]).max() < 1e-12
    tie = EC.near_tie(want[3], 1e-9)                                # dyadic positions do land on exact ties
    assert np.array_equal(got[1][:, 0][~tie], want[1][:, 0][~tie]) and tie.mean() < 0.2
    assert (want[1] > 0).any() and (want[0] != 0).any()
    # flag 0: the affine rule itself, the lattice unread
    nan = np.full_like(P, np.nan)
    got0 = ER.teacher_batch(images, labels, lut, volume, [rot, rot], origin, roi, affine, [0, 0], [nan, nan])
    want0 = SR.teacher_batch(images, labels, lut, volume, [rot, rot], origin, roi, affine)
    assert all(np.array_equal(a, b) for a, b in zip(got0, want0))


# ---------------------------------------------------------------------------------------------- the draws
def _expected(seed, B, nodes, p, lo, hi, lb):
    """The documented order a second time."""
    rs = np.random.RandomState(seed)
    flags, lat = np.zeros(B, np.int32), np.zeros((B, 3) + nodes, np.float32)
    for b in range(B):
        if rs.random_sample() < p:
            flags[b] = 1
            m = rs.uniform(lo, hi)
            for c in range(3):
                for j0 in range(nodes[0]):
                    for j1 in range(nodes[1]):
                        for j2 in range(nodes[2]):
                            v = rs.uniform(-m, m)
                            locked = any(j < lb or j >= n - lb for j, n in zip((j0, j1, j2), nodes))
                            lat[b, c, j0, j1, j2] = 0.0 if locked else v
    return flags, lat, rs


@pytest.mark.parametrize("nodes,lb", [((7, 7, 7), 2), ((5, 4, 6), 1), ((4, 4, 4), 0)])
def test_draw_order_determinism_and_locked_borders(nodes, lb):
    B, roi = 6, (96, 96, 96)
    rs = np.random.RandomState(21)
    d = BT.draw_elastic(rs, B, roi, nodes=nodes, p_elastic=0.6, magnitude_range=(0.5, 2.0), locked_borders=lb)
    flags, lat, rs_want = _expected(21, B, nodes, 0.6, 0.5, 2.0, lb)
    assert isinstance(d, BT.ElasticDraws) and d.batch == B and d.flags.dtype == np.int32 and d.lattice.dtype == np.float32
    assert d.lattice.shape == (B, 3) + nodes and 0 < flags.sum() < B
    assert np.array_equal(d.flags, flags) and np.array_equal(d.lattice, lat)
    assert rs.random_sample() == rs_want.random_sample()           # the stream stands where the documented order leaves it
    again = BT.draw_elastic(np.random.RandomState(21), B, roi, nodes=nodes, p_elastic=0.6, magnitude_range=(0.5, 2.0),
                            locked_borders=lb)
    assert np.array_equal(again.flags, d.flags) and np.array_equal(again.lattice, d.lattice)
    other = BT.draw_elastic(np.random.RandomState(22), B, roi, nodes=nodes, p_elastic=0.6, magnitude_range=(0.5, 2.0),
                            locked_borders=lb)
    assert not np.array_equal(other.lattice, d.lattice)
    assert np.abs(d.lattice).max() <= 2.0 and not d.lattice[d.flags == 0].any()
    free = np.zeros(nodes, bool)
    free[lb:nodes[0] - lb, lb:nodes[1] - lb, lb:nodes[2] - lb] = True
    assert free.any() and not d.lattice[:, :, ~free].any() and d.lattice[d.flags == 1][:, :, free].all()


def test_zero_probability_gives_the_identity_and_consumes_only_the_coins():
    rs, ref = np.random.RandomState(4), np.random.RandomState(4)
    d = BT.draw_elastic(rs, 5, (32, 32, 32), magnitude_range=(0., 2.))
    ident = BT.ElasticDraws.identity(5, (7, 7, 7))
    assert np.array_equal(d.flags, ident.flags) and np.array_equal(d.lattice, ident.lattice)
    assert not ident.flags.any() and not ident.lattice.any() and ident.lattice.shape == (5, 3, 7, 7, 7)
    ref.random_sample(5)
    assert rs.random_sample() == ref.random_sample()
    d = BT.draw_elastic(np.random.RandomState(4), 3, (32, 32, 32))  # the defaults: nothing is deformed
    assert not d.flags.any()
    d = BT.draw_elastic(np.random.RandomState(4), 3, (32, 32, 32), p_elastic=1.0)       # a certain coin, magnitude 0
    assert d.flags.all() and not d.lattice.any()


def test_draw_refusals():
    rs = np.random.RandomState(1)
    ok = dict(nodes=(7, 7, 7), p_elastic=0.5, magnitude_range=(0., 2.), locked_borders=2)
    BT.draw_elastic(rs, 2, (96, 96, 96), **ok)
    for bad, match in [(dict(p_elastic=-0.1), "p_elastic"), (dict(p_elastic=1.5), "p_elastic"),
                       (dict(magnitude_range=(-1., 1.)), "magnitude_range"), (dict(magnitude_range=(2., 1.)), "magnitude_range"),
                       (dict(magnitude_range=(0., float("nan"))), "magnitude_range"),
                       (dict(locked_borders=4), "locked_borders"), (dict(locked_borders=-1), "locked_borders"),
                       (dict(nodes=(7, 4, 7)), "locked_borders"),      # 2 * 2 >= 4: no free node on axis 1
                       (dict(nodes=(3, 7, 7)), "nodes"), (dict(nodes=(7, 9, 7)), "nodes"), (dict(nodes=(7, 7)), "nodes"),
                       (dict(nodes=(7.0, 7, 7)), "nodes")]:
        with pytest.raises(ValueError, match=match):
            BT.draw_elastic(rs, 2, (96, 96, 96), **{**ok, **bad})
    # half a node spacing: roi 96 with 7 nodes is 12 voxels, roi 20 is 2.5
    BT.draw_elastic(rs, 2, (96, 96, 96), **{**ok, "magnitude_range": (0., 11.9)})
    with pytest.raises(ValueError, match="axis 0 .* fold"):
        BT.draw_elastic(rs, 2, (96, 96, 96), **{**ok, "magnitude_range": (0., 12.0)})
    with pytest.raises(ValueError, match="axis 2 .* fold"):
        BT.draw_elastic(rs, 2, (96, 96, 20), **{**ok, "magnitude_range": (0., 2.5)})
    BT.draw_elastic(rs, 2, (96, 96, 20), **{**ok, "magnitude_range": (0., 2.4)})
    with pytest.raises(ValueError):
        BT.draw_elastic(rs, 0, (96, 96, 96), **ok)


def test_check_refusals_name_the_sample():
    nodes = (5, 4, 6)
    good = BT.draw_elastic(np.random.RandomState(2), 3, (40, 40, 40), nodes=nodes, p_elastic=1., magnitude_range=(1., 2.),
                           locked_borders=1)
    assert good.check(3, nodes) is good
    with pytest.raises(ValueError, match=r"int32 \[4\]"):
        good.check(4, nodes)
    with pytest.raises(ValueError, match=r"float32 \[3, 3, 5, 4, 7\]"):
        good.check(3, (5, 4, 7))
    with pytest.raises(ValueError, match="nodes"):
        good.check(3, (5, 4, 9))
    with pytest.raises(ValueError, match="int32"):
        BT.ElasticDraws(good.flags.astype(np.int64), good.lattice).check(3, nodes)
    with pytest.raises(ValueError, match="int32"):
        BT.ElasticDraws(good.flags.tolist(), good.lattice).check(3, nodes)
    with pytest.raises(ValueError, match="float32"):
        BT.ElasticDraws(good.flags, good.lattice.astype(np.float64)).check(3, nodes)
    with pytest.raises(ValueError, match="float32"):
        BT.ElasticDraws(good.flags, good.lattice.reshape(3, 3, -1)).check(3, nodes)
    for b, value in [(1, np.nan), (2, np.inf), (0, -np.inf)]:
        p = good.lattice.copy()
        p[b, 2, 1, 1, 1] = value
        with pytest.raises(ValueError, match=f"sample {b}: a non-finite"):
            BT.ElasticDraws(good.flags, p).check(3, nodes)
    for b, value in [(0, 2), (2, -1)]:
        f = good.flags.copy()
        f[b] = value
        with pytest.raises(ValueError, match=f"sample {b}: flag {value}"):
            BT.ElasticDraws(f, good.lattice).check(3, nodes)
    big = good.lattice.copy()
    big[:] = 1e4                                                    # finite: allowed (the crop leaves the volume, zeros)
    BT.ElasticDraws(good.flags, big).check(3, nodes)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_elastic_entry_at_abi_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    assert re.search(r"^int\s+mivp_crop_fill_elastic\s*\(", text, flags=re.M)
    P = _lib.parse_header()
    assert len(P["mivp_crop_fill_elastic"][1]) == 16 == len(P["mivp_crop_fill_affine"][1]) + 3
    assert P["mivp_crop_fill_elastic"][1][:12] == P["mivp_crop_fill_affine"][1][:12]      # the affine entry's, then the three
    assert len(P["mivp_crop_fill_affine"][1]) == 13 and len(P["mivp_crop_fill_affine_debug"][1]) == 15      # kept
    assert _lib.ABI_VERSION == 18 and BT.ELASTIC_NODES == (4, 8)
    src = open(os.path.join(ROOT, "medical-image-segmentation-with-visual-prompts_amd", "csrc", "crops_affine.hip")).read()
    assert re.search(r"MAXN = 8;", src)


def test_library_exports_the_elastic_entry_at_abi_18():
    from mivp_amd import _lib
    lib = _lib.lib()
    assert lib.mivp_abi_version() == 18
    assert hasattr(lib, "mivp_crop_fill_elastic")


def test_device_classes_refuse_the_cpu_and_elastic_needs_spatial():
    with pytest.raises(ValueError, match="GPU"):
        BT.ElasticSlot(2, (7, 7, 7), "cpu")
    with pytest.raises(ValueError, match="nodes"):
        BT.ElasticSlot(2, (7, 7, 9), "cpu")


# ---------------------------------------------------------------------------------------------- the GPU test's inputs
def test_few_label_voxels_of_the_general_case_sit_near_a_rounding_tie():
    """On the exact inputs of the GPU tolerance test (test_hip_elastic_crops.py, the general case) the share of label
    voxels whose r + 0.5 lies within delta_r of an integer is far below the 1 % that test may leave out: its cap is a
    condition the reference meets by itself."""
    affine = EC.general_affine()
    assert np.abs(affine[0, :9].astype(np.float64) - BT.affine_matrix((False,) * 3, (0.3, -0.2, 0.5), (1.1, 0.9, 1.05))
                  .reshape(-1)).max() <= 2.0 ** -24 * 1.25
    delta_d, delta_r = EC.bounds(affine, EC.MAX_P)
    assert delta_d == 160 * 2.0 ** -24 * 2.0 and 1.7e-5 < delta_r < 1e-3
    shares = []
    for nodes in EC.GENERAL_NODES:
        for code, origin in EC.GENERAL_ORIGINS.items():
            lat = EC.general_lattice(nodes, code)
            assert lat.dtype == np.float32 and np.abs(lat).max() <= EC.MAX_P and (lat * 1024 != np.round(lat * 1024)).all()
            n_rot = BT.rotated_shape(EC.SHAPES[0], code)
            r = np.stack([ER.positions(affine[b], EC.ROI, origin, n_rot, 1, lat[b]) for b in range(2)])
            r0 = np.stack([ER.positions(affine[b], EC.ROI, origin, n_rot, 0, lat[b]) for b in range(2)])
            assert 0.2 < np.abs(r - r0).max() < 2.0 * np.abs(affine[:, :9]).reshape(2, 3, 3).sum(axis=2).max()
            shares.append(float(EC.near_tie(r, delta_r).mean()))
    print("share of label voxels near a tie per case:", shares, "delta_r", delta_r)
    assert max(shares) <= 0.01
