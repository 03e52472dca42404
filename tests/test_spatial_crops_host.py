"""CPU: the host side of the random flip / rotation / zoom of the batch filler (mivp_amd.batches: draw_spatial,
SpatialDraws), the C-ABI declarations, and the restatement the GPU tests compare against (tests/spatial_crops_ref.py)
pinned to ``torch.nn.functional.grid_sample`` -- code nobody here wrote."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

import mivp_amd  # noqa: F401
from mivp_amd import batches as BT

import spatial_crops_ref as SR


# ---------------------------------------------------------------------------------------------- the draw order
def _matrix(flips, angles, zoom):
    """A = F R2 R1 R0 diag(1 / zoom), written out a second time entry by entry (no matrix products of numpy)."""
    def mul(X, Y):
        return [[sum(X[i][k] * Y[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    import math
    c, s = [math.cos(a) for a in angles], [math.sin(a) for a in angles]
    R0 = [[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]]
    R1 = [[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]]
    R2 = [[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]]
    Fm = [[(-1.0 if flips[i] else 1.0) if i == j else 0.0 for j in range(3)] for i in range(3)]
    Z = [[1.0 / zoom[i] if i == j else 0.0 for j in range(3)] for i in range(3)]
    return np.array(mul(mul(mul(mul(Fm, R2), R1), R0), Z), dtype=np.float64)


def _expected(seed, B, p_flip, p_affine, rot, scale, isotropic, shift):
    """The documented order a second time; returns the words and the number of draws consumed."""
    rs = np.random.RandomState(seed)
    out, used = np.zeros((B, 12), np.float32), 0
    for b in range(B):
        flips = [rs.random_sample() < p_flip[k] for k in range(3)]
        used += 4
        angles, zoom = [0.0] * 3, [1.0] * 3
        if rs.random_sample() < p_affine:
            angles = [rs.uniform(-rot[k], rot[k]) for k in range(3)]
            zoom = [rs.uniform(*scale)] * 3 if isotropic else [rs.uniform(*scale) for _ in range(3)]
            used += 4 if isotropic else 6
        out[b, :9] = _matrix(flips, angles, zoom).reshape(-1).astype(np.float32)
        if shift:
            out[b, 9:] = [rs.uniform(-0.5, 0.5) for _ in range(3)]
            used += 3
    return out, used, rs


@pytest.mark.parametrize("isotropic,shift", [(True, False), (False, True), (True, True)])
def test_draw_order_and_determinism(isotropic, shift):
    kw = dict(p_flip=(0.5, 0.3, 0.7), p_affine=0.6, rotate_range=(0.26, 0.1, 0.4), scale_range=(0.8, 1.25),
              isotropic=isotropic, shift=shift)
    B = 9
    rs = np.random.RandomState(11)
    d = BT.draw_spatial(rs, B, **kw)
    want, used, rs_want = _expected(11, B, kw["p_flip"], kw["p_affine"], kw["rotate_range"], kw["scale_range"], isotropic, shift)
    assert isinstance(d, BT.SpatialDraws) and d.affine.dtype == np.float32 and d.affine.shape == (B, 12) and d.batch == B
    # A against the independent float64 composition: the two may associate differently, so to one fp32 step of an
    # entry of magnitude <= 1.25 / 0.8; the shifts are single draws and equal bit for bit
    assert np.abs(d.affine[:, :9] - want[:, :9]).max() <= 2.0 ** -23 and np.array_equal(d.affine[:, 9:], want[:, 9:])
    assert rs.random_sample() == rs_want.random_sample()           # and the stream stands where the documented order leaves it
    again = BT.draw_spatial(np.random.RandomState(11), B, **kw)
    assert np.array_equal(again.affine, d.affine)
    assert not np.array_equal(BT.draw_spatial(np.random.RandomState(12), B, **kw).affine, d.affine)
    # every A is a rotation times a zoom up to the signs: |det| = 1 / prod(zoom), within the drawn range
    det = np.abs(np.linalg.det(d.affine[:, :9].astype(np.float64).reshape(B, 3, 3)))
    assert ((det >= 1 / 1.25 ** 3 - 1e-6) & (det <= 1 / 0.8 ** 3 + 1e-6)).all()
    assert (np.abs(d.affine[:, 9:]) <= 0.5).all() and (shift or not d.affine[:, 9:].any())
    assert 0 < used < 13 * B


def test_zero_probabilities_give_the_identity_and_consume_only_their_draws():
    rs = np.random.RandomState(4)
    d = BT.draw_spatial(rs, 5)
    assert np.array_equal(d.affine, BT.SpatialDraws.identity(5).affine)
    assert np.array_equal(d.affine[0], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32))
    ref = np.random.RandomState(4)
    ref.random_sample(4 * 5)                                        # three flip draws and one apply draw per sample
    assert rs.random_sample() == ref.random_sample()
    rs, ref = np.random.RandomState(4), np.random.RandomState(4)
    d = BT.draw_spatial(rs, 5, rotate_range=(1., 1., 1.), scale_range=(0.5, 2.0), shift=True)      # p_affine = 0
    assert np.array_equal(d.affine[:, :9], BT.SpatialDraws.identity(5).affine[:, :9]) and d.affine[:, 9:].all()
    ref.random_sample(7 * 5)
    assert rs.random_sample() == ref.random_sample()
    # a certain flip, no affine: the signed identity
    d = BT.draw_spatial(np.random.RandomState(1), 2, p_flip=(1., 0., 1.))
    assert np.array_equal(d.affine[:, :9].reshape(2, 3, 3), np.stack([np.diag([-1., 1., -1.])] * 2).astype(np.float32))
    # zoom > 1 enlarges: the source offset per output voxel shrinks
    d = BT.draw_spatial(np.random.RandomState(1), 1, p_affine=1., scale_range=(2., 2.))
    assert np.array_equal(d.affine[0, :9].reshape(3, 3), np.diag([.5, .5, .5]).astype(np.float32))
    for bad in (dict(p_flip=(0., 2., 0.)), dict(p_affine=-0.1), dict(scale_range=(0., 1.)), dict(scale_range=(2., 1.)),
                dict(rotate_range=(0., float("nan"), 0.))):
        with pytest.raises(ValueError, match="draw_spatial"):
            BT.draw_spatial(np.random.RandomState(1), 2, **bad)


def test_check_refusals_name_the_sample():
    good = BT.draw_spatial(np.random.RandomState(2), 3, p_affine=1., rotate_range=(0.3, 0.3, 0.3), shift=True)
    assert good.check(3) is good
    with pytest.raises(ValueError, match=r"float32 \[4, 12\]"):
        good.check(4)
    with pytest.raises(ValueError, match="float32"):
        BT.SpatialDraws(good.affine.astype(np.float64)).check(3)
    with pytest.raises(ValueError, match="float32"):
        BT.SpatialDraws(good.affine.reshape(3, 3, 4)).check(3)
    with pytest.raises(ValueError, match="float32"):
        BT.SpatialDraws(good.affine.tolist()).check(3)
    for b, word, value, match in [(1, 4, np.nan, "sample 1: a non-finite"), (2, 11, np.inf, "sample 2: a non-finite"),
                                  (0, 8, 16.5, "sample 0: an entry of A"), (2, 0, -17.0, "sample 2: an entry of A"),
                                  (1, 9, 1.25, "sample 1: a shift"), (0, 11, -1.5, "sample 0: a shift")]:
        a = good.affine.copy()
        a[b, word] = value
        with pytest.raises(ValueError, match=match):
            BT.SpatialDraws(a).check(3)
    a = good.affine.copy()
    a[0, 0], a[0, 9] = 16.0, -1.0                                   # the bounds themselves are allowed
    BT.SpatialDraws(a).check(3)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_affine_entry_at_abi_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    for name in ("mivp_crop_fill_affine", "mivp_crop_fill_affine_debug"):
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    P = _lib.parse_header()
    assert len(P["mivp_crop_fill_affine"][1]) == 13 and len(P["mivp_crop_fill_affine_debug"][1]) == 15
    assert len(P["mivp_crop_fill"][1]) == 12 and len(P["mivp_crop_tensor"][1]) == 9 and len(P["mivp_crop_pick"][1]) == 11
    assert _lib.ABI_VERSION == 18
    assert BT.AFFINE_WORDS == 12 and BT.SPATIAL_BRICK == (8, 8, 16) and BT.SPATIAL_BOX_CELLS == 12288
    src = open(os.path.join(ROOT, "medical-image-segmentation-with-visual-prompts_amd", "csrc", "crops_affine.hip")).read()
    assert re.search(r"BH = 8, BW = 8, BD = 16;", src) and re.search(r"BOXV = 12288;", src)


def test_device_classes_refuse_the_cpu():
    with pytest.raises(ValueError, match="GPU"):
        BT.SpatialSlot(2, "cpu")
    with pytest.raises(ValueError):
        BT.BatchFiller(object(), (8, 8, 8), 2, spatial=True)


# ---------------------------------------------------------------------------------------------- the restatement itself
SHAPE, ROI, ORIGIN = (20, 18, 36), (12, 10, 20), (4, 3, 7)


def _volume(channels=2):
    g = torch.Generator().manual_seed(7)
    image = torch.rand((channels,) + SHAPE, generator=g, dtype=torch.float64).numpy() * 3.0 - 1.0
    labels = torch.randint(0, 6, SHAPE, generator=g, dtype=torch.uint8).numpy()
    return image, labels


def _cases():
    general = BT.affine_matrix((False, True, False), (0.3, -0.2, 0.5), (1.1, 0.9, 1.05))
    out = [np.concatenate([general.reshape(-1), [0.25, -0.4, 0.1]]).astype(np.float32),
           np.concatenate([(2.5 * np.eye(3)).reshape(-1), [0, 0, 0]]).astype(np.float32),          # leaves the volume
           BT.SpatialDraws.identity(1).affine[0]]
    return out


def _grid(r, m):
    """grid_sample's normalised grid ([1, h, w, d, 3], x = the LAST volume axis) from positions r, align_corners=True."""
    g = [2.0 * r[k] / (m[k] - 1) - 1.0 for k in (2, 1, 0)]
    return torch.from_numpy(np.stack(g, axis=-1))[None]


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_restatement_equals_grid_sample(rot):
    image, labels = _volume()
    lut = BT.label_table([1, 3, 4])
    outside = 0
    for affine in _cases():
        img, mask, coord, r = SR.teacher_crop(image, labels, lut, rot, ORIGIN, ROI, affine)
        vol = torch.from_numpy(np.ascontiguousarray(SR.rotate(image, rot)))[None]
        m = vol.shape[2:]
        assert img.shape == (2,) + ROI and mask.shape == (1,) + ROI and coord.shape == (3,) + ROI and r.shape == (3,) + ROI
        want = F.grid_sample(vol, _grid(r, m), mode="bilinear", padding_mode="zeros", align_corners=True)[0].numpy()
        span = image.max() - image.min()
        assert np.abs(img - want).max() <= 1e-5 * span
        mapped = torch.from_numpy(np.ascontiguousarray(SR.rotate(lut[labels].astype(np.float64), rot)))[None, None]
        want = F.grid_sample(mapped, _grid(r, m), mode="nearest", padding_mode="zeros", align_corners=True)[0].numpy()
        frac = r - np.floor(r)
        tie = (np.abs(frac - 0.5) < 1e-9).any(axis=0)               # torch rounds half to even, the rule half up
        assert np.array_equal(mask[:, ~tie], want[:, ~tie])
        if np.array_equal(affine, BT.SpatialDraws.identity(1).affine[0]):
            assert not tie.any() and np.array_equal(r, np.round(r))
        # the coordinates: those of the stored volume's grid, gathered like the image (linear functions interpolate exactly)
        axes = [np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in SHAPE]
        stored = np.stack(np.meshgrid(*axes, indexing="ij"))
        _, ok = SR.nearest_inside(r, m)
        deep = ok & (r >= 0).all(axis=0) & np.all([r[k] <= m[k] - 1 for k in range(3)], axis=0)   # no zero corner involved
        lin = SR.trilinear(SR.rotate(stored, rot), r)
        assert np.abs(coord - lin)[:, deep].max() < 1e-9 and not coord[:, ~ok].any()
        outside += int((~ok).sum())
    assert outside > 0                                              # the zero rule was exercised


def test_restatement_non_finite_positions_read_zero():
    image, labels = _volume(1)
    affine = BT.SpatialDraws.identity(1).affine[0].copy()
    affine[4] = np.inf
    img, mask, coord, r = SR.teacher_crop(image, labels, BT.label_table(None), 0, ORIGIN, ROI, affine)
    assert np.isfinite(r[0]).all() and np.isfinite(r[2]).all() and not np.isfinite(r[1]).any()     # one axis is enough
    assert not img.any() and not mask.any() and not coord.any()
