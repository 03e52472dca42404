"""CPU tests of mivp_amd.scan: the geometry from hand-made affines, the orientation round trip over all 48 axis
permutation x flip combinations, the per-axis resize tables against torch's CPU interpolate, and the argument checks of
the four functions and of SlidingWindowPredictor.predict_scan (which run before anything touches the device)."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scan_ref

SIZE_PAIRS = [(50, 64), (97, 40), (23, 32), (512, 333), (96, 96), (7, 20)]
COMBOS = [(p, f) for p in itertools.permutations(range(3)) for f in itertools.product((False, True), repeat=3)]


def _rot(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    r = np.eye(4)
    i, j = [a for a in range(3) if a != axis]
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def _gather(src, geom, kind):
    """Apply a section-0 table of the geometry in numpy: out[k0, k1, k2] = src at the tabled indices."""
    src_dims, out_dims, axes, _, tab = geom.tables(kind)
    assert tuple(src.shape) == src_dims
    idx, off = [], 0
    for n in out_dims:
        idx.append(tab[off:off + n])
        off += n
    return src.transpose(axes)[np.ix_(*idx)]


AFFINES = {
    "identity": (np.eye(4), (0, 1, 2), (False, False, False), (1.0, 1.0, 1.0)),
    "lps": (np.diag([-1.0, -1.0, 1.0, 1.0]), (0, 1, 2), (True, True, False), (1.0, 1.0, 1.0)),
    # native axis 0 runs along world z (2.5 mm), axis 1 along x, axis 2 along y (0.7 mm each)
    "swap": (scan_ref.affine_for((1, 2, 0), (False, False, False), zooms=(2.5, 0.7, 0.7)), (1, 2, 0),
             (False, False, False), (0.7, 0.7, 2.5)),
}


@pytest.mark.parametrize("name", sorted(AFFINES))
@pytest.mark.parametrize("oblique", [None, 0, 1, 2])
def test_from_affine_known_answers(name, oblique):
    from mivp_amd.scan import ScanGeometry
    aff, perm, flip, spacing = AFFINES[name]
    if oblique is not None:
        aff = _rot(oblique, 10.0) @ aff
    aff = aff.copy()
    aff[:3, 3] = (12.5, -40.0, 7.0)
    g = ScanGeometry.from_affine((5, 6, 7), aff)
    assert g.perm == perm and g.flip == flip
    assert g.oriented_shape == tuple((5, 6, 7)[p] for p in perm)
    assert np.allclose(g.spacing, spacing, rtol=0, atol=1e-12)
    assert g.size == g.oriented_shape and not g.resized
    g2 = ScanGeometry.from_affine((5, 6, 7), aff, out_size=(8, 9, 10))
    assert g2.size == (8, 9, 10) and g2.resized
    assert np.allclose(g2.model_spacing, [s * n / m for s, n, m in zip(spacing, g2.oriented_shape, (8, 9, 10))])


def test_from_affine_other_axcodes_and_identity():
    from mivp_amd.scan import ScanGeometry
    g = ScanGeometry.from_affine((5, 6, 7), np.eye(4), axcodes="LPS")
    assert g.perm == (0, 1, 2) and g.flip == (True, True, False)
    g = ScanGeometry.from_affine((5, 6, 7), np.eye(4), axcodes="SAR")
    assert g.perm == (2, 1, 0) and g.flip == (False, False, False) and g.oriented_shape == (7, 6, 5)
    g = ScanGeometry.identity((4, 5, 6), spacing=(0.5, 0.5, 2.0))
    assert g.perm == (0, 1, 2) and g.flip == (False,) * 3 and g.spacing == (0.5, 0.5, 2.0) and g.size == (4, 5, 6)


def test_from_affine_errors():
    from mivp_amd.scan import ScanGeometry
    sing = np.eye(4)
    sing[:3, 2] = sing[:3, 1]
    zero = np.eye(4)
    zero[:3, 0] = 0.0
    for aff in (sing, zero, np.eye(5), np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            ScanGeometry.from_affine((5, 6, 7), aff)
    for codes in ("RA", "RAX", "RLS", "RRS", 7):
        with pytest.raises(ValueError):
            ScanGeometry.from_affine((5, 6, 7), np.eye(4), axcodes=codes)
    for shape in ((5, 6), (5, 0, 7), (5, -1, 7)):
        with pytest.raises(ValueError):
            ScanGeometry.from_affine(shape, np.eye(4))
    for out in ((5, 6), (5, 0, 7)):
        with pytest.raises(ValueError):
            ScanGeometry.from_affine((5, 6, 7), np.eye(4), out_size=out)
    with pytest.raises(ValueError):
        ScanGeometry.identity((5, 6, 7), spacing=(1.0, 0.0, 1.0))


@pytest.mark.parametrize("perm,flip", COMBOS)
def test_orientation_round_trip_all_48(perm, flip):
    from mivp_amd.scan import ScanGeometry
    x = torch.arange(5 * 6 * 7, dtype=torch.int32).reshape(5, 6, 7)
    g = ScanGeometry.from_affine((5, 6, 7), scan_ref.affine_for(perm, flip, zooms=(0.7, 1.1, 2.5)))
    assert g.perm == perm and g.flip == flip
    assert np.allclose(g.spacing, [(0.7, 1.1, 2.5)[p] for p in perm])
    y = scan_ref.orient(x, g.perm, g.flip)
    assert tuple(y.shape) == g.oriented_shape
    assert torch.equal(scan_ref.unorient(y, g.perm, g.flip), x)
    # the tables both launches read state the same maps
    for kind in ("image", "labels"):
        assert np.array_equal(_gather(x.numpy(), g, kind), y.numpy()), kind
    for kind in ("restore_labels", "restore_logits"):
        assert np.array_equal(_gather(y.numpy(), g, kind), x.numpy()), kind


@pytest.mark.parametrize("n_in,n_out", SIZE_PAIRS)
def test_nearest_table_equals_torch(n_in, n_out):
    from mivp_amd.scan import nearest_indices
    tab = nearest_indices(n_in, n_out)
    assert tab.dtype == np.int32 and tab.shape == (n_out,)
    for dt in (torch.float32, torch.uint8):
        src = torch.arange(n_in).to(dt) if n_in <= 256 else None
        if src is None:
            if dt == torch.uint8:
                continue
            src = torch.arange(n_in).to(dt)
        got = F.interpolate(src.reshape(1, 1, n_in, 1, 1), size=(n_out, 1, 1), mode="nearest").reshape(-1)
        assert np.array_equal(got.long().numpy(), tab.astype(np.int64)), dt


@pytest.mark.parametrize("n_in,n_out", SIZE_PAIRS)
def test_linear_taps_equal_torch_float64(n_in, n_out):
    from mivp_amd.scan import linear_taps
    lo, hi, w = linear_taps(n_in, n_out)
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and w.dtype == np.float64
    assert lo.min() >= 0 and hi.max() <= n_in - 1 and np.all(hi - lo <= 1) and np.all((w >= 0) & (w < 1))
    x = torch.randn(n_in, dtype=torch.float64, generator=torch.Generator().manual_seed(n_in * 1000 + n_out))
    want = F.interpolate(x.reshape(1, 1, n_in), size=n_out, mode="linear", align_corners=False).reshape(-1).numpy()
    got = x.numpy()[lo] * (1.0 - w) + x.numpy()[hi] * w
    assert np.abs(got - want).max() <= 1e-12
    if n_in == n_out:
        assert np.array_equal(lo, np.arange(n_out)) and not w.any()


def test_resize_tables_in_three_dimensions():
    from mivp_amd.scan import ScanGeometry
    g = ScanGeometry((7, 23, 9), (2, 0, 1), (True, False, True), out_size=(20, 5, 32))
    x = torch.randint(0, 200, (7, 23, 9), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    want = scan_ref.prepare_labels(x, g)
    assert np.array_equal(_gather(x.numpy(), g, "labels"), want.numpy())
    back = scan_ref.restore_labels(want, g)
    assert np.array_equal(_gather(want.numpy(), g, "restore_labels"), back.numpy())
    # trilinear sections: evaluate lower / upper / weight in float64 against the float64 restatement
    src_dims, out_dims, axes, interp, tab = g.tables("image")
    assert interp and tab.shape == (3 * sum(out_dims),)
    K = sum(out_dims)
    v = x.double().numpy().transpose(axes)
    off = 0
    for a, n in enumerate(out_dims):
        lo, hi = tab[off:off + n], tab[K + off:K + off + n]
        w = tab[2 * K + off:2 * K + off + n].view(np.float32).astype(np.float64)
        shape = [-1 if i == a else 1 for i in range(3)]
        v = np.take(v, lo, axis=a) * (1 - w.reshape(shape)) + np.take(v, hi, axis=a) * w.reshape(shape)
        off += n
    ref = scan_ref.trilinear_f64(scan_ref.orient(x.double(), g.perm, g.flip), g.size).numpy()
    assert np.abs(v - ref).max() < 200 * 3 * 2.0 ** -24        # the fp32 rounding of three weights on values < 200


def test_intensity_map_definition():
    from mivp_amd.scan import intensity_map
    s, t, lo, hi = intensity_map()
    assert (s, t, lo, hi) == (float(np.float32(0.0005)), 0.5, 0.0, 1.0)
    for bad in (dict(a_min=5, a_max=5), dict(a_min=1, a_max=0), dict(b_min=1, b_max=0), dict(a_min=float("nan"))):
        with pytest.raises(ValueError):
            intensity_map(**bad)


# ------------------------------------------------------------------------------------------------ argument checks
def _geom(out_size=None):
    from mivp_amd.scan import ScanGeometry
    return ScanGeometry((5, 6, 7), (2, 0, 1), (False, True, False), out_size=out_size)


def test_prepare_scan_argument_errors():
    from mivp_amd import scan
    g = _geom()
    ok = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, "RAS")
    with pytest.raises(ValueError):
        scan.prepare_scan(ok.numpy(), g)
    with pytest.raises(ValueError):
        scan.prepare_scan(torch.zeros((1, 5, 6, 8), dtype=torch.int16), g)
    with pytest.raises(ValueError):
        scan.prepare_scan(torch.zeros((5, 5, 6, 7), dtype=torch.int16), g)          # more than 4 channels
    with pytest.raises(ValueError):
        scan.prepare_scan(torch.zeros((2, 1, 5, 6, 7), dtype=torch.int16), g)
    with pytest.raises(ValueError):
        scan.prepare_scan(ok.to(torch.int64), g)
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, a_min=3.0, a_max=3.0)
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, out=torch.zeros((1, 1, 5, 6, 7)))                  # the model grid is 7 x 5 x 6
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, out=torch.zeros((1, 1, 7, 5, 6), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU"):
        scan.prepare_scan(ok, g)


def test_label_functions_argument_errors():
    from mivp_amd import scan
    g, gr = _geom(), _geom(out_size=(4, 4, 4))
    seg = torch.zeros((5, 6, 7), dtype=torch.uint8)
    with pytest.raises(ValueError):
        scan.prepare_labels(seg, None)
    with pytest.raises(ValueError):
        scan.prepare_labels(torch.zeros((6, 5, 7), dtype=torch.uint8), g)
    with pytest.raises(ValueError):
        scan.prepare_labels(torch.zeros((1, 2, 5, 6, 7), dtype=torch.uint8), g)
    with pytest.raises(ValueError):
        scan.prepare_labels(seg.to(torch.float64), g)
    with pytest.raises(ValueError):
        scan.prepare_labels(seg, gr, out=torch.zeros((1, 1, 7, 5, 6), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU"):
        scan.prepare_labels(seg, g)

    lab = torch.zeros((1, 1, 7, 5, 6), dtype=torch.uint8)
    with pytest.raises(ValueError):
        scan.restore_labels(lab, gr)                                                # gr's model grid is 4 x 4 x 4
    with pytest.raises(ValueError):
        scan.restore_labels(lab.float(), g)
    with pytest.raises(ValueError):
        scan.restore_labels(lab, g, out=torch.zeros((7, 5, 6), dtype=torch.uint8))  # the native grid is 5 x 6 x 7
    with pytest.raises(ValueError):
        scan.restore_labels(lab, {})
    with pytest.raises(RuntimeError, match="no CPU"):
        scan.restore_labels(lab, g)

    lg = torch.zeros((1, 3, 7, 5, 6))
    with pytest.raises(ValueError):
        scan.restore_labels_from_logits(lg, gr)
    with pytest.raises(ValueError):
        scan.restore_labels_from_logits(lg.double(), g)
    with pytest.raises(ValueError):
        scan.restore_labels_from_logits(torch.zeros((1, 17, 7, 5, 6)), g)
    with pytest.raises(ValueError):
        scan.restore_labels_from_logits(torch.zeros((2, 3, 7, 5, 6)), g)
    with pytest.raises(ValueError):
        scan.restore_labels_from_logits(lg[0, 0], g)
    with pytest.raises(RuntimeError, match="no CPU"):
        scan.restore_labels_from_logits(lg, g)


def test_predict_scan_argument_errors():
    """predict_scan's checks need no device: a predictor shell with the fields they read."""
    from mivp_amd.inference import SlidingWindowPredictor
    p = object.__new__(SlidingWindowPredictor)
    p.image_size, p.cin, p.ncls, p.graph_mode, p.vol = (7, 5, 6), 1, 2, False, None
    g = _geom()
    raw = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    with pytest.raises(ValueError):
        p.predict_scan(raw, g, restore="nearest")
    with pytest.raises(ValueError):
        p.predict_scan(raw, g, restore="logits", postprocess={"largest": True})
    with pytest.raises(ValueError):
        p.predict_scan(raw, g, postprocess={"smallest": True})
    with pytest.raises(ValueError):
        p.predict_scan(raw, g, gamma=2.0)
    with pytest.raises(ValueError):
        p.predict_scan(raw, _geom(out_size=(8, 8, 8)))                              # not the predictor's image size
    with pytest.raises(ValueError):
        p.predict_scan(torch.zeros((2, 5, 6, 7), dtype=torch.int16), g)             # built for one channel
    with pytest.raises(ValueError):
        p.predict_scan(raw, (0, 1, 2))
    with pytest.raises(ValueError):
        p.evaluate_scan(raw, torch.zeros((5, 6, 7), dtype=torch.uint8), g, a_min=1.0, a_max=1.0)
    with pytest.raises(RuntimeError, match="no CPU"):
        p.predict_scan(raw, g)


def test_package_exports():
    import mivp_amd
    for name in ("ScanGeometry", "prepare_scan", "prepare_labels", "restore_labels", "restore_labels_from_logits",
                 "predict_scan_volume"):
        assert callable(getattr(mivp_amd, name)), name
    assert mivp_amd.scan.ScanGeometry is mivp_amd.ScanGeometry
