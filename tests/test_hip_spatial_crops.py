"""GPU tests of the random flip / rotation / zoom of the batch filler (mivp_amd.batches with ``spatial=True``;
csrc/crops_affine.hip) against the numpy float64 restatement in tests/spatial_crops_ref.py, which
tests/test_spatial_crops_host.py pins to ``grid_sample``.  Identity and flips are compared bit for bit with the plain
filler, dyadic maps on integer voxels bit for bit with the restatement (every fp32 step is exact there), a general
rotation and zoom within bounds derived from fp32's step.  ``fill`` takes the direct path (the staged one measured slower,
DESIGN.md 4.28); the staged path runs through ``mivp_crop_fill_affine_debug``, which also reports, per workgroup, which
path the launcher took."""
import numpy as np
import pytest
import torch

import class_crops_ref as CR
import crops_ref as R
import spatial_crops_ref as SR
from batch_outputs import outs as _outs, poison as _poison

pytestmark = pytest.mark.gpu
DEV = "cuda"

# volume 0 is the issue's (20, 18, 36); 1 has odd extents; 2 is smaller than most rois (the pad rule); 3 is large enough
# for a brick's source box under A = 4 I to exceed the staged path's budget
SHAPES = [(20, 18, 36), (21, 19, 37), (6, 8, 5), (40, 36, 70)]
ROIS = [(8, 12, 5), (12, 10, 20), (9, 10, 70)]       # the last: several bricks along d, partial ones on every axis
ACTIVE, NCLS = [2, 5], 3
_state = {}


def _bank(channels, integer=True):
    """(VolumeBank, numpy images, numpy labels): integer voxel values in 0..255 (or uniform floats), labels 0..7."""
    from mivp_amd import batches as BT
    key = (channels, integer)
    if key not in _state:
        g = torch.Generator().manual_seed(31 + channels)
        bank, images, labels = BT.VolumeBank(DEV, channels), [], []
        for s in SHAPES:
            shape = (channels,) + s
            img = torch.randint(0, 256, shape, generator=g).float() if integer else torch.rand(shape, generator=g) * 4 - 1
            lab = torch.randint(0, 8, s, generator=g, dtype=torch.uint8)
            bank.add(img.to(DEV), lab.to(DEV))
            images.append(img.numpy())
            labels.append(lab.numpy())
        _state[key] = (bank, images, labels)
    return _state[key]


def _lut():
    from mivp_amd import batches as BT
    return BT.label_table(ACTIVE)


def _draws(rs, ids, codes, roi, sizes=()):
    """CropDraws with a uniform valid origin per sample."""
    from mivp_amd import batches as BT
    B = len(ids)
    origin = np.zeros((B, 3), np.int32)
    for b in range(B):
        n_rot = BT.rotated_shape(SHAPES[ids[b]], codes[b])
        origin[b] = [rs.randint(0, max(n_rot[k] - roi[k], 0) + 1) for k in range(3)]
    st = np.zeros((len(sizes), B, 3), np.int32)
    for s, size in enumerate(sizes):
        st[s] = [[rs.randint(0, max(roi[k] - size[k], 0) + 1) for k in range(3)] for _ in range(B)]
    return BT.CropDraws(np.asarray(ids, np.int32), np.asarray(codes, np.int32), origin, st).check(SHAPES, roi, sizes)


def _spatial(mats, shifts=None):
    from mivp_amd import batches as BT
    a = np.zeros((len(mats), 12), np.float32)
    for b, m in enumerate(mats):
        a[b, :9] = np.asarray(m, np.float64).reshape(-1)
        if shifts is not None:
            a[b, 9:] = shifts[b]
    return BT.SpatialDraws(a).check(len(mats))


def _teacher(f):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (f.image, f.mask, f.coord)]


def _paths(f, force_fallback=False):
    """The filler's teacher launch through the debug entry, on the slots as they stand, with the staged path switched on
    (or off: ``force_fallback``, what ``fill`` itself issues): int32 [B, bricks], 1 = staged."""
    from mivp_amd import _lib as L
    from mivp_amd._host import i3
    from mivp_amd import batches as BT
    bricks = int(np.prod([-(-f.roi[k] // BT.SPATIAL_BRICK[k]) for k in range(3)]))
    paths = torch.full((f.B, bricks), -1, dtype=torch.int32, device=DEV)
    L.call("mivp_crop_fill_affine_debug", L.ptr(f.bank.table), f.bank.capacity, f.bank.channels, L.ptr(f.slot.records),
           f.slot.words, L.ptr(f.spatial_slot.words), f.B, i3(f.roi), L.ptr(f.lut), L.ptr(f.image), L.ptr(f.mask),
           L.ptr(f.coord), int(not force_fallback), L.ptr(paths), L.stream())
    torch.cuda.synchronize()
    return paths.cpu().numpy()


def _ref(channels, d, sp, roi, integer=True):
    _, images, labels = _bank(channels, integer)
    return SR.teacher_batch(images, labels, _lut(), d.volume, d.rot, d.origin, roi, sp.affine)


def _assert_bits(got, want, what):
    for name, g, w in zip(("image", "mask", "coord"), got, want):
        assert not np.isnan(g).any(), f"{what}: {name}: an output voxel was not written"
        w32 = w.astype(np.float32)
        assert np.array_equal(w32.astype(np.float64), w), f"{what}: {name}: the reference is not exact in fp32"
        assert np.array_equal(g, w32), f"{what}: {name}: {int((g != w32).sum())} voxels differ"


# ------------------------------------------------------------------------------------------------ 1. the identity
@pytest.mark.parametrize("channels", [1, 2])
def test_identity_is_bit_equal_to_the_plain_fill(channels):
    from mivp_amd import batches as BT
    bank, _, _ = _bank(channels)
    rs = np.random.RandomState(3)
    for roi in ROIS + [(24, 10, 40)]:                               # the last is larger than volume 0 on two axes
        plain = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True)
        own = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, spatial=True)
        assert plain.spatial_slot is None and own.spatial_slot.words.shape == (48,)
        assert torch.equal(own.spatial_slot.words.cpu(), torch.from_numpy(BT.SpatialDraws.identity(4).affine.reshape(-1)))
        for code in range(4):
            d = _draws(rs, [0, 1, 2, 0], [code] * 4, roi)
            _poison(own)
            plain.fill(d)
            own.fill(d)                                             # spatial=None: the slot as made, the identity
            torch.cuda.synchronize()
            for name in ("image", "mask", "coord"):
                a, b = getattr(own, name), getattr(plain, name)
                assert torch.equal(a, b), (roi, code, name, int((a != b).sum()))
            _assert_bits(_teacher(own), _ref(channels, d, BT.SpatialDraws.identity(4), roi)[:3], (roi, code))


# ------------------------------------------------------------------------------------------------ 2. flips
def test_flips_equal_torch_flip_of_the_plain_crop():
    from mivp_amd import batches as BT
    bank, _, _ = _bank(2)
    rs = np.random.RandomState(5)
    flips = [(True, False, False), (False, True, True), (True, True, True), (False, False, True)]
    sp = _spatial([np.diag([-1.0 if f else 1.0 for f in fl]) for fl in flips])
    for roi in ROIS[:2]:                                            # volumes 0, 1 and 3 are at least as large
        plain = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True)
        own = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, spatial=True)
        for code in range(4):
            d = _draws(rs, [0, 1, 3, 1], [code] * 4, roi)
            _poison(own)
            plain.fill(d)
            own.fill(d, spatial=sp)
            torch.cuda.synchronize()
            for b, fl in enumerate(flips):
                dims = [1 + k for k in range(3) if fl[k]]
                for name in ("image", "mask", "coord"):         # coord too: a flipped crop holds the mirrored voxels'
                    want = torch.flip(getattr(plain, name)[b], dims)
                    assert torch.equal(getattr(own, name)[b], want), (roi, code, b, name)
            _assert_bits(_teacher(own), _ref(2, d, sp, roi)[:3], (roi, code))


# ------------------------------------------------------------------------------------------------ 3. exact operands
DYADIC = [[[0, -1, 0], [1, 0, 0], [0, 0, 1]],                       # a permutation with a sign
          [[0.5, 0.125, 0], [0, 1.25, 0], [0, 0, 1]],               # anisotropic scales and a shear
          [[1, 0, 0.125], [0, -0.5, 0], [0.25, 0, 1.25]],
          [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]]
DYADIC_SHIFT = [[0.125, -0.375, 0.5], [0.5, 0.25, -0.125], [0, 0, 0], [-0.5, 0.5, 0.875]]


@pytest.mark.parametrize("channels", [1, 2])
def test_dyadic_maps_are_bit_equal_to_the_restatement_on_the_staged_path(channels):
    """Entries of A and s in eighths, voxels in 0..255: r is a multiple of 1/16, each weight too, and the three steps
    a + w (b - a) need 8 + 12 bits -- exact in fp32 however the compiler contracts them."""
    from mivp_amd import batches as BT
    bank, _, _ = _bank(channels)
    rs = np.random.RandomState(7)
    sp = _spatial(DYADIC, DYADIC_SHIFT)
    seen = set()
    for roi in ROIS:
        own = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, spatial=True)
        for code in range(4):
            d = _draws(rs, [0, 1, 3, 2], [code] * 4, roi)
            _poison(own)
            own.fill(d, spatial=sp)
            got = _teacher(own)
            want = _ref(channels, d, sp, roi)
            _assert_bits(got, want[:3], (roi, code))
            assert (want[3] != np.floor(want[3])).any() and (want[1] > 0).any()        # weights and labels were in play
            _poison(own)
            paths = _paths(own)
            _assert_bits(_teacher(own), want[:3], (roi, code, "debug entry"))
            seen |= set(np.unique(paths).tolist())
            if roi == (12, 10, 20):
                assert (paths[:3] == 1).all(), paths               # crops inside their volumes: every brick is staged
            _poison(own)
            forced = _paths(own, force_fallback=True)
            assert (forced == 0).all()
            _assert_bits(_teacher(own), want[:3], (roi, code, "forced fallback"))
    assert seen <= {0, 1} and 1 in seen


def test_strong_minification_takes_the_fallback_path_with_the_same_bits():
    """A = 4 I on the (40, 36, 70) volume: a full 8 x 8 x 16 brick reads a (28 + 4) x (28 + 4) x (60 + 4) box, far over the
    12288-cell budget, so the launcher itself reports the fallback.  The crops sit in the middle of the volume: near a
    face the clip to the volume could bring a box back under the budget."""
    from mivp_amd import batches as BT
    bank, _, _ = _bank(2)
    roi = (8, 16, 16)
    own = BT.BatchFiller(bank, roi, 3, active_labels=ACTIVE, with_coord=True, spatial=True)
    sp = _spatial([4 * np.eye(3)] * 3, [[0.375, -0.25, 0.125], [0, 0, 0], [0.5, 0.5, 0.5]])
    assert 32 * 32 * 65 > BT.SPATIAL_BOX_CELLS
    rs = np.random.RandomState(9)
    for code in range(4):
        d = _draws(rs, [3, 3, 3], [code] * 3, roi)
        d.origin[:] = (np.asarray(BT.rotated_shape(SHAPES[3], code)) - np.asarray(roi)) // 2
        _poison(own)
        own.fill(d.check(SHAPES, roi), spatial=sp)
        want = _ref(2, d, sp, roi)
        _assert_bits(_teacher(own), want[:3], code)
        _poison(own)
        paths = _paths(own)
        assert paths.shape == (3, 2) and (paths == 0).all(), paths
        _assert_bits(_teacher(own), want[:3], (code, "debug entry"))
        inside = SR.nearest_inside(want[3][0], BT.rotated_shape(SHAPES[3], code))[1]
        assert 0.3 < inside.mean() <= 1.0


# ------------------------------------------------------------------------------------------------ 4. rotation and zoom
@pytest.mark.parametrize("code,origin", [(0, (4, 3, 7)), (1, (3, 4, 7)), (2, (11, 3, 0)), (3, (4, 12, 0))])
def test_general_rotation_and_zoom_within_fp32_bounds(code, origin):
    """Volume (20, 18, 36), roi (12, 10, 20), angles (0.3, -0.2, 0.5), zooms (1.1, 0.9, 1.05); code 0 with origin (4, 3, 7)
    is the stated case, the other codes turn the same volume.  delta = 8 * 2^-24 * max(extent) bounds the fp32 error of r
    (three products and three sums of terms below the extent); the image may move by delta times one value range per axis
    plus its own rounding, coord by 2 delta, and the mask may differ only where r + 0.5 is within delta of an integer."""
    from mivp_amd import batches as BT
    bank, images, _ = _bank(2, integer=False)
    roi = (12, 10, 20)
    A = BT.affine_matrix((False, False, False), (0.3, -0.2, 0.5), (1.1, 0.9, 1.05))
    sp = _spatial([A, A], [[0, 0, 0], [0.3, -0.45, 0.2]])
    d = BT.CropDraws(np.zeros(2, np.int32), np.full(2, code, np.int32), np.asarray([origin, origin], np.int32),
                     np.zeros((0, 2, 3), np.int32)).check(SHAPES, roi)
    own = BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, with_coord=True, spatial=True)
    _poison(own)
    own.fill(d, spatial=sp)
    got = _teacher(own)
    want = _ref(2, d, sp, roi, integer=False)
    delta = 8 * 2.0 ** -24 * max(SHAPES[0])
    assert 1.7e-5 < delta < 1.8e-5
    span = float(images[0].max() - images[0].min())
    assert not any(np.isnan(g).any() for g in got)
    err_i, err_c = np.abs(got[0] - want[0]).max(), np.abs(got[2] - want[2]).max()
    h = want[3] + 0.5
    near = (np.abs(h - np.round(h)) <= delta).any(axis=1)
    differ = (got[1][:, 0] != want[1][:, 0]) & ~near
    inside = np.stack([SR.nearest_inside(want[3][b], BT.rotated_shape(SHAPES[0], code))[1] for b in range(2)])
    print(f"code {code}: image err {err_i:.3e} (bound {(3 * delta + 8 * 2.0 ** -24) * span:.3e}), coord err {err_c:.3e} "
          f"(bound {2 * delta:.3e}), mask left out {near.mean():.5f}, differing {int(differ.sum())}, inside {inside.mean():.4f}")
    assert err_i <= (3 * delta + 8 * 2.0 ** -24) * span
    assert err_c <= 2 * delta
    assert near.mean() <= 0.01 and not differ.any()
    # the zero rule is exercised but does not dominate (code 3: the roi is wider than the turned volume, the pad is zeros)
    assert (0.98 if code == 0 else 0.8) < inside.mean() < 1.0
    # both paths give the same bits
    a = [t.clone() for t in (own.image, own.mask, own.coord)]
    assert (_paths(own) == 1).all()
    b = [t.clone() for t in (own.image, own.mask, own.coord)]
    assert (_paths(own, force_fallback=True) == 0).all()
    for x, y, z in zip(a, b, (own.image, own.mask, own.coord)):
        assert torch.equal(x, y) and torch.equal(x, z)


# ------------------------------------------------------------------------------------------------ 5. students
def test_students_are_crops_of_the_augmented_teacher():
    from mivp_amd import batches as BT
    bank, _, _ = _bank(2)
    roi, sizes = (12, 10, 20), [(12, 10, 20), (7, 6, 9)]
    own = BT.BatchFiller(bank, roi, 4, student_sizes=sizes, active_labels=ACTIVE, spatial=True)
    rs = np.random.RandomState(13)
    d = _draws(rs, [0, 1, 3, 2], [0, 1, 2, 3], roi, sizes)
    sp = BT.draw_spatial(rs, 4, p_flip=(0.5, 0.5, 0.5), p_affine=1.0, rotate_range=(0.26, 0.26, 0.26), scale_range=(0.8, 1.25),
                         isotropic=False, shift=True)
    _poison(own)
    batch = own.fill(d, spatial=sp)
    torch.cuda.synchronize()
    assert batch is own.batch and sorted(batch) == ["coord", "coord_st", "image", "image_st", "mask_st_0"]
    assert not any(torch.isnan(t).any() for t in _outs(own))
    for i, size in enumerate(sizes):
        assert torch.equal(own.image_st[i], R.student_view(own.image, d.student_origin[i], size))
        assert torch.equal(own.coord_st[i], R.student_view(own.coord, d.student_origin[i], size))
    assert torch.equal(own.mask_st_0, R.student_view(own.mask, d.student_origin[0], sizes[0]))
    plain = BT.BatchFiller(bank, roi, 4, student_sizes=sizes, active_labels=ACTIVE)
    plain.fill(d)
    assert not torch.equal(plain.image, own.image)                  # and the teacher was augmented


# ------------------------------------------------------------------------------------------------ 6. class-balanced
def test_class_balanced_centres_are_honoured():
    from mivp_amd import batches as BT
    bank, _, labels = _bank(1)
    index = BT.ClassIndex(bank, NCLS, ACTIVE).update()
    roi = (9, 7, 11)
    own = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, class_index=index, spatial=True)
    rs = np.random.RandomState(17)
    moved_any, free_any = False, False
    for sp in (BT.SpatialDraws.identity(4), _spatial(DYADIC, DYADIC_SHIFT)):
        for _ in range(3):
            d = BT.draw_class_crops(rs, index, [0, 1, 3, 0], roi, 1, (1, 2, 0), True)
            _poison(own)
            own.fill(d, spatial=sp)
            origin = own.slot.resolved_origins()
            want_origin, moved = CR.origins(labels, _lut(), NCLS, d, roi)
            assert np.array_equal(origin, want_origin)
            want = SR.teacher_batch(_bank(1)[1], labels, _lut(), d.volume, d.rot, origin, roi, sp.affine)
            _assert_bits(_teacher(own), want[:3], "class-balanced")
            if not sp.affine[:, 9:].any():                         # the identity: the centre voxel carries the drawn class
                centre = own.mask[:, 0, 4, 3, 5].cpu().numpy()
                assert np.array_equal(centre[~moved], d.cls[~moved].astype(np.float32))
                moved_any, free_any = moved_any or moved.any(), free_any or (~moved).any()
    assert free_any


# ------------------------------------------------------------------------------------------------ 7. recording
def test_a_recorded_fill_follows_both_slots():
    from mivp_amd import batches as BT
    bank, _, _ = _bank(2, integer=False)
    roi, sizes = (12, 10, 20), [(8, 8, 8)]
    own = BT.BatchFiller(bank, roi, 3, student_sizes=sizes, active_labels=ACTIVE, spatial=True)
    ref = BT.BatchFiller(bank, roi, 3, student_sizes=sizes, active_labels=ACTIVE, spatial=True)
    rs = np.random.RandomState(19)
    kw = dict(p_flip=(0.5, 0.5, 0.5), p_affine=1.0, rotate_range=(0.26, 0.26, 0.26), scale_range=(0.8, 1.25), shift=True)
    loads = [(_draws(rs, [0, 3, 1], [rs.randint(4) for _ in range(3)], roi, sizes), BT.draw_spatial(rs, 3, **kw))
             for _ in range(3)]
    own.fill(*loads[0])
    first = [t.clone() for t in _outs(own)]
    _poison(own)
    own.fill()                                                      # the same slots: the same bits
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, _outs(own)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        own.fill()
        own.spatial_slot.load(loads[1][1])                          # does nothing while recording
    assert own.spatial_slot.draws is loads[0][1]
    for d, sp in loads[::-1]:
        own.slot.load(d, bank, roi, sizes)
        own.spatial_slot.load(sp)
        _poison(own)
        graph.replay()
        ref.fill(d, spatial=sp)
        torch.cuda.synchronize()
        assert not any(torch.isnan(t).any() for t in _outs(own))
        assert all(torch.equal(a, b) for a, b in zip(_outs(own), _outs(ref)))
    assert all(torch.equal(a, b) for a, b in zip(first, _outs(own)))            # loads[0] came last
    other = BT.SpatialSlot(3, DEV)                                  # a slot of one's own is used as it stands
    other.load(loads[2][1])
    own.fill(loads[2][0], spatial=other)
    ref.fill(*loads[2])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_outs(own), _outs(ref)))


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_come_before_any_launch():
    from mivp_amd import batches as BT
    bank, _, _ = _bank(1)
    roi = (8, 12, 5)
    d = _draws(np.random.RandomState(1), [0, 1], [0, 3], roi)
    other = _draws(np.random.RandomState(2), [1, 0], [2, 1], roi)
    plain = BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE)
    own = BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, spatial=True)
    own.fill(d)
    plain.fill(d)
    torch.cuda.synchronize()
    before = [t.clone() for t in _outs(own) + _outs(plain)]
    records = own.slot.records.clone()
    nan = BT.SpatialDraws.identity(2)
    nan.affine[1, 5] = np.nan
    cases = [(plain, dict(spatial=BT.SpatialDraws.identity(2)), "built with spatial=True"),
             (plain, dict(spatial=BT.SpatialSlot(2, DEV)), "built with spatial=True"),
             (own, dict(spatial=nan), "sample 1: a non-finite"),
             (own, dict(spatial=BT.SpatialDraws.identity(3)), r"float32 \[2, 12\]"),
             (own, dict(spatial=BT.SpatialSlot(3, DEV)), "spatial slot of batch 3"),
             (own, dict(spatial=np.eye(3)), "SpatialDraws, a SpatialSlot")]
    for f, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            f.fill(other, **kw)                                     # new crop draws too: they must not be loaded either
    with pytest.raises(ValueError, match="sample 1"):
        own.spatial_slot.load(nan)
    with pytest.raises(ValueError, match="SpatialDraws expected"):
        own.spatial_slot.load(d)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, _outs(own) + _outs(plain)))
    assert torch.equal(records, own.slot.records) and own.slot.draws is d and plain.slot.draws is d
    assert torch.equal(own.spatial_slot.words.cpu(), torch.from_numpy(BT.SpatialDraws.identity(2).affine.reshape(-1)))
