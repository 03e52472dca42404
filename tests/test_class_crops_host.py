"""CPU: the host side of the class-balanced crop sampling (mivp_amd.batches: draw_class_crops, ClassCropDraws): the draw
order, the classes that are never drawn, the checks that keep a wrong draw from the device, the C-ABI declarations, and
one centre worked by hand that pins the restatement (tests/class_crops_ref.py) the GPU tests compare against."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT

import mivp_amd  # noqa: F401
from mivp_amd import batches as BT

import class_crops_ref as CR

# what the draws read of a ClassIndex: volume 1 lacks class 1, volume 2 lacks class 0, volume 3 lacks every class
INDEX = SimpleNamespace(counts=np.array([[2000, 450, 7], [240, 0, 0], [0, 5, 3], [0, 0, 0]], dtype=np.int64), num_classes=3)


# ---------------------------------------------------------------------------------------------- the draw order
def _expected_draws(seed, counts, ids, roi, num_samples, ratios, random_orientation, student_sizes):
    """The documented order, written out a second time: rotations per volume; per sample the class, then the rank; then the
    students' origins per sample, student and axis."""
    rs = np.random.RandomState(seed)
    rot = []
    for _ in ids:
        code = int(rs.randint(3)) + 1 if random_orientation else 0
        rot += [code] * num_samples
    vol = [v for v in ids for _ in range(num_samples)]
    cls, rank = [], []
    for v in vol:
        p = np.asarray(ratios, dtype=np.float64) * (counts[v] > 0)
        cls.append(int(rs.choice(len(ratios), p=p / p.sum())))
        rank.append(int(rs.randint(0, counts[v][cls[-1]])))
    st = np.zeros((len(student_sizes), len(vol), 3), dtype=np.int64)
    for b in range(len(vol)):
        for s, size in enumerate(student_sizes):
            for k in range(3):
                st[s, b, k] = rs.randint(0, roi[k] - min(size[k], roi[k]) + 1)
    return vol, rot, cls, rank, st


@pytest.mark.parametrize("random_orientation", [False, True])
def test_draw_class_crops_follows_the_documented_order(random_orientation):
    ids, roi, ns, sizes, ratios = [1, 2, 0, 2], (8, 8, 8), 4, [(8, 8, 8), (6, 6, 6)], (1.0, 2.0, 0.5)
    d = BT.draw_class_crops(np.random.RandomState(11), INDEX, ids, roi, ns, ratios, random_orientation, sizes)
    vol, rot, cls, rank, st = _expected_draws(11, INDEX.counts, ids, roi, ns, ratios, random_orientation, sizes)
    assert d.batch == len(ids) * ns and d.n_students == 2
    assert d.volume.tolist() == vol and d.rot.tolist() == rot
    assert d.cls.tolist() == cls and d.rank.tolist() == rank
    assert np.array_equal(d.student_origin, st)
    assert (set(rot) <= {1, 2, 3}) if random_orientation else set(rot) == {0}
    assert all(a.dtype == np.int32 for a in (d.volume, d.rot, d.cls, d.rank, d.student_origin))
    assert len(set(cls)) == 3                                   # the batch saw every class
    assert d.check(INDEX, roi, sizes) is d
    assert d.pack().shape == (16, BT.record_words(2)) and not d.pack()[:, 2:5].any()     # the origin words are the device's
    assert d.picks().tolist() == [[c, r] for c, r in zip(cls, rank)] and d.picks().dtype == np.int32


def test_a_zero_ratio_and_an_absent_class_are_never_drawn():
    rs = np.random.RandomState(3)
    d = BT.draw_class_crops(rs, INDEX, [0], (8, 8, 8), 400, (1.0, 0.0, 1.0))
    assert set(d.cls.tolist()) == {0, 2}                        # ratio 0: class 1 of volume 0 (450 voxels) never
    assert d.rank[d.cls == 2].max() <= 6 and d.rank[d.cls == 0].max() > 1000
    d = BT.draw_class_crops(rs, INDEX, [1, 2], (8, 8, 8), 200, (1.0, 1.0, 1.0))
    assert set(d.cls[:200].tolist()) == {0}                     # volume 1 holds class 0 only
    assert set(d.cls[200:].tolist()) == {1, 2}                  # volume 2 lacks class 0
    assert d.check(INDEX, (8, 8, 8)) is d
    # ratios (neg, pos) over two classes: RandCropByPosNegLabeld
    two = SimpleNamespace(counts=INDEX.counts[:1, :2], num_classes=2)
    d = BT.draw_class_crops(rs, two, [0], (8, 8, 8), 2000, (1, 3))
    assert 0.70 < float((d.cls == 1).mean()) < 0.80             # 3 / 4, within 5 sigma of 2000 draws (sigma = 0.0097)


def test_no_drawable_class_raises_naming_the_volume():
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError, match="volume 3"):
        BT.draw_class_crops(rs, INDEX, [0, 3], (8, 8, 8), 1, (1, 1, 1))
    with pytest.raises(ValueError, match="volume 1"):
        BT.draw_class_crops(rs, INDEX, [1], (8, 8, 8), 1, (0, 1, 1))       # its only class has ratio 0
    for bad in ((1, 1), (1, -1, 1), (1, float("nan"), 1)):
        with pytest.raises(ValueError, match="ratios"):
            BT.draw_class_crops(rs, INDEX, [0], (8, 8, 8), 1, bad)
    with pytest.raises(ValueError, match="volume_ids"):
        BT.draw_class_crops(rs, INDEX, [4], (8, 8, 8), 1, (1, 1, 1))
    with pytest.raises(ValueError, match="volume_ids"):
        BT.draw_class_crops(rs, INDEX, [], (8, 8, 8), 1, (1, 1, 1))
    with pytest.raises(ValueError):
        BT.draw_class_crops(rs, INDEX, [0], (8, 8, 8), 0, (1, 1, 1))


# ---------------------------------------------------------------------------------------------- the checks
def _draws():
    return BT.ClassCropDraws(np.array([0, 2, 1], np.int32), np.array([0, 2, 3], np.int32), np.array([1, 2, 0], np.int32),
                             np.array([449, 2, 239], np.int32),             # each rank the last of its class
                             np.array([[[0, 0, 0]] * 3, [[2, 1, 0], [0, 2, 2], [1, 1, 1]]], np.int32))


def test_check_accepts_the_extremes_and_names_the_bad_sample():
    roi, sizes = (8, 8, 8), [(8, 8, 8), (6, 6, 6)]
    d = _draws()
    assert d.check(INDEX, roi, sizes) is d

    def bad(match, **change):
        e = _draws()
        for k, v in change.items():
            a = getattr(e, k).copy()
            a[v[0]] = v[1]
            setattr(e, k, a)
        with pytest.raises(ValueError, match=match):
            e.check(INDEX, roi, sizes)

    bad("sample 1: volume id 4 is not indexed", volume=(1, 4))
    bad("sample 0: volume id -1", volume=(0, -1))
    bad("sample 2: rotation code 4", rot=(2, 4))
    bad("sample 2: rotation code -1", rot=(2, -1))
    bad("sample 0: class 3 outside 0..2", cls=(0, 3))
    bad("sample 1: class -1", cls=(1, -1))
    bad("sample 0: rank 450 outside \\[0, 450\\)", rank=(0, 450))
    bad("sample 1: rank -1", rank=(1, -1))
    bad("sample 2: rank 239 outside \\[0, 0\\)", cls=(2, 1))      # volume 1 holds no voxel of class 1: no rank is valid
    bad("sample 1: origin .* student 1", student_origin=((1, 1, 1), 3))
    bad("sample 0: origin .* student 0", student_origin=((0, 0, 2), 1))
    bad("sample 2: origin .* student 1", student_origin=((1, 2, 0), -1))
    with pytest.raises(ValueError, match="one batch size"):
        BT.ClassCropDraws(d.volume, d.rot, d.cls[:2], d.rank, d.student_origin).check(INDEX, roi, sizes)
    with pytest.raises(ValueError, match="one batch size"):
        d.check(INDEX, roi, sizes[:1])
    with pytest.raises(ValueError, match="integer"):
        BT.ClassCropDraws(d.volume, d.rot, d.cls, d.rank.astype(np.float32), d.student_origin).check(INDEX, roi, sizes)
    with pytest.raises(ValueError, match="not indexed"):        # an index that holds no volume yet
        d.check(SimpleNamespace(counts=np.zeros((0, 3), np.int64), num_classes=3), roi, sizes)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_class_entries_at_abi_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    for name in ("mivp_label_index_build", "mivp_crop_pick"):
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    P = _lib.parse_header()
    assert len(P["mivp_label_index_build"][1]) == 7 and len(P["mivp_crop_pick"][1]) == 11
    assert len(P["mivp_crop_fill"][1]) == 12 and len(P["mivp_crop_tensor"][1]) == 9      # the filler's entries are as they were
    assert _lib.ABI_VERSION == 18
    assert BT.ClassIndex.CHUNK == 1024


def test_device_classes_refuse_the_cpu():
    with pytest.raises(ValueError, match="VolumeBank"):
        BT.ClassIndex(object(), 2)
    with pytest.raises(ValueError, match="GPU"):
        BT.CropSlot(2, 0, "cpu", class_index=object())
    with pytest.raises(ValueError):
        BT.BatchFiller(object(), (8, 8, 8), 2, class_index=object())


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_reference_by_hand_code_2_on_3x4x5():
    """Labels ``arange(60) % 8`` on a 3 x 4 x 5 volume, active [2, 7]: class 1 is label 7, the voxels 7, 15, 23, 31, ... in C
    order, so rank 3 of class 1 is voxel 31 = stored (1, 2, 1) (31 = 1 * 20 + 2 * 5 + 1).  rot90(k=1) over the spatial axes
    (0, 2) gives 5 x 4 x 3 with out[i0, i1, i2] = in[i2, i1, 4 - i0], so stored (1, 2, 1) is rotated (4 - 1, 2, 1) =
    (3, 2, 1) (the voxel of tests/test_batches_host.py's hand case).  roi (2, 2, 2): origin = r - 1 = (2, 1, 0), inside
    [0, (3, 2, 1)]: no clamp.  roi (8, 2, 3): axis 0 is smaller than the roi, origin 0; axis 2: r - 1 = 0 and the maximum
    is 3 - 3 = 0.  roi (2, 4, 2): axis 1: r - 2 = 0, the maximum 0.  Unrotated, roi (2, 2, 4): p = (1, 2, 1), origin
    (0, 1, max(1 - 2, 0) = 0): clamped below on axis 2.  The last voxel of class 1 is rank 6, voxel 55 = (2, 3, 0)."""
    lab = (np.arange(60) % 8).astype(np.uint8).reshape(3, 4, 5)
    lut = BT.label_table([2, 7])
    assert CR.voxel(lab, lut, 2, 1, 3) == 31
    assert CR.rank_of(lab, lut, 2, (1, 2, 1)) == (1, 3)
    assert CR.rank_of(lab, lut, 2, (0, 0, 2)) == (0, 2)         # label 2 is active and maps to class 0, like every other label
    pos, n_rot = CR.rotated_positions((3, 4, 5), 2)
    assert n_rot == (5, 4, 3) and np.unravel_index(pos[31], n_rot) == (3, 2, 1)
    assert CR.origin(lab, lut, 2, 2, 1, 3, (2, 2, 2)) == ([2, 1, 0], False)
    assert CR.origin(lab, lut, 2, 2, 1, 3, (8, 2, 3)) == ([0, 1, 0], True)
    assert CR.origin(lab, lut, 2, 2, 1, 3, (2, 4, 2)) == ([2, 0, 0], False)
    assert CR.origin(lab, lut, 2, 0, 1, 3, (2, 2, 4)) == ([0, 1, 0], True)
    assert CR.origin(lab, lut, 2, 0, 1, 6, (2, 2, 2)) == ([1, 2, 0], True)  # the last, voxel 55 = (2, 3, 0): r - 1 = (1, 2, -1)
    d = SimpleNamespace(volume=[0, 0, 0], rot=[2, 0, 2], cls=[1, 1, 1], rank=[3, 6, 3])
    got, moved = CR.origins([lab], lut, 2, d, (2, 2, 2))
    assert got.tolist() == [[2, 1, 0], [1, 2, 0], [2, 1, 0]] and moved.tolist() == [False, True, False]
    pre = CR.chunk_prefix(lab, lut, 2, chunk=16)                # 60 voxels in chunks of 16: class 1 has 2 per full chunk
    assert pre.tolist() == [[0, 14, 28, 42, 53], [0, 2, 4, 6, 7]]
