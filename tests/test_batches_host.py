"""CPU: the host side of the training-batch sampling (mivp_amd.batches): the draw order, the slot records, the checks that
keep a wrong draw from ever reaching the device, the label table, the C-ABI declarations, and one hand-computed voxel
that pins the plain restatement (tests/crops_ref.py) the GPU tests compare against."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import mivp_amd  # noqa: F401
from mivp_amd import batches as BT
from mivp_amd.students_teacher import coord_grid

import crops_ref as R

SHAPES = [(13, 9, 21), (70, 5, 67), (6, 8, 5)]


def _grid(shape, device):
    return coord_grid(shape, device)


# ---------------------------------------------------------------------------------------------- the draw order
def _expected_draws(seed, shapes, ids, roi, num_samples, random_orientation, student_sizes):
    """The documented order, written out a second time: rotations per volume, then origins per sample and axis, then the
    students' origins per sample, student and axis."""
    rs = np.random.RandomState(seed)
    swap = {0: (0, 1, 2), 1: (1, 0, 2), 2: (2, 1, 0), 3: (0, 2, 1)}
    rot = []
    for _ in ids:
        code = int(rs.randint(3)) + 1 if random_orientation else 0
        rot += [code] * num_samples
    vol = [v for v in ids for _ in range(num_samples)]
    origin = []
    for v, code in zip(vol, rot):
        n_rot = [shapes[v][k] for k in swap[code]]
        origin.append([int(rs.randint(0, n_rot[k] - min(roi[k], n_rot[k]) + 1)) for k in range(3)])
    st = np.zeros((len(student_sizes), len(vol), 3), dtype=np.int64)
    for b in range(len(vol)):
        for s, size in enumerate(student_sizes):
            for k in range(3):
                st[s, b, k] = rs.randint(0, roi[k] - min(size[k], roi[k]) + 1)
    return vol, rot, origin, st


@pytest.mark.parametrize("random_orientation", [False, True])
def test_draw_crops_follows_the_documented_order(random_orientation):
    # volume 2 is smaller than the roi on two axes (origin 0 there); student 2 is larger than the roi on one axis
    ids, roi, ns, sizes = [1, 2, 0, 2], (8, 8, 8), 3, [(8, 8, 8), (6, 6, 6), (10, 8, 4)]
    d = BT.draw_crops(np.random.RandomState(11), SHAPES, ids, roi, ns, random_orientation, sizes)
    vol, rot, origin, st = _expected_draws(11, SHAPES, ids, roi, ns, random_orientation, sizes)
    assert d.batch == len(ids) * ns and d.n_students == 3
    assert d.volume.tolist() == vol and d.rot.tolist() == rot
    assert d.origin.tolist() == origin
    assert np.array_equal(d.student_origin, st)
    assert (set(rot) <= {1, 2, 3} and len(set(rot)) > 1) if random_orientation else set(rot) == {0}
    for b in range(d.batch):
        n_rot = BT.rotated_shape(SHAPES[vol[b]], rot[b])
        for k in range(3):
            if n_rot[k] <= roi[k]:
                assert d.origin[b, k] == 0                      # nothing to choose where the volume is not larger
            assert 0 <= d.origin[b, k] <= max(n_rot[k] - roi[k], 0)
    assert not d.student_origin[0].any()                        # a student of the roi's size sits at 0
    assert not d.student_origin[2][:, 0].any()                  # ... and so does one that is larger, on that axis
    assert d.student_origin[1].max() <= 2 and d.student_origin[2][:, 2].max() <= 4
    assert d.check(SHAPES, roi, sizes) is d


def test_draw_crops_refuses_bad_arguments():
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError):
        BT.draw_crops(rs, SHAPES, [3], (8, 8, 8), 1)
    with pytest.raises(ValueError):
        BT.draw_crops(rs, SHAPES, [], (8, 8, 8), 1)
    with pytest.raises(ValueError):
        BT.draw_crops(rs, SHAPES, [0], (8, 8), 1)
    with pytest.raises(ValueError):
        BT.draw_crops(rs, SHAPES, [0], (8, 8, 8), 0)


# ---------------------------------------------------------------------------------------------- records and checks
def _draws():
    return BT.CropDraws(np.array([0, 1, 2], np.int32), np.array([0, 2, 3], np.int32),
                        np.array([[5, 1, 13], [59, 0, 62], [0, 0, 0]], np.int32),
                        np.array([[[0, 0, 0]] * 3, [[2, 1, 0], [0, 2, 2], [1, 1, 1]]], np.int32))


def test_pack_unpack_round_trip():
    d = _draws()
    w = d.pack()
    assert w.dtype == np.int32 and w.shape == (3, 5 + 3 * 2) == (3, BT.record_words(2))
    assert w[1].tolist() == [1, 2, 59, 0, 62, 0, 0, 0, 0, 2, 2]
    back = BT.CropDraws.unpack(w.reshape(-1), 2)
    for name in ("volume", "rot", "origin", "student_origin"):
        assert np.array_equal(getattr(back, name), getattr(d, name)), name
        assert getattr(back, name).dtype == np.int32
    none = BT.CropDraws(d.volume, d.rot, d.origin, np.zeros((0, 3, 3), np.int32))
    assert none.pack().shape == (3, 5)
    assert BT.CropDraws.unpack(none.pack(), 0).student_origin.shape == (0, 3, 3)


def test_check_accepts_the_extremes_and_names_the_bad_sample():
    roi, sizes = (8, 8, 8), [(8, 8, 8), (6, 6, 6)]
    d = _draws()                  # sample 1: volume (70, 5, 67) under code 2 is (67, 5, 70): origin (59, 0, 62) is the maximum
    assert d.check(SHAPES, roi, sizes) is d

    def bad(match, **change):
        e = _draws()
        for k, v in change.items():
            a = getattr(e, k).copy()
            a[v[0]] = v[1]
            setattr(e, k, a)
        with pytest.raises(ValueError, match=match):
            e.check(SHAPES, roi, sizes)

    bad("sample 1: volume id 3", volume=(1, 3))
    bad("sample 0: volume id -1", volume=(0, -1))
    bad("sample 2: rotation code 4", rot=(2, 4))
    bad("sample 2: rotation code -1", rot=(2, -1))
    bad("sample 1: origin .* axis 0", origin=((1, 0), 60))
    bad("sample 1: origin .* axis 2", origin=((1, 2), 63))
    bad("sample 0: origin .* axis 1", origin=((0, 1), -1))
    bad("sample 2: origin .* axis 0", origin=((2, 0), 1))       # (6, 8, 5) under code 3 is (6, 5, 8): smaller than the roi
    bad("sample 1: origin .* student 1 .* axis 1", student_origin=((1, 1, 1), 3))
    bad("sample 0: origin .* student 0 .* axis 2", student_origin=((0, 0, 2), 1))
    bad("sample 2: origin .* student 1", student_origin=((1, 2, 0), -1))
    with pytest.raises(ValueError, match="one batch size"):
        BT.CropDraws(d.volume, d.rot[:2], d.origin, d.student_origin).check(SHAPES, roi, sizes)
    with pytest.raises(ValueError, match="one batch size"):
        d.check(SHAPES, roi, sizes[:1])                         # one student size for two students' origins
    with pytest.raises(ValueError, match="integer"):
        BT.CropDraws(d.volume, d.rot, d.origin.astype(np.float32), d.student_origin).check(SHAPES, roi, sizes)


# ---------------------------------------------------------------------------------------------- the label table
@pytest.mark.parametrize("active", [[1, 2], [0, 3, 7], [5]])
def test_label_table_is_map_label_indices(active):
    values = torch.arange(256, dtype=torch.uint8)
    want = R.map_label_indices(values, list(active))
    t = BT.label_table(list(reversed(active)))                  # (the reference sorts the list itself)
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert np.array_equal(t.astype(np.float32), want.numpy())
    assert t[active[-1]] == len(active) - 1


def test_label_table_identity_and_refusals():
    assert np.array_equal(BT.label_table(None), np.arange(256, dtype=np.uint8))
    for bad in ([], [1, 1], [-1], [256]):
        with pytest.raises(ValueError):
            BT.label_table(bad)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_entries_at_abi_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    for name in ("mivp_crop_fill", "mivp_crop_tensor"):
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    P = _lib.parse_header()
    assert len(P["mivp_crop_fill"][1]) == 12 and len(P["mivp_crop_tensor"][1]) == 9
    assert _lib.ABI_VERSION == 18


def test_device_classes_refuse_the_cpu():
    with pytest.raises(ValueError, match="GPU"):
        BT.VolumeBank("cpu", 1)
    with pytest.raises(ValueError):
        BT.BatchFiller(object(), (8, 8, 8), 2)


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_reference_by_hand_code_2_on_3x4x5():
    """rot90(k=1) over the spatial axes (0, 2) of a 3 x 4 x 5 volume gives 5 x 4 x 3 with out[i0, i1, i2] =
    in[i2, i1, 4 - i0].  Rotated voxel (3, 2, 1) is therefore stored voxel (1, 2, 1): value 1 * 20 + 2 * 5 + 1 = 31 of an
    arange volume, coordinates (1 - 1, 2 - 1.5, 1 - 2) = (0, 0.5, -1) -- those of the STORED volume, in the stored channel
    order.  A 2 x 2 x 2 crop at origin (3, 2, 1) has it at (0, 0, 0); an 8 x 2 x 2 crop of the 5 voxels along axis 0 pads
    (8 - 5) // 2 = 1 voxel before and 2 after."""
    vol = torch.arange(60, dtype=torch.float32).reshape(1, 3, 4, 5)
    lab = (torch.arange(60) % 8).to(torch.uint8).reshape(3, 4, 5)
    img, mask, coord = R.teacher_crop(vol, lab, 2, [3, 2, 1], (2, 2, 2), [2, 7], _grid)
    assert tuple(img.shape) == (1, 2, 2, 2) and tuple(mask.shape) == (1, 2, 2, 2) and tuple(coord.shape) == (3, 2, 2, 2)
    assert float(img[0, 0, 0, 0]) == 31.0
    assert coord[:, 0, 0, 0].tolist() == [0.0, 0.5, -1.0]
    assert float(mask[0, 0, 0, 0]) == 1.0                        # label 31 % 8 = 7, the second of the active [2, 7]
    assert float(img[0, 1, 1, 1]) == 2 * 20 + 3 * 5 + 0          # rotated (4, 3, 2) = stored (2, 3, 0)
    assert BT.rotated_shape((3, 4, 5), 2) == (5, 4, 3)
    img, mask, coord = R.teacher_crop(vol, lab, 2, [0, 2, 1], (8, 2, 2), [2, 7], _grid)
    assert float(img[0, 4, 0, 0]) == 31.0 and coord[:, 4, 0, 0].tolist() == [0.0, 0.5, -1.0]
    for t in (img, mask, coord):
        assert not t[:, 0].any() and not t[:, 6:].any()           # the pad: zero in every output, coordinates included
    assert img[0, 1:6].min() > 0
