"""GPU tests of the training-batch sampling (mivp_amd.batches, csrc/crops.hip) against the plain restatement in
tests/crops_ref.py -- ``torch.rot90`` of the whole volume, slicing, ``F.pad``.  The kernel only moves and maps values, so
every comparison is bit-exact (``torch.equal``).  Nothing here hands the device a draw that the host checks refuse."""
import copy

import numpy as np
import pytest
import torch

import class_crops_ref as CR
import crops_ref as R
from batch_outputs import grid as _grid, poison as _poison

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (13, 9, 21): plain; (70, 5, 67): odd D, the large source; (6, 8, 5): smaller than the roi.  The rois cut from this bank are
# at most 12 wide: one work unit per output plane.  WIDE below holds the rois that take several units and partial tiles.
SHAPES = [(13, 9, 21), (70, 5, 67), (6, 8, 5)]
ACTIVE = [2, 5]
STUDENTS = [(8, 8, 8), (6, 6, 6), (10, 8, 4)]           # the last one is larger than the roi (8, 8, 8) on axis 0: padded
_banks = {}


def _bank(channels):
    """(VolumeBank, images, labels): arange-based images (every voxel value of the bank is unique), labels 0..7."""
    from mivp_amd import batches as BT
    if channels not in _banks:
        g = torch.Generator().manual_seed(7)
        bank, images, labels, first = BT.VolumeBank(DEV, channels), [], [], 1
        for s in SHAPES:
            n = channels * s[0] * s[1] * s[2]
            images.append(torch.arange(first, first + n, dtype=torch.float32).reshape((channels,) + s).to(DEV))
            labels.append(torch.randint(0, 8, s, generator=g, dtype=torch.uint8).to(DEV))
            first += n
            bank.add(images[-1], labels[-1])
        _banks[channels] = (bank, images, labels)
    return _banks[channels]


def _draws(volume, rot, roi, where, student_sizes=(), student_where="lo"):
    """Draws at the extremes: ``where`` = 'lo' (origin 0), 'hi' (the maximum) or 'odd' (an odd origin where there is room:
    a 16-byte store then starts at a misaligned source address)."""
    from mivp_amd import batches as BT
    B = len(volume)
    origin = np.zeros((B, 3), np.int32)
    for b in range(B):
        n_rot = BT.rotated_shape(SHAPES[volume[b]], rot[b])
        for k in range(3):
            hi = max(n_rot[k] - roi[k], 0)
            origin[b, k] = {"lo": 0, "hi": hi, "odd": min((1, 3, 5)[k], hi)}[where]
    st = np.zeros((len(student_sizes), B, 3), np.int32)
    for s, size in enumerate(student_sizes):
        for b in range(B):
            for k in range(3):
                hi = max(roi[k] - size[k], 0)
                st[s, b, k] = {"lo": 0, "hi": hi, "mix": (hi, 0, hi // 2)[(b + k + s) % 3]}[student_where]
    return BT.CropDraws(np.asarray(volume, np.int32), np.asarray(rot, np.int32), origin, st)


def _check_teacher(filler, draws, channels, roi):
    _, images, labels = _bank(channels)
    want = R.teacher_batch(images, labels, draws, roi, ACTIVE, _grid)
    torch.cuda.synchronize()
    for name, got, ref in zip(("image", "mask", "coord"), (filler.image, filler.mask, filler.coord), want):
        assert not torch.isnan(got).any(), f"{name}: an output voxel was not written"
        assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} voxels differ"


# ------------------------------------------------------------------------------------------------ 1. teacher crops
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("roi", [(8, 8, 8), (8, 12, 4)])
def test_teacher_crops_equal_the_restatement(roi, channels):
    """B = 5 samples of different volumes in one launch, all four codes, origins at 0 / the maximum / an odd value."""
    from mivp_amd import batches as BT
    bank, _, _ = _bank(channels)
    filler = BT.BatchFiller(bank, roi, 5, active_labels=ACTIVE, with_coord=True)
    volume = [0, 1, 2, 1, 0]
    for where in ("lo", "hi", "odd"):
        for rot in ([0, 1, 2, 3, 0], [1, 2, 3, 0, 3], [2, 3, 0, 1, 2], [3, 0, 1, 2, 1]):
            draws = _draws(volume, rot, roi, where)
            _poison(filler)
            filler.fill(draws)
            _check_teacher(filler, draws, channels, roi)
    assert filler.xy[0] is filler.image and filler.xy[1] is filler.mask and filler.batch is filler.xy


def test_a_launch_of_one_code_only_and_the_identity_table():
    """Every sample under the same code (the other path's workgroups all return), labels passed through unchanged, and a
    volume without labels (mask 0)."""
    from mivp_amd import batches as BT
    _, images, labels = _bank(1)
    bank = BT.VolumeBank(DEV, 1)
    for i, im in enumerate(images):
        bank.add(im[None] if i == 0 else im, None if i == 2 else (labels[i][None, None] if i == 0 else labels[i]))
    roi = (8, 8, 8)
    filler = BT.BatchFiller(bank, roi, 3, with_coord=True)
    for code in range(4):
        draws = _draws([0, 1, 2], [code] * 3, roi, "odd")
        _poison(filler)
        filler.fill(draws)
        img, mask, coord = R.teacher_batch(images, [labels[0], labels[1], None], draws, roi, None, _grid)
        torch.cuda.synchronize()
        assert torch.equal(filler.image, img) and torch.equal(filler.mask, mask) and torch.equal(filler.coord, coord)
        assert not filler.mask[2].any() and filler.mask[:2].max() == 7


# ------------------------------------------------------------------------------------------------ 1b. several work units
# The kernel tiles the OUTPUT.  Tiles path (codes 2, 3): 64 x 64 tiles over (exchanged output axis, d), so the roi must
# exceed 64 on both for the unit decode, e0 / d0 and the partial-tile guards to matter.  Rows path (codes 0, 1): 256 / LX
# rows along w per unit, LX = 1, 2, 4 .. 64 lanes for ceil(d / 4) groups, a stride loop over d beyond 256 voxels.
WIDE_SHAPES = [(70, 5, 67), (5, 69, 71), (3, 4, 300)]
WIDE = [(66, 5, 67),        # code 2 from (70, 5, 67): 2 x 2 tiles, 2 and 3 voxels wide at the far side; d % 4 = 3
        (4, 66, 67),        # code 3 from (5, 69, 71): 2 x 2 tiles over (w, d)
        (3, 70, 67),        # rows: LX = 32, 8 rows per unit -> 9 chunks along w, the last one partial; scalar tail
        (2, 9, 261),        # rows: LX = 64 and two strides along d, 3 chunks along w; tiles: 5 tiles along d
        (5, 70, 40),        # rows: LX = 16, 5 chunks along w
        (3, 70, 13)]        # rows: LX = 4, 2 chunks along w
_wide = {}


def _wide_bank():
    from mivp_amd import batches as BT
    if not _wide:
        g = torch.Generator().manual_seed(17)
        bank, images, labels, first = BT.VolumeBank(DEV, 2), [], [], 1
        for s in WIDE_SHAPES:
            n = 2 * s[0] * s[1] * s[2]
            images.append(torch.arange(first, first + n, dtype=torch.float32).reshape((2,) + s).to(DEV))
            labels.append(torch.randint(0, 8, s, generator=g, dtype=torch.uint8).to(DEV))
            first += n
            bank.add(images[-1], labels[-1])
        _wide.update(bank=bank, images=images, labels=labels)
    return _wide["bank"], _wide["images"], _wide["labels"]


def _wide_draws(rot, roi, where):
    from mivp_amd import batches as BT
    origin = np.zeros((3, 3), np.int32)
    for b in range(3):
        n_rot = BT.rotated_shape(WIDE_SHAPES[b], rot[b])
        for k in range(3):
            hi = max(n_rot[k] - roi[k], 0)
            origin[b, k] = hi if where == "hi" else min((1, 3, 1)[k], hi)
    return BT.CropDraws(np.arange(3, dtype=np.int32), np.asarray(rot, np.int32), origin, np.zeros((0, 3, 3), np.int32))


@pytest.mark.parametrize("roi", WIDE)
def test_rois_of_several_work_units_and_partial_tiles(roi):
    """C = 2, mask and coordinates, NaN-prefilled, one sample per volume: every code alone (only one path's units do
    work) and mixed in one launch, origins at the maximum and at odd values."""
    from mivp_amd import batches as BT
    bank, images, labels = _wide_bank()
    filler = BT.BatchFiller(bank, roi, 3, active_labels=ACTIVE, with_coord=True)
    for where in ("hi", "odd"):
        for rot in ([0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [2, 3, 0], [1, 2, 3]):
            draws = _wide_draws(rot, roi, where)
            _poison(filler)
            filler.fill(draws)
            want = R.teacher_batch(images, labels, draws, roi, ACTIVE, _grid)
            torch.cuda.synchronize()
            for name, got, ref in zip(("image", "mask", "coord"), (filler.image, filler.mask, filler.coord), want):
                assert not torch.isnan(got).any(), f"{name} {rot} {where}: an output voxel was not written"
                assert torch.equal(got, ref), f"{name} {rot} {where}: {int((got != ref).sum())} voxels differ"


@pytest.mark.parametrize("roi", [(8, 12, 5), (66, 5, 67)])
def test_image_alone_and_image_with_coordinates(roi):
    """``with_mask=False``: no table and no mask pointer reach the kernel; with and without the coordinates."""
    from mivp_amd import batches as BT
    bank, images, labels = _wide_bank()
    for with_coord in (False, True):
        filler = BT.BatchFiller(bank, roi, 3, with_coord=with_coord, with_mask=False)
        assert filler.mask is None and filler.lut is None and filler.xy == (filler.image, None)
        for rot in ([0, 1, 0], [2, 3, 2], [3, 0, 1]):
            draws = _wide_draws(rot, roi, "odd")
            _poison(filler)
            filler.fill(draws)
            img, _, coord = R.teacher_batch(images, labels, draws, roi, None, _grid)
            torch.cuda.synchronize()
            assert torch.equal(filler.image, img)
            assert filler.coord is None if not with_coord else torch.equal(filler.coord, coord)


# ------------------------------------------------------------------------------------------------ 2. the pad rule
@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_pad_rule_centres_the_crop_and_zeroes_every_output(code):
    """Volume (6, 8, 5) in roi (8, 8, 8) without rotation: pads (2, 0, 3) split as (1 | 1), (0 | 0), (1 | 2), so the crop
    sits at offsets (1, 0, 1).  Under a rotation the same rule holds for the rotated extents."""
    from mivp_amd import batches as BT
    bank, images, labels = _bank(1)
    roi = (8, 8, 8)
    filler = BT.BatchFiller(bank, roi, 1, active_labels=ACTIVE, with_coord=True)
    draws = _draws([2], [code], roi, "hi")
    n_rot = BT.rotated_shape(SHAPES[2], code)
    assert draws.origin.tolist() == [[0, max(n_rot[1] - 8, 0), 0]]
    _poison(filler)
    filler.fill(draws)
    _check_teacher(filler, draws, 1, roi)
    off = [(8 - min(8, n)) // 2 for n in n_rot]
    if code == 0:
        assert off == [1, 0, 1]
    inside = torch.zeros(roi, dtype=torch.bool, device=DEV)
    inside[off[0]:off[0] + min(8, n_rot[0]), off[1]:off[1] + min(8, n_rot[1]), off[2]:off[2] + min(8, n_rot[2])] = True
    for t in (filler.image, filler.mask, filler.coord):
        assert not t[0][:, ~inside].any()                       # the pad: zero in image, mask and all three coordinates
    assert (filler.image[0][:, inside] > 0).all()
    # the first voxel of the crop is rotated voxel `origin`: for code 0 stored voxel (0, 0, 0)
    if code == 0:
        assert float(filler.image[0, 0, 1, 0, 1]) == float(images[2][0, 0, 0, 0])
        assert filler.coord[0, :, 1, 0, 1].tolist() == [-2.5, -3.5, -2.0]


# ------------------------------------------------------------------------------------------------ 3. student views
@pytest.mark.parametrize("channels", [1, 2])
def test_student_views_are_crops_of_the_teacher_tensors(channels):
    from mivp_amd import batches as BT
    bank, _, _ = _bank(channels)
    roi = (8, 8, 8)
    filler = BT.BatchFiller(bank, roi, 5, student_sizes=STUDENTS, active_labels=ACTIVE)
    assert sorted(filler.batch) == ["coord", "coord_st", "image", "image_st", "mask_st_0"]
    for where, st_where in (("odd", "lo"), ("hi", "hi"), ("lo", "mix")):
        draws = _draws([0, 1, 2, 1, 0], [0, 1, 2, 3, 2], roi, where, STUDENTS, st_where)
        _poison(filler)
        batch = filler.fill(draws)
        _check_teacher(filler, draws, channels, roi)
        for i, size in enumerate(STUDENTS):
            assert torch.equal(batch["image_st"][i], R.student_view(filler.image, draws.student_origin[i], size))
            assert torch.equal(batch["coord_st"][i], R.student_view(filler.coord, draws.student_origin[i], size))
            assert tuple(batch["image_st"][i].shape) == (5, channels) + size
        assert torch.equal(batch["mask_st_0"], R.student_view(filler.mask, draws.student_origin[0], STUDENTS[0]))
        # the student larger than the roi: one zero slice before and one after the 8 teacher voxels, coordinates included
        for t in (batch["image_st"][2], batch["coord_st"][2]):
            assert not t[:, :, 0].any() and not t[:, :, 9].any()
        assert batch["image"] is filler.image and batch["coord"] is filler.coord


# ------------------------------------------------------------------------------------------------ 4. reproducibility, reload
def test_same_slot_same_bits_and_a_reload_gives_the_other_crops():
    from mivp_amd import batches as BT
    bank, _, _ = _bank(2)
    roi = (8, 12, 4)
    filler = BT.BatchFiller(bank, roi, 5, active_labels=ACTIVE, with_coord=True)
    slot = BT.CropSlot(5, 0, DEV)
    d1 = _draws([0, 1, 2, 1, 0], [0, 1, 2, 3, 2], roi, "odd")
    d2 = _draws([1, 0, 1, 2, 1], [3, 2, 0, 1, 1], roi, "hi")
    slot.load(d1, bank, roi)
    filler.fill(slot)
    first = [t.clone() for t in (filler.image, filler.mask, filler.coord)]
    _poison(filler)
    filler.fill(slot)
    assert all(torch.equal(a, b) for a, b in zip(first, (filler.image, filler.mask, filler.coord)))
    _check_teacher(filler, d1, 2, roi)
    slot.load(d2, bank, roi)
    filler.fill(slot)                                           # the same call, other crops
    _check_teacher(filler, d2, 2, roi)
    assert not torch.equal(first[0], filler.image)


# ------------------------------------------------------------------------------------------------ 5. graph
def test_recorded_fill_follows_the_slot():
    """``fill`` recorded once in a graph; three replays after three slot loads (other volumes, codes and origins, the
    students' origins too) each equal the eager fill of the same draws."""
    from mivp_amd import batches as BT
    bank, _, _ = _bank(1)
    roi, sizes = (8, 8, 8), STUDENTS[:2]
    own = BT.BatchFiller(bank, roi, 5, student_sizes=sizes, active_labels=ACTIVE)
    ref = BT.BatchFiller(bank, roi, 5, student_sizes=sizes, active_labels=ACTIVE)
    loads = [_draws([0, 1, 2, 1, 0], [0, 1, 2, 3, 2], roi, "odd", sizes, "mix"),
             _draws([1, 1, 0, 2, 2], [2, 3, 1, 0, 1], roi, "hi", sizes, "hi"),
             _draws([2, 0, 1, 0, 1], [3, 2, 0, 1, 2], roi, "lo", sizes, "lo")]
    own.fill(loads[0])                                          # eager once: the source table and the slot exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        own.fill()
    names = ("image", "coord", "mask", "mask_st_0")
    for draws in loads[::-1]:
        own.slot.load(draws, bank, roi, sizes)
        _poison(own)
        graph.replay()
        ref.fill(draws)
        torch.cuda.synchronize()
        for n in names:
            assert torch.equal(getattr(own, n), getattr(ref, n)), n
        for i in range(len(sizes)):
            assert torch.equal(own.image_st[i], ref.image_st[i]) and torch.equal(own.coord_st[i], ref.coord_st[i])
        _check_teacher(own, draws, 1, roi)


def test_a_recorded_fill_sees_volumes_added_later():
    """The source table is one fixed allocation written in place: a graph recorded when the bank held one volume keeps a
    valid table and serves draws of volumes added afterwards."""
    from mivp_amd import batches as BT
    _, images, labels = _bank(1)
    bank = BT.VolumeBank(DEV, 1, capacity=4)
    bank.add(images[0], labels[0])
    table = bank.table.data_ptr()
    roi = (8, 8, 8)
    filler = BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, with_coord=True)
    filler.fill(_draws([0, 0], [0, 2], roi, "odd"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        filler.fill()
    with pytest.raises(ValueError, match="sample 1"):
        filler.slot.load(_draws([0, 1], [0, 0], roi, "lo"), bank, roi)    # volume 1 does not exist yet
    bank.add(images[1], labels[1])
    bank.add(images[2])
    assert bank.table.data_ptr() == table and len(bank) == 3
    for volume, rot in (([1, 2], [3, 1]), ([2, 0], [2, 0])):
        draws = _draws(volume, rot, roi, "hi")
        filler.slot.load(draws, bank, roi)
        _poison(filler)
        graph.replay()
        want = R.teacher_batch(images, [labels[0], labels[1], None], draws, roi, ACTIVE, _grid)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((filler.image, filler.mask, filler.coord), want))
    bank.add(images[0])
    with pytest.raises(ValueError, match="full"):
        bank.add(images[1])


# ------------------------------------------------------------------------------------------------ 6. feeding a recorded step
def test_fill_feeds_a_recorded_train_step():
    """The smallest ``downstream`` configuration of tests/test_hip_graph.py ("tiny"): a ``graphed_train_step`` recorded on the
    filler's tensors, a ``fill`` before each of two replays, against two eager ``train_step`` calls on clones of the same
    crops.  That file compares graph and eager with equality (test_hip_graph.py:66-67), so this does too."""
    from mivp_amd import batches as BT, train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, size, batch = train.make_conf("tiny")
    assert conf.training_mode == "downstream"
    g = torch.Generator().manual_seed(3)
    bank = BT.VolumeBank(DEV, conf.input_channels)
    shapes = [(size + 5, size + 2, size + 9), (size, size + 7, size + 1)]
    for s in shapes:
        bank.add(torch.rand((conf.input_channels,) + s, generator=g).to(DEV),
                 torch.randint(0, 4, s, generator=g, dtype=torch.uint8).to(DEV))
    roi = (size, size, size)
    filler = BT.BatchFiller(bank, roi, batch, active_labels=list(range(conf.output_channels_downstream)))
    rs = np.random.RandomState(5)
    draws = [BT.draw_crops(rs, bank.shapes, [i % 2] * batch, roi, 1, random_orientation=True) for i in range(4)]
    torch.manual_seed(5)
    ref = SwinUnetR(conf).to(DEV).train()
    own = copy.deepcopy(ref)
    o_ref = train.build_optimizer(ref, conf)
    o_own = train.build_optimizer(own, conf, capturable=True)
    x, y = filler.xy
    filler.fill(draws[0])                                       # the two warm-up steps of the recording run on these crops
    x0, y0 = x.clone(), y.clone()
    step = train.graphed_train_step(own, o_own, conf, x, y, warmup=2)
    for _ in range(2):
        train.train_step(ref, o_ref, conf, x0, y0)
    for d in draws[1:3]:
        filler.fill(d)
        l_own = float(step())
        l_ref = float(train.train_step(ref, o_ref, conf, x.clone(), y.clone()))
        assert l_own == l_ref
    torch.cuda.synchronize()
    assert y.max() <= conf.output_channels_downstream - 1
    assert [k for k, v in ref.state_dict().items() if not torch.equal(v, own.state_dict()[k])] == []


# ------------------------------------------------------------------------------------------------ 7. host refusals
def test_bad_draws_and_bad_outputs_are_refused_before_any_launch():
    from mivp_amd import batches as BT
    bank, _, _ = _bank(1)
    roi = (8, 8, 8)
    good = _draws([0, 1, 2], [0, 2, 3], roi, "hi")
    slot = BT.CropSlot(3, 0, DEV)
    slot.load(good, bank, roi)
    torch.cuda.synchronize()
    before = slot.records.clone()
    for field, index, value in (("volume", 1, 3), ("volume", 0, -1), ("rot", 2, 4), ("origin", (0, 2), 14),
                                ("origin", (1, 0), -1)):
        bad = copy.deepcopy(good)
        getattr(bad, field)[index] = value
        with pytest.raises(ValueError, match="sample"):
            slot.load(bad, bank, roi)
    with pytest.raises(ValueError, match="batch"):
        slot.load(_draws([0, 1], [0, 0], roi, "lo"), bank, roi)
    torch.cuda.synchronize()
    assert torch.equal(slot.records, before) and slot.draws is good          # nothing was uploaded

    filler = BT.BatchFiller(bank, roi, 3, with_coord=True)
    with pytest.raises(ValueError, match="no draws"):
        filler.fill()
    with pytest.raises(ValueError, match="sample 1"):
        bad = copy.deepcopy(good)
        bad.volume[1] = 7
        filler.fill(bad)
    with pytest.raises(ValueError):
        filler.fill(BT.CropSlot(2, 0, DEV))
    with pytest.raises(ValueError, match="another bank"):
        other = BT.CropSlot(3, 0, DEV)
        other.load(good, bank, (8, 8, 4))
        filler.fill(other)
    for name, wrong in (("image", torch.zeros(3, 1, 8, 8, 4, device=DEV)),
                        ("mask", torch.zeros(3, 1, 8, 8, 8, device=DEV, dtype=torch.float16)),
                        ("coord", torch.zeros(3, 3, 8, 8, 8)),
                        ("image", torch.zeros(3, 1, 8, 8, 16, device=DEV)[..., ::2])):
        keep = getattr(filler, name)
        setattr(filler, name, wrong)
        with pytest.raises(ValueError, match=name):
            filler.fill(good)
        setattr(filler, name, keep)
    filler.fill(good)                                           # and the filler still works
    torch.cuda.synchronize()
    assert torch.equal(filler.image, R.teacher_batch(_bank(1)[1], _bank(1)[2], good, roi)[0])

    with pytest.raises(ValueError):
        bank.add(torch.zeros(2, 4, 4, 4, device=DEV))           # the bank's channel count is 1
    with pytest.raises(ValueError):
        bank.add(torch.zeros(1, 4, 4, 4, device=DEV), torch.zeros(4, 4, 4, device=DEV))      # labels must be uint8
    with pytest.raises(RuntimeError):
        bank.add(torch.zeros(1, 4, 4, 4))                       # no CPU fallback
    assert len(bank) == 3
    late = torch.zeros(1, 4, 4, 4, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        filler.fill()                                           # recording a fill is fine, growing the bank is not
        with pytest.raises(RuntimeError, match="recorded"):
            bank.add(late)
    assert len(bank) == 3


# ------------------------------------------------------------------------------------------------ 8. device refusals
@pytest.mark.parametrize("entry", ["mivp_crop_fill", "mivp_crop_fill_affine", "mivp_crop_pick"])
def test_an_empty_row_and_a_wild_code_leave_the_sample_unwritten(entry):
    """The two fills decode the slot record and the table row through csrc/crops_common.hpp, the pick with its own code.  Called
    raw on records the host checks refuse: a bank of capacity 2 that holds one (6, 8, 5) volume, roi (4, 4, 4), B = 3 -- a
    valid record, one with volume id 1 (the empty row) and one with code 7.  Sample 0 equals the restatement, samples 1 and
    2 stay as prefilled (NaN; -7 in the origin words for the pick).  Documented returns of the kernels, not faults."""
    from mivp_amd import _lib as L, batches as BT
    from mivp_amd._host import i3
    shape, roi, ncls = SHAPES[2], (4, 4, 4), 3
    g = torch.Generator().manual_seed(41)
    image = torch.arange(1, 1 + int(np.prod(shape)), dtype=torch.float32).reshape((1,) + shape).to(DEV)
    lab = torch.randint(0, 8, shape, generator=g, dtype=torch.uint8)
    labels = lab.to(DEV)
    bank = BT.VolumeBank(DEV, 1, capacity=2)
    bank.add(image, labels)
    records = torch.tensor([[0, 1, 1, 2, 1], [1, 0, 0, 0, 0], [0, 7, 0, 0, 0]], dtype=torch.int32)
    if entry == "mivp_crop_pick":
        index = BT.ClassIndex(bank, ncls, ACTIVE).update()
        records[:, 2:] = -7
        slot = records.to(DEV)
        picks = torch.tensor([[1, 0], [0, 0], [0, 0]], dtype=torch.int32, device=DEV)
        assert int(index.counts[0][1]) >= 1
        L.call("mivp_crop_pick", L.ptr(bank.table), L.ptr(index.table), bank.capacity, L.ptr(index.lut), ncls, L.ptr(slot), 5,
               L.ptr(picks), 3, i3(roi), L.stream())
        got = slot.cpu().numpy()
        assert got[0, 2:].tolist() == CR.origin(lab.numpy(), BT.label_table(ACTIVE), ncls, 1, 1, 0, roi)[0]
        assert got[1:].tolist() == [[1, 0, -7, -7, -7], [0, 7, -7, -7, -7]]
        return
    slot = records.to(DEV)
    lut = torch.from_numpy(BT.label_table(ACTIVE)).to(DEV)
    outs = [torch.full((3, c) + roi, float("nan"), device=DEV) for c in (1, 1, 3)]
    table, rec, r3, st = L.ptr(bank.table), L.ptr(slot), i3(roi), L.stream()

    def plain_fill(image, mask, coord):
        L.call("mivp_crop_fill", table, bank.capacity, 1, rec, 5, 3, r3, L.ptr(lut), L.ptr(image), L.ptr(mask), L.ptr(coord), st)

    if entry == "mivp_crop_fill":
        plain_fill(*outs)
    else:
        maps = torch.from_numpy(BT.SpatialDraws.identity(3).affine.reshape(-1)).to(DEV)
        L.call("mivp_crop_fill_affine", table, bank.capacity, 1, rec, 5, L.ptr(maps), 3, r3, L.ptr(lut), L.ptr(outs[0]),
               L.ptr(outs[1]), L.ptr(outs[2]), st)
    draws = BT.CropDraws(np.zeros(1, np.int32), np.ones(1, np.int32), np.asarray([[1, 2, 1]], np.int32),
                         np.zeros((0, 1, 3), np.int32)).check([shape], roi)
    want = R.teacher_batch([image], [labels], draws, roi, ACTIVE, _grid)
    torch.cuda.synchronize()
    for name, t, ref in zip(("image", "mask", "coord"), outs, want):
        assert torch.equal(t[:1], ref), f"{name}: sample 0 differs from the restatement"
        assert torch.isnan(t[1:]).all(), f"{name}: a refused sample was written"
    if entry == "mivp_crop_fill_affine":                        # the identity map: the plain fill's bits
        plain = [torch.full_like(t, float("nan")) for t in outs]
        plain_fill(*plain)
        torch.cuda.synchronize()
        assert all(torch.equal(a[:1], b[:1]) and torch.isnan(b[1:]).all() for a, b in zip(outs, plain))
