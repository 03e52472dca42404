"""GPU tests of the students' corruption of the batch filler (mivp_amd.batches with ``corruption=True``;
csrc/crops_corrupt.hip) against the numpy restatement in tests/corrupt_crops_ref.py, BIT for bit: the reference is applied
to the student tensors of the same fill without corruption.  tests/test_corrupt_crops_host.py shows the reference's
permutation to be a bijection and its modes to keep what they must; the properties are asserted here again on the device's
own output."""
import numpy as np
import pytest
import torch

import corrupt_crops_ref as CR
from batch_outputs import outs as _outs, poison as _poison

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(20, 18, 14), (18, 20, 15), (21, 19, 14)]
ACTIVE = [1, 2]
ROI, SIZES, B = (16, 12, 10), [(12, 10, 9), (7, 8, 5)], 3          # D extents 9 and 5: the vector tail runs
_state = {}


def _bank(channels, constant=None):
    from mivp_amd import batches as BT
    key = (channels, constant)
    if key not in _state:
        rs = np.random.RandomState(41 + channels)
        bank = BT.VolumeBank(DEV, channels)
        for shape in SHAPES:
            img = rs.uniform(-3, 7, (channels,) + shape).astype(np.float32) if constant is None \
                else np.full((channels,) + shape, constant, np.float32)
            bank.add(torch.from_numpy(img).to(DEV), torch.from_numpy(rs.randint(0, 4, shape).astype(np.uint8)).to(DEV))
        _state[key] = bank
    return _state[key]


def _crops(rs, roi, sizes, codes=(0, 1, 0)):
    """CropDraws of volumes 0, 1, 2, volume 1 stored rotated (code 1), uniform valid origins."""
    from mivp_amd import batches as BT
    n = len(codes)
    origin = np.zeros((n, 3), np.int32)
    for b in range(n):
        n_rot = BT.rotated_shape(SHAPES[b], codes[b])
        origin[b] = [rs.randint(0, max(n_rot[k] - roi[k], 0) + 1) for k in range(3)]
    st = np.zeros((len(sizes), n, 3), np.int32)
    for s, size in enumerate(sizes):
        st[s] = [[rs.randint(0, max(roi[k] - size[k], 0) + 1) for k in range(3)] for _ in range(n)]
    return BT.CropDraws(np.arange(n, dtype=np.int32), np.asarray(codes, np.int32), origin, st).check(SHAPES, roi, sizes)


def _holes(ext, rs):
    """Three samples' hole lists [(origin, size)] inside ``ext``: 0 -- two overlapping holes at odd origins and a 1-voxel
    hole in the last corner; 1 -- the whole student; 2 -- eight holes, the first clipped to the extent along D (what
    ``min(draw, extent)`` gives), the others small and random (overlaps among them are likely)."""
    a = [((1, 3, 1), (ext[0] // 2, ext[1] // 2, ext[2] // 2 + 1)), ((3, 1, 1), (ext[0] // 2, ext[1] // 2 + 1, ext[2] - 2)),
         (tuple(e - 1 for e in ext), (1, 1, 1))]
    b = [((0, 0, 0), tuple(ext))]
    c = [((1, 1, 0), (3, 2, ext[2]))]
    for _ in range(7):
        e = [int(rs.randint(1, min(5, ext[k]) + 1)) for k in range(3)]
        c.append((tuple(int(rs.randint(0, ext[k] - e[k] + 1)) for k in range(3)), tuple(e)))
    return [a, b, c]


def _draws(modes, sizes, seed, holes=None):
    """CorruptionDraws with ``modes`` [S][B] and, per (student, sample), the holes of ``_holes`` (or ``holes[s][b]``)."""
    from mivp_amd import batches as BT
    rs = np.random.RandomState(seed)
    d = BT.CorruptionDraws.identity(len(modes[0]), len(sizes))
    for s, ext in enumerate(sizes):
        lists = holes[s] if holes is not None else _holes(ext, rs)
        for b, hs in enumerate(lists):
            d.mode[s, b], d.n_holes[s, b] = modes[s][b], len(hs)
            d.key[s, b] = rs.randint(0, 2 ** 32, dtype=np.uint32)
            for k, (o, e) in enumerate(hs):
                d.origin[s, b, k], d.size[s, b, k] = o, e
                d.hole_key[s, b, k] = rs.randint(0, 2 ** 32, dtype=np.uint32)
    return d.check(len(modes[0]), sizes)


def _np(tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


CASES = {"dropout": [[1, 1, 1], [1, 1, 1]], "keep": [[2, 2, 2], [2, 2, 2]], "shuffle": [[3, 3, 3], [3, 3, 3]],
         "mixed": [[0, 1, 3], [2, 3, 0]]}


def _run(case, channels):
    """One fill of the plain filler and one of the corrupting one on the same crops -> (draws, plain student images,
    corrupted student images, plain other outputs, corrupted other outputs), cached."""
    from mivp_amd import batches as BT
    key = ("run", case, channels)
    if key not in _state:
        bank = _bank(channels)
        plain = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE)
        own = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, corruption=True)
        assert plain.corruption_slot is None and not own.corruption_slot.buffer.any()      # every record mode 0 at first
        crops = _crops(np.random.RandomState(7), ROI, SIZES)
        cd = _draws(CASES[case], SIZES, 100 + len(case))
        plain.fill(crops)
        _poison(own)
        assert own.fill(crops, corruption=cd) is own.batch and own.corruption_slot.draws is cd
        others = lambda f: [f.image, f.mask, f.coord, f.mask_st_0] + f.coord_st
        _state[key] = (cd, _np(plain.image_st), _np(own.image_st), _np(others(plain)), _np(others(own)))
    return _state[key]


# ------------------------------------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize("case,channels", [("dropout", 1), ("keep", 1), ("shuffle", 1), ("mixed", 2), ("shuffle", 2)])
def test_bit_equal_to_the_reference_on_the_plain_students(case, channels):
    cd, before, after, others_plain, others_own = _run(case, channels)
    for s in range(len(SIZES)):
        want = CR.corrupt_student(before[s], cd, s)
        assert not np.isnan(after[s]).any(), (s, "a student voxel was not written")
        differ = after[s].view(np.uint32) != want.view(np.uint32)
        assert not differ.any(), (case, s, int(differ.sum()), np.argwhere(differ)[:4].tolist())
        for b in range(B):                                          # (keep around a hole that is the whole student acts nowhere)
            idle = int(cd.mode[s, b]) == 0 or (int(cd.mode[s, b]) == 2 and CR.union_mask(SIZES[s], CR.holes_of(cd, s, b)).all())
            assert idle == _bits(after[s][b], before[s][b]), (s, b)
    # coord_st, mask_st_0 and the teacher's tensors carry the uncorrupted filler's bits
    assert all(_bits(a, b) for a, b in zip(others_plain, others_own))


# ------------------------------------------------------------------------------------------------ 2. the properties
def test_voxels_that_must_stay_keep_their_bits_and_noise_lies_in_the_range():
    for case, channels in (("dropout", 1), ("keep", 1), ("shuffle", 1), ("mixed", 2)):
        cd, before, after, _, _ = _run(case, channels)
        for s in range(len(SIZES)):
            for b in range(B):
                mode = int(cd.mode[s, b])
                inside = CR.union_mask(SIZES[s], CR.holes_of(cd, s, b))
                x, y = before[s][b], after[s][b]
                if mode in (1, 3):
                    assert _bits(y[:, ~inside], x[:, ~inside]), (case, s, b)
                if mode == 2:
                    assert _bits(y[:, inside], x[:, inside]), (case, s, b)
                if mode in (1, 2):
                    fresh = y[:, inside] if mode == 1 else y[:, ~inside]
                    lo, hi = x.min(), x.max()
                    assert fresh.size or (mode == 2 and inside.all())
                    assert (fresh >= lo).all() and (fresh < hi).all(), (case, s, b)
                    assert len(np.unique(fresh)) >= 0.9 * fresh.size        # noise, not a fill value


def test_shuffle_keeps_the_multiset_of_each_disjoint_hole_per_channel():
    from mivp_amd import batches as BT
    bank = _bank(2)
    holes = [[[((0, 0, 0), (5, 4, 3)), ((5, 4, 3), (7, 6, 6)), ((0, 5, 4), (4, 5, 5))]] * B,
             [[((1, 1, 1), (3, 3, 3)), ((4, 4, 0), (3, 4, 5)), ((0, 0, 4), (1, 8, 1))]] * B]
    cd = _draws(CASES["shuffle"], SIZES, 5, holes)
    own = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, corruption=True)
    crops = _crops(np.random.RandomState(9), ROI, SIZES)
    own.fill(crops)
    before = _np(own.image_st)
    own.fill(corruption=cd)
    after = _np(own.image_st)
    for s in range(2):
        assert CR.union_mask(SIZES[s], CR.holes_of(cd, s, 0)).sum() == sum(int(np.prod(e)) for _, e in holes[s][0])   # disjoint
        for b in range(B):
            for o, e in holes[s][b]:
                sl = (slice(o[0], o[0] + e[0]), slice(o[1], o[1] + e[1]), slice(o[2], o[2] + e[2]))
                for c in range(2):
                    x, y = before[s][b, c][sl].reshape(-1), after[s][b, c][sl].reshape(-1)
                    assert _bits(np.sort(x), np.sort(y)) and (x.size < 4 or not _bits(x, y)), (s, b, o, c)
                moved = before[s][b, 0][sl].reshape(-1) != after[s][b, 0][sl].reshape(-1)
                assert np.array_equal(moved, before[s][b, 1][sl].reshape(-1) != after[s][b, 1][sl].reshape(-1))     # one permutation


def test_a_constant_student_gives_exactly_its_value():
    from mivp_amd import batches as BT
    bank = _bank(1, constant=2.5)
    roi, sizes = (12, 10, 9), [(12, 10, 9), (7, 8, 5)]              # inside every volume: no zero padding
    own = BT.BatchFiller(bank, roi, B, student_sizes=sizes, active_labels=ACTIVE, corruption=True)
    crops = _crops(np.random.RandomState(3), roi, sizes, codes=(0, 0, 0))
    _poison(own)
    own.fill(crops, corruption=_draws([[1, 2, 1], [2, 1, 2]], sizes, 17))
    for t in _np(own.image_st):
        assert (t == np.float32(2.5)).all()


# ------------------------------------------------------------------------------------------------ 3. a 16^3 shuffle hole
def test_a_shuffle_hole_of_exactly_4096_voxels():
    """roi (18, 17, 16), one student of (16, 16, 16): sample 0 shuffles the whole student and then a second, overlapping
    hole; sample 1 the whole student in dropout; sample 2 keeps a 16 x 16 x 1 slab."""
    from mivp_amd import batches as BT
    bank = _bank(1)
    roi, sizes = (18, 17, 16), [(16, 16, 16)]
    holes = [[[((0, 0, 0), (16, 16, 16)), ((3, 5, 7), (13, 11, 9))], [((0, 0, 0), (16, 16, 16))], [((0, 0, 15), (16, 16, 1))]]]
    cd = _draws([[3, 1, 2]], sizes, 23, holes)
    assert int(np.prod(cd.size[0, 0, 0])) == BT.MAX_SHUFFLE_VOXELS
    own = BT.BatchFiller(bank, roi, B, student_sizes=sizes, active_labels=ACTIVE, corruption=True)
    crops = _crops(np.random.RandomState(5), roi, sizes)
    own.fill(crops)
    before = _np(own.image_st)[0]
    _poison(own)
    own.fill(corruption=cd)
    after = _np(own.image_st)[0]
    assert _bits(after, CR.corrupt_student(before, cd, 0))
    assert _bits(np.sort(after[0].reshape(-1)), np.sort(before[0].reshape(-1))) and not _bits(after[0], before[0])
    assert (after[1] != before[1]).mean() > 0.99 and _bits(after[2][..., 15], before[2][..., 15])


# ------------------------------------------------------------------------------------------------ 4. mode 0, repeats
def test_an_all_zero_slot_gives_the_plain_fillers_bits_and_a_repeat_the_same_bits():
    from mivp_amd import batches as BT
    bank = _bank(2)
    plain = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE)
    own = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, corruption=True)
    crops = _crops(np.random.RandomState(11), ROI, SIZES)
    plain.fill(crops)
    _poison(own)
    own.fill(crops)                                                 # corruption=None: the slot as made
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_outs(plain), _outs(own)))
    own.fill(crops, corruption=BT.CorruptionDraws.identity(B, 2))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_outs(plain), _outs(own)))
    cd = _draws(CASES["mixed"], SIZES, 31)
    own.fill(corruption=cd)
    first = [t.clone() for t in _outs(own)]
    assert not all(torch.equal(a, b) for a, b in zip(_outs(plain), first))
    _poison(own)
    own.fill()                                                      # the same slots: the same bits
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, _outs(own)))


def test_a_malformed_record_on_the_device_leaves_its_sample_unwritten():
    """The host check refuses these; written straight into the slot they must still send no workgroup out of the tensor:
    the kernel checks every word it forms an address from and leaves the sample as the student crop made it."""
    from mivp_amd import batches as BT
    bank = _bank(1)
    plain = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE)
    own = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, corruption=True)
    crops = _crops(np.random.RandomState(13), ROI, SIZES)
    plain.fill(crops)
    cd = _draws(CASES["dropout"], SIZES, 37)
    words = cd.pack()
    words[0, 0, 0] = 5                                              # a mode above 3
    words[0, 1, 1] = 9                                              # more than 8 holes
    words[0, 2, 3 + 2] = 8                                          # hole 0 of sample 2: origin 8 + extent 9 along D
    words[1, 0, 3 + 3] = 0                                          # an empty hole
    words[1, 1, 0], words[1, 1, 3:9] = 1, (0, 0, 0, -1, 8, 5)       # a negative size
    own.corruption_slot.buffer.copy_(torch.from_numpy(words.reshape(-1)))
    own.fill(crops)
    torch.cuda.synchronize()
    assert torch.equal(own.image_st[0], plain.image_st[0])
    assert torch.equal(own.image_st[1][:2], plain.image_st[1][:2]) and not torch.equal(own.image_st[1][2], plain.image_st[1][2])


# ------------------------------------------------------------------------------------------------ 5. recording
def test_a_recorded_fill_follows_the_corruption_slot():
    from mivp_amd import batches as BT
    bank = _bank(2)
    own = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, corruption=True)
    ref = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, corruption=True)
    crops = _crops(np.random.RandomState(15), ROI, SIZES)
    first, other = _draws(CASES["mixed"], SIZES, 51), _draws([[3, 2, 1], [1, 0, 3]], SIZES, 52)
    own.fill(crops, corruption=first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        own.fill()
        own.corruption_slot.load(other)                             # does nothing while recording
    assert own.corruption_slot.draws is first
    for cd in (other, first):
        own.corruption_slot.load(cd)
        _poison(own)
        graph.replay()
        ref.fill(crops, corruption=cd)
        torch.cuda.synchronize()
        assert not any(torch.isnan(t).any() for t in _outs(own))
        assert all(torch.equal(a, b) for a, b in zip(_outs(own), _outs(ref)))
    mine = BT.CorruptionSlot(B, SIZES, DEV)                         # a slot of one's own is used as it stands
    mine.load(other)
    own.fill(crops, corruption=mine)
    ref.fill(crops, corruption=other)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_outs(own), _outs(ref)))
    assert own.corruption_slot.draws is first                       # and the filler's own slot was left alone


# ------------------------------------------------------------------------------------------------ 6. with the others
def test_composes_with_class_index_spatial_and_elastic():
    """The reference applied on top of the SAME filler's student tensors, filled once with every record at mode 0."""
    from mivp_amd import batches as BT
    bank = _bank(1)
    index = BT.ClassIndex(bank, 3, ACTIVE).update()
    nodes = (5, 4, 6)
    own = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, class_index=index, spatial=True,
                         elastic=nodes, corruption=True)
    rs = np.random.RandomState(19)
    crops = BT.draw_class_crops(rs, index, [0, 1, 2], ROI, 1, (1, 2, 1), True, SIZES)
    sp = BT.draw_spatial(rs, B, p_flip=(0.5, 0.5, 0.5), p_affine=1.0, rotate_range=(0.26, 0.26, 0.26), scale_range=(0.8, 1.25))
    ed = BT.draw_elastic(rs, B, ROI, nodes=nodes, p_elastic=1.0, magnitude_range=(0.5, 0.8), locked_borders=1)
    own.fill(crops, spatial=sp, elastic=ed)
    before, others = _np(own.image_st), _np([own.image, own.mask, own.coord, own.mask_st_0] + own.coord_st)
    cd = _draws(CASES["mixed"], SIZES, 61)
    _poison(own)
    own.fill(corruption=cd)
    after = _np(own.image_st)
    for s in range(2):
        assert _bits(after[s], CR.corrupt_student(before[s], cd, s)), s
        assert not _bits(after[s], before[s])
    assert all(_bits(a, b) for a, b in zip(others, _np([own.image, own.mask, own.coord, own.mask_st_0] + own.coord_st)))


def test_the_students_intensity_chain_takes_the_corrupted_students_in_place():
    """The recipe of DESIGN 4.30: ``augment_intensity`` accepts ``image_st[i]`` as it stands, one ``IntensitySlot`` per
    student; with no step fired it leaves the corrupted bits, with every step fired it changes the student alone."""
    from mivp_amd import augment as AU, batches as BT
    bank = _bank(1)
    own = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, corruption=True)
    own.fill(_crops(np.random.RandomState(25), ROI, SIZES), corruption=_draws(CASES["mixed"], SIZES, 81))
    before = [t.clone() for t in _outs(own)]
    slots = [AU.IntensitySlot(B, DEV) for _ in SIZES]
    for prob in (0.0, 1.0):
        for i, slot in enumerate(slots):
            slot.load(AU.draw_intensity(np.random.RandomState(90 + i), B, prob=prob, std_factors=(0.0, 0.2)))
            assert AU.augment_intensity(own.image_st[i], slot, out=own.image_st[i]) is own.image_st[i]
        torch.cuda.synchronize()
        same = [torch.equal(a, b) for a, b in zip(before, _outs(own))]
        students = [any(t is u for u in own.image_st) for t in _outs(own)]
        assert same == [True] * len(same) if prob == 0.0 else same == [not st for st in students]
        assert all(bool(torch.isfinite(t).all()) for t in own.image_st)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_come_before_any_launch_and_any_load():
    from mivp_amd import _lib as L, batches as BT
    from mivp_amd._host import i3
    bank = _bank(1)
    with pytest.raises(ValueError, match="corruption=True needs student_sizes"):
        BT.BatchFiller(bank, ROI, B, active_labels=ACTIVE, corruption=True)
    plain = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE)
    own = BT.BatchFiller(bank, ROI, B, student_sizes=SIZES, active_labels=ACTIVE, corruption=True)
    crops, other = _crops(np.random.RandomState(21), ROI, SIZES), _crops(np.random.RandomState(22), ROI, SIZES)
    good = _draws(CASES["mixed"], SIZES, 71)
    own.fill(crops, corruption=good)
    plain.fill(crops)
    torch.cuda.synchronize()
    before = [t.clone() for t in _outs(own) + _outs(plain)]
    records, buffer = own.slot.records.clone(), own.corruption_slot.buffer.clone()

    def broken(field, index, value):
        d = BT.CorruptionDraws(*(getattr(good, k).copy() for k in ("mode", "n_holes", "key", "origin", "size", "hole_key")))
        getattr(d, field)[index] = value
        return d

    cases = [(plain, good, "built with corruption=True"),
             (plain, BT.CorruptionSlot(B, SIZES, DEV), "built with corruption=True"),
             (own, broken("mode", (0, 1), 4), "student 0: sample 1: mode 4"),
             (own, broken("n_holes", (1, 0), 9), "student 1: sample 0: n_holes 9"),
             (own, broken("origin", (0, 1, 0, 2), 1), "student 0: sample 1: hole 0 .* outside"),
             (own, BT.CorruptionDraws.identity(B + 1, 2), r"int32 \[2, 3\]"),
             (own, BT.CorruptionDraws.identity(B, 1), r"int32 \[2, 3\]"),
             (own, BT.CorruptionSlot(B + 1, SIZES, DEV), "corruption slot of batch 4"),
             (own, BT.CorruptionSlot(B, SIZES[::-1], DEV), "corruption slot of batch 3"),
             (own, BT.CorruptionSlot(B, SIZES[:1], DEV), "corruption slot of batch 3"),
             (own, np.zeros(3), "CorruptionDraws, a CorruptionSlot")]
    if torch.cuda.device_count() > 1:
        cases.append((own, BT.CorruptionSlot(B, SIZES, "cuda:1"), "corruption slot of batch 3"))
    for f, c, match in cases:
        with pytest.raises(ValueError, match=match):
            f.fill(other, corruption=c)                             # new crop draws too: they may not be loaded either
    with pytest.raises(ValueError, match="student 1: sample 0"):
        own.corruption_slot.load(broken("n_holes", (1, 0), 9))
    with pytest.raises(ValueError, match="CorruptionDraws expected"):
        own.corruption_slot.load(crops)
    # the C entries: null and misaligned pointers and bad sizes are refused on the host with MIVP_EINVAL (-1)
    x, rec, rng = L.ptr(own.image_st[0]), L.ptr(own.corruption_slot.records[0]), L.ptr(own.corruption_range[0])

    def refused(x_, c_, dims_, rec_, b_, rng_):
        with pytest.raises(RuntimeError, match="mivp_crop_corrupt_range failed with code -1"):
            L.call("mivp_crop_corrupt_range", x_, c_, dims_, rec_, b_, rng_, L.stream())
        with pytest.raises(RuntimeError, match="mivp_crop_corrupt failed with code -1"):
            L.call("mivp_crop_corrupt", x_, c_, dims_, rec_, b_, rng_, L.stream())

    ok = i3(SIZES[0])
    for args in ((None, 1, ok, rec, B, rng), (x, 1, ok, None, B, rng), (x, 1, ok, rec, B, None), (x + 2, 1, ok, rec, B, rng),
                 (x, 1, ok, rec + 1, B, rng), (x, 1, ok, rec, B, rng + 2), (x, 0, ok, rec, B, rng), (x, 17, ok, rec, B, rng),
                 (x, 1, i3((12, 0, 9)), rec, B, rng), (x, 1, ok, rec, 0, rng), (x, 1, None, rec, B, rng)):
        refused(*args)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, _outs(own) + _outs(plain)))
    assert torch.equal(records, own.slot.records) and own.slot.draws is crops and plain.slot.draws is crops
    assert torch.equal(buffer, own.corruption_slot.buffer) and own.corruption_slot.draws is good
