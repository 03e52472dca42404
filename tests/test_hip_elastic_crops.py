"""GPU tests of the elastic deformation of the batch filler (mivp_amd.batches with ``spatial=True, elastic=nodes``; the
second kernel of csrc/crops_affine.hip) against the numpy float64 restatement in tests/elastic_crops_ref.py, which
tests/test_elastic_crops_host.py pins to scipy's basis and to the affine restatement.  A zero lattice and a flag of 0 are
compared bit for bit with the ``spatial=True`` filler; a linear lattice with the AFFINE restatement under the composed map
and a general lattice with the elastic one, within bounds derived from fp32's step (tests/elastic_cases.py: ``bounds``).
The bank is that of test_hip_spatial_crops.py (its first three volumes)."""
import numpy as np
import pytest
import torch

import class_crops_ref as CR
import crops_ref as R
import elastic_cases as EC
import elastic_crops_ref as ER
import spatial_crops_ref as SR
from batch_outputs import outs as _outs, poison as _poison

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES, ACTIVE, NCLS = EC.SHAPES, EC.ACTIVE, 3
ROIS = [(8, 12, 5), (12, 10, 20), (9, 10, 70)]       # the last: several bricks along d, partial ones on every axis
TYPICAL = dict(p_flip=(0.5, 0.5, 0.5), p_affine=1.0, rotate_range=(0.26, 0.26, 0.26), scale_range=(0.8, 1.25),
               isotropic=False, shift=True)
_state = {}


def _bank(channels, integer=True):
    """(VolumeBank, numpy images, numpy labels)."""
    from mivp_amd import batches as BT
    key = (channels, integer)
    if key not in _state:
        images, labels = EC.bank_arrays(channels, integer)
        bank = BT.VolumeBank(DEV, channels)
        for img, lab in zip(images, labels):
            bank.add(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV))
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


def _fixed(code, B):
    """CropDraws of B samples of volume 0 at the general case's origin under ``code``."""
    from mivp_amd import batches as BT
    return BT.CropDraws(np.zeros(B, np.int32), np.full(B, code, np.int32), np.asarray([EC.GENERAL_ORIGINS[code]] * B, np.int32),
                        np.zeros((0, B, 3), np.int32)).check(SHAPES, EC.ROI)


def _teacher(f):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (f.image, f.mask, f.coord)]


def _equal_samples(own, ref, samples, what):
    for name in ("image", "mask", "coord"):
        a, b = getattr(own, name)[samples], getattr(ref, name)[samples]
        assert not torch.isnan(a).any(), (what, name, "an output voxel was not written")
        assert torch.equal(a, b), (what, name, int((a != b).sum()))


def _assert_within(got, want, delta_r, span, what):
    """The bounds of the general case for the samples handed in: (image, mask, coord) against (image, mask, coord, r)."""
    assert not any(np.isnan(g).any() for g in got), (what, "an output voxel was not written")
    err_i, err_c = np.abs(got[0] - want[0]).max(), np.abs(got[2] - want[2]).max()
    near = EC.near_tie(want[3], delta_r)
    differ = (got[1][:, 0] != want[1][:, 0]) & ~near
    print(f"{what}: image err {err_i:.3e} (bound {(3 * delta_r + 8 * EC.EPS) * span:.3e}), coord err {err_c:.3e} (bound "
          f"{2 * delta_r:.3e}), mask left out {near.mean():.5f}, differing {int(differ.sum())}")
    assert err_i <= (3 * delta_r + 8 * EC.EPS) * span
    assert err_c <= 2 * delta_r
    assert near.mean() <= 0.01 and not differ.any()


# ------------------------------------------------------------------------------------------------ 1. d = 0 and flag 0
@pytest.mark.parametrize("nodes", [(7, 7, 7), (4, 5, 8)])
def test_zero_lattice_and_flag_zero_are_bit_equal_to_the_spatial_fill(nodes):
    """Samples 0 and 2 carry flag 1 and a lattice of zeros (d = +0: q + d = q), samples 1 and 3 flag 0 and a lattice of
    NaN written straight into the slot (the host check would refuse it): were it read, r would be NaN and the sample zeros."""
    from mivp_amd import batches as BT
    bank, _, _ = _bank(2)
    rs = np.random.RandomState(3)
    flags = np.asarray([1, 0, 1, 0], np.int32)
    for roi in ROIS + [(24, 10, 40)]:                               # the last is larger than volume 0 on two axes
        ref = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, spatial=True)
        own = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, spatial=True, elastic=nodes)
        assert ref.elastic_slot is None and own.elastic_slot.nodes == nodes
        assert not own.elastic_slot.flags.any() and not own.elastic_slot.lattice.any()      # the identity at first
        assert own.elastic_slot.lattice.shape == (4 * 3 * int(np.prod(nodes)),) and own.elastic_slot.flags.dtype == torch.int32
        for code in range(4):
            d = _draws(rs, [0, 1, 2, 0], [code] * 4, roi)
            sp = BT.draw_spatial(rs, 4, **TYPICAL)
            ref.fill(d, spatial=sp)
            _poison(own)
            own.fill(d, spatial=sp)                                 # elastic=None: the slot as made, nothing deformed
            torch.cuda.synchronize()
            _equal_samples(own, ref, slice(None), (roi, code, "the slot as made"))
            own.elastic_slot.load(BT.ElasticDraws(flags, np.zeros((4, 3) + nodes, np.float32)))
            own.elastic_slot.lattice.view(4, -1)[1::2] = float("nan")
            _poison(own)
            own.fill(d, spatial=sp)
            torch.cuda.synchronize()
            assert own.elastic_slot.flags.tolist() == [1, 0, 1, 0] and torch.isnan(own.elastic_slot.lattice.view(4, -1)[1::2]).all()
            _equal_samples(own, ref, slice(None), (roi, code))
            own.elastic_slot.load(BT.ElasticDraws.identity(4, nodes))
        assert (ref.image != 0).any() and (ref.mask > 0).any()


# ------------------------------------------------------------------------------------------------ 2. a linear lattice
@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_linear_lattice_equals_the_affine_restatement_under_the_composed_map(code):
    """P[c][j] = alpha_c j_c: the spline is affine in u, so the AFFINE restatement under the composed map is an independent
    reference (test_elastic_crops_host.py).  Nodes (6, 8, 8) on roi (12, 10, 20), dyadic alpha and A and shifts that are odd
    multiples of 2^-16 keep the composed words exact in fp32 and r + 0.5 off the integers.  Bounds: those of the general
    case with max|P| = 2.5."""
    from mivp_amd import batches as BT
    bank, images, labels = _bank(2, integer=False)
    roi, nodes, alpha = EC.ROI, (6, 8, 8), (0.5, -0.25, 0.25)
    affine = np.zeros((2, 12), np.float32)
    affine[:, :9] = np.asarray([[[0.5, 0.125, 0], [0, 1.25, 0], [0, 0, 1]], [[1, 0, 0.125], [0, -0.5, 0], [0.25, 0, 1.25]]]).reshape(2, 9)
    affine[:, 9:] = (np.floor(np.asarray([[0.3, -0.45, 0.2], [-0.15, 0.4, 0.33]]) * 32768) * 2 + 1) / 65536
    P = ER.linear_lattice(alpha, nodes).astype(np.float32)
    composed = np.stack([ER.composed_affine(a, alpha, nodes, roi) for a in affine])
    assert np.array_equal(composed.astype(np.float32).astype(np.float64), composed) and np.abs(P).max() == 2.5
    d = _fixed(code, 2)
    own = BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, with_coord=True, spatial=True, elastic=nodes)
    _poison(own)
    own.fill(d, spatial=BT.SpatialDraws(affine).check(2), elastic=BT.ElasticDraws(np.ones(2, np.int32), np.stack([P, P])).check(2, nodes))
    got = _teacher(own)
    want = SR.teacher_batch(images, labels, _lut(), d.volume, d.rot, d.origin, roi, composed.astype(np.float32))
    plain = SR.teacher_batch(images, labels, _lut(), d.volume, d.rot, d.origin, roi, affine)
    assert np.abs(want[3] - plain[3]).max() > 1.0                   # the lattice moved the crop by more than a voxel
    delta_d, delta_r = EC.bounds(affine, 2.5)
    assert delta_r < 1e-3
    span = float(images[0].max() - images[0].min())
    _assert_within(got, want, delta_r, span, f"linear, code {code}")
    assert (want[1] > 0).any() and (want[0] != 0).any()


# ------------------------------------------------------------------------------------------------ 3. the general case
@pytest.mark.parametrize("nodes", EC.GENERAL_NODES)
@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_general_lattice_within_fp32_bounds(code, nodes):
    """Volume (20, 18, 36), roi (12, 10, 20), B = 2, the affine map of the existing general test (angles (0.3, -0.2, 0.5),
    zooms (1.1, 0.9, 1.05)), lattices of non-dyadic values in +-2 voxels.  delta_d = K 2^-24 max|P| with K = 160 counted from
    the kernel's evaluation order (60 for the two roundings of x_k, 48 for the basis weights, 21 for the sums: 129, and room
    for the second-order terms; written out at elastic_cases.bounds), delta_r = delta + (max row sum of |A|) delta_d with the
    existing test's delta = 8 * 2^-24 * 36.  The image may move by delta_r times one value range per axis plus its own
    rounding, coord by 2 delta_r, and the mask may differ only where r + 0.5 is within delta_r of an integer -- at most 1 %
    of the voxels, which test_elastic_crops_host.py shows the reference to meet by itself on these inputs.  delta_r < 1e-3:
    a wrong basis or an index off by one moves r by a fraction of a voxel and cannot pass."""
    from mivp_amd import batches as BT
    bank, images, labels = _bank(2, integer=False)
    roi = EC.ROI
    affine, lattice = EC.general_affine(), EC.general_lattice(nodes, code)
    d = _fixed(code, 2)
    own = BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, with_coord=True, spatial=True, elastic=nodes)
    _poison(own)
    own.fill(d, spatial=BT.SpatialDraws(affine).check(2), elastic=BT.ElasticDraws(np.ones(2, np.int32), lattice).check(2, nodes))
    got = _teacher(own)
    want = ER.teacher_batch(images, labels, _lut(), d.volume, d.rot, d.origin, roi, affine, [1, 1], lattice)
    delta_d, delta_r = EC.bounds(affine, EC.MAX_P)
    assert delta_d == 160 * 2.0 ** -24 * 2.0 and delta_r < 1e-3
    span = float(images[0].max() - images[0].min())
    _assert_within(got, want, delta_r, span, f"general, code {code}, nodes {nodes}")
    inside = np.stack([SR.nearest_inside(want[3][b], BT.rotated_shape(SHAPES[0], code))[1] for b in range(2)])
    assert 0.5 < inside.mean() < 1.0 and (want[1] > 0).any()        # the zero rule is exercised but does not dominate
    plain = SR.teacher_batch(images, labels, _lut(), d.volume, d.rot, d.origin, roi, affine)
    assert np.abs(want[3] - plain[3]).max() > 0.2                   # and the lattice did move the positions


# ------------------------------------------------------------------------------------------------ 4. out of the volume
def test_a_displacement_out_of_the_volume_gives_zeros_and_disturbs_nothing_else():
    from mivp_amd import batches as BT
    bank, images, labels = _bank(2)
    roi, nodes = (9, 10, 70), (5, 4, 7)
    ref = BT.BatchFiller(bank, roi, 3, active_labels=ACTIVE, with_coord=True, spatial=True)
    own = BT.BatchFiller(bank, roi, 3, active_labels=ACTIVE, with_coord=True, spatial=True, elastic=nodes)
    rs = np.random.RandomState(23)
    lattice = np.zeros((3, 3) + nodes, np.float32)
    lattice[1] = 1e4
    ed = BT.ElasticDraws(np.asarray([0, 1, 0], np.int32), lattice).check(3, nodes)
    for code in range(4):
        d = _draws(rs, [0, 1, 0], [code] * 3, roi)
        sp = BT.draw_spatial(rs, 3, **TYPICAL)
        want = ER.teacher_batch(images, labels, _lut(), d.volume, d.rot, d.origin, roi, sp.affine, ed.flags, ed.lattice)
        assert not want[0][1].any() and not want[1][1].any() and not want[2][1].any() and np.abs(want[3][1]).min() > 100
        ref.fill(d, spatial=sp)
        _poison(own)
        own.fill(d, spatial=sp, elastic=ed)
        torch.cuda.synchronize()
        for name in ("image", "mask", "coord"):
            assert not getattr(own, name)[1].any(), (code, name)    # zeros, not NaN: every voxel was written
        _equal_samples(own, ref, [0, 2], code)
        assert (ref.image[1] != 0).any()


# ------------------------------------------------------------------------------------------------ 5. a mixed batch
def test_mixed_batch_flag_zero_keeps_the_spatial_bits():
    from mivp_amd import batches as BT
    bank, images, labels = _bank(2, integer=False)
    roi, nodes = EC.ROI, (5, 4, 7)
    ref = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, spatial=True)
    own = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, spatial=True, elastic=nodes)
    affine = np.concatenate([EC.general_affine(), EC.general_affine()])
    lattice = np.concatenate([EC.general_lattice(nodes, 0), EC.general_lattice(nodes, 1)])
    ed = BT.ElasticDraws(np.asarray([1, 0, 1, 0], np.int32), lattice).check(4, nodes)
    sp = BT.SpatialDraws(affine).check(4)
    span = float(images[0].max() - images[0].min())
    _, delta_r = EC.bounds(affine, EC.MAX_P)
    for code in range(4):
        d = _fixed(code, 4)
        ref.fill(d, spatial=sp)
        _poison(own)
        own.fill(d, spatial=sp, elastic=ed)
        got = _teacher(own)
        _equal_samples(own, ref, [1, 3], code)
        want = ER.teacher_batch(images, labels, _lut(), d.volume, d.rot, d.origin, roi, affine, ed.flags, lattice)
        _assert_within([g[0::2] for g in got], [w[0::2] for w in want], delta_r, span, f"mixed, code {code}")
        assert not torch.equal(own.image[0], ref.image[0])          # and the flagged samples were deformed


# ------------------------------------------------------------------------------------------------ 6. students, classes
def test_students_are_crops_of_the_deformed_teacher():
    from mivp_amd import batches as BT
    bank, _, _ = _bank(2)
    roi, sizes, nodes = (12, 10, 20), [(12, 10, 20), (7, 6, 9)], (7, 7, 7)
    own = BT.BatchFiller(bank, roi, 4, student_sizes=sizes, active_labels=ACTIVE, spatial=True, elastic=nodes)
    rs = np.random.RandomState(13)
    d = _draws(rs, [0, 1, 2, 0], [0, 1, 2, 3], roi, sizes)
    sp = BT.draw_spatial(rs, 4, **TYPICAL)
    ed = BT.draw_elastic(rs, 4, roi, nodes=nodes, p_elastic=1.0, magnitude_range=(0.5, 0.8), locked_borders=2)
    _poison(own)
    batch = own.fill(d, spatial=sp, elastic=ed)
    torch.cuda.synchronize()
    assert batch is own.batch and sorted(batch) == ["coord", "coord_st", "image", "image_st", "mask_st_0"]
    assert not any(torch.isnan(t).any() for t in _outs(own))
    for i, size in enumerate(sizes):
        assert torch.equal(own.image_st[i], R.student_view(own.image, d.student_origin[i], size))
        assert torch.equal(own.coord_st[i], R.student_view(own.coord, d.student_origin[i], size))
    assert torch.equal(own.mask_st_0, R.student_view(own.mask, d.student_origin[0], sizes[0]))
    plain = BT.BatchFiller(bank, roi, 4, student_sizes=sizes, active_labels=ACTIVE, spatial=True)
    plain.fill(d, spatial=sp)
    assert not torch.equal(plain.image, own.image)                  # and the teacher was deformed


def test_class_balanced_centres_are_honoured():
    """The pick still runs first: the origins are the index's, and with a zero lattice on a flagged sample (and the identity
    map) the centre voxel carries the drawn class; with a drawn lattice the batch is the restatement's at those origins."""
    from mivp_amd import batches as BT
    bank, images, labels = _bank(1)
    index = BT.ClassIndex(bank, NCLS, ACTIVE).update()
    roi, nodes = (9, 7, 11), (4, 4, 5)
    own = BT.BatchFiller(bank, roi, 4, active_labels=ACTIVE, with_coord=True, class_index=index, spatial=True, elastic=nodes)
    rs = np.random.RandomState(17)
    free_any = False
    zero = BT.ElasticDraws(np.ones(4, np.int32), np.zeros((4, 3) + nodes, np.float32))
    drawn = BT.draw_elastic(rs, 4, roi, nodes=nodes, p_elastic=1.0, magnitude_range=(1.0, 1.4), locked_borders=0)
    span = 255.0
    for ed in (zero, drawn):
        for _ in range(2):
            d = BT.draw_class_crops(rs, index, [0, 2, 0, 2], roi, 1, (1, 2, 0), True)
            _poison(own)
            own.fill(d, elastic=ed)
            origin = own.slot.resolved_origins()
            want_origin, moved = CR.origins(labels, _lut(), NCLS, d, roi)
            assert np.array_equal(origin, want_origin)
            ident = BT.SpatialDraws.identity(4).affine
            want = ER.teacher_batch(images, labels, _lut(), d.volume, d.rot, origin, roi, ident, ed.flags, ed.lattice)
            _, delta_r = EC.bounds(ident, 1.4)
            _assert_within(_teacher(own), want, delta_r, span, "class-balanced")
            if ed is zero:
                centre = own.mask[:, 0, 4, 3, 5].cpu().numpy()
                assert np.array_equal(centre[~moved], d.cls[~moved].astype(np.float32))
                free_any = free_any or (~moved).any()
    assert free_any


# ------------------------------------------------------------------------------------------------ 7. recording
def test_a_recorded_fill_follows_all_three_slots():
    from mivp_amd import batches as BT
    bank, _, _ = _bank(2, integer=False)
    roi, sizes, nodes = (12, 10, 20), [(8, 8, 8)], (6, 5, 7)
    own = BT.BatchFiller(bank, roi, 3, student_sizes=sizes, active_labels=ACTIVE, spatial=True, elastic=nodes)
    ref = BT.BatchFiller(bank, roi, 3, student_sizes=sizes, active_labels=ACTIVE, spatial=True, elastic=nodes)
    rs = np.random.RandomState(19)
    ekw = dict(nodes=nodes, p_elastic=0.7, magnitude_range=(0.5, 1.2), locked_borders=1)
    loads = [(_draws(rs, [0, 2, 1], [rs.randint(4) for _ in range(3)], roi, sizes), BT.draw_spatial(rs, 3, **TYPICAL),
              BT.draw_elastic(rs, 3, roi, **ekw)) for _ in range(3)]
    assert all(0 < ed.flags.sum() for _, _, ed in loads) and len({tuple(ed.flags) for _, _, ed in loads}) > 1
    own.fill(loads[0][0], spatial=loads[0][1], elastic=loads[0][2])
    first = [t.clone() for t in _outs(own)]
    _poison(own)
    own.fill()                                                      # the same slots: the same bits
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, _outs(own)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        own.fill()
        own.elastic_slot.load(loads[1][2])                          # does nothing while recording
    assert own.elastic_slot.draws is loads[0][2]
    for d, sp, ed in loads[::-1]:
        own.slot.load(d, bank, roi, sizes)
        own.spatial_slot.load(sp)
        own.elastic_slot.load(ed)
        _poison(own)
        graph.replay()
        ref.fill(d, spatial=sp, elastic=ed)
        torch.cuda.synchronize()
        assert not any(torch.isnan(t).any() for t in _outs(own))
        assert all(torch.equal(a, b) for a, b in zip(_outs(own), _outs(ref)))
    assert all(torch.equal(a, b) for a, b in zip(first, _outs(own)))            # loads[0] came last
    other = BT.ElasticSlot(3, nodes, DEV)                           # a slot of one's own is used as it stands
    other.load(loads[2][2])
    own.fill(loads[2][0], spatial=loads[2][1], elastic=other)
    ref.fill(loads[2][0], spatial=loads[2][1], elastic=loads[2][2])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_outs(own), _outs(ref)))
    assert own.elastic_slot.draws is loads[0][2]                    # and the filler's own slot was left alone


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_come_before_any_launch():
    from mivp_amd import _lib as L, batches as BT
    from mivp_amd._host import i3
    bank, _, _ = _bank(1)
    roi, nodes = (8, 12, 5), (5, 4, 6)
    with pytest.raises(ValueError, match="needs spatial=True"):
        BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, elastic=nodes)
    with pytest.raises(ValueError, match="nodes"):
        BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, spatial=True, elastic=(5, 4, 9))
    d = _draws(np.random.RandomState(1), [0, 1], [0, 3], roi)
    other = _draws(np.random.RandomState(2), [1, 0], [2, 1], roi)
    spatial = BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, with_coord=True, spatial=True)
    own = BT.BatchFiller(bank, roi, 2, active_labels=ACTIVE, with_coord=True, spatial=True, elastic=nodes)
    own.fill(d)
    spatial.fill(d)
    torch.cuda.synchronize()
    before = [t.clone() for t in _outs(own) + _outs(spatial)]
    records, words, buffer = own.slot.records.clone(), own.spatial_slot.words.clone(), own.elastic_slot.buffer.clone()
    good = BT.draw_elastic(np.random.RandomState(3), 2, roi, nodes=nodes, p_elastic=1.0, magnitude_range=(0.5, 0.7), locked_borders=1)
    nan = BT.ElasticDraws(good.flags.copy(), good.lattice.copy())
    nan.lattice[1, 0, 2, 2, 2] = np.nan
    flag = BT.ElasticDraws(np.asarray([1, 3], np.int32), good.lattice)
    moved = BT.draw_spatial(np.random.RandomState(4), 2, **TYPICAL)
    cases = [(spatial, dict(elastic=good), "built with elastic=nodes"),
             (spatial, dict(elastic=BT.ElasticSlot(2, nodes, DEV)), "built with elastic=nodes"),
             (own, dict(elastic=nan), "sample 1: a non-finite"),
             (own, dict(elastic=flag), "sample 1: flag 3"),
             (own, dict(elastic=BT.ElasticDraws.identity(3, nodes)), r"int32 \[2\]"),
             (own, dict(elastic=BT.ElasticDraws.identity(2, (5, 4, 7))), r"float32 \[2, 3, 5, 4, 6\]"),
             (own, dict(elastic=BT.ElasticSlot(3, nodes, DEV)), "elastic slot of batch 3"),
             (own, dict(elastic=BT.ElasticSlot(2, (5, 4, 7), DEV)), "elastic slot of batch 2"),
             (own, dict(elastic=np.zeros(2)), "ElasticDraws, an ElasticSlot")]
    if torch.cuda.device_count() > 1:
        cases.append((own, dict(elastic=BT.ElasticSlot(2, nodes, "cuda:1")), "elastic slot of batch 2"))
    for f, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            f.fill(other, spatial=moved, **kw)                      # new crop and spatial draws too: neither may be loaded
    with pytest.raises(ValueError, match="sample 1"):
        own.elastic_slot.load(nan)
    with pytest.raises(ValueError, match="ElasticDraws expected"):
        own.elastic_slot.load(moved)
    # the C entry: node counts outside 4..8 are refused on the host with MIVP_EINVAL (-1), nothing is launched
    _poison(own)
    for bad in ((3, 4, 4), (4, 9, 4), (4, 4, 0)):
        with pytest.raises(RuntimeError, match="mivp_crop_fill_elastic failed with code -1"):
            L.call("mivp_crop_fill_elastic", L.ptr(bank.table), bank.capacity, bank.channels, L.ptr(own.slot.records),
                   own.slot.words, L.ptr(own.spatial_slot.words), own.B, i3(roi), L.ptr(own.lut), L.ptr(own.image),
                   L.ptr(own.mask), L.ptr(own.coord), L.ptr(own.elastic_slot.flags), L.ptr(own.elastic_slot.lattice), i3(bad),
                   L.stream())
    with pytest.raises(RuntimeError, match="failed with code -1"):
        L.call("mivp_crop_fill_elastic", L.ptr(bank.table), bank.capacity, bank.channels, L.ptr(own.slot.records),
               own.slot.words, L.ptr(own.spatial_slot.words), own.B, i3(roi), L.ptr(own.lut), L.ptr(own.image),
               L.ptr(own.mask), L.ptr(own.coord), None, L.ptr(own.elastic_slot.lattice), i3(nodes), L.stream())
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in _outs(own))            # still poisoned: no launch was made
    assert all(torch.equal(a, b) for a, b in zip(before[len(_outs(own)):], _outs(spatial)))
    assert torch.equal(records, own.slot.records) and own.slot.draws is d and spatial.slot.draws is d
    assert torch.equal(words, own.spatial_slot.words) and torch.equal(buffer, own.elastic_slot.buffer)
    assert not own.elastic_slot.draws.flags.any()
