"""CPU: the host side of the students' corruption of the batch filler (mivp_amd.batches: draw_student_corruption,
CorruptionDraws, CorruptionSlot), the C-ABI declaration, and the numpy restatement the GPU tests compare against
(tests/corrupt_crops_ref.py)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import mivp_amd  # noqa: F401
from mivp_amd import batches as BT

import corrupt_crops_ref as CR

KEYS = [0, 1, 0xDEADBEEF, 0xFFFFFFFF, 123456789]
FIELDS = ("mode", "n_holes", "key", "origin", "size", "hole_key")


# ---------------------------------------------------------------------------------------------- the permutation
def test_the_reference_permutation_is_a_bijection():
    for n in list(range(1, 301)) + [511, 512, 513, 4095, 4096]:
        for key in KEYS[:3] if n <= 300 else KEYS:
            p = CR.permutation(n, key)
            assert p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n)), (n, key)


def test_different_keys_give_different_permutations():
    perms = [tuple(CR.permutation(64, key)) for key in KEYS + [2, 3, 4]]
    assert len(set(perms)) == len(perms)
    assert all(p != tuple(range(64)) for p in perms)                # and none is the identity
    assert tuple(CR.permutation(64, 7)) == tuple(CR.permutation(64, 7))


def test_the_reference_noise_is_uniform_and_keyed():
    u = CR.uniform(np.arange(1 << 16), 12345)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    # 65536 uniform values: the mean's standard deviation is 1 / sqrt(12 * 65536) = 1.1e-3; six of them
    assert abs(float(u.mean()) - 0.5) < 6.8e-3
    counts = np.histogram(u, 8, (0, 1))[0]
    assert np.abs(counts - 8192).max() < 6 * np.sqrt(8192 * 7 / 8)
    assert not np.array_equal(u, CR.uniform(np.arange(1 << 16), 12346))
    x = CR.noise(np.float32(3.5), np.float32(3.5), np.arange(100), 9)
    assert x.dtype == np.float32 and (x == np.float32(3.5)).all()   # lo == hi gives exactly lo
    lo, hi = CR.value_range(np.asarray([[-0.0, 2.0]], np.float32))
    assert lo == 0 and not np.signbit(lo) and hi == 2


# ---------------------------------------------------------------------------------------------- the draws
SIZES = [(72, 72, 8), (12, 10, 9)]


def test_draws_are_deterministic_and_every_hole_lies_inside_its_student():
    d = BT.draw_student_corruption(np.random.RandomState(5), 40, SIZES, weights=(0.1, 0.3, 0.3, 0.3))
    again = BT.draw_student_corruption(np.random.RandomState(5), 40, SIZES, weights=(0.1, 0.3, 0.3, 0.3))
    other = BT.draw_student_corruption(np.random.RandomState(6), 40, SIZES, weights=(0.1, 0.3, 0.3, 0.3))
    assert isinstance(d, BT.CorruptionDraws) and d.batch == 40 and d.n_students == 2
    assert all(np.array_equal(getattr(d, k), getattr(again, k)) for k in FIELDS)
    assert not all(np.array_equal(getattr(d, k), getattr(other, k)) for k in FIELDS)
    assert set(d.mode.reshape(-1).tolist()) == {0, 1, 2, 3}
    clipped = False
    for s, ext in enumerate(SIZES):
        for b in range(40):
            mode, n = int(d.mode[s, b]), int(d.n_holes[s, b])
            assert (n == 0) == (mode == 0) and n <= BT.MAX_HOLES
            assert n in {0: (0,), 1: (1, 2, 3), 2: (5,), 3: (1, 2, 3)}[mode]
            for k in range(n):
                o, e = d.origin[s, b, k], d.size[s, b, k]
                assert (e >= 1).all() and (o >= 0).all() and (o + e <= np.asarray(ext)).all()
                lo, hi = (32, 48) if mode == 2 else (4, 16)
                assert all(e[a] == ext[a] if ext[a] < lo else lo <= e[a] <= min(hi, ext[a]) for a in range(3)), (mode, e, ext)
                clipped = clipped or any(e[a] == ext[a] < lo for a in range(3))
            assert not d.origin[s, b, n:].any() and not d.size[s, b, n:].any() and not d.hole_key[s, b, n:].any()
            assert (d.key[s, b] == 0) if mode in (0, 3) else True
    assert clipped                                                  # keep's 32..48 on the extents 8, 12, 10, 9
    assert d.check(40, SIZES) is d


def test_keep_stays_valid_on_the_ymls_student_and_the_documented_order_holds():
    """keep's 32..48 on (72, 72, 8): the D extent is clipped to 8 and the origin there is 0.  The stream is consumed in the
    documented order: the mode, the count, per hole three extents then three origins, then the key."""
    rs, ref = np.random.RandomState(11), np.random.RandomState(11)
    d = BT.draw_student_corruption(rs, 3, [(72, 72, 8)], weights=(0, 0, 1, 0))
    assert (d.mode == 2).all() and (d.n_holes == 5).all()
    assert (d.size[..., :5, 2] == 8).all() and (d.origin[..., :5, 2] == 0).all()
    assert ((d.size[..., :5, :2] >= 32) & (d.size[..., :5, :2] <= 48)).all()
    for b in range(3):
        assert ref.choice(4, p=[0, 0, 1, 0]) == 2 and ref.randint(5, 6) == 5
        for k in range(5):
            e = [min(int(ref.randint(32, 49)), ext) for ext in (72, 72, 8)]
            o = [int(ref.randint(0, ext - e[a] + 1)) for a, ext in enumerate((72, 72, 8))]
            assert d.size[0, b, k].tolist() == e and d.origin[0, b, k].tolist() == o
        assert d.key[0, b] == ref.randint(0, 2 ** 32, dtype=np.uint32)
    assert rs.random_sample() == ref.random_sample()
    # mode 0 consumes the mode's draw only
    rs, ref = np.random.RandomState(12), np.random.RandomState(12)
    d = BT.draw_student_corruption(rs, 4, SIZES, weights=(1, 0, 0, 0))
    ident = BT.CorruptionDraws.identity(4, 2)
    assert all(np.array_equal(getattr(d, k), getattr(ident, k)) for k in FIELDS)
    for _ in range(8):
        ref.choice(4, p=[1, 0, 0, 0])
    assert rs.random_sample() == ref.random_sample()


def test_mode_frequencies_follow_the_weights():
    N, w = 4000, (0.7, 0.1, 0.1, 0.1)
    d = BT.draw_student_corruption(np.random.RandomState(3), N, [(16, 16, 16)])
    for mode, p in enumerate(w):
        freq = float((d.mode == mode).mean())
        print(f"mode {mode}: frequency {freq:.4f}, weight {p}, bound {5 * np.sqrt(p * (1 - p) / N):.4f}")
        assert abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N)


def test_draw_refusals():
    rs = np.random.RandomState(1)
    for kw, match in [(dict(weights=(0.5, 0.5, 0.5)), "weights"), (dict(weights=(0, 0, 0, 0)), "weights"),
                      (dict(weights=(1, -1, 1, 1)), "weights"), (dict(dropout=dict(holes=1)), "dropout takes"),
                      (dict(dropout=dict(holes=1, spatial_size=4, fill_value=0)), "dropout takes"),
                      (dict(keep=dict(holes=9, spatial_size=4)), "max_holes <= 8"),
                      (dict(keep=dict(holes=3, max_holes=2, spatial_size=4)), "holes <= max_holes"),
                      (dict(shuffle=dict(holes=1, spatial_size=8, max_spatial_size=4)), "spatial_size <= max_spatial_size"),
                      (dict(shuffle=dict(holes=1, spatial_size=0)), "spatial_size")]:
        with pytest.raises(ValueError, match=match):
            BT.draw_student_corruption(rs, 2, SIZES, **kw)
    with pytest.raises(ValueError, match="student size"):
        BT.draw_student_corruption(rs, 2, [])
    with pytest.raises(ValueError):
        BT.draw_student_corruption(rs, 0, SIZES)
    with pytest.raises(ValueError, match="more than 4096"):       # 17^3 voxels in a shuffle hole
        BT.draw_student_corruption(rs, 2, [(32, 32, 32)], weights=(0, 0, 0, 1), shuffle=dict(holes=1, spatial_size=17))
    d = BT.draw_student_corruption(rs, 2, [(32, 32, 32)], weights=(0, 1, 0, 0), dropout=dict(holes=8, spatial_size=(17, 1, 2)))
    assert (d.n_holes == 8).all() and (d.size[..., :, :] == (17, 1, 2)).all()   # max_* default to the minimum; dropout may be large


# ---------------------------------------------------------------------------------------------- pack, check
def test_pack_unpack_round_trip():
    d = BT.draw_student_corruption(np.random.RandomState(8), 7, SIZES, weights=(0.1, 0.3, 0.3, 0.3))
    w = d.pack()
    assert w.dtype == np.int32 and w.shape == (2, 7, BT.CORRUPT_WORDS) and BT.CORRUPT_WORDS == 59
    u = BT.CorruptionDraws.unpack(w, 2)
    for k in FIELDS:
        assert np.array_equal(getattr(d, k), getattr(u, k)) and getattr(d, k).dtype == getattr(u, k).dtype, k
    assert (d.key > 2 ** 31).any() and (d.hole_key > 2 ** 31).any()     # the sign bit survives the int32 words
    assert u.check(7, SIZES) is u
    assert np.array_equal(w[1, 3, :3], [d.mode[1, 3], d.n_holes[1, 3], d.key[1, 3].view(np.int32)])
    assert np.array_equal(w[1, 3, 3:10], list(d.origin[1, 3, 0]) + list(d.size[1, 3, 0]) + [d.hole_key[1, 3, 0].view(np.int32)])
    ident = BT.CorruptionDraws.identity(7, 2)
    assert not ident.pack().any() and ident.check(7, SIZES) is ident


def _good():
    d = BT.CorruptionDraws.identity(3, 2)
    d.mode[:] = [[1, 2, 3], [3, 0, 1]]
    d.n_holes[:] = [[2, 1, 1], [8, 0, 1]]
    d.size[:] = 1
    d.size[0, 0, 0] = (72, 72, 8)
    d.size[1, 0, :8] = (8, 8, 8)
    return d.check(3, SIZES)


def test_check_refuses_each_malformed_field_by_name():
    def refused(match, **change):
        d = _good()
        for name, (index, value) in change.items():
            getattr(d, name)[index] = value
        with pytest.raises(ValueError, match=match):
            d.check(3, SIZES)

    refused("student 1: sample 2: mode 4 outside 0..3", mode=((1, 2), 4))
    refused("student 0: sample 1: mode -1", mode=((0, 1), -1))
    refused("student 0: sample 2: n_holes 9 outside 0..8", n_holes=((0, 2), 9))
    refused("student 1: sample 2: n_holes -1", n_holes=((1, 2), -1))
    refused("student 0: sample 0: hole 1 .* outside the student's extents", origin=((0, 0, 1, 2), 8))
    refused("student 0: sample 0: hole 1 .* outside", origin=((0, 0, 1, 0), -1))
    refused("student 1: sample 0: hole 7 .* empty or outside", size=((1, 0, 7, 1), 0))
    refused("student 1: sample 0: hole 3 .* outside", size=((1, 0, 3, 2), 10))
    refused("student 0: sample 2: shuffle hole 0 .* 4608 voxels, more than 4096", size=((0, 2, 0), (24, 24, 8)))
    d = _good()
    d.size[0, 0, 1] = (24, 24, 8)                                   # the same hole in dropout mode is allowed
    d.origin[0, 1, 5] = 1000                                        # and a hole that is not read may hold anything
    d.check(3, SIZES)
    for name in FIELDS:
        d = _good()
        setattr(d, name, getattr(d, name).astype(np.int64))
        with pytest.raises(ValueError, match=f"CorruptionDraws: {name} must be a"):
            d.check(3, SIZES)
        d = _good()
        setattr(d, name, getattr(d, name)[:, :2])
        with pytest.raises(ValueError, match=f"CorruptionDraws: {name} must be a"):
            d.check(3, SIZES)
        d = _good()
        setattr(d, name, getattr(d, name).tolist())
        with pytest.raises(ValueError, match=f"CorruptionDraws: {name} must be a"):
            d.check(3, SIZES)
    with pytest.raises(ValueError, match="mode must be a int32"):
        _good().check(4, SIZES)
    with pytest.raises(ValueError, match="mode must be a int32"):
        _good().check(3, SIZES[:1])
    with pytest.raises(ValueError, match="outside the student's extents"):
        _good().check(3, [(72, 72, 7), (12, 10, 9)])


# ---------------------------------------------------------------------------------------------- the reference itself
def test_the_reference_keeps_what_each_mode_must_keep():
    rs = np.random.RandomState(2)
    x = rs.uniform(-2, 5, (2, 9, 8, 7)).astype(np.float32)
    holes = [((1, 2, 0), (4, 3, 5), 77), ((3, 3, 2), (5, 4, 5), 78)]          # overlapping
    inside = CR.union_mask(x.shape[1:], holes)
    assert 0 < inside.sum() < 4 * 3 * 5 + 5 * 4 * 5
    lo, hi = CR.value_range(x)
    y = CR.corrupt_sample(x, 1, holes, 5)
    assert np.array_equal(y[:, ~inside], x[:, ~inside]) and (y[:, inside] != x[:, inside]).all()
    assert (y >= lo).all() and (y[:, inside] < hi).all()
    z = CR.corrupt_sample(x, 2, holes, 5)
    assert np.array_equal(z[:, inside], x[:, inside]) and (z[:, ~inside] != x[:, ~inside]).all()
    full = CR.noise(lo, hi, np.arange(x.size, dtype=np.uint64).reshape(x.shape), 5)
    assert np.array_equal(np.where(inside, y, z), full)             # the two modes are complementary parts of one field
    s = CR.corrupt_sample(x, 3, holes, 0)
    assert np.array_equal(s[:, ~inside], x[:, ~inside]) and not np.array_equal(s, x)
    assert np.array_equal(np.sort(s[0][inside]), np.sort(x[0][inside]))       # the union keeps its multiset
    swapped = CR.corrupt_sample(x, 3, holes[::-1], 0)
    assert not np.array_equal(swapped, s)                           # and the order of overlapping holes matters
    one = CR.corrupt_sample(x, 3, holes[:1], 0)
    box = (slice(None), slice(1, 5), slice(2, 5), slice(0, 5))
    perm = CR.permutation(60, 77)
    assert np.array_equal(one[box].reshape(2, -1), x[box].reshape(2, -1)[:, perm])        # every channel, one permutation
    assert np.array_equal(CR.corrupt_sample(x, 0, holes, 5), x)


# ---------------------------------------------------------------------------------------------- the C ABI, the filler
def test_header_declares_the_corruption_entries_at_abi_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    P = _lib.parse_header()
    assert len(P["mivp_crop_corrupt_range"][1]) == 7 and len(P["mivp_crop_corrupt"][1]) == 7
    assert _lib.ABI_VERSION == 18
    for name, value in (("MAX_HOLES", BT.MAX_HOLES), ("RECORD_WORDS", BT.CORRUPT_WORDS),
                        ("SHUFFLE_VOXELS", BT.MAX_SHUFFLE_VOXELS), ("PARTIALS", BT.CORRUPT_PARTIALS)):
        assert re.search(rf"^#define MIVP_CORRUPT_{name} {value}$", text, flags=re.M), name
    assert (BT.MAX_HOLES, BT.MAX_SHUFFLE_VOXELS, BT.CORRUPT_WORDS) == (8, 4096, 3 + 8 * 7)
    assert len(P["mivp_crop_fill_elastic"][1]) == 16 and len(P["mivp_crop_tensor"][1]) == 9       # the neighbours: kept


def test_library_exports_the_corruption_entries_at_abi_18():
    from mivp_amd import _lib
    lib = _lib.lib()
    assert lib.mivp_abi_version() == 18
    assert hasattr(lib, "mivp_crop_corrupt_range") and hasattr(lib, "mivp_crop_corrupt")


def test_filler_and_slot_arguments_that_need_no_device():
    with pytest.raises(ValueError, match="GPU"):
        BT.CorruptionSlot(2, SIZES, "cpu")
    with pytest.raises(ValueError, match="at least one student"):
        BT.CorruptionSlot(2, [], "cpu")
    with pytest.raises(ValueError, match="VolumeBank"):
        BT.BatchFiller(object(), (8, 8, 8), 2, student_sizes=SIZES, corruption=True)
    bank = object.__new__(BT.VolumeBank)                            # the type alone: the refusal comes before any use of it
    with pytest.raises(ValueError, match="corruption=True needs student_sizes"):
        BT.BatchFiller(bank, (8, 8, 8), 2, corruption=True)
