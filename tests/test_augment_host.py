"""Host side of the random intensity augmentation (mivp_amd.augment): the draws, the slot records, the numpy restatement
of the chain the GPU tests compare with (tests/intensity_ref.py), the C ABI declarations and the argument checks."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import intensity_ref as R
from conftest import ROOT

SYMBOLS = ("mivp_intensity_ws", "mivp_intensity_stats", "mivp_intensity_apply")


def _aug():
    import mivp_amd  # noqa: F401
    from mivp_amd import augment
    return augment


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype
               for k in ("flags", "coeffs", "shift", "gamma", "scale", "n_points", "floating"))


def _off(B=1):
    return _aug().draw_intensity(np.random.RandomState(0), B, prob=0.0)


# ------------------------------------------------------------------------------------------------ draws
def test_draws_repeat_for_a_seed_and_differ_between_seeds():
    A = _aug()
    a = A.draw_intensity(np.random.RandomState(7), 16, prob=0.5)
    b = A.draw_intensity(np.random.RandomState(7), 16, prob=0.5)
    c = A.draw_intensity(np.random.RandomState(8), 16, prob=0.5)
    assert _same(a, b) and not _same(a, c)
    assert a.batch == 16 and a.flags.dtype == np.int32 and a.coeffs.shape == (16, 20) and a.floating.shape == (16, 12)


def test_draws_follow_the_documented_stream():
    """One RandomState; per sample and step ``rand() < prob``, then the parameters only if the step fired."""
    A = _aug()
    d = A.draw_intensity(np.random.RandomState(3), 6, prob=0.5)
    rs = np.random.RandomState(3)
    for b in range(6):
        flags = 0
        if rs.rand() < 0.5:
            flags |= 1
            assert np.array_equal(d.coeffs[b], rs.uniform(0.0, 0.1, 20).astype(np.float32))
        if rs.rand() < 0.5:
            flags |= 2
            assert d.shift[b] == np.float32(rs.uniform(0.0, 0.1))
        if rs.rand() < 0.5:
            flags |= 4
            assert d.gamma[b] == np.float32(rs.uniform(0.5, 4.5))
        if rs.rand() < 0.5:
            flags |= 8
            assert d.scale[b] == np.float32(rs.uniform(-2.0, 2.0))
        if rs.rand() < 0.5:
            flags |= 16
            n = rs.randint(8, 13)
            fl = np.linspace(0.0, 1.0, n)
            for i in range(1, n - 1):
                fl[i] = rs.uniform(fl[i - 1], fl[i + 1])
            assert d.n_points[b] == n and np.array_equal(d.floating[b, :n], fl.astype(np.float32))
        assert d.flags[b] == flags


def test_draw_parameters_lie_in_their_ranges():
    A = _aug()
    d = A.draw_intensity(np.random.RandomState(11), 400, prob=0.6)
    f32 = np.float32
    assert set(np.unique(d.flags)) <= set(range(32)) and len(np.unique(d.flags)) > 8
    assert (d.coeffs >= 0).all() and (d.coeffs <= f32(0.1)).all()
    assert (d.shift >= 0).all() and (d.shift <= f32(0.1)).all()
    assert (d.gamma >= f32(0.5)).all() and (d.gamma <= f32(4.5)).all()
    assert (d.scale >= -2).all() and (d.scale <= 2).all()
    assert (d.n_points >= 8).all() and (d.n_points <= 12).all() and len(np.unique(d.n_points)) == 5
    for b in range(d.batch):
        n = int(d.n_points[b])
        fl = d.floating[b, :n]
        assert fl[0] == 0.0 and fl[-1] == 1.0 and (np.diff(fl) >= 0).all()
        assert (d.floating[b, n:] == 1.0).all()
    # a step that did not fire keeps neutral parameters
    off = (d.flags & A.FLAG_CONTRAST) == 0
    assert off.any() and (d.gamma[off] == 1.0).all()
    assert (d.coeffs[(d.flags & A.FLAG_BIAS) == 0] == 0).all() and (d.scale[(d.flags & A.FLAG_SCALE) == 0] == 0).all()
    # custom ranges are honoured
    e = A.draw_intensity(np.random.RandomState(1), 50, prob=1.0, coeff_range=(0.2, 0.3), std_factors=(0.5, 0.6),
                         gamma=(1.5, 2.0), scale=0.25, control_points=(3, 4))
    assert (e.coeffs >= f32(0.2)).all() and (e.coeffs <= f32(0.3)).all() and (e.shift >= f32(0.5)).all()
    assert (e.gamma >= 1.5).all() and (e.gamma <= 2.0).all() and (np.abs(e.scale) <= 0.25).all()
    assert set(np.unique(e.n_points)) == {3, 4}


def test_prob_zero_is_all_off_and_prob_one_is_all_on():
    A = _aug()
    assert (A.draw_intensity(np.random.RandomState(0), 32, prob=0.0).flags == 0).all()
    assert (A.draw_intensity(np.random.RandomState(0), 32, prob=1.0).flags == A.FLAG_ALL).all()
    d = A.draw_intensity(np.random.RandomState(5), 4000)                     # the default: the reference's 0.05 per step
    rate = np.mean([(d.flags & bit) != 0 for bit in (1, 2, 4, 8, 16)])
    assert 0.04 < rate < 0.06
    with pytest.raises(ValueError):
        A.draw_intensity(np.random.RandomState(0), 2, control_points=(8, 13))
    with pytest.raises(ValueError):
        A.draw_intensity(np.random.RandomState(0), 0)


# ------------------------------------------------------------------------------------------------ slot records
def test_records_pack_and_unpack_round_trip():
    A = _aug()
    d = A.draw_intensity(np.random.RandomState(2), 9, prob=0.5)
    w = d.pack()
    assert w.dtype == np.int32 and w.shape == (9, A.RECORD) and A.RECORD == 40
    assert _same(A.IntensityDraws.unpack(w), d)
    assert _same(A.IntensityDraws.unpack(w.reshape(-1)), d)
    f = w.view(np.float32)
    assert np.array_equal(w[:, 0], d.flags) and np.array_equal(w[:, 1], d.n_points)
    assert np.array_equal(f[:, 2], d.shift) and np.array_equal(f[:, 3], d.gamma) and np.array_equal(f[:, 4], d.scale)
    assert np.array_equal(f[:, 5:25], d.coeffs) and np.array_equal(f[:, 25:37], d.floating) and (w[:, 37:] == 0).all()


# ------------------------------------------------------------------------------------------------ restatement
def _x(shape, seed=0):
    return np.clip(1.4 * np.random.RandomState(seed).rand(*shape) - 0.2, 0.0, 1.0)


def _one(**kw):
    d = dict(flags=0, coeffs=np.zeros(20), shift=0.0, gamma=1.0, scale=0.0, n_points=8, floating=np.linspace(0, 1, 8))
    d.update(kw)
    return d


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_all_off_is_the_identity(dtype):
    x = _x((2, 5, 4, 3)).astype(dtype)
    assert np.array_equal(R.chain_sample(x, **_one(), dtype=dtype), x)
    d = _off(3)
    xb = _x((3, 1, 4, 4, 2)).astype(dtype)
    assert np.array_equal(R.chain(xb, d, dtype), xb)


def test_restatement_bias_field_is_the_legendre_sum():
    """leggrid3d against the sum written out: exp(sum c_ijk P_i(h) P_j(w) P_k(d)) on linspace(-1, 1, dim), an axis of
    length 1 at -1, the same field on every channel."""
    rs = np.random.RandomState(4)
    c = rs.uniform(0, 0.1, 20)
    dims = (5, 1, 4)
    P = [lambda t: np.ones_like(t), lambda t: t, lambda t: (3 * t ** 2 - 1) / 2, lambda t: (5 * t ** 3 - 3 * t) / 2]
    ax = [np.linspace(-1, 1, n) for n in dims]
    assert ax[1][0] == -1.0
    want, it = np.zeros(dims), iter(c)
    for i in range(4):
        for j in range(4 - i):
            for k in range(4 - i - j):
                want += next(it) * P[i](ax[0])[:, None, None] * P[j](ax[1])[None, :, None] * P[k](ax[2])[None, None, :]
    assert np.allclose(R.bias_field(c, dims, np.float64), np.exp(want), rtol=1e-13, atol=0)
    x = _x((2,) + dims)
    y = R.chain_sample(x, **_one(flags=R.BIAS, coeffs=c))
    assert np.allclose(y[0] / np.exp(want), x[0], rtol=1e-13) and np.allclose(y[1] / np.exp(want), x[1], rtol=1e-13)


def test_restatement_negative_scale_swaps_min_and_max():
    x = _x((1, 6, 5, 4), seed=1)
    y = R.chain_sample(x, **_one(flags=R.SCALE, scale=-1.75))
    assert np.array_equal(y, x * (1 - 1.75))
    assert y.min() == x.max() * -0.75 and y.max() == x.min() * -0.75
    # followed by the histogram step: the knots run from the new minimum to the new maximum
    fl = np.array([0, 0.05, 0.3, 0.35, 0.6, 0.8, 0.9, 1.0])
    z = R.chain_sample(x, **_one(flags=R.SCALE | R.HIST, scale=-1.75, floating=fl))
    assert np.isfinite(z).all() and z.min() == y.min() and z.max() == y.max()
    assert np.allclose(z, np.interp(y, np.linspace(0, 1, 8) * (y.max() - y.min()) + y.min(),
                                    fl * (y.max() - y.min()) + y.min()), rtol=0, atol=1e-15)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_constant_image_survives_contrast_and_histogram(dtype):
    x = np.full((1, 4, 4, 4), 0.37, dtype=dtype)
    y = R.chain_sample(x, **_one(flags=R.SHIFT | R.CONTRAST | R.HIST, shift=0.1, gamma=0.5), dtype=dtype)
    assert np.isfinite(y).all() and np.array_equal(y, x)           # std = 0, 0 ** gamma * 0 + min, histogram passes through
    y = R.chain_sample(x, **_one(flags=R.CONTRAST, gamma=4.5), dtype=dtype)
    assert np.array_equal(y, x)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_scale_minus_one_gives_zeros_that_pass_the_histogram(dtype):
    x = _x((1, 4, 5, 3)).astype(dtype)
    y = R.chain_sample(x, **_one(flags=R.SCALE | R.HIST, scale=-1.0, floating=np.linspace(0, 1, 8) ** 2), dtype=dtype)
    assert (y == 0).all() and np.isfinite(y).all()


def test_restatement_contrast_and_shift_formulas():
    x = _x((2, 4, 4, 3), seed=2)
    y = R.chain_sample(x, **_one(flags=R.SHIFT, shift=0.07))
    assert np.allclose(y, x + 0.07 * np.sqrt(np.mean((x - x.mean()) ** 2)), rtol=1e-14)       # population std, all channels
    y = R.chain_sample(x, **_one(flags=R.CONTRAST, gamma=0.5))
    lo, rng = x.min(), x.max() - x.min()
    assert np.allclose(y, np.sqrt((x - lo) / (rng + 1e-7)) * rng + lo, rtol=1e-14)
    assert y.min() == lo                                                                       # voxels at the minimum stay


def test_float32_restatement_tracks_the_oracle():
    """The yardstick is sane: single precision stays within a few 1e-6 of the range on the inputs the GPU tests use."""
    A = _aug()
    x = _x((3, 1, 13, 10, 9), seed=3)
    worst = 0.0
    for seed in range(10):
        d = A.draw_intensity(np.random.RandomState(seed), 3, prob=0.7)
        want = R.chain(x.astype(np.float32).astype(np.float64), d, np.float64)
        got = R.chain(x.astype(np.float32), d, np.float32)
        assert got.dtype == np.float32
        worst = max(worst, max(R.rel_err(got[b], want[b]) for b in range(3)))
    assert 0 < worst < 1e-5, worst


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_intensity_symbols_within_abi_18():
    A = _aug()
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    names = set(re.findall(r"\b(mivp_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    for n in SYMBOLS[1:]:
        m = re.search(r"int %s\(([^;]*)\);" % n, text)
        assert m and m.group(1).replace("\n", " ").split(",")[-1].strip() == "mivp_stream_t stream", n
    assert re.search(r"size_t mivp_intensity_ws\(int32_t B, int64_t voxels_per_sample\);", text)
    assert A.RECORD == 40 and "[B][40]" in text


def test_library_exports_intensity_symbols():
    import ctypes as C
    _aug()
    from mivp_amd import _lib
    lib = _lib.lib()
    assert lib.mivp_abi_version() == 18
    for n in SYMBOLS:
        assert hasattr(lib, n), n
    ws = lambda B, n: lib.mivp_intensity_ws(C.c_int32(B), C.c_int64(n))   # noqa: E731
    assert ws(1, 1) == 32 and ws(3, 13 * 10 * 9) == 3 * 32 and ws(1, 40 * 36 * 33) == 12 * 32
    assert ws(4, 96 ** 3) == 4 * 216 * 32 and ws(2, 1 << 40) == 2 * 256 * 32 and ws(2, 512 ** 3) == ws(2, 1 << 40)
    assert ws(0, 10) == 0 and ws(2, 0) == 0


def test_package_exports():
    import mivp_amd
    A = _aug()
    for n in ("IntensityDraws", "IntensitySlot", "draw_intensity", "augment_intensity"):
        assert getattr(mivp_amd, n) is getattr(A, n)


# ------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_raise_value_error():
    A = _aug()
    slot = A.IntensitySlot(2, "cpu")
    assert slot.buf.numel() == 2 * 40 + 2 * 256 * 8 and slot.records.numel() == 80
    assert slot.ws.data_ptr() == slot.buf.data_ptr() + 320                    # one allocation
    x = torch.rand(2, 1, 4, 4, 4)
    with pytest.raises(ValueError):                                           # no draws loaded yet
        A.augment_intensity(x, slot)
    slot.draws = _off(2)                                                      # (what load() records; the checks are host-side)
    for bad in (torch.rand(2, 4, 4, 4), torch.rand(3, 1, 4, 4, 4), torch.rand(2, 1, 4, 4, 4).double(),
                torch.rand(2, 1, 4, 4, 8)[..., ::2], torch.rand(2, 1, 4, 4, 4).half()):
        with pytest.raises(ValueError):
            A.augment_intensity(bad, slot)
    for out in (torch.empty(2, 1, 4, 4, 5), torch.empty(2, 1, 4, 4, 4, dtype=torch.float64)):
        with pytest.raises(ValueError):
            A.augment_intensity(x, slot, out=out)
    with pytest.raises(ValueError):
        A.augment_intensity(x, SimpleNamespace(B=2))
    with pytest.raises(ValueError):                                           # draws of another batch size
        slot.load(_off(3))
    with pytest.raises(ValueError):
        A.as_slot(_off(3), x)
    with pytest.raises(ValueError):
        A.as_slot("draws", x)
    d = _off(2)
    d.n_points[1] = 13
    with pytest.raises(ValueError):
        slot.load(d)
    d = _off(2)
    d.flags[0] = 32
    with pytest.raises(ValueError):
        slot.load(d)
    with pytest.raises(ValueError):
        A.IntensitySlot(0, "cpu")
    assert A.as_slot(slot, x) is slot
    # the product path has no CPU fallback: valid arguments on the host reach the binding's device check
    with pytest.raises(RuntimeError):
        A.augment_intensity(x, slot)


def test_step_functions_accept_augment_and_default_to_none():
    _aug()
    from mivp_amd import multiview, students_teacher, train
    for fn in (multiview.multiview_step, multiview.graphed_multiview_step, students_teacher.students_teacher_step,
               students_teacher.graphed_students_teacher_step):
        p = inspect.signature(fn).parameters
        assert "augment" in p and p["augment"].default is None, fn.__name__
    assert "augment" not in inspect.signature(train.train_step).parameters     # the downstream step has no intensity chain
