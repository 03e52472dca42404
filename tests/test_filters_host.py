"""Host side of the noise / blur / low-resolution augmentation (mivp_amd.augment): the draws, the slot records, the taps,
the numpy restatement the GPU tests compare with (tests/filters_ref.py) -- its index rules against torch's own
``interpolate`` on the CPU, its noise against the statistics of a unit Gaussian -- and the argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import filters_ref as R
from conftest import ROOT

FIELDS = ("flags", "noise_key", "noise_mean", "noise_std", "radius", "taps", "low_size")
GPU_SHAPES = [(3, 1, 13, 10, 9), (2, 2, 8, 8, 1), (1, 1, 40, 36, 33)]        # those of test_hip_filters.py


def _aug():
    import mivp_amd  # noqa: F401
    from mivp_amd import augment
    return augment


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype for k in FIELDS)


# ------------------------------------------------------------------------------------------------ draws and records
def test_draws_repeat_for_a_seed_and_differ_between_seeds():
    A = _aug()
    a = A.draw_filters(np.random.RandomState(7), 16, (13, 10, 9), prob=0.5)
    b = A.draw_filters(np.random.RandomState(7), 16, (13, 10, 9), prob=0.5)
    c = A.draw_filters(np.random.RandomState(8), 16, (13, 10, 9), prob=0.5)
    assert _same(a, b) and not _same(a, c)
    assert a.batch == 16 and a.flags.dtype == np.int32 and a.noise_key.dtype == np.uint32
    assert a.radius.shape == (16, 3) and a.taps.shape == (16, 3, 17) and a.taps.dtype == np.float32
    assert a.low_size.shape == (16, 3) and a.low_size.dtype == np.int32
    assert len(set(int(f) for f in a.flags)) >= 4


def test_draws_follow_the_documented_stream():
    """One RandomState; per sample noise, smooth, low-res: ``rand() < prob``, then the parameters only if the step fired."""
    A = _aug()
    dims = (13, 10, 9)
    d = A.draw_filters(np.random.RandomState(3), 8, dims, prob=0.5)
    rs = np.random.RandomState(3)
    for b in range(8):
        flags, std, radius, low = 0, 0.0, [0, 0, 0], list(dims)
        if rs.rand() < 0.5:
            flags |= 1
            key = rs.randint(0, 2 ** 32, dtype=np.uint32)
            std = rs.uniform(0.0, 0.1)
            assert d.noise_key[b] == key
        if rs.rand() < 0.5:
            flags |= 2
            for a in range(3):
                radius[a], taps = A.gaussian_taps(rs.uniform(0.25, 1.5))
                assert np.array_equal(d.taps[b, a], taps)
        if rs.rand() < 0.5:
            flags |= 4
            z = rs.uniform(0.5, 1.0)
            low = [max(1, int(n * z + 0.5)) for n in dims]
        assert d.flags[b] == flags and d.noise_std[b] == np.float32(std) and d.noise_mean[b] == 0
        assert d.radius[b].tolist() == radius and d.low_size[b].tolist() == low
        if not flags & 2:
            assert not d.taps[b].any()


def test_a_step_switched_off_leaves_only_the_earlier_steps_draws_unchanged():
    """The draw order: noise, smooth, low-res share one stream, so removing a step (its parameters are no longer drawn)
    keeps what comes before it in the first sample that had fired it and shifts everything after."""
    A = _aug()
    dims = (20, 18, 16)

    class Gate:
        """A RandomState whose ``rand()`` answers 1.0 -- the step does not fire -- at every third call from ``off``."""
        def __init__(self, seed, off):
            self.rs, self.off, self.n = np.random.RandomState(seed), off, 0

        def rand(self):
            v = self.rs.rand()
            self.n += 1
            return 1.0 if (self.n - 1) % 3 == self.off else v

        def __getattr__(self, k):
            return getattr(self.rs, k)

    full = A.draw_filters(np.random.RandomState(5), 1, dims, prob=1.0)
    no_low = A.draw_filters(Gate(5, 2), 1, dims, prob=1.0)                    # the last step off: both earlier ones unchanged
    assert no_low.flags[0] == 3 and no_low.noise_key[0] == full.noise_key[0] and no_low.noise_std[0] == full.noise_std[0]
    assert np.array_equal(no_low.taps, full.taps) and no_low.low_size[0].tolist() == list(dims)
    no_smooth = A.draw_filters(Gate(5, 1), 1, dims, prob=1.0)                 # the middle one off: noise unchanged, low-res moved
    assert no_smooth.flags[0] == 5 and no_smooth.noise_key[0] == full.noise_key[0]
    assert no_smooth.noise_std[0] == full.noise_std[0] and not no_smooth.radius.any()
    assert no_smooth.low_size[0].tolist() != full.low_size[0].tolist()
    no_noise = A.draw_filters(Gate(5, 0), 1, dims, prob=1.0)                  # the first one off: everything after it moved
    assert no_noise.flags[0] == 6 and not np.array_equal(no_noise.taps, full.taps)
    assert no_noise.low_size[0].tolist() != full.low_size[0].tolist()
    # prob = 0 draws exactly three numbers per sample and leaves the neutral parameters
    rs = np.random.RandomState(9)
    off = A.draw_filters(rs, 4, dims, prob=0.0)
    ref = np.random.RandomState(9)
    ref.rand(12)
    assert rs.rand() == ref.rand()
    assert not off.flags.any() and not off.noise_std.any() and not off.radius.any() and not off.taps.any()
    assert (off.low_size == np.asarray(dims)).all()


def test_records_pack_and_unpack_round_trip():
    A = _aug()
    d = A.draw_filters(np.random.RandomState(2), 9, (13, 10, 9), prob=0.5)
    d.noise_mean[:] = np.random.RandomState(1).randn(9)
    d.noise_key[0] = 0xFFFFFFFF                                                # the sign bit travels as a bit pattern
    w = d.pack()
    assert w.dtype == np.int32 and w.shape == (9, A.FILTER_RECORD) and A.FILTER_RECORD == 64
    assert _same(A.FilterDraws.unpack(w), d)
    assert _same(A.FilterDraws.unpack(w.reshape(-1)), d)
    assert w[:, 0].tolist() == d.flags.tolist() and w[:, 4:7].tolist() == d.radius.tolist()
    assert w[:, 7:10].tolist() == d.low_size.tolist()
    f = w.view(np.float32)
    b = int(np.flatnonzero(d.flags & 2)[0])
    for a in range(3):
        r = int(d.radius[b, a])
        for k in range(-r, r + 1):
            assert f[b, 10 + 17 * a + 8 + k] == d.taps[b, a, 8 + k] > 0
    assert not w[:, 61:].any()


def test_check_refuses_and_names_the_sample():
    A = _aug()

    def bad(**kw):
        d = A.draw_filters(np.random.RandomState(0), 3, (8, 8, 8), prob=1.0)
        for k, (idx, v) in kw.items():
            getattr(d, k)[idx] = v
        with pytest.raises(ValueError, match="sample 1"):
            d.check()

    bad(flags=(1, 8))
    bad(radius=((1, 2), 9))
    bad(radius=((1, 0), -1))
    bad(taps=((1, 0, 8), -0.25))
    bad(taps=((1, 2, 3), np.nan))
    bad(taps=((1, 1, 16), np.inf))
    bad(noise_std=(1, -0.1))
    bad(noise_std=(1, np.inf))
    bad(noise_mean=(1, np.nan))
    bad(low_size=((1, 1), 0))
    d = A.draw_filters(np.random.RandomState(0), 3, (8, 8, 8), prob=1.0)
    assert d.check() is d
    d.radius = d.radius[:2]
    with pytest.raises(ValueError):
        d.check()


def test_draw_filters_refuses_ranges_it_cannot_serve():
    A = _aug()
    rs = np.random.RandomState(0)
    for kw in (dict(sigma=(0.25, 2.2)), dict(sigma=(0.0, 1.0)), dict(sigma=(1.5, 0.5)), dict(zoom=(0.5, 1.5)),
               dict(zoom=(0.0, 1.0)), dict(noise_std=(-0.1, 0.1))):
        with pytest.raises(ValueError):
            A.draw_filters(rs, 2, (8, 8, 8), **kw)
    with pytest.raises(ValueError):
        A.draw_filters(rs, 0, (8, 8, 8))
    A.draw_filters(rs, 2, (8, 8, 8), prob=1.0, sigma=(2.124, 2.124))           # radius 8 exactly
    assert A.gaussian_taps(2.124)[0] == 8
    with pytest.raises(ValueError):
        A.gaussian_taps(2.125)


@pytest.mark.parametrize("sigma", [0.25, 0.3, 0.62, 1.0, 1.37, 1.5, 2.0])
def test_taps_follow_the_documented_erf_formula(sigma):
    A = _aug()
    r, taps = A.gaussian_taps(sigma)
    assert r == int(max(4.0 * sigma, 0.5) + 0.5) and 1 <= r <= 8
    assert taps.dtype == np.float32 and taps.shape == (17,)
    for k in range(-8, 9):
        want = 0.0
        if abs(k) <= r:
            t = 1.0 / (sigma * math.sqrt(2.0))
            want = max(0.5 * (math.erf((k + 0.5) * t) - math.erf((k - 0.5) * t)), 0.0)
        assert taps[8 + k] == np.float32(want)
    assert (taps >= 0).all() and np.array_equal(taps, taps[::-1])
    total = float(taps.astype(np.float64).sum())
    assert 0.99 < total <= 1.0                                                 # the truncated tails are missing: not normalised


# ------------------------------------------------------------------------------------------------ restated index rules
def _pairs():
    A = _aug()
    pairs = {(N, n) for N in range(1, 41) for n in range(1, N + 1)}
    for si, shape in enumerate(GPU_SHAPES):                                    # every pair the GPU tests' draws produce
        for k in range(40):
            d = A.draw_filters(np.random.RandomState(1000 * si + k), shape[0], shape[2:], prob=0.7)
            pairs |= {(shape[2 + a], int(d.low_size[b, a])) for b in range(shape[0]) for a in range(3)}
    return sorted(pairs)


def test_nearest_rule_is_torchs():
    for N, n in _pairs():
        want = F.interpolate(torch.arange(N, dtype=torch.float32).view(1, 1, N), size=n, mode="nearest").view(-1).numpy()
        got = R.nearest_index(N, n)
        assert got.shape == (n,) and np.array_equal(got, want.astype(np.int64)), (N, n)
        if n == N:
            assert np.array_equal(got, np.arange(N))


def test_linear_rule_is_torchs():
    rs = np.random.RandomState(0)
    for N, n in _pairs():
        low = rs.rand(n)
        for dtype, tol in ((np.float64, 1e-13), (np.float32, 2e-6)):
            lo, hi, w = R.linear_taps(n, N, dtype)
            assert lo.min() >= 0 and hi.max() <= n - 1 and ((hi == lo) | (hi == lo + 1)).all()
            assert (w >= 0).all() and (w < 1).all()
            src = low.astype(dtype)
            got = src[lo] + w * (src[hi] - src[lo])
            want = F.interpolate(torch.from_numpy(src).view(1, 1, n), size=N, mode="linear", align_corners=False)
            assert np.abs(got - want.view(-1).numpy()).max() <= tol, (N, n, dtype)
            if n == N:
                assert np.array_equal(lo, np.arange(N)) and not w.any()


def test_low_res_restatement_is_interpolate_down_and_up():
    """The composed step against torch on the CPU, on a volume: nearest to the low grid, trilinear back."""
    rs = np.random.RandomState(1)
    x = rs.rand(2, 13, 10, 9)
    for low in ((7, 5, 9), (13, 10, 9), (1, 1, 1), (12, 9, 5)):
        t = torch.from_numpy(x)[None]
        want = F.interpolate(F.interpolate(t, size=low, mode="nearest"), size=x.shape[1:], mode="trilinear",
                             align_corners=False)[0].numpy()
        got = R.low_res(x, low, np.float64)
        assert np.abs(got - want).max() <= 1e-13, low
        got32 = R.low_res(x.astype(np.float32), low, np.float32)
        assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 2e-6
    assert np.array_equal(R.low_res(x.astype(np.float32), (13, 10, 9), np.float32), x.astype(np.float32))


# ------------------------------------------------------------------------------------------------ restated hash and noise
def test_drop_hash_restatement_multiplies_24_bits():
    """Written out with Python integers: __umul24 keeps the low 24 bits of both operands and the low 32 of the product."""
    def one(i, key):
        m = 0xFFFFFFFF
        t = (i + key) & m
        t ^= t >> 16
        t = ((t & 0xFFFFFF) * 0xB5AD4F) & m
        t ^= t >> 13
        return (((t & 0xFFFFFF) * 0x6C62B9) + (t >> 8) + (((key << 13) | (key >> 19)) & m)) & m

    idx = np.array([0, 1, 2, 3, 0xFFFFFF, 0x1000000, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF, 123456789], dtype=np.uint32)
    for key in (0, 1, 0x9E3779B1, 0xFFFFFFFF):
        got = R.drop_hash(idx, key)
        assert got.dtype == np.uint32 and got.tolist() == [one(int(i), key) for i in idx]
    u1, u2 = R.uniforms(1000, 77)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert np.array_equal(u1 * 2 ** 24, np.round(u1 * 2 ** 24))


def test_noise_restatement_is_a_unit_gaussian():
    """Five standard errors on the mean, the variance and the lag-1 autocovariance of N = 47,520 values (the largest GPU
    test shape), for each of 20 keys; none left out."""
    N = 40 * 36 * 33
    assert N == 47520
    keys = np.random.RandomState(0).randint(0, 2 ** 32, size=20, dtype=np.uint32)
    for key in keys:
        g = R.gaussian(N, int(key), np.float64)
        assert g.dtype == np.float64 and np.isfinite(g).all()
        mean, var = g.mean(), g.var()
        lag1 = np.mean((g[:-1] - mean) * (g[1:] - mean))
        print(f"[noise] key {int(key):#010x}: mean {mean:+.5f} var {var:.5f} lag-1 {lag1:+.5f}")
        assert abs(mean) <= 5 / math.sqrt(N), (key, mean)
        assert abs(var - 1) <= 5 * math.sqrt(2 / N), (key, var)
        assert abs(lag1) <= 5 / math.sqrt(N), (key, lag1)
    g32 = R.gaussian(N, int(keys[0]), np.float32)
    assert g32.dtype == np.float32
    assert np.abs(g32 - R.gaussian(N, int(keys[0]), np.float64)).max() < 1e-5


def test_blur_restatement():
    A = _aug()
    r, taps = A.gaussian_taps(1.1)
    x = np.zeros((1, 11, 12, 13), np.float32)
    x[0, 5, 6, 7] = 1.0
    radius, tp = [r, 0, r], np.stack([taps, np.zeros(17, np.float32), taps])
    y = R.blur(x, radius, tp, np.float32)
    t = taps[8 - r:8 + r + 1]
    want = np.zeros_like(x)
    want[0, 5 - r:5 + r + 1, 6, 7 - r:7 + r + 1] = np.outer(t, t)              # one-hot in, the taps' outer product out
    assert y.dtype == np.float32 and np.array_equal(y, want)
    x = np.random.RandomState(0).rand(2, 5, 4, 3).astype(np.float32)
    assert R.blur(x, [0, 0, 0], tp, np.float32) is x                           # radius 0: untouched
    y64 = R.blur(x.astype(np.float64), [r, r, r], np.stack([taps] * 3), np.float64)
    full = np.pad(x.astype(np.float64), [(0, 0), (r, r), (r, r), (r, r)])
    k = t.astype(np.float64)
    want = np.einsum("chwd,h,w,d->c", full[:, 1:1 + 2 * r + 1, 0:2 * r + 1, 0:2 * r + 1], k, k, k)
    assert np.allclose(y64[:, 1, 0, 0], want, rtol=1e-13)                      # zero padding at the borders


def test_restatement_all_off_is_the_identity_and_the_yardstick_is_sane():
    A = _aug()
    x = np.random.RandomState(3).rand(3, 1, 13, 10, 9).astype(np.float32)
    off = A.draw_filters(np.random.RandomState(0), 3, (13, 10, 9), prob=0.0)
    assert np.array_equal(R.chain(x, off, np.float32), x)
    worst = 0.0
    for k in range(10):
        d = A.draw_filters(np.random.RandomState(k), 3, (13, 10, 9), prob=0.7)
        w64, w32 = R.chain(x.astype(np.float64), d, np.float64), R.chain(x, d, np.float32)
        worst = max(worst, max(R.rel_err(w32[b], w64[b]) for b in range(3)))
    assert 1e-8 < worst < 1e-5, worst


# ------------------------------------------------------------------------------------------------ C ABI and arguments
def test_header_and_library_declare_the_filter_entry_points():
    _aug()
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    protos = _lib.parse_header()
    assert len(protos["mivp_filter_ws"][1]) == 3 and len(protos["mivp_filter_apply"][1]) == 9
    assert re.search(r"#define MIVP_FILTER_RECORD_WORDS 64\b", text)
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    lib = _lib.lib()
    dims = lambda *d: (C.c_int32 * 3)(*d)   # noqa: E731
    assert lib.mivp_filter_ws(3, 1, dims(13, 10, 9)) == 2 * 4 * 3512           # two temporaries of 3510 floats, each rounded
    assert lib.mivp_filter_ws(1, 1, dims(1, 1, 1)) == 32                       # up to a multiple of 16 bytes
    assert lib.mivp_filter_ws(2, 2, dims(8, 8, 1)) == 2 * 4 * 256
    assert lib.mivp_filter_ws(1, 1, dims(0, 4, 4)) == 0 and lib.mivp_filter_ws(1, 2, dims(1024, 1024, 1024)) == 0


def test_package_exports():
    import mivp_amd
    A = _aug()
    for n in ("FilterDraws", "FilterSlot", "draw_filters", "augment_filters"):
        assert getattr(mivp_amd, n) is getattr(A, n)
    assert (A.FLAG_NOISE, A.FLAG_SMOOTH, A.FLAG_LOWRES) == (1, 2, 4)


def test_bad_arguments_raise_value_error():
    A = _aug()
    slot = A.FilterSlot(2, 1, (4, 4, 4), "cpu")
    assert slot.records.numel() == 2 * 64 and slot.buf.numel() == 2 * 64 + 2 * 2 * 64
    assert slot.ws.data_ptr() == slot.buf.data_ptr() + 4 * 128                 # one allocation
    x = torch.rand(2, 1, 4, 4, 4)
    with pytest.raises(ValueError, match="no draws"):
        A.augment_filters(x, slot)
    with pytest.raises(ValueError):                                            # draws of another batch size
        slot.load(A.draw_filters(np.random.RandomState(0), 3, (4, 4, 4)))
    d = A.draw_filters(np.random.RandomState(0), 2, (4, 4, 4), prob=1.0)
    d.low_size[1, 2] = 5
    with pytest.raises(ValueError, match="sample 1"):                          # a low grid larger than the volume
        slot.load(d)
    d.low_size[1, 2] = 4
    d.radius[0, 0] = 9
    with pytest.raises(ValueError, match="sample 0"):
        slot.load(d)
    assert slot.draws is None
    slot.draws = A.draw_filters(np.random.RandomState(0), 2, (4, 4, 4))         # (loading needs a device)
    for bad in (x[:1], torch.rand(2, 2, 4, 4, 4), torch.rand(2, 1, 4, 4, 5), x.double(), x.permute(0, 1, 3, 2, 4), x[0]):
        with pytest.raises(ValueError):
            A.augment_filters(bad, slot)
    with pytest.raises(ValueError):
        A.augment_filters(x, slot, out=torch.empty(2, 1, 4, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        A.augment_filters(x, A.IntensitySlot(2, "cpu"))
    for args in ((0, 1, (4, 4, 4)), (2, 0, (4, 4, 4)), (2, 1, (4, 4)), (2, 1, (4, 0, 4)), (1, 2, (1024, 1024, 1024))):
        with pytest.raises(ValueError):
            A.FilterSlot(*args, "cpu")
    # the product path has no CPU fallback: valid arguments on the host reach the binding's device check
    with pytest.raises(RuntimeError):
        A.augment_filters(x, slot)


def test_as_slot_takes_both_kinds_and_lists():
    A = _aug()
    x = torch.rand(2, 1, 4, 4, 4)
    fs, its = A.FilterSlot(2, 1, (4, 4, 4), "cpu"), A.IntensitySlot(2, "cpu")
    assert A.as_slot(fs, x) is fs and A.as_slot(its, x) is its
    assert A.as_slots(fs, x) == [fs] and A.as_slots([its, fs], x) == [its, fs] and A.as_slots((fs, its), x) == [fs, its]
    with pytest.raises(ValueError):
        A.as_slot("noise", x)
    with pytest.raises(ValueError):
        A.as_slots([its, None], x)
    with pytest.raises(ValueError):                                            # draws of another batch size
        A.as_slot(A.draw_filters(np.random.RandomState(0), 3, (4, 4, 4)), x)
    chain = A.AugmentChain([its, fs], x)
    assert chain.augment_slot == [its, fs] and A.AugmentChain(fs, x).augment_slot is fs
