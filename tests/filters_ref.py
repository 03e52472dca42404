"""numpy restatement of the noise / blur / low-resolution chain (mivp_amd.augment.augment_filters, csrc/filters.hip),
parameterised by dtype: float64 is the oracle, float32 the yardstick of what single precision can give -- and, for the blur,
the exact arithmetic the kernel has to reproduce bit for bit.

  noise    v = x + (mean + std g), g = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((h1 >> 8) + 1) 2^-24, u2 = (h2 >> 8) 2^-24,
           h1 / h2 = drop_hash(2 idx / 2 idx + 1, key), idx the element's C-order index inside the sample (uint32)
  smooth   D, then W, then H: out[i] = sum_{k = -r..r} tap[k] in[i + k] over a zero-padded axis, accumulated from -r upwards
           into +0.0, every product and every sum rounded on its own; radius 0 leaves the axis alone
  low-res  torch's nearest down-sampling to the low grid, then trilinear up-sampling (align_corners=False), D, W, H

Deliberately another formulation than the kernel's: whole-array shifts of a padded copy instead of tiles with halos, and a
low-resolution volume that is materialised and then up-sampled instead of eight reads of the full grid per voxel."""
import numpy as np

NOISE, SMOOTH, LOWRES = 1, 2, 4
MAX_RADIUS = 8
_M32 = np.uint64(0xFFFFFFFF)


def _umul24(a, b):
    """__umul24: the low 24 bits of each operand, the low 32 bits of the product."""
    return ((a.astype(np.uint64) & np.uint64(0xFFFFFF)) * np.uint64(b & 0xFFFFFF) & _M32).astype(np.uint32)


def drop_hash(idx, key):
    """csrc/common.hpp drop_hash on a uint32 array of counters under one uint32 key."""
    key = int(key) & 0xFFFFFFFF
    t = ((np.asarray(idx).astype(np.uint64) + np.uint64(key)) & _M32).astype(np.uint32)
    t ^= t >> np.uint32(16)
    t = _umul24(t, 0xB5AD4F)
    t ^= t >> np.uint32(13)
    rot = ((key << 13) | (key >> 19)) & 0xFFFFFFFF
    s = _umul24(t, 0x6C62B9).astype(np.uint64) + (t >> np.uint32(8)).astype(np.uint64) + np.uint64(rot)
    return (s & _M32).astype(np.uint32)


def uniforms(n, key):
    """The exact uniforms of elements 0..n-1 as float64 (both are multiples of 2^-24): u1 in (0, 1], u2 in [0, 1)."""
    idx = np.arange(n, dtype=np.uint64)
    h1 = drop_hash((2 * idx) & _M32, key)
    h2 = drop_hash((2 * idx + 1) & _M32, key)
    return ((h1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24, (h2 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def gaussian(n, key, dtype):
    """Box-Muller values of elements 0..n-1, every operation in ``dtype`` (2 pi rounded to it first)."""
    t = np.dtype(dtype).type
    u1, u2 = (u.astype(dtype) for u in uniforms(n, key))
    rad = np.sqrt(t(-2.0) * np.log(u1))
    g = rad * np.cos(t(2.0 * np.pi) * u2)
    assert g.dtype == np.dtype(dtype)
    return g


def add_noise(v, key, mean, std, dtype):
    t = np.dtype(dtype).type
    g = gaussian(v.size, key, dtype).reshape(v.shape)
    return v + (t(mean) + t(std) * g)


def blur_axis(v, axis, r, taps17, dtype):
    """One pass along ``axis``; ``taps17`` is the centred float32 row of the draws."""
    r = int(r)
    if r == 0:
        return v
    n = v.shape[axis]
    pad = [(0, 0)] * v.ndim
    pad[axis] = (r, r)
    p = np.pad(v, pad)
    acc = np.zeros_like(v)
    for k in range(-r, r + 1):
        sl = [slice(None)] * v.ndim
        sl[axis] = slice(r + k, r + k + n)
        prod = np.dtype(dtype).type(taps17[MAX_RADIUS + k]) * p[tuple(sl)]
        acc = acc + prod
    assert acc.dtype == np.dtype(dtype)
    return acc


def blur(v, radius, taps, dtype):
    """[C, H, W, D]: the D pass, the W pass, the H pass; radius / taps in axis order H, W, D."""
    for a in (2, 1, 0):
        v = blur_axis(v, 1 + a, radius[a], taps[a], dtype)
    return v


def nearest_index(N, n):
    """Full-grid index that low-grid index j reads, j = 0..n-1: torch's ``nearest`` rule, always in float32."""
    scale = np.float32(N) / np.float32(n)
    return np.minimum(np.floor(np.arange(n, dtype=np.float32) * scale).astype(np.int64), N - 1)


def linear_taps(n, N, dtype):
    """Up-sampling n -> N, torch's ``linear`` rule with align_corners=False in ``dtype``: (lo, hi, weight of hi)."""
    t = np.dtype(dtype).type
    scale = t(n) / t(N)
    s = np.maximum(scale * (np.arange(N, dtype=dtype) + t(0.5)) - t(0.5), t(0))
    lo = np.minimum(s.astype(np.int64), n - 1)
    hi = np.minimum(lo + 1, n - 1)
    w = s - lo.astype(dtype)
    assert w.dtype == np.dtype(dtype)
    return lo, hi, w


def _blend(a, b, w):
    with np.errstate(invalid="ignore"):
        return np.where(w == 0, a, a + w * (b - a))


def low_res(v, low, dtype):
    """[C, H, W, D] down to the grid ``low`` (nearest) and back (trilinear: D, then W, then H)."""
    dims = v.shape[1:]
    lowvol = v
    for a in range(3):
        lowvol = np.take(lowvol, nearest_index(dims[a], int(low[a])), axis=1 + a)
    out = lowvol
    for a in (2, 1, 0):
        lo, hi, w = linear_taps(int(low[a]), dims[a], dtype)
        shape = [1] * 4
        shape[1 + a] = dims[a]
        out = _blend(np.take(out, lo, axis=1 + a), np.take(out, hi, axis=1 + a), w.reshape(shape))
    assert out.dtype == np.dtype(dtype) and out.shape == v.shape
    return out


def chain_sample(x, flags, key, mean, std, radius, taps, low, dtype=np.float64):
    v = np.asarray(x, dtype=dtype).copy()
    if flags & NOISE:
        v = add_noise(v, key, mean, std, dtype)
    if flags & SMOOTH:
        v = blur(v, radius, taps, dtype)
    if flags & LOWRES:
        v = low_res(v, low, dtype)
    assert v.dtype == np.dtype(dtype)
    return v


def chain(x, d, dtype=np.float64):
    """A batch [B, C, H, W, D] through the draws ``d`` (augment.FilterDraws)."""
    return np.stack([chain_sample(x[b], int(d.flags[b]), int(d.noise_key[b]), d.noise_mean[b], d.noise_std[b], d.radius[b],
                                  d.taps[b], d.low_size[b], dtype) for b in range(x.shape[0])])


def rel_err(got, want64):
    """max |got - oracle| / (max - min of the oracle); an oracle without range (a constant output) is measured against
    max(|value|, 1)."""
    want64 = np.asarray(want64, dtype=np.float64)
    span = float(want64.max() - want64.min())
    if span == 0.0:
        span = max(abs(float(want64.max())), 1.0)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want64).max() / span)
