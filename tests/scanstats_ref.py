"""numpy restatement of mivp_amd.scanstats (the module docstring there has the definitions): the shifted-bincount
histogram, the nearest-rank order statistic, the integer moments, and the two window plans through ``scan.intensity_map``.
Everything here works on the selected values themselves, not on a histogram, so it shares no step with the kernels."""
import math

import numpy as np

NBINS, OFFSET = 65536, 32768
FLT_MAX = float(np.finfo(np.float32).max)


def selected(raw_c, mask=None, above=None):
    """The selected values of one channel ([H, W, D] integer array) as a flat int64 array."""
    v = np.asarray(raw_c).astype(np.int64)
    keep = np.ones(v.shape, dtype=bool)
    if mask is not None:
        keep &= np.asarray(mask) != 0
    if above is not None:
        keep &= v > int(above)
    return v[keep]


def histogram(raw, mask=None, above=None):
    """int64 [C, 65536] of raw [C, H, W, D] (int16 or uint8): bin = value + 32768."""
    raw = np.asarray(raw)
    return np.stack([np.bincount(selected(raw[c], mask, above) + OFFSET, minlength=NBINS).astype(np.int64)
                     for c in range(raw.shape[0])])


def rank(q, n):
    """k = max(1, ceil(q * N)) with one float64 multiply."""
    return max(1, int(math.ceil(float(q) * float(n))))


def order_statistic(v, q):
    """np.sort(v)[k - 1]; 0 for an empty selection."""
    v = np.asarray(v).reshape(-1)
    if v.size == 0:
        return 0
    return int(np.sort(v)[rank(q, v.size) - 1])


def moments(v):
    """(N, S1, S2) as Python integers and (mean, population std) in float64; (0, 0) for an empty selection."""
    v = np.asarray(v).reshape(-1).astype(np.int64)
    n = int(v.size)
    s1, s2 = int(v.sum()), int((v * v).sum())                    # |v| <= 2^15 and N < 2^31: both fit int64
    if n == 0:
        return 0, 0, 0, 0.0, 0.0
    mean = float(s1) / float(n)
    std = math.sqrt(max(0.0, float(s2) / float(n) - mean * mean))
    return n, s1, s2, mean, std


def fma_f32(x, s, t):
    """Correctly rounded fp32 ``x * s + t`` for fp32 ``s``, ``t`` and integer (or fp32) ``x`` with |x| < 2^24, any shape.
    The product is exact in float64; the sum is rounded to odd there (its error is recovered exactly with TwoSum), so the
    final rounding to fp32 is the one of the infinitely precise result."""
    p = np.asarray(x).astype(np.float64) * np.float64(np.float32(s))
    tt = np.float64(np.float32(t))
    sm = p + tt
    bb = sm - p
    err = (p - (sm - bb)) + (tt - bb)
    even = (sm.view(np.int64) & 1) == 0
    nudge = np.nextafter(sm, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, nudge, sm).astype(np.float32)


def apply_map(x, words, clip=True):
    """v = clamp(fma(x, s, t), lo, hi) in fp32 with words = (s, t, lo, hi, ...)."""
    y = fma_f32(x, words[0], words[1])
    if clip:
        y = np.minimum(np.maximum(y, np.float32(words[2])), np.float32(words[3]))
    return y.astype(np.float32)


def percentile_plan(v, q_lo, q_hi, b_min=0.0, b_max=1.0):
    """The eight slot words of IntensityWindow.percentile as float64 values (round each to fp32 to compare)."""
    from mivp_amd.scan import intensity_map
    a_lo, a_hi = order_statistic(v, q_lo), order_statistic(v, q_hi)
    _, _, _, mean, std = moments(v)
    if a_hi == a_lo:
        head = (0.0, float(np.float32(b_min)), float(np.float32(b_min)), float(np.float32(b_max)))
    else:
        head = intensity_map(a_lo, a_hi, b_min, b_max)
    return np.array(head + (float(a_lo), float(a_hi), mean, std), dtype=np.float64)


def zscore_plan(v, clip=None):
    """The eight slot words of IntensityWindow.zscore as float64 values; lo / hi are the fp32 fma of the ROUNDED s, t."""
    q_lo, q_hi = (0.0, 1.0) if clip is None else clip
    a_lo, a_hi = order_statistic(v, q_lo), order_statistic(v, q_hi)
    n, _, _, mean, std = moments(v)
    if n == 0 or std == 0.0:
        s, t = 1.0, -mean
    else:
        s, t = 1.0 / std, -mean / std
    if clip is None:
        lo, hi = -FLT_MAX, FLT_MAX
    else:
        lo, hi = float(fma_f32(a_lo, s, t)), float(fma_f32(a_hi, s, t))
    return np.array((s, t, lo, hi, float(a_lo), float(a_hi), mean, std), dtype=np.float64)


def ulp_distance(a, b):
    """Steps between two finite fp32 values along the fp32 number line."""
    def key(x):
        i = int(np.float32(x).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))
