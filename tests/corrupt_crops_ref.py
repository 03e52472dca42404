"""Plain numpy restatement of the students' corruption of the batch filler (mivp_amd.batches with ``corruption=True``,
csrc/crops_corrupt.hip; the rule is written out in include/mivp.h), for the tests.  Integers are computed in uint64 and
masked to 32 bits; the noise is computed in float32 numpy operations, one rounding each, so the device must give the same
BITS.  The slow, obvious form: boolean masks per hole, a copy per shuffle hole."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
M24 = np.uint64(0xFFFFFF)


def hash32(counter, key):
    """The counter-based hash (common.hpp's dropout hash) of uint32 counters under a 32-bit key -> uint32 array."""
    key = np.uint64(int(key) & 0xFFFFFFFF)
    t = (np.asarray(counter).astype(np.uint64) + key) & M32
    t ^= t >> np.uint64(16)
    t = ((t & M24) * np.uint64(0xB5AD4F)) & M32
    t ^= t >> np.uint64(13)
    rot = ((key << np.uint64(13)) | (key >> np.uint64(19))) & M32
    return ((((t & M24) * np.uint64(0x6C62B9)) & M32) + (t >> np.uint64(8)) + rot) & M32


def uniform(counter, key):
    """u in [0, 1): the top 24 bits of the hash times 2^-24, exact in float32."""
    return (hash32(counter, key) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def value_range(x):
    """(lo, hi) of one sample over all channels, a zero extreme as +0."""
    return np.float32(x.min()) + np.float32(0), np.float32(x.max()) + np.float32(0)


def noise(lo, hi, counter, key):
    """lo + (hi - lo) * u in float32: the difference, the product and the sum rounded one by one."""
    span = np.float32(hi) - np.float32(lo)
    t = (span * uniform(counter, key)).astype(np.float32)
    return (np.float32(lo) + t).astype(np.float32)


def permutation(n, key):
    """int64 [n]: P(j), the keyed bijection of {0 .. n-1} (four Feistel rounds over the next even bit count, cycle
    walking)."""
    n = int(n)
    bits = (n - 1).bit_length() if n > 1 else 0
    bits = max(2, (bits + 1) & ~1)
    half = bits // 2
    mask = np.uint64((1 << half) - 1)
    v = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, bool)
    for _ in range(1 << bits):
        left, right = v[todo] >> np.uint64(half), v[todo] & mask
        for rnd in range(4):
            left, right = right, left ^ ((hash32(right + np.uint64(64 * rnd), key) >> np.uint64(16)) & mask)
        v[todo] = (left << np.uint64(half)) | right
        todo = v >= n
        if not todo.any():
            break
    assert not todo.any()
    return v.astype(np.int64)


def holes_of(draws, s, b):
    """[(origin, size, key)] of (student s, sample b), the holes that are read."""
    return [(tuple(int(a) for a in draws.origin[s, b, k]), tuple(int(a) for a in draws.size[s, b, k]),
             int(draws.hole_key[s, b, k])) for k in range(int(draws.n_holes[s, b]))]


def union_mask(shape, holes):
    """bool [H, W, D]: the union of the holes."""
    m = np.zeros(shape, bool)
    for o, e, _ in holes:
        m[o[0]:o[0] + e[0], o[1]:o[1] + e[1], o[2]:o[2] + e[2]] = True
    return m


def corrupt_sample(x, mode, holes, key):
    """One sample ``x`` float32 [C, H, W, D] -> its corrupted copy."""
    x = np.array(x, dtype=np.float32)
    if mode == 0:
        return x
    if mode in (1, 2):
        lo, hi = value_range(x)
        inside = union_mask(x.shape[1:], holes)
        replace = np.broadcast_to(inside if mode == 1 else ~inside, x.shape)
        fresh = noise(lo, hi, np.arange(x.size, dtype=np.uint64).reshape(x.shape), key)
        return np.where(replace, fresh, x)
    for o, e, hole_key in holes:                                    # in list order: later holes see earlier ones
        sl = (slice(None), slice(o[0], o[0] + e[0]), slice(o[1], o[1] + e[1]), slice(o[2], o[2] + e[2]))
        perm = permutation(e[0] * e[1] * e[2], hole_key)
        old = x[sl].reshape(x.shape[0], -1).copy()
        x[sl] = old[:, perm].reshape((x.shape[0],) + e)
    return x


def corrupt_student(image_st, draws, s):
    """``image_st`` float32 [B, C, H, W, D] of student ``s`` -> the corrupted batch."""
    return np.stack([corrupt_sample(image_st[b], int(draws.mode[s, b]), holes_of(draws, s, b), int(draws.key[s, b]))
                     for b in range(image_st.shape[0])])
