"""numpy float64 restatement of the interpolating teacher crop (mivp_amd.batches with ``spatial=True``,
csrc/crops_affine.hip; the rule is written out in include/mivp.h), for the tests.

Deliberately the slow, obvious form: ``np.rot90`` of the WHOLE volume, one dense array of source positions, eight gathers
from a zero-padded copy.  The fp32 ``affine`` words are taken as given; everything after them is float64.  Nothing here
shares code with the kernel or with ``batches.py``."""
import numpy as np

ROT_AXES = {1: (0, 1), 2: (0, 2), 3: (1, 2)}


def rotate(v, rot):
    """``v`` [..., H, W, D] under rotation code ``rot``."""
    if rot == 0:
        return v
    a, b = ROT_AXES[rot]
    nd = v.ndim - 3
    return np.rot90(v, 1, (nd + a, nd + b))


def positions(affine, roi, origin, n_rot):
    """float64 [3, h, w, d]: where output voxel u reads in the rotated volume."""
    affine = np.asarray(affine)
    assert affine.dtype == np.float32 and affine.shape == (12,)
    A = affine[:9].astype(np.float64).reshape(3, 3)
    s = affine[9:].astype(np.float64)
    roi = np.asarray(roi, np.int64)
    n_rot = np.asarray(n_rot, np.int64)
    pad_before = (roi - np.minimum(roi, n_rot)) // 2
    half = (roi - 1) / 2.0
    u = np.stack(np.meshgrid(*[np.arange(int(k), dtype=np.float64) for k in roi], indexing="ij"))
    q = u - half[:, None, None, None]
    t = half + (np.asarray(origin, np.int64) - pad_before) + s
    return np.einsum("kj,jhwd->khwd", A, q) + t[:, None, None, None]


def trilinear(vol, r):
    """``vol`` [C, m0, m1, m2] at positions ``r`` [3, ...]: zero outside, along D, then W, then H."""
    vol = np.asarray(vol, np.float64)
    m = np.array(vol.shape[1:])
    finite = np.isfinite(r).all(axis=0)
    r = np.where(finite, r, -5.0)
    i = np.floor(r)
    w = r - i
    i = i.astype(np.int64)
    padded = np.pad(vol, ((0, 0), (1, 1), (1, 1), (1, 1)))          # index c + 1; the rim holds the zeros
    far = ((i < -1) | (i > (m - 1).reshape(3, *[1] * (r.ndim - 1)))).any(axis=0)    # every corner outside

    def corner(e0, e1, e2):
        c = [np.clip(i[k] + e + 1, 0, m[k] + 1) for k, e in enumerate((e0, e1, e2))]
        return padded[:, c[0], c[1], c[2]]

    def lerp(a, b, wk):
        return a + wk * (b - a)

    c00, c01 = lerp(corner(0, 0, 0), corner(0, 0, 1), w[2]), lerp(corner(0, 1, 0), corner(0, 1, 1), w[2])
    c10, c11 = lerp(corner(1, 0, 0), corner(1, 0, 1), w[2]), lerp(corner(1, 1, 0), corner(1, 1, 1), w[2])
    out = lerp(lerp(c00, c01, w[1]), lerp(c10, c11, w[1]), w[0])
    return np.where(far | ~finite, 0.0, out)


def nearest_inside(r, m):
    """(j int64 [3, ...], inside bool [...]): j = floor(r + 0.5), inside the volume on every axis."""
    finite = np.isfinite(r).all(axis=0)
    j = np.floor(np.where(finite, r, -5.0) + 0.5).astype(np.int64)
    ok = finite.copy()
    for k in range(3):
        ok &= (j[k] >= 0) & (j[k] < m[k])
    return j, ok


def teacher_crop(image, labels, lut, rot, origin, roi, affine):
    """One sample.  image float [C, H, W, D], labels uint8 [H, W, D] or None, lut uint8 [256] -> float64 image [C, roi],
    mask [1, roi], coord [3, roi], and the positions r [3, roi]."""
    image = np.asarray(image)
    n = image.shape[1:]
    vol = rotate(image, rot)
    m = vol.shape[1:]
    r = positions(affine, roi, origin, m)
    img = trilinear(vol, r)
    j, ok = nearest_inside(r, m)
    jc = [np.clip(j[k], 0, m[k] - 1) for k in range(3)]
    if labels is None:
        mask = np.zeros((1,) + tuple(roi))
    else:
        mapped = rotate(np.asarray(lut)[np.asarray(labels)].astype(np.float64), rot)
        mask = np.where(ok, mapped[jc[0], jc[1], jc[2]], 0.0)[None]
    p = [r[0], r[1], r[2]]
    if rot:
        a, b = ROT_AXES[rot]
        p[a], p[b] = r[b], (n[b] - 1) - r[a]
    coord = np.stack([np.where(ok, p[k] - (n[k] - 1) / 2.0, 0.0) for k in range(3)])
    return img, mask, coord, r


def teacher_batch(images, labels, lut, volume, rot, origin, roi, affine):
    """The stacked float64 batch (image, mask, coord, r) from lists of numpy volumes."""
    out = [teacher_crop(images[int(v)], labels[int(v)], lut, int(c), [int(x) for x in o], roi, np.asarray(a, np.float32))
           for v, c, o, a in zip(volume, rot, origin, affine)]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))
