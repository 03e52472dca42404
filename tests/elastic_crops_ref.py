"""numpy float64 restatement of the elastic teacher crop (mivp_amd.batches with ``spatial=True, elastic=nodes``; the second
kernel of csrc/crops_affine.hip; the rule is written out in include/mivp.h), for the tests.

Built on tests/spatial_crops_ref.py: its ``rotate``, ``trilinear`` and ``nearest_inside`` do everything downstream of the
source position ``r``; what is new here is ``r = A (q + d(u)) + t`` with ``d`` the cubic B-spline of the control lattice,
in the slow, obvious form (64 gathers from the lattice per output voxel).  The fp32 ``affine`` and ``lattice`` words are
taken as given; everything after them is float64.  Nothing here shares code with the kernel or with ``batches.py``."""
import numpy as np

import spatial_crops_ref as SR


def basis(f):
    """float64 [4, ...]: the uniform cubic B-spline basis B0..B3 at ``f`` in [0, 1]."""
    f = np.asarray(f, np.float64)
    return np.stack([(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6,
                     f ** 3 / 6])


def knots(roi_k, n_k):
    """(i int64 [roi_k], f float64 [roi_k]) of the output indices 0 .. roi_k - 1 on one axis of ``n_k`` nodes."""
    x = (np.arange(int(roi_k), dtype=np.float64) + 0.5) * (int(n_k) - 3) / int(roi_k)
    i = np.minimum(np.floor(x), int(n_k) - 4).astype(np.int64)
    return i, x - i


def displacement(lattice, roi):
    """float64 [3, h, w, d]: d_c(u) from the lattice float32 [3, n0, n1, n2]."""
    lattice = np.asarray(lattice)
    assert lattice.dtype == np.float32 and lattice.ndim == 4 and lattice.shape[0] == 3
    P = lattice.astype(np.float64)
    i, B = zip(*[(ik, basis(fk)) for ik, fk in (knots(roi[k], lattice.shape[1 + k]) for k in range(3))])
    d = np.zeros((3,) + tuple(int(v) for v in roi))
    for a in range(4):
        for b in range(4):
            for e in range(4):
                w = B[0][a][:, None, None] * B[1][b][None, :, None] * B[2][e][None, None, :]
                d += w[None] * P[:, (i[0] + a)[:, None, None], (i[1] + b)[None, :, None], (i[2] + e)[None, None, :]]
    return d


def positions(affine, roi, origin, n_rot, flag, lattice):
    """float64 [3, h, w, d]: r = A (q + d) + t; with ``flag`` 0 the affine rule's r, the lattice unread."""
    affine = np.asarray(affine)
    assert affine.dtype == np.float32 and affine.shape == (12,)
    A = affine[:9].astype(np.float64).reshape(3, 3)
    roi_a, n_rot = np.asarray(roi, np.int64), np.asarray(n_rot, np.int64)
    pad_before = (roi_a - np.minimum(roi_a, n_rot)) // 2
    half = (roi_a - 1) / 2.0
    u = np.stack(np.meshgrid(*[np.arange(int(k), dtype=np.float64) for k in roi_a], indexing="ij"))
    q = u - half[:, None, None, None]
    if int(flag):
        q = q + displacement(lattice, roi)
    t = half + (np.asarray(origin, np.int64) - pad_before) + affine[9:].astype(np.float64)
    return np.einsum("kj,jhwd->khwd", A, q) + t[:, None, None, None]


def teacher_crop(image, labels, lut, rot, origin, roi, affine, flag, lattice):
    """One sample, as ``spatial_crops_ref.teacher_crop``: float64 image [C, roi], mask [1, roi], coord [3, roi], r [3, roi]."""
    image = np.asarray(image)
    n = image.shape[1:]
    vol = SR.rotate(image, rot)
    m = vol.shape[1:]
    r = positions(affine, roi, origin, m, flag, lattice)
    img = SR.trilinear(vol, r)
    j, ok = SR.nearest_inside(r, m)
    jc = [np.clip(j[k], 0, m[k] - 1) for k in range(3)]
    if labels is None:
        mask = np.zeros((1,) + tuple(roi))
    else:
        mapped = SR.rotate(np.asarray(lut)[np.asarray(labels)].astype(np.float64), rot)
        mask = np.where(ok, mapped[jc[0], jc[1], jc[2]], 0.0)[None]
    p = [r[0], r[1], r[2]]
    if rot:
        a, b = SR.ROT_AXES[rot]
        p[a], p[b] = r[b], (n[b] - 1) - r[a]
    coord = np.stack([np.where(ok, p[k] - (n[k] - 1) / 2.0, 0.0) for k in range(3)])
    return img, mask, coord, r


def teacher_batch(images, labels, lut, volume, rot, origin, roi, affine, flags, lattice):
    """The stacked float64 batch (image, mask, coord, r) from lists of numpy volumes."""
    out = [teacher_crop(images[int(v)], labels[int(v)], lut, int(c), [int(x) for x in o], roi, np.asarray(a, np.float32), int(f),
                        np.asarray(p, np.float32))
           for v, c, o, a, f, p in zip(volume, rot, origin, affine, flags, lattice)]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def linear_lattice(alpha, nodes):
    """float64 [3, n0, n1, n2]: P[c][j] = alpha_c * j_c, whose spline is d_c = alpha_c * (x_c + 1) -- affine in u."""
    P = np.zeros((3,) + tuple(nodes))
    for c in range(3):
        shape = [1, 1, 1]
        shape[c] = nodes[c]
        P[c] = alpha[c] * np.arange(nodes[c], dtype=np.float64).reshape(shape)
    return P


def composed_affine(affine, alpha, nodes, roi):
    """float64 [12]: the affine words under which the AFFINE rule gives the r of ``affine`` with ``linear_lattice(alpha,
    nodes)``.  q + d = diag(1 + alpha s) q + alpha (s roi / 2 + 1) with s = (n - 3) / roi, so A' = A diag(1 + alpha s) and
    the shift grows by A alpha ((n - 3) / 2 + 1)."""
    affine = np.asarray(affine, np.float64)
    A, alpha = affine[:9].reshape(3, 3), np.asarray(alpha, np.float64)
    s = (np.asarray(nodes, np.float64) - 3) / np.asarray(roi, np.float64)
    shift = affine[9:] + A @ (alpha * ((np.asarray(nodes, np.float64) - 3) / 2 + 1))
    return np.concatenate([(A * (1 + alpha * s)[None, :]).reshape(-1), shift])
