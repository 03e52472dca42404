"""numpy / Python restatement of mivp_amd.skeleton for the tests.  It does not import the package and uses no
scikit-image: the skeletons are defined by the algorithm written out here, not by Lee94.

The neighbourhood of a voxel is a 26-bit mask, bit k for ``OFFSETS26[k]`` (the offsets in lexicographic order without the
centre).  ``ADJ26[k]`` / ``ADJ6[k]`` are the masks of the neighbourhood positions 26- / 6-adjacent to position k; the two
connectivity tests are flood fills over them, one position at a time.

``skeletonize_ref`` is a per-voxel loop: mark the border on the state an iteration starts from, then eight sub-passes over
the subfields ``(h&1)<<2 | (w&1)<<1 | (d&1)`` in the order 0..7, each deleting, one voxel after the other and in place, the
marked voxels that are simple on the current state (and no end points, when those are kept).  Voxels of one subfield are
never adjacent, so deleting them one after the other is what a parallel sub-pass does."""
import itertools
import math

import numpy as np

OFFSETS26 = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
FORWARD_OFFSETS = [o for o in OFFSETS26 if o > (0, 0, 0)]                  # first non-zero component positive
_IDX27 = [9 * (a + 1) + 3 * (b + 1) + (c + 1) for a, b, c in OFFSETS26]    # positions in a raveled 3 x 3 x 3 block


def _adjacent(k, j, face_only):
    diff = [abs(a - b) for a, b in zip(OFFSETS26[k], OFFSETS26[j])]
    if k == j:
        return False
    return sum(diff) == 1 if face_only else max(diff) == 1


ADJ26 = [sum(1 << j for j in range(26) if _adjacent(k, j, False)) for k in range(26)]
ADJ6 = [sum(1 << j for j in range(26) if _adjacent(k, j, True)) for k in range(26)]
N6_MASK = sum(1 << k for k, o in enumerate(OFFSETS26) if sum(abs(a) for a in o) == 1)
N18_MASK = sum(1 << k for k, o in enumerate(OFFSETS26) if sum(abs(a) for a in o) <= 2)


def _flood(seed, allowed, adj):
    """the component of the one-bit mask `seed` within `allowed` under the adjacency table `adj`"""
    comp, frontier = seed, seed
    while frontier:
        k = frontier.bit_length() - 1
        frontier &= ~(1 << k)
        new = adj[k] & allowed & ~comp
        comp |= new
        frontier |= new
    return comp


def simple_point(obj):
    """(26, 6) simple point from the 26-bit mask of object neighbours"""
    if obj == 0:
        return False
    if _flood(obj & -obj, obj, ADJ26) != obj:
        return False
    bg = ~obj & N18_MASK
    bg6 = bg & N6_MASK
    if bg6 == 0:
        return False
    return bg6 & ~_flood(bg6 & -bg6, bg, ADJ6) == 0


def end_point(obj):
    return bin(obj).count("1") <= 1


def select_classes(labels, num_classes, classes=None):
    """uint8 map: the class where it is an integer in [0, C) and in `classes` (default 1..C-1), else 0"""
    x = np.asarray(labels)
    cls = list(range(1, num_classes)) if classes is None else list(classes)
    xf = x.astype(np.float64)
    ok = (xf >= 0) & (xf < num_classes) & (xf == np.floor(xf)) & np.isin(xf, cls)
    return np.where(ok, xf, 0).astype(np.uint8)


def _obj_mask(pad, h, w, d):
    """26-bit mask of the neighbours of the padded voxel (h, w, d) that hold its value"""
    block = pad[h - 1:h + 2, w - 1:w + 2, d - 1:d + 2].ravel()
    c = block[13]
    return sum(1 << k for k, i in enumerate(_IDX27) if block[i] == c)


def border_marks(pad):
    """object voxels of the zero-padded state with a face neighbour that does not hold their value"""
    c = pad[1:-1, 1:-1, 1:-1]
    diff = np.zeros(c.shape, dtype=bool)
    for axis in range(3):
        for side in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[axis] = slice(side, pad.shape[axis] - 2 + side)
            diff |= pad[tuple(sl)] != c
    return (c != 0) & diff


def skeletonize_ref(labels, num_classes, classes=None, keep_endpoints=True, max_iter=None):
    """-> (skeleton uint8 of the input's shape, iterations, converged): `iterations` counts the iterations that ran, the
    one that deleted nothing included; with `max_iter` the loop stops after that many at the latest."""
    x = np.asarray(labels)
    shape = x.shape
    vol = select_classes(x.reshape(shape[-3:]), num_classes, classes)
    pad = np.pad(vol, 1)
    it, converged = 0, False
    while not converged and (max_iter is None or it < max_iter):
        it += 1
        marks = border_marks(pad)
        deleted = 0
        for s in range(8):
            ph, pw, pd = (s >> 2) & 1, (s >> 1) & 1, s & 1
            sub = np.argwhere(marks[ph::2, pw::2, pd::2])
            for kh, kw, kd in sub.tolist():
                h, w, d = 2 * kh + ph + 1, 2 * kw + pw + 1, 2 * kd + pd + 1
                obj = _obj_mask(pad, h, w, d)
                if simple_point(obj) and not (keep_endpoints and end_point(obj)):
                    pad[h, w, d] = 0
                    deleted += 1
        converged = deleted == 0
    return pad[1:-1, 1:-1, 1:-1].copy().reshape(shape), it, converged


# ------------------------------------------------------------------------------------------------------- counts and metrics
def centerline_counts(pred, target, skel_pred, skel_target, num_classes):
    """int64 [C, 4]: |S_P|, |S_P and V_L|, |S_L|, |S_L and V_P| per class (the label maps read as select_classes reads them,
    with every class selected)."""
    every = list(range(num_classes))
    p, t = select_classes(pred, num_classes, every).reshape(-1), select_classes(target, num_classes, every).reshape(-1)
    sp, sl = np.asarray(skel_pred).reshape(-1), np.asarray(skel_target).reshape(-1)
    out = np.zeros((num_classes, 4), dtype=np.int64)
    for c in range(1, num_classes):
        out[c] = [(sp == c).sum(), ((sp == c) & (t == c)).sum(), (sl == c).sum(), ((sl == c) & (p == c)).sum()]
    return out


def _ratio(num, den):
    return np.float64(num) / np.float64(den) if den > 0 else np.float64(0.0)


def centerline_metrics(counts, classes):
    """-> dict: tprec, tsens, cldice float64 [C] (0 where a denominator is 0) and their means over `classes`, the terms
    added in ascending class order"""
    C = counts.shape[0]
    tprec = np.array([_ratio(counts[c, 1], counts[c, 0]) for c in range(C)], dtype=np.float64)
    tsens = np.array([_ratio(counts[c, 3], counts[c, 2]) for c in range(C)], dtype=np.float64)
    cl = np.array([np.float64(2.0) * p * s / (p + s) if p + s > 0 else np.float64(0.0) for p, s in zip(tprec, tsens)],
                  dtype=np.float64)
    out = dict(tprec=tprec, tsens=tsens, cldice=cl)
    for k, v in (("mean_tprec", tprec), ("mean_tsens", tsens), ("mean_cldice", cl)):
        acc = np.float64(0.0)
        for i, c in enumerate(sorted(classes)):
            acc = v[c] if i == 0 else acc + v[c]
        out[k] = acc / np.float64(len(classes))
    return out


def skeleton_stats(skel, num_classes, classes=None):
    """int64 [C, 18] per class of `classes`: voxels; voxels with 0, 1, 2, >= 3 same-class 26-neighbours; the 13 forward edge
    counts"""
    vol = select_classes(np.asarray(skel).reshape(np.asarray(skel).shape[-3:]), num_classes, classes)
    pad = np.pad(vol, 1)
    out = np.zeros((num_classes, 18), dtype=np.int64)
    for h, w, d in np.argwhere(pad != 0).tolist():
        c = int(pad[h, w, d])
        obj = _obj_mask(pad, h, w, d)
        out[c, 0] += 1
        out[c, 1 + min(bin(obj).count("1"), 3)] += 1
        for k, off in enumerate(FORWARD_OFFSETS):
            if pad[h + off[0], w + off[1], d + off[2]] == c:
                out[c, 5 + k] += 1
    return out


def length_mm(stats, spacing):
    """float64 [C]: sum_k edges_k * |offset_k * spacing|, added in the order of FORWARD_OFFSETS"""
    weights = [math.sqrt(sum((o * float(s)) ** 2 for o, s in zip(off, spacing))) for off in FORWARD_OFFSETS]
    acc = None
    for k, wgt in enumerate(weights):
        term = stats[:, 5 + k].astype(np.float64) * np.float64(wgt)
        acc = term if acc is None else acc + term
    return acc


def voxel_dice(pred, target, c):
    p, t = np.asarray(pred) == c, np.asarray(target) == c
    return 2.0 * (p & t).sum() / (p.sum() + t.sum())


# ------------------------------------------------------------------------------------------------------- test volumes
def blobs(shape, seed, num_classes=3, threshold=0.1, sigma=2.0):
    """Gaussian-filtered noise thresholded at +-threshold: class 1 above, class 2 below (and class 3 in a band around 0 when
    num_classes == 4); values are uint8"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal(shape), sigma)
    f = f / np.abs(f).max()
    out = np.zeros(shape, dtype=np.uint8)
    out[f > threshold] = 1
    if num_classes >= 3:
        out[f < -threshold] = 2
    if num_classes >= 4:
        out[np.abs(f) < threshold / 4] = 3
    return out


def bar(shape=(9, 9, 20), size=(7, 7, 18)):
    x = np.zeros(shape, dtype=np.uint8)
    at = [(a - b) // 2 for a, b in zip(shape, size)]
    x[at[0]:at[0] + size[0], at[1]:at[1] + size[1], at[2]:at[2] + size[2]] = 1
    return x


def thick_ring(n=13, r_out=5.5, r_in=2.5, thick=3):
    """a ring of square-ish cross-section in the h-w plane, `thick` planes along d: one tunnel"""
    x = np.zeros((n, n, thick + 2), dtype=np.uint8)
    c = (n - 1) / 2.0
    hh, ww = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    r = np.sqrt((hh - c) ** 2 + (ww - c) ** 2)
    x[(r <= r_out) & (r >= r_in), 1:1 + thick] = 1
    return x


def shell(n=9):
    """a cube of side n - 2 with a 3^3 cavity in the middle"""
    x = np.zeros((n, n, n), dtype=np.uint8)
    x[1:-1, 1:-1, 1:-1] = 1
    m = n // 2
    x[m - 1:m + 2, m - 1:m + 2, m - 1:m + 2] = 0
    return x


def tube(length=24, radius=2, shape=(9, 9, 28)):
    """a straight tube along d"""
    x = np.zeros(shape, dtype=np.uint8)
    ch, cw = shape[0] // 2, shape[1] // 2
    hh, ww = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    disc = (hh - ch) ** 2 + (ww - cw) ** 2 <= radius * radius
    at = (shape[2] - length) // 2
    x[disc, at:at + length] = 1
    return x
