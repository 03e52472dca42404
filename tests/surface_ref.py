"""numpy restatement of the surface-distance metrics of mivp_amd.surface (test helper, not a test module).

The surface is found by explicit 6-neighbour checks on a zero-padded copy and the directed distances by brute-force
pairwise distances, so nothing here shares an algorithm with the HIP kernels (or with scipy).  ``scipy_metrics`` states
the same definitions through scipy.ndimage for volumes too large for brute force."""
import math

import numpy as np

KEYS = ("hd", "hd_p", "assd", "nsd")


def class_mask(labels, c):
    """labels == c for a class map of any dtype (values outside [0, C) or non-integer floats match no class)."""
    lab = np.asarray(labels)
    return lab == c


def surface(mask):
    """In the mask with at least one of the 6 face neighbours outside the mask or outside the volume."""
    m = np.asarray(mask, dtype=bool)
    p = np.zeros(tuple(s + 2 for s in m.shape), dtype=bool)
    p[1:-1, 1:-1, 1:-1] = m
    inner = np.ones_like(m)
    H, W, D = m.shape
    for a in range(3):
        for s in (-1, 1):
            sl = [slice(1, H + 1), slice(1, W + 1), slice(1, D + 1)]
            sl[a] = slice(1 + s, m.shape[a] + 1 + s)
            inner &= p[tuple(sl)]
    return m & ~inner


def surface_map(labels, num_classes):
    """uint8 map: the class on its surface voxels, 255 elsewhere; and the per-class counts."""
    lab = np.asarray(labels)
    out = np.full(lab.shape, 255, dtype=np.uint8)
    counts = np.zeros(num_classes, dtype=np.int64)
    for c in range(num_classes):
        s = surface(class_mask(lab, c))
        out[s] = c
        counts[c] = int(s.sum())
    return out, counts


def directed(src, dst, spacing, chunk=2048):
    """For every True voxel of src, the distance in mm to the nearest True voxel of dst (brute force, float64)."""
    a = np.argwhere(src).astype(np.float64) * np.asarray(spacing, dtype=np.float64)
    b = np.argwhere(dst).astype(np.float64) * np.asarray(spacing, dtype=np.float64)
    if len(b) == 0:
        return np.full(len(a), np.inf)
    out = np.empty(len(a))
    for i in range(0, len(a), chunk):
        d2 = ((a[i:i + chunk, None, :] - b[None, :, :]) ** 2).sum(-1)
        out[i:i + chunk] = np.sqrt(d2.min(1))
    return out


def combine(d_ab, d_ba, percentile, tolerance):
    """The per-class values from the two directed sets, with the empty-surface rules."""
    na, nb = len(d_ab), len(d_ba)
    if na == 0 and nb == 0:
        return {k: math.nan for k in KEYS}
    if na == 0 or nb == 0:
        return {"hd": math.inf, "hd_p": math.inf, "assd": math.inf, "nsd": 0.0}
    return {"hd": max(d_ab.max(), d_ba.max()),
            "hd_p": max(np.percentile(d_ab, percentile, method="linear"), np.percentile(d_ba, percentile, method="linear")),
            "assd": (d_ab.sum() + d_ba.sum()) / (na + nb),
            "nsd": (int((d_ab <= tolerance).sum()) + int((d_ba <= tolerance).sum())) / (na + nb)}


def _metrics(pred, target, num_classes, spacing, percentile, tolerance, include_background, directed_fn, surface_fn):
    out = {k: np.full(num_classes, np.nan) for k in KEYS}
    counts = np.zeros((num_classes, 2), dtype=np.int64)
    for c in range(num_classes):
        sa, sb = surface_fn(class_mask(pred, c)), surface_fn(class_mask(target, c))
        counts[c] = (int(sa.sum()), int(sb.sum()))
        if c == 0 and not include_background:
            continue
        v = combine(directed_fn(sa, sb, spacing), directed_fn(sb, sa, spacing), percentile, tolerance)
        for k in KEYS:
            out[k][c] = v[k]
    out["surface_voxels"] = counts
    return out


def metrics(pred, target, num_classes, spacing=(1.0, 1.0, 1.0), percentile=95.0, tolerance=1.0,
            include_background=False):
    """Brute-force restatement: dict of float64 [C] hd, hd_p, assd, nsd and int64 surface_voxels [C, 2]."""
    return _metrics(np.asarray(pred), np.asarray(target), num_classes, spacing, percentile, tolerance,
                    include_background, directed, surface)


def scipy_surface(mask):
    from scipy.ndimage import binary_erosion, generate_binary_structure
    m = np.asarray(mask, dtype=bool)
    return m & ~binary_erosion(m, generate_binary_structure(3, 1), border_value=0)


def scipy_directed(src, dst, spacing):
    from scipy.ndimage import distance_transform_edt
    if not dst.any():
        return np.full(int(src.sum()), np.inf)
    return distance_transform_edt(~dst, sampling=spacing)[src]


def scipy_metrics(pred, target, num_classes, spacing=(1.0, 1.0, 1.0), percentile=95.0, tolerance=1.0,
                  include_background=False):
    """The same definitions through scipy.ndimage (binary_erosion, distance_transform_edt)."""
    return _metrics(np.asarray(pred), np.asarray(target), num_classes, spacing, percentile, tolerance,
                    include_background, scipy_directed, scipy_surface)


def assert_metrics_close(got, want, rel):
    """Equal nan / inf pattern and relative error <= rel on the finite values; exact surface counts."""
    for k in KEYS:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape, k
        assert np.array_equal(np.isnan(g), np.isnan(w)), (k, g, w)
        assert np.array_equal(np.isinf(g), np.isinf(w)), (k, g, w)
        f = np.isfinite(w)
        err = np.abs(g[f] - w[f]) / np.maximum(np.abs(w[f]), 1e-300)
        assert np.all((err <= rel) | (g[f] == w[f])), (k, g, w, err)
    assert np.array_equal(np.asarray(got["surface_voxels"]), np.asarray(want["surface_voxels"]))


def ellipsoid_pair(shape, seed=0):
    """A 2-class target (ellipsoid) and a perturbed prediction (shifted, rescaled ellipsoid), uint8 numpy maps."""
    rng = np.random.default_rng(seed)
    H, W, D = shape
    h, w, d = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij")
    c = np.array([H, W, D], dtype=np.float64) / 2
    r = np.array([H, W, D], dtype=np.float64) * 0.3
    tgt = (((h - c[0]) / r[0]) ** 2 + ((w - c[1]) / r[1]) ** 2 + ((d - c[2]) / r[2]) ** 2 <= 1.0)
    c2 = c + rng.uniform(-3, 3, 3)
    r2 = r * rng.uniform(0.9, 1.1, 3)
    prd = (((h - c2[0]) / r2[0]) ** 2 + ((w - c2[1]) / r2[1]) ** 2 + ((d - c2[2]) / r2[2]) ** 2 <= 1.0)
    return prd.astype(np.uint8), tgt.astype(np.uint8)
