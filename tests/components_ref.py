"""numpy / scipy restatement of mivp_amd.components for the tests.  It does not import the package.

- ``label_by_value``: connected components of voxels holding the same nonzero value (scipy.ndimage.label per distinct
  value), numbered 1..n in the raster order of each component's first voxel.
- ``postprocess``: the keep / remove filter (size >= min_size and, when ``largest``, the largest component of its
  class; ties to the component whose first voxel comes first)."""
import numpy as np
from scipy import ndimage

CONNECTIVITY = {6: 1, 18: 2, 26: 3}


def structure(connectivity):
    return ndimage.generate_binary_structure(3, CONNECTIVITY[connectivity])


def _components(mask, connectivity):
    """(scipy labels, n, first linear index of each component 1..n)."""
    lab, n = ndimage.label(mask, structure(connectivity))
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    first = np.full(n + 1, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, flat[idx], idx)
    return lab, n, first[1:]


def label_by_value(x, connectivity=6):
    """x [H, W, D] -> (int32 labels, n)."""
    x = np.asarray(x)
    flat_lab = np.zeros(x.size, dtype=np.int64)
    firsts, base = [], 0
    vals = np.unique(x[(x != 0) & (x == x)])          # (NaN voxels are singletons; the tests do not use them)
    for v in vals:
        lab, n, first = _components(x == v, connectivity)
        if n == 0:
            continue
        sel = lab.ravel() > 0
        flat_lab[sel] = lab.ravel()[sel] + base
        firsts.append(first)
        base += n
    out = np.zeros(x.size, dtype=np.int32)
    if base:
        first = np.concatenate(firsts)
        rank = np.empty(base, dtype=np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(base)
        sel = flat_lab > 0
        out[sel] = rank[flat_lab[sel] - 1] + 1
    return out.reshape(x.shape), base


def class_map(x, num_classes):
    """The class of every voxel, -1 for values outside [0, C) and non-integer floats."""
    x = np.asarray(x)
    if np.issubdtype(x.dtype, np.floating):
        with np.errstate(invalid="ignore"):
            ok = (x >= 0) & (x < num_classes) & (x == np.floor(x))
    else:
        ok = (x >= 0) & (x < num_classes)
    c = np.full(x.shape, -1, dtype=np.int64)
    c[ok] = x[ok].astype(np.int64)
    return c


def postprocess(x, num_classes, largest=True, min_size=0, classes=None, connectivity=26):
    """The post-processed copy of the class map x [H, W, D] (same dtype)."""
    x = np.asarray(x)
    out = x.copy()
    cm = class_map(x, num_classes)
    for c in (range(1, num_classes) if classes is None else classes):
        lab, n, first = _components(cm == c, connectivity)
        if n == 0:
            continue
        sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        keep = sizes >= min_size
        if largest:
            top = np.flatnonzero(sizes == sizes.max())
            best = top[np.argmin(first[top])]
            only = np.zeros(n, dtype=bool)
            only[best] = True
            keep &= only
        remove = np.concatenate([[False], ~keep])
        out[remove[lab]] = 0
    return out
