"""A numpy restatement of the box and scribble prompts (mivp_amd.strokes, csrc/strokes.hip), and the cases the host and the
GPU tests share.  Nothing here imports the package: the restatement is the definition, written a second time.  The error
regions, the padded depth and the squared spacings are those of clicks_ref, the thinning that of skeleton_ref.

Rasteriser.  Step i of a -> b is a + floor((2 i delta + n) / (2 n)), n = max |delta| (numpy's // floors towards minus
infinity).  Encoding.  max(box, stroke) per voxel and channel; the stroke's m is the smallest squared distance to a scribble
voxel of the channel, here as a minimum over those voxels.  Simulated box.  The tight box of the valid object voxels, widened
by margin and jitter and clamped so that it stays inside the volume and meets the object (where inward jitter makes the
corners cross on an axis, hi' = lo' there).  Simulated scribble.  The skeleton
of {depth^2 >= min_depth^2} of each error region, per sample, E_pos as class 1 and E_neg as class 2 of one map."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clicks_ref import DEFAULT_MASK, EXACT_SPACING, SHAPES, classes_of, depth_sq, error_regions, spacing_sq  # noqa: E402,F401
from skeleton_ref import skeletonize_ref  # noqa: E402

DEGENERATE = ((5, 1, 1), (1, 1, 9), (4, 3, 1))


# ---------------------------------------------------------------------------------------------------------- rasteriser
def segment_ref(a, b):
    """int64 [n + 1, 3]: the voxels of the segment a -> b."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    delta = b - a
    n = int(np.abs(delta).max())
    if n == 0:
        return a[None].copy()
    i = np.arange(n + 1, dtype=np.int64)[:, None]
    return a[None] + (2 * i * delta[None] + n) // (2 * n)


def raster_ref(points):
    """The voxels of the polyline, in drawing order (with repetitions)."""
    pts = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    if len(pts) == 1:
        return pts.copy()
    return np.concatenate([segment_ref(pts[i], pts[i + 1]) for i in range(len(pts) - 1)])


def draw_ref(mask, b, points, channel):
    """``mask`` uint8 [B, H, W, D] with the polyline's voxels of sample b or-ed with 1 << channel (a copy)."""
    out = np.array(mask, dtype=np.uint8)
    v = raster_ref(points)
    out[b, v[:, 0], v[:, 1], v[:, 2]] |= np.uint8(1 << channel)
    return out


# ------------------------------------------------------------------------------------------------------------ encoding
def box_ref(boxes, count, dims, mode="filled"):
    """bool [B, 2, H, W, D]: the voxels inside a box of the channel (filled) or on its surface (frame)."""
    boxes, count = np.asarray(boxes), np.asarray(count)
    B, KB = boxes.shape[:2]
    g = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    out = np.zeros((B, 2, *dims), dtype=bool)
    for b in range(B):
        for i in range(min(max(int(count[b]), 0), KB)):
            row = [int(v) for v in boxes[b, i]]
            if row[6] not in (0, 1):
                continue
            lo, hi = row[:3], row[3:6]
            inside = np.ones(dims, dtype=bool)
            edge = np.zeros(dims, dtype=bool)
            for a in range(3):
                inside &= (g[a] >= lo[a]) & (g[a] <= hi[a])
                edge |= (g[a] == lo[a]) | (g[a] == hi[a])
            out[b, row[6]] |= inside & edge if mode == "frame" else inside
    return out


def stroke_dist_sq(seeds, spacing=(1, 1, 1), dtype=np.float64):
    """[H, W, D] of ``dtype``: the smallest squared distance in mm to a voxel of the bool map ``seeds`` (+inf without one), as
    the composition min over the seeds of (a0 dh^2 + a1 dw^2) + a2 dd^2, every step in ``dtype``."""
    dims = seeds.shape
    a = spacing_sq(spacing).astype(dtype)
    hh, ww, dd = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    m = np.full(dims, np.inf, dtype=dtype)
    for h, w, d in np.argwhere(seeds).tolist():
        dist = (a[0] * ((hh - h).astype(dtype) ** 2) + a[1] * ((ww - w).astype(dtype) ** 2)) + a[2] * ((dd - d).astype(dtype) ** 2)
        m = np.minimum(m, dist.astype(dtype))
    return m


def stroke_value(m, kind="disk", radius=2.0, sigma=2.0, dtype=np.float64):
    if kind == "gaussian":
        return np.exp(-m / dtype(np.float32(2.0 * sigma * sigma))).astype(dtype)
    return (m <= dtype(np.float32(radius * radius))).astype(dtype)


def encode_ref(boxes, count, mask, spacing=(1, 1, 1), box="filled", kind="disk", radius=2.0, sigma=2.0, dtype=np.float64):
    """[B, 2, H, W, D] of ``dtype``: max(box, stroke)."""
    mask = np.asarray(mask)
    B, dims = mask.shape[0], mask.shape[1:]
    bx = box_ref(boxes, count, dims, box)
    out = np.zeros((B, 2, *dims), dtype=dtype)
    for b in range(B):
        for ch in range(2):
            m = stroke_dist_sq(((mask[b] >> ch) & 1).astype(bool), spacing, dtype)
            out[b, ch] = np.maximum(bx[b, ch].astype(dtype), stroke_value(m, kind, radius, sigma, dtype))
    return out


# ---------------------------------------------------------------------------------------------------------- simulation
def _object_mask(object_classes):
    return DEFAULT_MASK if object_classes is None else sum(1 << int(c) for c in object_classes)


def object_of(target, object_classes=None, ignore_index=None):
    """bool: the valid voxels of the object."""
    t = classes_of(target)
    valid = t >= 0
    if ignore_index is not None:
        valid &= t != ignore_index
    mask = _object_mask(object_classes)
    bit = np.array([(mask >> c) & 1 for c in range(32)], dtype=bool)
    return valid & bit[np.maximum(t, 0)]


def simulate_box_ref(target, boxes, count, object_classes=None, ignore_index=None, margin=(0, 0, 0), jitter=None, channel=0):
    """New (boxes, count, last) after one simulated box per sample."""
    boxes, count = np.array(boxes, dtype=np.int32), np.array(count, dtype=np.int32)
    B, KB = boxes.shape[:2]
    target = np.asarray(target)
    target = target[:, 0] if target.ndim == 5 else target
    dims = target.shape[1:]
    last = np.zeros((B, 8), dtype=np.int32)
    for b in range(B):
        at = np.argwhere(object_of(target[b], object_classes, ignore_index))
        if len(at) == 0:
            last[b, :6] = -1
            continue
        lo, hi = at.min(axis=0), at.max(axis=0)
        j = np.zeros(6, dtype=np.int64) if jitter is None else np.asarray(jitter[b], dtype=np.int64)
        new_lo = [int(min(max(lo[a] - margin[a] + j[a], 0), hi[a])) for a in range(3)]
        new_hi = [int(min(max(hi[a] + margin[a] + j[3 + a], lo[a]), dims[a] - 1)) for a in range(3)]
        new_hi = [max(new_hi[a], new_lo[a]) for a in range(3)]     # jitter that makes the two corners cross: one voxel thick
        placed = 0 <= count[b] < KB
        if placed:
            boxes[b, count[b]] = new_lo + new_hi + [channel]
            count[b] += 1
        last[b] = new_lo + new_hi + [int(placed), 0]
    return boxes, count, last


def core_map(pred, target, spacing=(1, 1, 1), object_classes=None, ignore_index=None, min_depth=1.5):
    """uint8 [H, W, D] of one sample: 1 in the core of E_pos, 2 in the core of E_neg, 0 elsewhere (float32 depths, as stored)."""
    md2 = np.float32(float(min_depth) * float(min_depth))
    out = np.zeros(np.asarray(pred).shape, dtype=np.uint8)
    for cls, reg in enumerate(error_regions(pred, target, _object_mask(object_classes), ignore_index), start=1):
        out[reg & (depth_sq(reg, spacing).astype(np.float32) >= md2)] = cls
    return out


def simulate_scribbles_ref(pred, target, mask, spacing=(1, 1, 1), object_classes=None, ignore_index=None, min_depth=1.5,
                           max_iter=32, keep_endpoints=True):
    """New (mask, last) after one round of simulated scribbles."""
    mask = np.array(mask, dtype=np.uint8)
    pred, target = np.asarray(pred), np.asarray(target)
    pred = pred[:, 0] if pred.ndim == 5 else pred
    target = target[:, 0] if target.ndim == 5 else target
    B = pred.shape[0]
    last = np.zeros((B, 8), dtype=np.int32)
    converged = True
    for b in range(B):
        core = core_map(pred[b], target[b], spacing, object_classes, ignore_index, min_depth)
        skel, _, conv = skeletonize_ref(core, 3, max_iter=max_iter, keep_endpoints=keep_endpoints)
        converged &= bool(conv)
        for ch in range(2):
            new = (skel == ch + 1) & (((mask[b] >> ch) & 1) == 0)
            last[b, ch] = int(new.sum())
            mask[b][skel == ch + 1] |= np.uint8(1 << ch)
    last[:, 2] = int(converged)
    return mask, last


# -------------------------------------------------------------------------------------------------------------- cases
def _box(dims, lo, hi, value=1):
    m = np.zeros(dims, dtype=np.int64)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = value
    return m


def strokes_for(dims):
    """name -> (points, channel) on a volume of ``dims``: axis-aligned, diagonal, steep, a single point, a polyline that
    revisits voxels; every sign octant occurs."""
    H, W, D = (n - 1 for n in dims)
    return {
        "axis": ([(0, 0, 0), (H, 0, 0)], 0),
        "axis_back": ([(H, W, D), (H, 0, D)], 1),
        "diagonal": ([(0, 0, 0), (min(H, W, D),) * 3], 0),
        "steep": ([(0, W, 0), (H, max(W - 2, 0), min(1, D))], 1),
        "mixed_signs": ([(H, 0, D), (0, W, 0)], 0),
        "point": ([(H // 2, W // 2, D // 2)], 1),
        "revisit": ([(0, 0, 0), (H, W, D), (0, 0, 0), (H, 0, D), (H // 2, W, 0), (H, 0, D)], 0),
    }


def scribble_cases():
    """name -> dict(pred, target [B, H, W, D] uint8, kwargs): sample 0 is the named situation."""
    d1, d0, d2 = SHAPES[1], SHAPES[0], SHAPES[2]
    zero1 = np.zeros(d1, dtype=np.int64)
    blob = _box(d1, (2, 3, 2), (13, 12, 10))                       # 11 x 9 x 8: a thick missing blob
    sliver = _box(d1, (4, 4, 4), (12, 6, 6))                       # 8 x 2 x 2: depth 1 everywhere
    both_p, both_t = _box(d1, (1, 1, 1), (7, 8, 9)), _box(d1, (9, 7, 2), (15, 15, 11))
    cases = {
        "thick_blob": dict(pred=np.stack([zero1, sliver]), target=np.stack([blob, zero1]), kwargs={}),
        "sliver": dict(pred=np.stack([zero1, zero1]), target=np.stack([sliver, blob]), kwargs={}),
        "both_regions": dict(pred=np.stack([both_p, zero1]), target=np.stack([both_t, blob]), kwargs={}),
        "no_error": dict(pred=np.stack([blob, both_t]), target=np.stack([blob, both_t]), kwargs={}),
        "one_iteration": dict(pred=np.stack([zero1, both_p]), target=np.stack([blob, both_t]), kwargs=dict(max_iter=1)),
        "no_endpoints": dict(pred=np.stack([zero1, both_p]), target=np.stack([blob, both_t]),
                             kwargs=dict(keep_endpoints=False, min_depth=1.0)),
        "anisotropic": dict(pred=np.stack([zero1, both_p]), target=np.stack([blob, both_t]),
                            kwargs=dict(spacing=EXACT_SPACING, min_depth=1.0)),
    }
    # B = 3 with odd H: a sample's slabs start at an even offset of the stacked map, or its skeleton changes
    odd = [(_box(d2, (0, 0, 0), (0, 0, 0)), _box(d2, (3 + b, 2, 1), (20 + 4 * b, 15 + b, 8))) for b in range(3)]
    cases["odd_batch"] = dict(pred=np.stack([p for p, _ in odd]), target=np.stack([t for _, t in odd]), kwargs={})
    t0 = _box(d0, (1, 1, 0), (12, 9, 7))
    t0[6] = np.where(t0[6] > 0, 2, 0)
    cases["ignore_and_classes"] = dict(pred=np.zeros((2, *d0), dtype=np.int64), target=np.stack([t0, _box(d0, (2, 2, 1), (11, 8, 6), 3)]),
                                       kwargs=dict(ignore_index=2, object_classes=(1, 3), min_depth=1.0))
    for c in cases.values():
        c["pred"], c["target"] = c["pred"].astype(np.uint8), c["target"].astype(np.uint8)
    return cases
