"""numpy restatement of fitting the prediction windows to the foreground bounding box (mivp_amd.inference.WindowFit,
csrc/window_fit.hip): the box of the foreground and the fitted tiling with its work list.  Shared by
tests/test_predict_fit_host.py and tests/test_hip_predict_fit.py."""
import numpy as np


def foreground(vol=None, channel=0, threshold=0.0025, mask=None):
    """bool [H, W, D]: ``vol[channel] > threshold`` (strict, in fp32: NaN is not foreground) of an fp32 [C, H, W, D]
    volume, or ``mask != 0`` of a uint8 [H, W, D] mask."""
    if mask is not None:
        return np.asarray(mask) != 0
    with np.errstate(invalid="ignore"):
        return np.asarray(vol, dtype=np.float32)[channel] > np.float32(threshold)


def box_of(fg):
    """int32 [6] = (lo0, lo1, lo2, hi0, hi1, hi2), inclusive, in image coordinates; empty: lo = dims, hi = -1."""
    if not fg.any():
        return np.array(list(fg.shape) + [-1, -1, -1], dtype=np.int32)
    idx = np.nonzero(fg)
    return np.array([int(i.min()) for i in idx] + [int(i.max()) for i in idx], dtype=np.int32)


def interval_of(r, overlap):
    return max(int(r * (1.0 - float(overlap))), 1)


def count_of(n, r, interval):
    """ceil((n - r) / interval) + 1 in integers."""
    return -(-(n - r) // interval) + 1


def axis_starts(lo, hi, pad, p, r, m, interval):
    """Window starts of one axis on the padded volume for the inclusive box [lo, hi] in image coordinates."""
    b0 = max(lo + pad - m, 0)
    b1 = min(hi + pad + m + 1, p)
    n = b1 - b0
    if n < r:
        b0 = min(max(b0 - (r - n) // 2, 0), p - r)
        n = r
    return [b0 + min(i * interval, n - r) for i in range(count_of(n, r, interval))]


def fitted_origins(box, image_size, roi, overlap, margin=(0, 0, 0)):
    """int32 [N, 3]: origins of the fitted tiling, row-major over the three counts; an empty box gives no window."""
    from mivp_amd.inference import window_padding
    pad, pdims = window_padding(image_size, roi)
    box = [int(b) for b in box]
    if any(box[3 + a] < box[a] for a in range(3)):
        return np.zeros((0, 3), dtype=np.int32)
    axes = [axis_starts(box[a], box[3 + a], pad[a], pdims[a], roi[a], margin[a], interval_of(roi[a], overlap))
            for a in range(3)]
    g = np.stack(np.meshgrid(*[np.asarray(a, dtype=np.int32) for a in axes], indexing="ij"), axis=-1)
    return g.reshape(-1, 3).astype(np.int32)


def fitted_table(origins, rows, codes):
    """(int32 [rows, 4] work list, meta int32 [2] = (windows, entries)): entry w * F + j = window w under codes[j]
    (window-major, flip-minor), word 3 = 1 | code << 1; every remaining row is zero."""
    f = len(codes)
    n = origins.shape[0] * f
    assert n <= rows
    t = np.zeros((rows, 4), dtype=np.int32)
    for w in range(origins.shape[0]):
        for j, m in enumerate(codes):
            t[w * f + j] = (origins[w, 0], origins[w, 1], origins[w, 2], 1 | int(m) << 1)
    return t, np.array([origins.shape[0], n], dtype=np.int32)


def covered(origins, roi, pdims):
    """bool [pdims]: voxels inside at least one window."""
    cov = np.zeros(pdims, dtype=bool)
    for a, b, c in origins.tolist():
        cov[a:a + roi[0], b:b + roi[1], c:c + roi[2]] = True
    return cov
