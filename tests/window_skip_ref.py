"""numpy restatement of window skipping in whole-volume prediction (mivp_amd.inference.WindowSkip, csrc/window_skip.hip):
the foreground count of every window, the compacted work list and the fill of the uncovered voxels.  Shared by
tests/test_predict_skip_host.py (checked there against a second, voxel-by-voxel form) and tests/test_hip_predict_skip.py."""
import numpy as np


def padded_foreground(image_size, roi, vol=None, channel=0, threshold=0.0025, mask=None):
    """bool [pdims]: the foreground of the zero-padded volume.  ``vol`` fp32 [C, H, W, D] with ``vol[channel] > threshold``
    (strict, in fp32: NaN is not foreground), or ``mask`` uint8 [H, W, D] with ``mask != 0``; padding is never foreground."""
    from mivp_amd.inference import window_padding
    pad, pdims = window_padding(image_size, roi)
    if mask is not None:
        fg = np.asarray(mask) != 0
    else:
        with np.errstate(invalid="ignore"):
            fg = np.asarray(vol, dtype=np.float32)[channel] > np.float32(threshold)
    assert fg.shape == tuple(image_size)
    out = np.zeros(pdims, dtype=bool)
    n = image_size
    out[pad[0]:pad[0] + n[0], pad[1]:pad[1] + n[1], pad[2]:pad[2] + n[2]] = fg
    return out


def occupancy(origins, roi, fg_padded):
    """int32 [N]: foreground voxels per window, by slicing the padded foreground."""
    return np.array([int(fg_padded[a:a + roi[0], b:b + roi[1], c:c + roi[2]].sum()) for a, b, c in origins.tolist()],
                    dtype=np.int32)


def compact(full_table, counts, n_flips, min_voxels):
    """(active table int32 like ``full_table``, meta int32 [2] = (kept windows, kept entries)): the valid entries of the
    windows with ``counts >= min_voxels`` first, in their original order and unchanged, then zero rows."""
    n = counts.shape[0]
    rows = [full_table[e] for e in range(full_table.shape[0])
            if (full_table[e, 3] & 1) and e // n_flips < n and counts[e // n_flips] >= min_voxels]
    out = np.zeros_like(full_table)
    if rows:
        out[:len(rows)] = np.stack(rows)
    kept_windows = int((counts >= min_voxels).sum())
    assert len(rows) == kept_windows * n_flips
    return out, np.array([kept_windows, len(rows)], dtype=np.int32)


def covered(origins, roi, pdims, keep):
    """bool [pdims]: voxels inside at least one kept window."""
    cov = np.zeros(pdims, dtype=bool)
    for (a, b, c), k in zip(origins.tolist(), keep):
        if k:
            cov[a:a + roi[0], b:b + roi[1], c:c + roi[2]] = True
    return cov


def fill(acc, wsum, fill_class, fill_logit):
    """The fill pass on copies of acc [pdims, C] / wsum [pdims]: where wsum == 0, acc = +-fill_logit and wsum = 1."""
    acc, wsum = acc.copy(), wsum.copy()
    empty = wsum == 0
    row = np.full(acc.shape[-1], -fill_logit, dtype=acc.dtype)
    row[fill_class] = fill_logit
    acc[empty] = row
    wsum[empty] = 1
    return acc, wsum
