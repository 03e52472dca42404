"""Plain numpy restatement of the class-balanced crop centres (mivp_amd.batches.ClassIndex / ClassCropDraws,
csrc/crops_index.hip), for the tests.

Deliberately the obvious form: the class map is ``lut[lab]``, the ``rank``-th voxel of class ``c`` is
``np.flatnonzero(class_map.ravel() == c)[rank]``, its position is ``np.unravel_index``, the rotation is ``np.rot90`` of a
volume that holds every voxel's own flat index (where that index lands is where the voxel goes), and the origin is the
clamp of ``correct_crop_centers``.  No prefix sums, no chunks except in ``chunk_prefix``, which counts chunk by chunk."""
import numpy as np

ROT_AXES = {1: (0, 1), 2: (0, 2), 3: (1, 2)}
CHUNK = 1024


def class_map(lab, lut, num_classes):
    """int64 [H, W, D]: the class of every voxel, -1 where ``lut[lab] >= num_classes`` (no class)."""
    c = np.asarray(lut)[np.asarray(lab)].astype(np.int64)
    c[c >= num_classes] = -1
    return c


def chunk_prefix(lab, lut, num_classes, chunk=CHUNK):
    """int64 [num_classes][nchunks + 1]: exclusive prefix sums of the per-chunk class counts, the last column the total."""
    c = class_map(lab, lut, num_classes).ravel()
    nch = -(-c.size // chunk)
    out = np.zeros((num_classes, nch + 1), dtype=np.int64)
    for k in range(num_classes):
        for j in range(nch):
            out[k, j + 1] = out[k, j] + np.count_nonzero(c[j * chunk:(j + 1) * chunk] == k)
    return out


def rotated_positions(shape, rot):
    """(pos, n_rot): ``pos[q]`` is the flat position, in the volume rotated by code ``rot``, of stored voxel ``q``."""
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    turned = idx if rot == 0 else np.rot90(idx, 1, ROT_AXES[rot])
    pos = np.empty(idx.size, dtype=np.int64)
    pos[turned.ravel()] = np.arange(idx.size)
    return pos, turned.shape


def voxel(lab, lut, num_classes, c, rank):
    """The flat index of the ``rank``-th voxel of class ``c``."""
    return int(np.flatnonzero(class_map(lab, lut, num_classes).ravel() == c)[rank])


def rank_of(lab, lut, num_classes, p):
    """(class, rank) of stored voxel ``p``: how many voxels of its class come before it."""
    c = class_map(lab, lut, num_classes)
    q = int(np.ravel_multi_index(p, c.shape))
    k = int(c.ravel()[q])
    return k, int(np.count_nonzero(c.ravel()[:q] == k))


def origin(lab, lut, num_classes, rot, c, rank, roi):
    """(origin, clamped): the crop origin in the rotated frame of the sample (c, rank) under code ``rot``, and whether the
    clamp moved it on any axis."""
    pos, n_rot = rotated_positions(np.shape(lab), rot)
    r = np.unravel_index(pos[voxel(lab, lut, num_classes, c, rank)], n_rot)
    want = [int(r[k]) - roi[k] // 2 for k in range(3)]
    got = [min(max(want[k], 0), max(n_rot[k] - roi[k], 0)) for k in range(3)]
    return got, got != want


def origins(labels, lut, num_classes, draws, roi):
    """(int32 [B, 3], bool [B]) of ``draws`` (fields ``volume``, ``rot``, ``cls``, ``rank``) from the list of label maps:
    ``origin`` for every sample, the per-volume work shared."""
    vol, rot = np.asarray(draws.volume), np.asarray(draws.rot)
    cls, rank = np.asarray(draws.cls), np.asarray(draws.rank)
    out = np.zeros((len(vol), 3), dtype=np.int32)
    moved = np.zeros(len(vol), dtype=bool)
    for v in np.unique(vol):
        cm = class_map(labels[int(v)], lut, num_classes).ravel()
        of_class = {int(c): np.flatnonzero(cm == c) for c in np.unique(cls[vol == v])}
        for code in np.unique(rot[vol == v]):
            pos, n_rot = rotated_positions(np.shape(labels[int(v)]), int(code))
            for c, members in of_class.items():
                sel = np.flatnonzero((vol == v) & (rot == code) & (cls == c))
                if not len(sel):
                    continue
                r = np.stack(np.unravel_index(pos[members[rank[sel]]], n_rot), axis=1)
                want = r - np.asarray(roi) // 2
                got = np.minimum(np.maximum(want, 0), np.maximum(np.asarray(n_rot) - np.asarray(roi), 0))
                out[sel] = got
                moved[sel] = (got != want).any(axis=1)
    return out, moved
