"""Plain torch / numpy restatement of the training-batch sampling (mivp_amd.batches, csrc/crops.hip), for the tests.

Deliberately the slow, obvious form: ``torch.rot90`` of the WHOLE volume, then slicing, then ``F.pad`` with zeros -- no
index arithmetic.  The coordinate grid is ``students_teacher.coord_grid`` of the stored volume, rotated and cropped like
the image (the reference loads the grid before ``Rotate90d``, datasets/transforms.py:182-197), and the label map is the loop
of ``map_label_indices`` (modules/utils.py:372-388).  Works on CPU and GPU tensors alike."""
import torch
import torch.nn.functional as F

ROT_AXES = {1: (0, 1), 2: (0, 2), 3: (1, 2)}


def map_label_indices(masks: torch.Tensor, active_labels):
    """modules/utils.py:372-388, on a float copy."""
    masks = masks.clone().float()
    active = sorted(active_labels)
    keep = torch.zeros_like(masks, dtype=torch.bool)
    for label in active:
        keep |= masks == float(label)
    masks[~keep] = 0
    for new, label in enumerate(active):
        masks[masks == label] = float(new)
    return masks


def rotate(v: torch.Tensor, rot: int) -> torch.Tensor:
    """``v`` [..., H, W, D] under rotation code ``rot`` (0: as it is)."""
    if rot == 0:
        return v
    a, b = ROT_AXES[rot]
    nd = v.dim() - 3
    return torch.rot90(v, 1, (nd + a, nd + b))


def crop_pad(v: torch.Tensor, origin, size) -> torch.Tensor:
    """``v`` [..., n0, n1, n2] -> [..., size]: the slice of min(size, n) voxels at ``origin``, then SpatialPad's symmetric
    zero pad (the larger half after the crop)."""
    sl, pads = [], []
    for k in range(3):
        n = v.shape[v.dim() - 3 + k]
        take = min(size[k], n)
        sl.append(slice(int(origin[k]), int(origin[k]) + take))
        total = size[k] - take
        pads.append((total // 2, total - total // 2))
    v = v[(Ellipsis, *sl)]
    flat = [p for k in (2, 1, 0) for p in pads[k]]              # F.pad counts from the last axis
    return F.pad(v, flat).contiguous()


def teacher_crop(image, labels, rot, origin, roi, active_labels=None, coord_grid=None):
    """One sample: image [C, H, W, D] (+ uint8 labels [H, W, D] or None) -> (image [C, roi], mask [1, roi], coord [3, roi])."""
    img = crop_pad(rotate(image, rot), origin, roi)
    if labels is None:
        mask = torch.zeros((1,) + tuple(roi), dtype=torch.float32, device=image.device)
    else:
        lab = labels.float() if active_labels is None else map_label_indices(labels, list(active_labels))
        mask = crop_pad(rotate(lab[None], rot), origin, roi)
    coord = None
    if coord_grid is not None:
        coord = crop_pad(rotate(coord_grid(tuple(image.shape[1:]), image.device), rot), origin, roi)
    return img, mask, coord


def teacher_batch(images, labels, draws, roi, active_labels=None, coord_grid=None):
    """The stacked batch of ``draws`` (fields ``volume``, ``rot``, ``origin``) from lists of volumes."""
    out = [teacher_crop(images[int(v)], labels[int(v)], int(r), [int(a) for a in o], roi, active_labels, coord_grid)
           for v, r, o in zip(draws.volume, draws.rot, draws.origin)]
    img = torch.stack([o[0] for o in out])
    mask = torch.stack([o[1] for o in out])
    coord = torch.stack([o[2] for o in out]) if coord_grid is not None else None
    return img, mask, coord


def student_view(t: torch.Tensor, origins, size) -> torch.Tensor:
    """``t`` [B, C, roi] -> [B, C, size]: per sample the crop at ``origins[b]`` with the same pad rule."""
    return torch.stack([crop_pad(t[b], [int(a) for a in origins[b]], size) for b in range(t.shape[0])])
