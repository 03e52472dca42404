"""Training batches sampled on the device from a bank of resident scans: the reference's ``Rotate90d`` (a ``OneOf`` over
three axis pairs), ``RandSpatialCropSamplesd``, ``SpatialPadd``, ``CopyItemsd``, the per-student ``RandSpatialCropd`` +
``SpatialPadd``, ``LoadCoordGridd`` (datasets/transforms.py:84-98,186-212,299-313,323-344) and ``map_label_indices``
(modules/utils.py:372-388), as gathers of csrc/crops.hip from volumes that ``scan.prepare_scan`` / ``scan.prepare_labels``
left in HBM.

It follows ``augment`` and ``multiview``: the draws are made on the host (``draw_crops``), checked against the bank
(``CropDraws.check``) and held by a fixed device slot (``CropSlot``); ``BatchFiller.fill`` issues the launches, which read the
slot at run time, into output tensors allocated once.  Nothing is read back and nothing is allocated per step, so ``fill``
records into a graph, and a ``train.GraphedStep`` recorded on the filler's tensors is fed by a ``fill`` before each replay.

The draw rule restates MONAI's documented ``get_random_patch`` (a uniform integer origin per axis); MONAI's own draw
streams are not reproduced (``Compose`` reseeds every child transform), so parity is unpinned at that boundary, as for
``augment`` and ``scan``.  The draw ORDER documented at ``draw_crops`` is this project's.

Class-balanced crops (csrc/crops_index.hip): ``ClassIndex`` keeps, per volume, the prefix sums of the
per-chunk class counts of its label map; ``draw_class_crops`` draws a class and a rank among that class's voxels
(``RandCropByPosNegLabeld`` / ``RandCropByLabelClassesd``; MONAI's stream is not reproduced here either), and a class-mode
``CropSlot`` has the device turn (class, rank) into the crop origin -- ``resolve``, one launch in front of the teacher's --
so the label map is never read back and a recorded ``fill`` still follows the slot.

Random flip, rotation and zoom (csrc/crops_affine.hip): ``draw_spatial`` draws one affine map per sample
(``SpatialDraws``), a ``SpatialSlot`` holds the maps on the device beside the ``CropSlot``, and a filler built with
``spatial=True`` issues the interpolating teacher launch in place of the plain one -- trilinear for the image, nearest for
the labels, analytic coordinates; the pick and the students' launches are the same as without it.

Elastic deformation (the second kernel of csrc/crops_affine.hip): ``draw_elastic`` draws, per sample, a coin
and a small control lattice of displacements (``ElasticDraws``), an ``ElasticSlot`` holds them on the device beside the
other two slots, and a filler built with ``spatial=True, elastic=nodes`` issues ``mivp_crop_fill_elastic`` for the teacher:
the cubic B-spline of the lattice is added to the output offset in front of the affine map, evaluated on the fly.

The students' own corruption (csrc/crops_corrupt.hip): ``draw_student_corruption`` draws, per student and
sample, one of none / coarse dropout / coarse keep / coarse shuffle with its holes and keys (``CorruptionDraws``, the
reference's ``students_rand_ts``), a ``CorruptionSlot`` holds the records on the device, and a filler built with
``corruption=True`` corrupts ``image_st[i]`` in place after the student crops, two launches per student."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import check_gpu, check_int_from, i3, plain_int

HEAD = 5                        # int32 words per sample in front of the students' origins: volume, rot, origin[3] (mivp.h)
ROT_AXES = {1: (0, 1), 2: (0, 2), 3: (1, 2)}    # rotation code -> the spatial axes of torch.rot90(k=1)
MAX_CHANNELS = 16
MAX_CLASSES = 16                # of a ClassIndex (mivp.h)


def _size3(name: str, v) -> Tuple[int, int, int]:
    v = tuple(v) if not plain_int(v) else (v, v, v)
    if len(v) != 3:
        raise ValueError(f"{name} must be three sizes, got {v!r}")
    return tuple(check_int_from(name, a, 1) for a in v)


def _gpu_device(who: str, device) -> torch.device:
    """``device`` as a GPU device with its index filled in; ``ValueError`` in ``who``'s name for anything else."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who}: a GPU device expected (no CPU fallback)")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _refuse(who: str, bad: np.ndarray, what):
    """``ValueError`` naming the first sample at which ``bad`` [B] holds; ``what(b)`` says what is wrong with it."""
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{who}: sample {b}: {what(b)}")


def _check_rot_and_students(who: str, rot, st, roi, sizes):
    """What ``CropDraws.check`` and ``ClassCropDraws.check`` share: the rotation codes [B] and the students' origins
    [S, B, 3] against ``roi`` and the student ``sizes``."""
    _refuse(who, (rot < 0) | (rot > 3), lambda b: f"rotation code {int(rot[b])} outside 0..3")
    for s, size in enumerate(sizes):
        for k in range(3):
            hi = max(roi[k] - size[k], 0)
            _refuse(who, (st[s, :, k] < 0) | (st[s, :, k] > hi),
                    lambda b: f"origin {st[s, b].tolist()} of student {s} outside [0, {hi}] on axis {k} (roi {roi}, student "
                              f"size {size})")


def _draw_start(who: str, n_bank: int, ids_kind: str, volume_ids, roi, num_samples, student_sizes):
    """The prologue of ``draw_crops`` and ``draw_class_crops``: (roi, student sizes, ids, B, volume [B], rot [B] = 0,
    student_origin [S, B, 3] = 0) after the checks they share; no draw is made here."""
    roi = _size3("roi", roi)
    sizes = [_size3("student size", s) for s in student_sizes]
    ids = [int(v) for v in volume_ids]
    check_int_from("num_samples", num_samples, 1)
    if not ids or any(not 0 <= v < n_bank for v in ids):
        raise ValueError(f"{who}: volume_ids {ids} must be a non-empty list of {ids_kind} in 0..{n_bank - 1}")
    B = len(ids) * int(num_samples)
    return (roi, sizes, ids, B, np.repeat(np.asarray(ids, np.int32), int(num_samples)), np.zeros(B, np.int32),
            np.zeros((len(sizes), B, 3), np.int32))


def _draw_orientation(rs, rot, n_ids: int, num_samples: int):
    """Step 1 of both draw orders: one ``rs.randint(3)`` per volume, held by all its samples."""
    for i in range(n_ids):
        rot[i * num_samples:(i + 1) * num_samples] = int(rs.randint(3)) + 1


def _draw_student_origins(rs, st, roi, sizes):
    """Step 3 of both draw orders: per sample, per student and per axis one ``rs.randint(0, roi - min(s, roi) + 1)``."""
    for b in range(st.shape[1]):
        for s, size in enumerate(sizes):
            for k in range(3):
                st[s, b, k] = rs.randint(0, roi[k] - min(size[k], roi[k]) + 1)


def rotated_shape(shape, rot: int) -> Tuple[int, int, int]:
    """The extents of a stored ``[H, W, D]`` volume after rotation code ``rot``."""
    n = list(shape)
    if rot:
        a, b = ROT_AXES[int(rot)]
        n[a], n[b] = n[b], n[a]
    return tuple(n)


def record_words(n_students: int) -> int:
    return HEAD + 3 * int(n_students)


@dataclass
class CropDraws:
    """What one step draws on the host, one entry per sample of the batch."""
    volume: np.ndarray              # int32 [B]: the bank's volume id
    rot: np.ndarray                 # int32 [B]: 0 none, 1 / 2 / 3 = rot90(k=1) over the spatial axes (0,1) / (0,2) / (1,2)
    origin: np.ndarray              # int32 [B, 3]: the crop origin in the rotated frame
    student_origin: np.ndarray      # int32 [S, B, 3]: each student's origin inside the teacher crop

    @property
    def batch(self) -> int:
        return int(np.shape(self.volume)[0])

    @property
    def n_students(self) -> int:
        return int(np.shape(self.student_origin)[0])

    def pack(self) -> np.ndarray:
        """int32 [B, 5 + 3 S]: the slot's records."""
        B, S = self.batch, self.n_students
        w = np.zeros((B, record_words(S)), dtype=np.int32)
        w[:, 0], w[:, 1], w[:, 2:HEAD] = self.volume, self.rot, self.origin
        for s in range(S):
            w[:, HEAD + 3 * s:HEAD + 3 * s + 3] = self.student_origin[s]
        return w

    @classmethod
    def unpack(cls, words: np.ndarray, n_students: int) -> "CropDraws":
        w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, record_words(n_students))
        st = np.stack([w[:, HEAD + 3 * s:HEAD + 3 * s + 3] for s in range(n_students)]) if n_students \
            else np.zeros((0, w.shape[0], 3), np.int32)
        return cls(w[:, 0].copy(), w[:, 1].copy(), w[:, 2:HEAD].copy(), st.copy())

    def check(self, bank, roi, student_sizes=()):
        """Every draw against the bank (a ``VolumeBank`` or its list of shapes): a wrong id or origin would send the kernel
        to memory that is not the bank's, so nothing unchecked is ever uploaded.  Raises ``ValueError`` naming the sample."""
        shapes = bank.shapes if hasattr(bank, "shapes") else list(bank)
        roi = _size3("roi", roi)
        sizes = [_size3("student size", s) for s in student_sizes]
        arrays = [np.asarray(a) for a in (self.volume, self.rot, self.origin, self.student_origin)]
        if any(a.dtype.kind not in "iu" for a in arrays):
            raise ValueError("CropDraws: integer arrays expected")
        vol, rot, org, st = arrays
        B = vol.shape[0] if vol.ndim == 1 else -1
        if B < 1 or rot.shape != (B,) or org.shape != (B, 3) or st.shape != (len(sizes), B, 3):
            raise ValueError(f"CropDraws: volume [B], rot [B], origin [B, 3] and student_origin [{len(sizes)}, B, 3] of one "
                             f"batch size expected, got {vol.shape}, {rot.shape}, {org.shape}, {st.shape}")
        _refuse("CropDraws", (vol < 0) | (vol >= len(shapes)),
                lambda b: f"volume id {int(vol[b])} outside the bank's 0..{len(shapes) - 1}")
        _check_rot_and_students("CropDraws", rot, st, roi, sizes)
        for b in range(B):
            n_rot = rotated_shape(shapes[int(vol[b])], int(rot[b]))
            for k in range(3):
                hi = max(n_rot[k] - roi[k], 0)
                if not 0 <= int(org[b, k]) <= hi:
                    raise ValueError(f"CropDraws: sample {b}: origin {org[b].tolist()} outside [0, {hi}] on axis {k} (rotated "
                                     f"volume {n_rot}, roi {roi})")
        return self


def draw_crops(rs: np.random.RandomState, bank_shapes, volume_ids: Sequence[int], roi, num_samples: int,
               random_orientation: bool = False, student_sizes=()) -> CropDraws:
    """The host draws of one batch of ``len(volume_ids) * num_samples`` crops from ONE RandomState, in this order:

    1. for each volume of ``volume_ids``, in order: one ``rs.randint(3)`` if ``random_orientation`` (code = that + 1; it
       holds for all ``num_samples`` crops of the volume: the reference rotates before ``RandSpatialCropSamplesd``);
    2. then per sample and per axis: ``rs.randint(0, n_rot - min(roi, n_rot) + 1)``, the crop origin in the rotated frame;
    3. then per sample, per student and per axis: ``rs.randint(0, roi - min(s, roi) + 1)``.

    Sample ``i * num_samples + j`` is crop ``j`` of ``volume_ids[i]``.  The uniform origin restates MONAI's documented
    ``get_random_patch``; MONAI's own stream is NOT reproduced (``Compose`` reseeds every child), so parity is unpinned at the
    MONAI boundary and this order is the project's own."""
    shapes = list(bank_shapes)
    roi, sizes, ids, B, volume, rot, st = _draw_start("draw_crops", len(shapes), "ids", volume_ids, roi, num_samples,
                                                      student_sizes)
    d = CropDraws(volume, rot, np.zeros((B, 3), np.int32), st)
    if random_orientation:
        _draw_orientation(rs, d.rot, len(ids), num_samples)
    for b in range(B):
        n_rot = rotated_shape(shapes[int(d.volume[b])], int(d.rot[b]))
        for k in range(3):
            d.origin[b, k] = rs.randint(0, n_rot[k] - min(roi[k], n_rot[k]) + 1)
    _draw_student_origins(rs, d.student_origin, roi, sizes)
    return d


def label_table(active_labels=None) -> np.ndarray:
    """The 256-entry uint8 table of ``map_label_indices`` (modules/utils.py:372-388): a value of the sorted active list goes
    to its index, every other value to 0.  ``None``: the identity."""
    if active_labels is None:
        return np.arange(256, dtype=np.uint8)
    labels = sorted(int(v) for v in active_labels)
    if not labels or len(set(labels)) != len(labels) or labels[0] < 0 or labels[-1] > 255:
        raise ValueError(f"label_table: active_labels must be distinct values in 0..255, got {list(active_labels)!r}")
    t = np.zeros(256, dtype=np.uint8)
    for i, v in enumerate(labels):
        t[v] = i
    return t


class VolumeBank:
    """The resident volumes a batch is cut from: fp32 ``[C, H, W, D]`` images (what ``scan.prepare_scan`` returns; a leading
    batch axis of 1 is dropped) with optional uint8 ``[H, W, D]`` label maps (``scan.prepare_labels``).  Shapes differ from
    volume to volume, the channel count is the bank's.  The bank keeps the tensors alive -- the device source table holds
    their addresses.  The table is ONE allocation of ``capacity`` rows made here and never replaced: ``add`` writes its row
    in place (stream-ordered, non-blocking), an unused row holds a null image pointer, which the kernel refuses.  A ``fill``
    recorded in a graph therefore keeps a valid table pointer for the bank's lifetime and sees volumes added later."""

    def __init__(self, device, channels: int = 1, capacity: int = 256):
        self.device = _gpu_device("VolumeBank", device)
        self.channels = check_int_from("channels", channels, 1)
        if self.channels > MAX_CHANNELS:
            raise ValueError(f"VolumeBank: channels must be in 1..{MAX_CHANNELS}, got {channels}")
        self.capacity = check_int_from("capacity", capacity, 1)
        self.images, self.labels, self.shapes = [], [], []
        self.table = torch.zeros((self.capacity, 5), dtype=torch.int64, device=self.device)    # int64 [capacity, 5] (mivp.h)

    def __len__(self) -> int:
        return len(self.images)

    def add(self, image: torch.Tensor, labels: Optional[torch.Tensor] = None) -> int:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("VolumeBank.add: not while a graph is being recorded (the table row is copied from the host)")
        if len(self.images) >= self.capacity:
            raise ValueError(f"VolumeBank.add: the bank is full (capacity {self.capacity}; the source table is never "
                             "reallocated, recorded graphs hold its address)")
        check_gpu("image", image)
        if image.dim() == 5 and image.shape[0] == 1:
            image = image[0]
        if image.dim() != 4 or image.shape[0] != self.channels or image.dtype != torch.float32 or not image.is_contiguous() \
                or image.device != self.device or image.numel() == 0 or image.numel() >= 2 ** 31:
            raise ValueError(f"VolumeBank.add: image must be a contiguous fp32 [{self.channels}, H, W, D] tensor on "
                             f"{self.device} with fewer than 2^31 elements, got {image.dtype} {tuple(image.shape)} on "
                             f"{image.device}")
        shape = tuple(int(v) for v in image.shape[1:])
        if labels is not None:
            check_gpu("labels", labels)
            if labels.dim() == 5 and labels.shape[0] == 1 and labels.shape[1] == 1:
                labels = labels[0, 0]
            if labels.dtype != torch.uint8 or tuple(labels.shape) != shape or not labels.is_contiguous() \
                    or labels.device != self.device:
                raise ValueError(f"VolumeBank.add: labels must be a contiguous uint8 {shape} tensor on {self.device}, got "
                                 f"{labels.dtype} {tuple(labels.shape)} on {labels.device}")
        vid = len(self.images)
        row = torch.tensor([image.data_ptr(), 0 if labels is None else labels.data_ptr(), *shape], dtype=torch.int64)
        self.table[vid].copy_(row.pin_memory(), non_blocking=True)
        self.images.append(image)
        self.labels.append(labels)
        self.shapes.append(shape)
        return vid


class ClassIndex:
    """Where the voxels of each class are, per volume of ``bank``, for class-balanced crops.

    A voxel belongs to class ``c = label_table(active_labels)[lab]`` if ``c < num_classes`` (1..16), otherwise to no
    class; voxels count in C order of the stored ``[H, W, D]`` label map, in chunks of ``CHUNK`` voxels.  Each indexed volume
    gets an int32 ``[num_classes][nchunks + 1]`` tensor (``prefix[vid]``): the exclusive prefix sums of the per-chunk class
    counts, the last column the class total.  ``table`` -- int64 ``[bank.capacity][2]`` = (pointer to that tensor or 0,
    nchunks) -- is ONE allocation made here and never replaced, like the bank's source table: a graph recorded earlier
    serves volumes indexed later.

    ``update()`` indexes every bank volume not indexed yet (two launches each) and leaves ``counts`` on the host: numpy
    int64 ``[n_volumes][num_classes]``, what ``draw_class_crops`` and ``ClassCropDraws.check`` read.  It is outside the step:
    it makes one blocking read per call and refuses during a graph capture."""

    CHUNK = 1024

    def __init__(self, bank: "VolumeBank", num_classes: int, active_labels=None):
        if not isinstance(bank, VolumeBank):
            raise ValueError("ClassIndex: a VolumeBank expected (a GPU bank: no CPU fallback)")
        if not plain_int(num_classes) or not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"ClassIndex: num_classes must be an integer in 1..{MAX_CLASSES}, got {num_classes!r}")
        self.bank, self.num_classes = bank, int(num_classes)
        self.lut = torch.from_numpy(label_table(active_labels)).to(bank.device)
        self.table = torch.zeros((bank.capacity, 2), dtype=torch.int64, device=bank.device)      # (mivp.h)
        self.prefix = []
        self.counts = np.zeros((0, self.num_classes), dtype=np.int64)

    def __len__(self) -> int:
        return len(self.prefix)

    def update(self) -> "ClassIndex":
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClassIndex.update: not while a graph is being recorded (it reads the class totals back)")
        bank, first = self.bank, len(self.prefix)
        for vid in range(first, len(bank)):
            if bank.labels[vid] is None:
                raise ValueError(f"ClassIndex.update: volume {vid} of the bank has no label map")
        new = []
        for vid in range(first, len(bank)):
            lab = bank.labels[vid]
            nch = -(-lab.numel() // self.CHUNK)
            t = torch.empty((self.num_classes, nch + 1), dtype=torch.int32, device=bank.device)
            L.call("mivp_label_index_build", L.ptr(lab), lab.numel(), L.ptr(self.lut), self.num_classes, L.ptr(t), nch,
                   L.stream())
            new.append(t)
        if new:
            totals = torch.stack([t[:, -1] for t in new]).cpu().numpy().astype(np.int64)          # the one blocking read
            rows = torch.tensor([[t.data_ptr(), t.shape[1] - 1] for t in new], dtype=torch.int64)
            self.table[first:first + len(new)].copy_(rows.pin_memory(), non_blocking=True)
            self.prefix += new
            self.counts = np.concatenate([self.counts, totals])
        return self


@dataclass
class ClassCropDraws:
    """What one class-balanced step draws on the host, one entry per sample: the crop is centred on voxel ``rank`` (in C
    order of the stored label map) of class ``cls`` of ``volume``.  The origin is the one value only the device knows
    (``CropSlot.resolve``)."""
    volume: np.ndarray              # int32 [B]: the bank's volume id
    rot: np.ndarray                 # int32 [B]: the rotation code, as in CropDraws
    cls: np.ndarray                 # int32 [B]: the class of the centre voxel
    rank: np.ndarray                # int32 [B]: which voxel of that class, 0 .. counts[volume][cls] - 1
    student_origin: np.ndarray      # int32 [S, B, 3]: each student's origin inside the teacher crop

    @property
    def batch(self) -> int:
        return int(np.shape(self.volume)[0])

    @property
    def n_students(self) -> int:
        return int(np.shape(self.student_origin)[0])

    def pack(self) -> np.ndarray:
        """int32 [B, 5 + 3 S]: the slot's records, the origin words 0 (the pick launch writes them)."""
        return CropDraws(self.volume, self.rot, np.zeros((self.batch, 3), np.int32), self.student_origin).pack()

    def picks(self) -> np.ndarray:
        """int32 [B, 2] = (cls, rank): the slot's pick buffer."""
        return np.stack([np.asarray(self.cls), np.asarray(self.rank)], axis=1).astype(np.int32)

    def check(self, index, roi, student_sizes=()):
        """Every draw against ``index`` (a ``ClassIndex``, or anything with its ``counts`` and ``num_classes``): the volume is
        indexed, the code is in 0..3, the class exists, the rank is below the class's count in that volume and the students'
        origins are in range.  Nothing unchecked is ever uploaded.  Raises ``ValueError`` naming the sample."""
        counts, nc = np.asarray(index.counts), int(index.num_classes)
        roi = _size3("roi", roi)
        sizes = [_size3("student size", s) for s in student_sizes]
        arrays = [np.asarray(a) for a in (self.volume, self.rot, self.cls, self.rank, self.student_origin)]
        if any(a.dtype.kind not in "iu" for a in arrays):
            raise ValueError("ClassCropDraws: integer arrays expected")
        vol, rot, cls, rank, st = [a.astype(np.int64) for a in arrays]
        B = vol.shape[0] if vol.ndim == 1 else -1
        if B < 1 or rot.shape != (B,) or cls.shape != (B,) or rank.shape != (B,) or st.shape != (len(sizes), B, 3):
            raise ValueError(f"ClassCropDraws: volume, rot, cls and rank [B] and student_origin [{len(sizes)}, B, 3] of one "
                             f"batch size expected, got {vol.shape}, {rot.shape}, {cls.shape}, {rank.shape}, {st.shape}")

        who = "ClassCropDraws"
        _refuse(who, (vol < 0) | (vol >= len(counts)),
                lambda b: f"volume id {vol[b]} is not indexed (the index holds volumes 0..{len(counts) - 1})")
        _check_rot_and_students(who, rot, st, roi, sizes)
        _refuse(who, (cls < 0) | (cls >= nc), lambda b: f"class {cls[b]} outside 0..{nc - 1}")
        total = counts[vol, cls]
        _refuse(who, (rank < 0) | (rank >= total),
                lambda b: f"rank {rank[b]} outside [0, {total[b]}), the voxels of class {cls[b]} in volume {vol[b]}")
        return self


def draw_class_crops(rs: np.random.RandomState, index, volume_ids: Sequence[int], roi, num_samples: int, ratios,
                     random_orientation: bool = False, student_sizes=()) -> ClassCropDraws:
    """The host draws of one batch of ``len(volume_ids) * num_samples`` class-balanced crops from ONE RandomState, in this
    order (``counts = index.counts``, ``v`` the sample's volume):

    1. for each volume of ``volume_ids``, in order: one ``rs.randint(3)`` if ``random_orientation``, exactly as
       ``draw_crops`` step 1;
    2. then per sample: ``p = ratios * (counts[v] > 0)`` (``ValueError`` naming the volume if that sums to 0),
       ``cls = rs.choice(num_classes, p=p / p.sum())``, then ``rank = rs.randint(0, counts[v][cls])``;
    3. then per sample, per student and per axis: ``rs.randint(0, roi - min(s, roi) + 1)``, exactly as ``draw_crops`` step 3.

    ``ratios`` holds one non-negative weight per class of the index.  ``ratios=(neg, pos)`` with ``num_classes=2`` is
    MONAI's ``RandCropByPosNegLabeld``, longer ``ratios`` are ``RandCropByLabelClassesd``: a centre uniform among the voxels
    of a class chosen by the ratios, never a class the volume lacks.  MONAI's own stream is NOT reproduced (as for
    ``draw_crops``): parity is unpinned at the MONAI boundary and this order is the project's own."""
    counts, nc = np.asarray(index.counts), int(index.num_classes)
    roi, sizes, ids, B, volume, rot, st = _draw_start("draw_class_crops", len(counts), "indexed ids", volume_ids, roi,
                                                      num_samples, student_sizes)
    w = np.asarray(ratios, dtype=np.float64)
    if w.shape != (nc,) or not np.isfinite(w).all() or (w < 0).any():
        raise ValueError(f"draw_class_crops: ratios must be {nc} finite non-negative weights, got {ratios!r}")
    d = ClassCropDraws(volume, rot, np.zeros(B, np.int32), np.zeros(B, np.int32), st)
    if random_orientation:
        _draw_orientation(rs, d.rot, len(ids), num_samples)
    for b in range(B):
        v = int(d.volume[b])
        p = w * (counts[v] > 0)
        if not p.sum() > 0:
            raise ValueError(f"draw_class_crops: volume {v} holds no voxel of a class with a positive ratio (counts "
                             f"{counts[v].tolist()}, ratios {w.tolist()})")
        d.cls[b] = rs.choice(nc, p=p / p.sum())
        d.rank[b] = rs.randint(0, counts[v][d.cls[b]])
    _draw_student_origins(rs, d.student_origin, roi, sizes)
    return d


AFFINE_WORDS = 12               # fp32 words per sample of a spatial map: A row-major, then the sub-voxel shift (mivp.h)
SPATIAL_BRICK = (8, 8, 16)      # the output brick of one workgroup of mivp_crop_fill_affine (mivp.h)
SPATIAL_BOX_CELLS = 12288       # its staged path's box budget: e0 * e1 * (e2 | 1) cells (mivp.h)


@dataclass
class SpatialDraws:
    """The affine maps one step draws on the host: per sample the matrix ``A`` that takes an offset from the centre of the
    output crop to an offset in the (rotated) source volume, and a sub-voxel shift ``s`` of the crop centre."""
    affine: np.ndarray              # float32 [B, 12]: A row-major (9 words), then the sub-voxel shift s (3 words)

    @property
    def batch(self) -> int:
        return int(np.shape(self.affine)[0])

    @classmethod
    def identity(cls, B: int) -> "SpatialDraws":
        a = np.zeros((check_int_from("B", B, 1), AFFINE_WORDS), dtype=np.float32)
        a[:, [0, 4, 8]] = 1.0
        return cls(a)

    def check(self, B: int) -> "SpatialDraws":
        """float32 ``[B, 12]``, every word finite, ``|A_ij| <= 16`` and ``|s_k| <= 1``: what the kernel's box arithmetic
        and the documented error bounds assume.  Raises ``ValueError`` naming the sample."""
        a = self.affine
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.shape != (int(B), AFFINE_WORDS):
            got = f"{a.dtype} {a.shape}" if isinstance(a, np.ndarray) else repr(type(a))
            raise ValueError(f"SpatialDraws: affine must be a float32 [{int(B)}, {AFFINE_WORDS}] array (every sample of "
                             f"the batch), got {got}")
        for b in range(a.shape[0]):
            if not np.isfinite(a[b]).all():
                raise ValueError(f"SpatialDraws: sample {b}: a non-finite word in {a[b].tolist()}")
            if (np.abs(a[b, :9]) > 16).any():
                raise ValueError(f"SpatialDraws: sample {b}: an entry of A outside [-16, 16]: {a[b, :9].tolist()}")
            if (np.abs(a[b, 9:]) > 1).any():
                raise ValueError(f"SpatialDraws: sample {b}: a shift outside [-1, 1]: {a[b, 9:].tolist()}")
        return self


def _triple(name: str, v) -> Tuple[float, float, float]:
    v = tuple(float(x) for x in (v if np.ndim(v) else (v, v, v)))
    if len(v) != 3 or not np.isfinite(v).all():
        raise ValueError(f"draw_spatial: {name} must be three finite numbers, got {v!r}")
    return v


def affine_matrix(flips, angles, zoom) -> np.ndarray:
    """float64 ``A = F . R2 . R1 . R0 . diag(1 / zoom)``: output offset -> source offset.  ``F = diag(-1 where flipped)``;
    ``R_k`` turns by ``angles[k]`` radians about axis k of the ``[H, W, D]`` frame (R0 = [[1, 0, 0], [0, c, -s], [0, s, c]],
    R1 = [[c, 0, s], [0, 1, 0], [-s, 0, c]], R2 = [[c, -s, 0], [s, c, 0], [0, 0, 1]]); zoom > 1 enlarges the content."""
    c, s = np.cos(np.asarray(angles, np.float64)), np.sin(np.asarray(angles, np.float64))
    R0 = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]], np.float64)
    R1 = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]], np.float64)
    R2 = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]], np.float64)
    F = np.diag([-1.0 if f else 1.0 for f in flips])
    return F @ R2 @ R1 @ R0 @ np.diag(1.0 / np.asarray(zoom, np.float64))


def draw_spatial(rs: np.random.RandomState, B: int, p_flip=(0., 0., 0.), p_affine: float = 0., rotate_range=(0., 0., 0.),
                 scale_range=(1., 1.), isotropic: bool = True, shift: bool = False) -> SpatialDraws:
    """The spatial draws of one batch of ``B`` samples from ONE RandomState.  Per sample, in this order:

    1. three flip draws: axis k of the rotated ``[H, W, D]`` frame is mirrored if ``rs.random_sample() < p_flip[k]``;
    2. one apply draw: ``rs.random_sample() < p_affine``;
    3. if it applies: three angles ``rs.uniform(-rotate_range[k], rotate_range[k])`` in radians about axes 0, 1, 2, then
       ONE zoom ``rs.uniform(*scale_range)`` if ``isotropic``, else three;
    4. if ``shift``: three ``rs.uniform(-0.5, 0.5)``, the sub-voxel shift of the crop centre.

    A branch that does not apply consumes NO draws: a sample whose apply draw fails costs four draws (seven with
    ``shift``), and ``p_flip = 0`` / ``p_affine = 0`` still make their four comparisons' draws.  The matrix is
    ``affine_matrix`` composed in float64 and rounded to fp32 once.  MONAI's ``RandFlipd`` / ``RandAffined`` streams are
    NOT reproduced (``Compose`` reseeds every child, and MONAI resamples through a stored grid): parity is unpinned at the
    MONAI boundary, as for ``draw_crops``, and this order is the project's own."""
    B = check_int_from("B", B, 1)
    p_flip, rot = _triple("p_flip", p_flip), _triple("rotate_range", rotate_range)
    lo, hi = (float(v) for v in scale_range)
    if not (0 <= min(p_flip) and max(p_flip) <= 1 and 0 <= float(p_affine) <= 1):
        raise ValueError(f"draw_spatial: probabilities must be in [0, 1], got p_flip {p_flip}, p_affine {p_affine}")
    if not (np.isfinite([lo, hi]).all() and 0 < lo <= hi):
        raise ValueError(f"draw_spatial: scale_range must be 0 < low <= high, got {scale_range!r}")
    out = np.zeros((B, AFFINE_WORDS), dtype=np.float32)
    for b in range(B):
        flips = [rs.random_sample() < p_flip[k] for k in range(3)]
        angles, zoom = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        if rs.random_sample() < float(p_affine):
            angles = [rs.uniform(-rot[k], rot[k]) for k in range(3)]
            zoom = [rs.uniform(lo, hi)] * 3 if isotropic else [rs.uniform(lo, hi) for _ in range(3)]
        out[b, :9] = affine_matrix(flips, angles, zoom).reshape(-1)
        if shift:
            out[b, 9:] = [rs.uniform(-0.5, 0.5) for _ in range(3)]
    return SpatialDraws(out).check(B)


class SpatialSlot:
    """Fixed device memory of one batch's spatial maps -- ONE fp32 [B * 12] allocation made here, the identity at first --
    whose pointer a recorded graph keeps.  ``load`` checks the draws, then refreshes the words from a new pinned staging
    buffer without blocking; it does nothing while a graph is being recorded, exactly as ``CropSlot.load``."""

    def __init__(self, B: int, device):
        self.B = check_int_from("B", B, 1)
        self.words = torch.from_numpy(SpatialDraws.identity(self.B).affine.reshape(-1)).to(_gpu_device("SpatialSlot", device))
        self.draws = SpatialDraws.identity(self.B)

    def load(self, draws: SpatialDraws):
        if not isinstance(draws, SpatialDraws):
            raise ValueError("SpatialSlot.load: SpatialDraws expected")
        draws.check(self.B)
        if torch.cuda.is_current_stream_capturing():
            return
        self.words.copy_(torch.from_numpy(np.ascontiguousarray(draws.affine).reshape(-1)).pin_memory(), non_blocking=True)
        self.draws = draws


ELASTIC_NODES = (4, 8)          # the node count of a control lattice, per axis: at least one knot interval, at most 6 KiB (mivp.h)


def _nodes3(who: str, nodes) -> Tuple[int, int, int]:
    v = tuple(nodes) if not plain_int(nodes) else (nodes, nodes, nodes)
    lo, hi = ELASTIC_NODES
    if len(v) != 3 or any(not plain_int(a) or not lo <= int(a) <= hi for a in v):
        raise ValueError(f"{who}: nodes must be three integers in {lo}..{hi}, got {nodes!r}")
    return tuple(int(a) for a in v)


@dataclass
class ElasticDraws:
    """The elastic deformation one step draws on the host: per sample a flag and a control lattice ``P[c, j0, j1, j2]``, the
    displacement (component ``c``, in output voxels) of node ``j``; the cubic B-spline of the lattice is the displacement
    field (the rule is written out in include/mivp.h).  A sample whose flag is 0 is not deformed and its lattice is not read."""
    flags: np.ndarray               # int32 [B]: 1 = the sample is deformed
    lattice: np.ndarray             # float32 [B, 3, n0, n1, n2]

    @property
    def batch(self) -> int:
        return int(np.shape(self.flags)[0])

    @classmethod
    def identity(cls, B: int, nodes) -> "ElasticDraws":
        B, nodes = check_int_from("B", B, 1), _nodes3("ElasticDraws.identity", nodes)
        return cls(np.zeros(B, np.int32), np.zeros((B, 3) + nodes, np.float32))

    def check(self, B: int, nodes) -> "ElasticDraws":
        """int32 ``[B]`` flags, each 0 or 1, and a float32 ``[B, 3, n0, n1, n2]`` lattice of finite values.  Raises
        ``ValueError`` naming the sample."""
        nodes = _nodes3("ElasticDraws", nodes)
        f, p = self.flags, self.lattice
        if not isinstance(f, np.ndarray) or f.dtype != np.int32 or f.shape != (int(B),):
            got = f"{f.dtype} {f.shape}" if isinstance(f, np.ndarray) else repr(type(f))
            raise ValueError(f"ElasticDraws: flags must be an int32 [{int(B)}] array (every sample of the batch), got {got}")
        want = (int(B), 3) + nodes
        if not isinstance(p, np.ndarray) or p.dtype != np.float32 or p.shape != want:
            got = f"{p.dtype} {p.shape}" if isinstance(p, np.ndarray) else repr(type(p))
            raise ValueError(f"ElasticDraws: lattice must be a float32 {list(want)} array, got {got}")
        _refuse("ElasticDraws", (f != 0) & (f != 1), lambda b: f"flag {int(f[b])} is neither 0 nor 1")
        _refuse("ElasticDraws", ~np.isfinite(p).reshape(int(B), -1).all(axis=1), lambda b: "a non-finite displacement")
        return self


def draw_elastic(rs: np.random.RandomState, B: int, roi, nodes=(7, 7, 7), p_elastic: float = 0., magnitude_range=(0., 0.),
                 locked_borders: int = 2) -> ElasticDraws:
    """The elastic draws of one batch of ``B`` samples from ONE RandomState.  Per sample, in this order:

    1. one coin: the sample is deformed if ``rs.random_sample() < p_elastic``;
    2. if it is: one magnitude ``m = rs.uniform(lo, hi)`` in output voxels (``magnitude_range = (lo, hi)``);
    3. then every node component ``rs.uniform(-m, m)``, in C order of ``[3, n0, n1, n2]`` (the component slowest);
    4. then the outer ``locked_borders`` node layers on every axis are set to zero (no draw), so the rim of the crop does
       not move (TorchIO's ``locked_borders``).

    A sample that is not deformed consumes its coin only and keeps a zero lattice.  The draws are float64 and the lattice
    is rounded to fp32 once.  Refused: a probability outside [0, 1]; a range that is not ``0 <= lo <= hi``; ``hi >= 0.5 *
    roi_k / (n_k - 3)`` on any axis -- beyond half a node spacing the map can fold; ``locked_borders`` that leave no free
    node (``2 * locked_borders >= n_k``).  TorchIO's and MONAI's own streams are NOT reproduced (neither is installed; MONAI
    smooths full-resolution noise instead): parity is unpinned at that boundary and this order is the project's own
    (DESIGN.md 8)."""
    B, roi, nodes = check_int_from("B", B, 1), _size3("roi", roi), _nodes3("draw_elastic", nodes)
    if not isinstance(p_elastic, (int, float, np.floating)) or not 0 <= float(p_elastic) <= 1:
        raise ValueError(f"draw_elastic: p_elastic must be in [0, 1], got {p_elastic!r}")
    lo, hi = (float(v) for v in magnitude_range)
    if not (np.isfinite([lo, hi]).all() and 0 <= lo <= hi):
        raise ValueError(f"draw_elastic: magnitude_range must be 0 <= low <= high, got {magnitude_range!r}")
    for k in range(3):
        if hi >= 0.5 * roi[k] / (nodes[k] - 3):
            raise ValueError(f"draw_elastic: magnitude {hi} on axis {k} is not below half the node spacing "
                             f"{0.5 * roi[k] / (nodes[k] - 3):.4g} voxels (roi {roi}, nodes {nodes}): the map could fold")
    if not plain_int(locked_borders) or int(locked_borders) < 0 or any(2 * int(locked_borders) >= n for n in nodes):
        raise ValueError(f"draw_elastic: locked_borders {locked_borders!r} must be an integer >= 0 that leaves a free node "
                         f"on every axis of {nodes}")
    lb = int(locked_borders)
    d = ElasticDraws.identity(B, nodes)
    for b in range(B):
        if rs.random_sample() < float(p_elastic):
            m = rs.uniform(lo, hi)
            P = rs.uniform(-m, m, size=(3,) + nodes)
            if lb:
                free = np.zeros(nodes, bool)
                free[lb:nodes[0] - lb, lb:nodes[1] - lb, lb:nodes[2] - lb] = True
                P = np.where(free[None], P, 0.0)
            d.flags[b], d.lattice[b] = 1, P
    return d.check(B, nodes)


class ElasticSlot:
    """Fixed device memory of one batch's elastic draws -- ONE allocation made here, int32 flags [B] in front of the fp32
    lattice [B * 3 * n0 * n1 * n2], the identity (no sample deformed) at first -- whose pointers a recorded graph keeps.
    ``load`` checks the draws, then refreshes both from a new pinned staging buffer in one copy without blocking; it does
    nothing while a graph is being recorded, exactly as ``SpatialSlot.load``."""

    def __init__(self, B: int, nodes, device):
        self.B, self.nodes = check_int_from("B", B, 1), _nodes3("ElasticSlot", nodes)
        words = self.B * 3 * int(np.prod(self.nodes))
        self.buffer = torch.zeros(self.B + words, dtype=torch.float32, device=_gpu_device("ElasticSlot", device))
        self.flags, self.lattice = self.buffer[:self.B].view(torch.int32), self.buffer[self.B:]
        self.draws = ElasticDraws.identity(self.B, self.nodes)

    def load(self, draws: ElasticDraws):
        if not isinstance(draws, ElasticDraws):
            raise ValueError("ElasticSlot.load: ElasticDraws expected")
        draws.check(self.B, self.nodes)
        if torch.cuda.is_current_stream_capturing():
            return
        words = np.concatenate([np.ascontiguousarray(draws.flags).view(np.float32), draws.lattice.reshape(-1)])   # ONE upload
        self.buffer.copy_(torch.from_numpy(words).pin_memory(), non_blocking=True)
        self.draws = draws


MAX_HOLES = 8                   # holes per (student, sample) of a corruption record (mivp.h)
MAX_SHUFFLE_VOXELS = 4096       # of one shuffle hole: what the kernel stages in LDS (mivp.h)
HOLE_WORDS = 7                  # int32 words of one hole: origin[3], size[3], key
CORRUPT_WORDS = 3 + MAX_HOLES * HOLE_WORDS      # of one record: mode, hole count, noise key, then the holes (mivp.h)
CORRUPT_PARTIALS = 64           # (min, max) pairs per sample of the range scratch (mivp.h)
CORRUPT_MODES = ("none", "dropout", "keep", "shuffle")


@dataclass
class CorruptionDraws:
    """The students' own corruption one step draws on the host, one entry per (student, sample): a mode
    -- 0 none, 1 dropout (noise inside the holes), 2 keep (noise outside their union), 3 shuffle (voxels permuted inside
    each hole, in list order) --, up to ``MAX_HOLES`` boxes inside the student's extents, and the 32-bit keys of the
    counter-based noise and of each hole's permutation (the rule is written out in include/mivp.h).  Holes ``n_holes..``
    are not read."""
    mode: np.ndarray                # int32 [S, B]
    n_holes: np.ndarray             # int32 [S, B]: 0 .. MAX_HOLES
    key: np.ndarray                 # uint32 [S, B]: the noise key (modes 1 and 2)
    origin: np.ndarray              # int32 [S, B, MAX_HOLES, 3]
    size: np.ndarray                # int32 [S, B, MAX_HOLES, 3]
    hole_key: np.ndarray            # uint32 [S, B, MAX_HOLES]: each hole's permutation key (mode 3)

    @property
    def n_students(self) -> int:
        return int(np.shape(self.mode)[0])

    @property
    def batch(self) -> int:
        return int(np.shape(self.mode)[1])

    @classmethod
    def identity(cls, B: int, n_students: int) -> "CorruptionDraws":
        S, B = check_int_from("n_students", n_students, 1), check_int_from("B", B, 1)
        return cls(np.zeros((S, B), np.int32), np.zeros((S, B), np.int32), np.zeros((S, B), np.uint32),
                   np.zeros((S, B, MAX_HOLES, 3), np.int32), np.zeros((S, B, MAX_HOLES, 3), np.int32),
                   np.zeros((S, B, MAX_HOLES), np.uint32))

    def pack(self) -> np.ndarray:
        """int32 [S, B, CORRUPT_WORDS]: the slot's records."""
        S, B = self.n_students, self.batch
        w = np.zeros((S, B, CORRUPT_WORDS), dtype=np.int32)
        w[..., 0], w[..., 1], w[..., 2] = self.mode, self.n_holes, np.asarray(self.key, np.uint32).view(np.int32)
        holes = w[..., 3:].reshape(S, B, MAX_HOLES, HOLE_WORDS)
        holes[..., 0:3], holes[..., 3:6] = self.origin, self.size
        holes[..., 6] = np.asarray(self.hole_key, np.uint32).view(np.int32)
        return w

    @classmethod
    def unpack(cls, words: np.ndarray, n_students: int) -> "CorruptionDraws":
        w = np.ascontiguousarray(words, dtype=np.int32).reshape(int(n_students), -1, CORRUPT_WORDS)
        holes = w[..., 3:].reshape(w.shape[0], w.shape[1], MAX_HOLES, HOLE_WORDS)
        return cls(w[..., 0].copy(), w[..., 1].copy(), w[..., 2].copy().view(np.uint32), holes[..., 0:3].copy(),
                   holes[..., 3:6].copy(), holes[..., 6].copy().view(np.uint32))

    def check(self, B: int, student_sizes) -> "CorruptionDraws":
        """Every field against the batch and the students' extents: shapes and dtypes, a mode in 0..3, at most
        ``MAX_HOLES`` holes, every hole read non-empty and inside its student, a shuffle hole of at most
        ``MAX_SHUFFLE_VOXELS`` voxels.  A hole outside the tensor would send the kernel to memory that is not the student's,
        so nothing unchecked is ever uploaded.  Raises ``ValueError`` naming the field, the student and the sample."""
        sizes = [_size3("student size", s) for s in student_sizes]
        S, B = len(sizes), int(B)
        want = (("mode", np.int32, (S, B)), ("n_holes", np.int32, (S, B)), ("key", np.uint32, (S, B)),
                ("origin", np.int32, (S, B, MAX_HOLES, 3)), ("size", np.int32, (S, B, MAX_HOLES, 3)),
                ("hole_key", np.uint32, (S, B, MAX_HOLES)))
        for name, dtype, shape in want:
            a = getattr(self, name)
            if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != shape:
                got = f"{a.dtype} {a.shape}" if isinstance(a, np.ndarray) else repr(type(a))
                raise ValueError(f"CorruptionDraws: {name} must be a {np.dtype(dtype).name} {list(shape)} array (every "
                                 f"student and sample of the batch), got {got}")
        for s, ext in enumerate(sizes):
            who = f"CorruptionDraws: student {s}"
            mode, n = self.mode[s], self.n_holes[s]
            _refuse(who, (mode < 0) | (mode > 3), lambda b: f"mode {int(mode[b])} outside 0..3")
            _refuse(who, (n < 0) | (n > MAX_HOLES), lambda b: f"n_holes {int(n[b])} outside 0..{MAX_HOLES}")
            for b in range(B):
                for k in range(int(n[b])):
                    o, e = self.origin[s, b, k].astype(np.int64), self.size[s, b, k].astype(np.int64)
                    if (e < 1).any() or (o < 0).any() or (o + e > np.asarray(ext)).any():
                        raise ValueError(f"{who}: sample {b}: hole {k} with origin {o.tolist()} and size {e.tolist()} is "
                                         f"empty or outside the student's extents {ext}")
                    if int(mode[b]) == 3 and int(e.prod()) > MAX_SHUFFLE_VOXELS:
                        raise ValueError(f"{who}: sample {b}: shuffle hole {k} of size {e.tolist()} holds {int(e.prod())} "
                                         f"voxels, more than {MAX_SHUFFLE_VOXELS}")
        return self


def _hole_params(name: str, p) -> Tuple[int, int, Tuple[int, int, int], Tuple[int, int, int]]:
    """(holes, max_holes, spatial_size, max_spatial_size) of one ``draw_student_corruption`` dict; ``max_holes`` and
    ``max_spatial_size`` default to ``holes`` and ``spatial_size`` (MONAI's None)."""
    p = dict(p)
    unknown = set(p) - {"holes", "max_holes", "spatial_size", "max_spatial_size"}
    if unknown or "holes" not in p or "spatial_size" not in p:
        raise ValueError(f"draw_student_corruption: {name} takes holes, spatial_size and optionally max_holes, "
                         f"max_spatial_size, got {sorted(p)}")
    lo = check_int_from(f"{name}['holes']", p["holes"], 0)
    hi = lo if p.get("max_holes") is None else check_int_from(f"{name}['max_holes']", p["max_holes"], 0)
    small = _size3(f"{name}['spatial_size']", p["spatial_size"])
    large = small if p.get("max_spatial_size") is None else _size3(f"{name}['max_spatial_size']", p["max_spatial_size"])
    if not lo <= hi <= MAX_HOLES or any(a > b for a, b in zip(small, large)):
        raise ValueError(f"draw_student_corruption: {name} needs holes <= max_holes <= {MAX_HOLES} and spatial_size <= "
                         f"max_spatial_size, got {p}")
    return lo, hi, small, large


def draw_student_corruption(rs: np.random.RandomState, B: int, student_sizes, weights=(0.7, 0.1, 0.1, 0.1),
                            dropout=dict(holes=1, max_holes=3, spatial_size=4, max_spatial_size=16),
                            keep=dict(holes=5, max_holes=5, spatial_size=32, max_spatial_size=48),
                            shuffle=dict(holes=1, max_holes=3, spatial_size=4, max_spatial_size=16)) -> CorruptionDraws:
    """The corruption draws of one batch of ``B`` samples for the students of ``student_sizes`` from ONE RandomState: the
    reference's ``students_rand_ts`` (transforms.py:244-297), whose defaults these are.  Per sample, and within it per
    student, in this order:

    1. the mode: ``rs.choice(4, p=weights / sum(weights))`` -- none, dropout, keep, shuffle;
    2. mode 0 consumes nothing more.  Otherwise, with the dict of that mode: the number of holes
       ``rs.randint(holes, max_holes + 1)``;
    3. then per hole: three extents ``min(rs.randint(spatial_size[k], max_spatial_size[k] + 1), student extent k)``, then
       three origins ``rs.randint(0, student extent k - extent k + 1)``, then, in mode 3 only, the hole's key
       ``rs.randint(0, 2**32, dtype=np.uint32)``;
    4. then, in modes 1 and 2 only, the noise key ``rs.randint(0, 2**32, dtype=np.uint32)``.

    The hole rule restates MONAI's documented ``RandCoarseTransform`` (a uniform count, uniform extents clipped to the
    image, a uniform origin); MONAI's own streams are NOT reproduced (``Compose`` / ``OneOf`` reseed every child, and its
    noise is ``R.uniform`` per voxel): parity is unpinned at the MONAI boundary and this order is the project's own
    (DESIGN.md 8).  A shuffle hole above ``MAX_SHUFFLE_VOXELS`` voxels is refused by the final ``check``."""
    B = check_int_from("B", B, 1)
    sizes = [_size3("student size", s) for s in student_sizes]
    if not sizes:
        raise ValueError("draw_student_corruption: at least one student size expected")
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (4,) or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError(f"draw_student_corruption: weights must be 4 finite non-negative numbers with a positive sum "
                         f"(none, dropout, keep, shuffle), got {weights!r}")
    params = {1: _hole_params("dropout", dropout), 2: _hole_params("keep", keep), 3: _hole_params("shuffle", shuffle)}
    d = CorruptionDraws.identity(B, len(sizes))
    for b in range(B):
        for s, ext in enumerate(sizes):
            mode = int(rs.choice(4, p=w / w.sum()))
            d.mode[s, b] = mode
            if mode == 0:
                continue
            lo, hi, small, large = params[mode]
            n = int(rs.randint(lo, hi + 1))
            d.n_holes[s, b] = n
            for k in range(n):
                e = [min(int(rs.randint(small[a], large[a] + 1)), ext[a]) for a in range(3)]
                d.size[s, b, k] = e
                d.origin[s, b, k] = [rs.randint(0, ext[a] - e[a] + 1) for a in range(3)]
                if mode == 3:
                    d.hole_key[s, b, k] = rs.randint(0, 2 ** 32, dtype=np.uint32)
            if mode != 3:
                d.key[s, b] = rs.randint(0, 2 ** 32, dtype=np.uint32)
    return d.check(B, sizes)


class CorruptionSlot:
    """Fixed device memory of one batch's corruption draws -- ONE int32 [S * B * CORRUPT_WORDS] allocation made here, every
    record mode 0 at first -- whose pointer a recorded graph keeps; ``records[s]`` is student s's [B * CORRUPT_WORDS] view.
    ``load`` checks the draws against the slot's student sizes, then refreshes the records from a new pinned staging buffer
    without blocking; it does nothing while a graph is being recorded, exactly as ``ElasticSlot.load``."""

    def __init__(self, B: int, student_sizes, device):
        self.B = check_int_from("B", B, 1)
        self.student_sizes = [_size3("student size", s) for s in student_sizes]
        if not self.student_sizes:
            raise ValueError("CorruptionSlot: at least one student size expected")
        S = len(self.student_sizes)
        self.buffer = torch.zeros(S * self.B * CORRUPT_WORDS, dtype=torch.int32, device=_gpu_device("CorruptionSlot", device))
        self.records = list(self.buffer.view(S, self.B * CORRUPT_WORDS))
        self.draws = CorruptionDraws.identity(self.B, S)

    def load(self, draws: CorruptionDraws):
        if not isinstance(draws, CorruptionDraws):
            raise ValueError("CorruptionSlot.load: CorruptionDraws expected")
        draws.check(self.B, self.student_sizes)
        if torch.cuda.is_current_stream_capturing():
            return
        self.buffer.copy_(torch.from_numpy(draws.pack().reshape(-1)).pin_memory(), non_blocking=True)
        self.draws = draws


class CropSlot:
    """Fixed device memory of one batch's draws -- int32 [B][5 + 3 S] records -- whose pointer a recorded graph keeps.
    ``load`` checks the draws against the bank, then refreshes the records from a new pinned staging buffer without blocking;
    it does nothing while a graph is being recorded, exactly as ``augment.IntensitySlot.load``.

    With ``class_index`` the slot is in class mode for life: it also owns the int32 [B][2] pick buffer (class, rank) behind
    the records, ``load`` takes ``ClassCropDraws`` only and uploads records whose origin words are 0, and ``resolve`` issues
    the launch that writes them."""

    def __init__(self, B: int, n_students: int, device, class_index: Optional[ClassIndex] = None):
        self.B = check_int_from("B", B, 1)
        self.n_students = check_int_from("n_students", n_students, 0)
        self.words = record_words(self.n_students)
        self.class_index = class_index
        if class_index is None:
            self.buffer = self.records = torch.zeros(self.B * self.words, dtype=torch.int32, device=device)
            self.picks = None
        else:
            if not isinstance(class_index, ClassIndex) or torch.device(device).type != "cuda":
                raise ValueError("CropSlot: class_index must be a ClassIndex and the device its bank's GPU (no CPU fallback)")
            device = _gpu_device("CropSlot", device)
            if device != class_index.bank.device or self.B > 65535:
                raise ValueError(f"CropSlot: a class-mode slot of batch <= 65535 on {class_index.bank.device} expected, got "
                                 f"batch {self.B} on {device}")
            self.buffer = torch.zeros(self.B * (self.words + 2), dtype=torch.int32, device=device)     # ONE upload per load
            self.records, self.picks = self.buffer[:self.B * self.words], self.buffer[self.B * self.words:]
        self.student_views = [self.records[HEAD + 3 * s:] for s in range(self.n_students)]   # advanced to the origin words
        self.draws = None
        self.checked = None             # (bank shapes or the class index, roi, student sizes) the draws were checked against

    def resolve(self, roi):
        """Class mode: the pick launch alone, on the current stream -- it writes the crop origin of every sample into the
        records (words 2..4) from the index.  No host read; records into a graph."""
        index = self.class_index
        if index is None:
            raise ValueError("CropSlot.resolve: the slot has no class index (its draws carry their origins)")
        if self.draws is None:
            raise ValueError("CropSlot.resolve: the slot holds no draws (CropSlot.load)")
        roi = _size3("roi", roi)
        if roi != self.checked[1]:
            raise ValueError(f"CropSlot.resolve: roi {roi}, but the slot's draws were checked against roi {self.checked[1]}")
        L.call("mivp_crop_pick", L.ptr(index.bank.table), L.ptr(index.table), index.bank.capacity, L.ptr(index.lut),
               index.num_classes, L.ptr(self.records), self.words, L.ptr(self.picks), self.B, i3(roi), L.stream())

    def resolved_origins(self) -> np.ndarray:
        """int32 [B, 3]: the origin words as they stand on the device.  A BLOCKING read, for tests and debugging only."""
        return self.records.view(self.B, self.words)[:, 2:HEAD].cpu().numpy()

    def load(self, draws: CropDraws, bank, roi, student_sizes=()):
        index = self.class_index
        if index is None:
            if not isinstance(draws, CropDraws):
                raise ValueError("CropSlot.load: CropDraws expected")
        elif not isinstance(draws, ClassCropDraws):
            raise ValueError("CropSlot.load: a class-mode slot takes ClassCropDraws only")
        elif bank is not index and bank is not index.bank:
            raise ValueError("CropSlot.load: a class-mode slot loads against its own index (or that index's bank)")
        if len(tuple(student_sizes)) != self.n_students:
            raise ValueError(f"CropSlot: {len(tuple(student_sizes))} student sizes for a slot of {self.n_students} students")
        if draws.check(bank if index is None else index, roi, student_sizes).batch != self.B:
            raise ValueError(f"CropSlot: draws of batch {draws.batch} do not match the slot's batch {self.B}")
        if torch.cuda.is_current_stream_capturing():
            return
        words = [draws.pack().reshape(-1)] + ([] if index is None else [draws.picks().reshape(-1)])      # ONE upload
        self.buffer.copy_(torch.from_numpy(np.concatenate(words)).pin_memory(), non_blocking=True)
        self.draws = draws
        held = index if index is not None else tuple(tuple(s) for s in (bank.shapes if hasattr(bank, "shapes") else bank))
        self.checked = (held, _size3("roi", roi), [_size3("student size", s) for s in student_sizes])


class BatchFiller:
    """The output tensors of one training batch, allocated once, and the launches that fill them from ``bank``.

    ``batch`` is what the step functions take.  Without students it is the tuple ``xy = (image, mask)`` of ``train_step`` /
    ``graphed_train_step`` (``mask`` is None with ``with_mask=False``; ``coord`` is kept beside it when asked for).  With
    ``student_sizes`` it is the dict of ``students_teacher.synthetic_views``: ``image``, ``coord``, ``image_st`` and
    ``coord_st`` (one tensor per student) and ``mask_st_0``, student 0's view of the label map; the students are views of
    the teacher crop BEFORE any intensity augmentation, as in the reference, which copies the teacher crop and crops the
    copies (transforms.py:214-219,299-313).

    ``fill(draws_or_slot)`` issues one bank-mode launch for the teacher and one tensor-mode launch per student and kind on
    the current stream; no host read, no allocation.  The outputs are fixed tensors: a graph recorded on them (``fill``
    itself, or a ``GraphedStep`` whose inputs they are) sees every later ``fill``.

    With ``class_index`` the filler's own slot is in class mode and ``fill`` takes ``ClassCropDraws`` (or a class-mode slot
    of the same index): it issues the pick launch first (``CropSlot.resolve``), then the teacher, then the students, so a
    recorded ``fill`` contains the pick and is fed by ``slot.load`` before each replay, as without an index.

    With ``spatial=True`` the filler owns ``spatial_slot`` (the identity at first) and the teacher launch is the
    interpolating ``mivp_crop_fill_affine``: flips, rotation and zoom about the centre of the crop, which
    therefore stays centred on a picked voxel.  The pick runs first as before and the students are crops of the augmented
    teacher tensors, so image, coordinates and mask agree across the views.  ``spatial=False`` issues exactly the
    launches described above.

    With ``spatial=True, elastic=nodes`` (three node counts in 4..8) the filler also owns ``elastic_slot`` (no sample
    deformed at first) and the teacher launch is ``mivp_crop_fill_elastic``: the B-spline displacement of
    each flagged sample's control lattice is added in front of the affine map; a sample whose flag is 0 gets the bits of
    the ``spatial=True`` filler.  Pick and students as before.  Without ``elastic`` nothing changes.

    With ``corruption=True`` (students only) the filler owns ``corruption_slot`` (every record mode 0 at first) and, after
    the student crops, issues two launches per student on ``image_st[i]`` alone: the range of each sample
    that needs one, then the corruption in place.  ``coord_st``, ``mask_st_0`` and the teacher's tensors are never touched;
    a sample in mode 0 is not written, so an all-zero slot gives the bits of the filler built without the option.  The
    reference would have corrupted the roi-sized copy BEFORE the student crop; acting on the cropped student is a stated
    deviation (the noise range and the shuffle are defined on the tensor the student sees)."""

    def __init__(self, bank: VolumeBank, roi, batch: int, student_sizes=(), active_labels=None, with_coord: bool = False,
                 with_mask: bool = True, class_index: Optional[ClassIndex] = None, spatial: bool = False, elastic=None,
                 corruption: bool = False):
        if not isinstance(bank, VolumeBank):
            raise ValueError("BatchFiller: a VolumeBank expected")
        if class_index is not None and (not isinstance(class_index, ClassIndex) or class_index.bank is not bank):
            raise ValueError("BatchFiller: class_index must be a ClassIndex of this bank")
        if elastic is not None and not spatial:
            raise ValueError("BatchFiller: elastic= needs spatial=True (the displacement is added in front of the affine map)")
        if corruption and not len(tuple(student_sizes)):
            raise ValueError("BatchFiller: corruption=True needs student_sizes (it acts on the students' image tensors)")
        nodes = None if elastic is None else _nodes3("BatchFiller", elastic)
        self.class_index = class_index
        self.bank, self.roi, self.B = bank, _size3("roi", roi), check_int_from("batch", batch, 1)
        self.student_sizes = [_size3("student size", s) for s in student_sizes]
        if self.B > 65535 or any(v > 65535 for v in self.roi + tuple(a for s in self.student_sizes for a in s)):
            raise ValueError("BatchFiller: batch and every extent must be below 65536")
        S, dev, Cn = len(self.student_sizes), bank.device, bank.channels
        with_coord = bool(with_coord) or S > 0
        new = lambda c, size: torch.zeros((self.B, c) + tuple(size), dtype=torch.float32, device=dev)
        self.image = new(Cn, self.roi)
        self.mask = new(1, self.roi) if with_mask else None
        self.coord = new(3, self.roi) if with_coord else None
        self.lut = torch.from_numpy(label_table(active_labels)).to(dev) if with_mask else None
        self.image_st = [new(Cn, s) for s in self.student_sizes]
        self.coord_st = [new(3, s) for s in self.student_sizes]
        self.mask_st_0 = new(1, self.student_sizes[0]) if (S and with_mask) else None
        self.slot = CropSlot(self.B, S, dev, class_index=class_index)
        self.spatial_slot = SpatialSlot(self.B, dev) if spatial else None
        self.elastic_slot = ElasticSlot(self.B, nodes, dev) if nodes is not None else None
        self.corruption_slot = CorruptionSlot(self.B, self.student_sizes, dev) if corruption else None
        # the range launch's scratch: fp32 [S][B][CORRUPT_PARTIALS][2] (mivp.h)
        self.corruption_range = torch.zeros((S, self.B * CORRUPT_PARTIALS * 2), dtype=torch.float32, device=dev) \
            if corruption else None
        self.xy = (self.image, self.mask)
        if S:
            self.batch = dict(image=self.image, coord=self.coord, image_st=self.image_st, coord_st=self.coord_st)
            if self.mask_st_0 is not None:
                self.batch["mask_st_0"] = self.mask_st_0
        else:
            self.batch = self.xy

    def _outputs(self):
        """(name, tensor, shape) of every output: what ``fill`` checks before it launches."""
        out = [("image", self.image, (self.B, self.bank.channels) + self.roi)]
        if self.mask is not None:
            out.append(("mask", self.mask, (self.B, 1) + self.roi))
        if self.coord is not None:
            out.append(("coord", self.coord, (self.B, 3) + self.roi))
        for i, s in enumerate(self.student_sizes):
            out.append((f"image_st[{i}]", self.image_st[i], (self.B, self.bank.channels) + s))
            out.append((f"coord_st[{i}]", self.coord_st[i], (self.B, 3) + s))
        if self.mask_st_0 is not None:
            out.append(("mask_st_0", self.mask_st_0, (self.B, 1) + self.student_sizes[0]))
        return out

    def _check_outputs(self):
        for name, t, shape in self._outputs():
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32 \
                    or t.device != self.bank.device or not t.is_contiguous():
                got = f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else repr(t)
                raise ValueError(f"BatchFiller.fill: {name} must be a contiguous fp32 {shape} tensor on {self.bank.device}, "
                                 f"got {got}")

    @torch.no_grad()
    def fill(self, draws_or_slot=None, spatial=None, elastic=None, corruption=None):
        """``CropDraws`` (``ClassCropDraws`` on a filler with a class index): checked and loaded into the filler's own slot
        first.  A ``CropSlot``: used as it stands (its ``load`` did the checking).  ``None``: the filler's own slot as last
        loaded.  ``spatial`` (a filler built with ``spatial=True`` only): ``SpatialDraws``, checked and loaded into
        ``spatial_slot`` first; a ``SpatialSlot``, used as it stands; ``None``: ``spatial_slot`` as last loaded.
        ``elastic`` (a filler built with ``elastic=nodes`` only) follows the same rules with ``ElasticDraws``, an
        ``ElasticSlot`` and ``elastic_slot``, and ``corruption`` (a filler built with ``corruption=True`` only) with
        ``CorruptionDraws``, a ``CorruptionSlot`` and ``corruption_slot``.  Every refusal comes before the first launch and
        before any slot is loaded."""
        slot = self.slot
        sp_slot = self.spatial_slot
        el_slot = self.elastic_slot
        co_slot = self.corruption_slot
        if corruption is not None:
            if co_slot is None:
                raise ValueError("BatchFiller.fill: corruption= needs a filler built with corruption=True")
            if isinstance(corruption, CorruptionDraws):
                corruption.check(self.B, self.student_sizes)
            elif isinstance(corruption, CorruptionSlot):
                if corruption.B != self.B or corruption.student_sizes != self.student_sizes \
                        or corruption.buffer.device != self.bank.device:
                    raise ValueError(f"BatchFiller.fill: a corruption slot of batch {corruption.B} and student sizes "
                                     f"{corruption.student_sizes} on {corruption.buffer.device} for a filler of batch "
                                     f"{self.B} and student sizes {self.student_sizes} on {self.bank.device}")
                co_slot = corruption
            else:
                raise ValueError("BatchFiller.fill: corruption= takes CorruptionDraws, a CorruptionSlot, or nothing")
        if elastic is not None:
            if el_slot is None:
                raise ValueError("BatchFiller.fill: elastic= needs a filler built with elastic=nodes")
            if isinstance(elastic, ElasticDraws):
                elastic.check(self.B, el_slot.nodes)
            elif isinstance(elastic, ElasticSlot):
                if elastic.B != self.B or elastic.nodes != el_slot.nodes or elastic.buffer.device != self.bank.device:
                    raise ValueError(f"BatchFiller.fill: an elastic slot of batch {elastic.B} and nodes {elastic.nodes} on "
                                     f"{elastic.buffer.device} for a filler of batch {self.B} and nodes {el_slot.nodes} on "
                                     f"{self.bank.device}")
                el_slot = elastic
            else:
                raise ValueError("BatchFiller.fill: elastic= takes ElasticDraws, an ElasticSlot, or nothing")
        if spatial is not None:
            if sp_slot is None:
                raise ValueError("BatchFiller.fill: spatial= needs a filler built with spatial=True")
            if isinstance(spatial, SpatialDraws):
                spatial.check(self.B)
            elif isinstance(spatial, SpatialSlot):
                sp_slot = spatial
                if sp_slot.B != self.B or sp_slot.words.device != self.bank.device:
                    raise ValueError(f"BatchFiller.fill: a spatial slot of batch {sp_slot.B} on {sp_slot.words.device} for a "
                                     f"filler of batch {self.B} on {self.bank.device}")
            else:
                raise ValueError("BatchFiller.fill: spatial= takes SpatialDraws, a SpatialSlot, or nothing")
        if isinstance(draws_or_slot, (CropDraws, ClassCropDraws)):
            slot.load(draws_or_slot, self.bank, self.roi, self.student_sizes)
        elif isinstance(draws_or_slot, CropSlot):
            slot = draws_or_slot
        elif draws_or_slot is not None:
            raise ValueError("BatchFiller.fill takes CropDraws, a CropSlot with draws loaded, or nothing")
        if slot.B != self.B or slot.n_students != len(self.student_sizes) or slot.records.device != self.bank.device:
            raise ValueError(f"BatchFiller.fill: a slot of batch {slot.B} / {slot.n_students} students on "
                             f"{slot.records.device} for a filler of batch {self.B} / {len(self.student_sizes)} students on "
                             f"{self.bank.device}")
        if (slot.class_index is None) != (self.class_index is None):
            raise ValueError("BatchFiller.fill: a class-mode slot needs a filler with a class index, and a filler with a "
                             "class index a class-mode slot")
        if slot.draws is None:
            raise ValueError("BatchFiller.fill: the slot holds no draws (CropSlot.load)")
        shapes, roi, sizes = slot.checked
        if self.class_index is not None:
            if shapes is not self.class_index or roi != self.roi or sizes != self.student_sizes:
                raise ValueError("BatchFiller.fill: the slot's draws were checked against another index, roi or student sizes")
        elif shapes != tuple(self.bank.shapes[:len(shapes)]) or roi != self.roi or sizes != self.student_sizes:
            raise ValueError("BatchFiller.fill: the slot's draws were checked against another bank, roi or student sizes")
        self._check_outputs()
        if isinstance(spatial, SpatialDraws):
            sp_slot.load(spatial)
        if isinstance(elastic, ElasticDraws):
            el_slot.load(elastic)
        if isinstance(corruption, CorruptionDraws):
            co_slot.load(corruption)
        if self.class_index is not None:
            slot.resolve(self.roi)
        self._fill_teacher(slot, sp_slot, el_slot)
        self._fill_students(slot)
        if co_slot is not None:
            self._corrupt_students(co_slot)
        return self.batch

    def _fill_teacher(self, slot: CropSlot, spatial_slot: Optional[SpatialSlot] = None,
                      elastic_slot: Optional[ElasticSlot] = None):
        bank, roi, st = self.bank, i3(self.roi), L.stream()         # every argument is formed once, for either entry
        table, records, lut = L.ptr(bank.table), L.ptr(slot.records), L.ptr(self.lut)
        image, mask, coord = L.ptr(self.image), L.ptr(self.mask), L.ptr(self.coord)
        if spatial_slot is None:
            L.call("mivp_crop_fill", table, bank.capacity, bank.channels, records, slot.words, self.B, roi, lut, image, mask,
                   coord, st)
        elif elastic_slot is None:
            L.call("mivp_crop_fill_affine", table, bank.capacity, bank.channels, records, slot.words,
                   L.ptr(spatial_slot.words), self.B, roi, lut, image, mask, coord, st)
        else:
            L.call("mivp_crop_fill_elastic", table, bank.capacity, bank.channels, records, slot.words,
                   L.ptr(spatial_slot.words), self.B, roi, lut, image, mask, coord, L.ptr(elastic_slot.flags),
                   L.ptr(elastic_slot.lattice), i3(elastic_slot.nodes), st)

    def _fill_students(self, slot: CropSlot):
        st, Cn = L.stream(), self.bank.channels
        for i, size in enumerate(self.student_sizes):
            org = L.ptr(slot.student_views[i])
            L.call("mivp_crop_tensor", L.ptr(self.image), Cn, i3(self.roi), org, slot.words, self.B, i3(size),
                   L.ptr(self.image_st[i]), st)
            L.call("mivp_crop_tensor", L.ptr(self.coord), 3, i3(self.roi), org, slot.words, self.B, i3(size),
                   L.ptr(self.coord_st[i]), st)
        if self.mask_st_0 is not None:
            L.call("mivp_crop_tensor", L.ptr(self.mask), 1, i3(self.roi), L.ptr(slot.student_views[0]), slot.words, self.B,
                   i3(self.student_sizes[0]), L.ptr(self.mask_st_0), st)

    def _corrupt_students(self, slot: CorruptionSlot):
        st, Cn = L.stream(), self.bank.channels
        for i, size in enumerate(self.student_sizes):
            x, rec, rng = L.ptr(self.image_st[i]), L.ptr(slot.records[i]), L.ptr(self.corruption_range[i])
            L.call("mivp_crop_corrupt_range", x, Cn, i3(size), rec, self.B, rng, st)
            L.call("mivp_crop_corrupt", x, Cn, i3(size), rec, self.B, rng, st)
