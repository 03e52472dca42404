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
``augment`` and ``scan``.  The draw ORDER documented at ``draw_crops`` is this project's."""
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


def _size3(name: str, v) -> Tuple[int, int, int]:
    v = tuple(v) if not plain_int(v) else (v, v, v)
    if len(v) != 3:
        raise ValueError(f"{name} must be three sizes, got {v!r}")
    return tuple(check_int_from(name, a, 1) for a in v)


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
        for b in range(B):
            if not 0 <= int(vol[b]) < len(shapes):
                raise ValueError(f"CropDraws: sample {b}: volume id {int(vol[b])} outside the bank's 0..{len(shapes) - 1}")
            if not 0 <= int(rot[b]) <= 3:
                raise ValueError(f"CropDraws: sample {b}: rotation code {int(rot[b])} outside 0..3")
            n_rot = rotated_shape(shapes[int(vol[b])], int(rot[b]))
            for k in range(3):
                hi = max(n_rot[k] - roi[k], 0)
                if not 0 <= int(org[b, k]) <= hi:
                    raise ValueError(f"CropDraws: sample {b}: origin {org[b].tolist()} outside [0, {hi}] on axis {k} (rotated "
                                     f"volume {n_rot}, roi {roi})")
            for s, size in enumerate(sizes):
                for k in range(3):
                    hi = max(roi[k] - size[k], 0)
                    if not 0 <= int(st[s, b, k]) <= hi:
                        raise ValueError(f"CropDraws: sample {b}: origin {st[s, b].tolist()} of student {s} outside [0, {hi}] "
                                         f"on axis {k} (roi {roi}, student size {size})")
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
    roi = _size3("roi", roi)
    sizes = [_size3("student size", s) for s in student_sizes]
    shapes = list(bank_shapes)
    ids = [int(v) for v in volume_ids]
    check_int_from("num_samples", num_samples, 1)
    if not ids or any(not 0 <= v < len(shapes) for v in ids):
        raise ValueError(f"draw_crops: volume_ids {ids} must be a non-empty list of ids in 0..{len(shapes) - 1}")
    B = len(ids) * int(num_samples)
    d = CropDraws(np.repeat(np.asarray(ids, np.int32), int(num_samples)), np.zeros(B, np.int32), np.zeros((B, 3), np.int32),
                  np.zeros((len(sizes), B, 3), np.int32))
    if random_orientation:
        for i in range(len(ids)):
            d.rot[i * num_samples:(i + 1) * num_samples] = int(rs.randint(3)) + 1
    for b in range(B):
        n_rot = rotated_shape(shapes[int(d.volume[b])], int(d.rot[b]))
        for k in range(3):
            d.origin[b, k] = rs.randint(0, n_rot[k] - min(roi[k], n_rot[k]) + 1)
    for b in range(B):
        for s, size in enumerate(sizes):
            for k in range(3):
                d.student_origin[s, b, k] = rs.randint(0, roi[k] - min(size[k], roi[k]) + 1)
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
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("VolumeBank: a GPU device expected (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
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


class CropSlot:
    """Fixed device memory of one batch's draws -- int32 [B][5 + 3 S] records -- whose pointer a recorded graph keeps.
    ``load`` checks the draws against the bank, then refreshes the records from a new pinned staging buffer without blocking;
    it does nothing while a graph is being recorded, exactly as ``augment.IntensitySlot.load``."""

    def __init__(self, B: int, n_students: int, device):
        self.B = check_int_from("B", B, 1)
        self.n_students = check_int_from("n_students", n_students, 0)
        self.words = record_words(self.n_students)
        self.records = torch.zeros(self.B * self.words, dtype=torch.int32, device=device)
        self.student_views = [self.records[HEAD + 3 * s:] for s in range(self.n_students)]   # advanced to the origin words
        self.draws = None
        self.checked = None             # (bank shapes, roi, student sizes) the loaded draws were checked against

    def load(self, draws: CropDraws, bank, roi, student_sizes=()):
        if not isinstance(draws, CropDraws):
            raise ValueError("CropSlot.load: CropDraws expected")
        if len(tuple(student_sizes)) != self.n_students:
            raise ValueError(f"CropSlot: {len(tuple(student_sizes))} student sizes for a slot of {self.n_students} students")
        if draws.check(bank, roi, student_sizes).batch != self.B:
            raise ValueError(f"CropSlot: draws of batch {draws.batch} do not match the slot's batch {self.B}")
        if torch.cuda.is_current_stream_capturing():
            return
        self.records.copy_(torch.from_numpy(draws.pack().reshape(-1)).pin_memory(), non_blocking=True)
        self.draws = draws
        shapes = bank.shapes if hasattr(bank, "shapes") else bank
        self.checked = (tuple(tuple(s) for s in shapes), _size3("roi", roi), [_size3("student size", s) for s in student_sizes])


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
    itself, or a ``GraphedStep`` whose inputs they are) sees every later ``fill``."""

    def __init__(self, bank: VolumeBank, roi, batch: int, student_sizes=(), active_labels=None, with_coord: bool = False,
                 with_mask: bool = True):
        if not isinstance(bank, VolumeBank):
            raise ValueError("BatchFiller: a VolumeBank expected")
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
        self.slot = CropSlot(self.B, S, dev)
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
    def fill(self, draws_or_slot=None):
        """``CropDraws``: checked and loaded into the filler's own slot first.  A ``CropSlot``: used as it stands (its
        ``load`` did the checking).  ``None``: the filler's own slot as last loaded."""
        slot = self.slot
        if isinstance(draws_or_slot, CropDraws):
            slot.load(draws_or_slot, self.bank, self.roi, self.student_sizes)
        elif isinstance(draws_or_slot, CropSlot):
            slot = draws_or_slot
        elif draws_or_slot is not None:
            raise ValueError("BatchFiller.fill takes CropDraws, a CropSlot with draws loaded, or nothing")
        if slot.B != self.B or slot.n_students != len(self.student_sizes) or slot.records.device != self.bank.device:
            raise ValueError(f"BatchFiller.fill: a slot of batch {slot.B} / {slot.n_students} students on "
                             f"{slot.records.device} for a filler of batch {self.B} / {len(self.student_sizes)} students on "
                             f"{self.bank.device}")
        if slot.draws is None:
            raise ValueError("BatchFiller.fill: the slot holds no draws (CropSlot.load)")
        shapes, roi, sizes = slot.checked
        if shapes != tuple(self.bank.shapes[:len(shapes)]) or roi != self.roi or sizes != self.student_sizes:
            raise ValueError("BatchFiller.fill: the slot's draws were checked against another bank, roi or student sizes")
        self._check_outputs()
        self._fill_teacher(slot)
        self._fill_students(slot)
        return self.batch

    def _fill_teacher(self, slot: CropSlot):
        bank = self.bank
        L.call("mivp_crop_fill", L.ptr(bank.table), bank.capacity, bank.channels, L.ptr(slot.records), slot.words, self.B,
               i3(self.roi), L.ptr(self.lut), L.ptr(self.image), L.ptr(self.mask), L.ptr(self.coord), L.stream())

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
