"""Box and scribble prompts: boxes ("the object is in here") and strokes drawn along a structure or along an error, as two
guidance channels of the model input, and the simulated box and corrective scribble of interactive training and evaluation
(nnInteractive, SAM-Med3D, MONAI Label, DeepEdit).  DESIGN 4.47; the click prompts of ``clicks`` are the third
interaction and combine with these in ``StrokeModel``.

``StrokeSlot`` is the device record of a batch: ``boxes int32 [B, KB, 7]`` = (h0, w0, d0, h1, w1, d1, channel) with inclusive
corners, ``box_count int32 [B]``, ``mask uint8 [B, H, W, D]`` (bit 0 a positive scribble voxel, bit 1 a negative one) and
``last int32 [B, 8]``, the record of the latest simulation.  ``StrokeSlot.draw`` rasterises a user's polyline in one launch.
``encode_strokes`` turns the record into the two guidance channels in four launches: an exact batched distance transform of
the two bit planes on the line passes of ``csrc/edt_common.hpp`` and a closing pass that also evaluates the boxes.
``simulate_box`` stores the (jittered, clamped) bounding box of the object, ``simulate_scribbles`` the curve skeleton of the
core of each error region, with the error regions and the padded depth of ``simulate_clicks`` and the thinning of
``skeleton``; nothing is read back by any of them (csrc/strokes.hip).  ``StrokeModel`` puts the encoding in front of a model
as ``clicks.GuidedModel`` does; ``scribble_rounds`` and ``box_then_scribbles`` are the loops built from these calls.

Out of scope: lasso / free-form regions, geodesic distances, random cropping or displacement of simulated scribbles, a
fused arg-max, strokes on a scan's native grid."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Iterable, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import clicks as CK
from ._host import (LABEL_DTYPES, check_at_least, check_flag, check_gpu, check_int_from, check_spacing, i3, label_batch,
                    plain_int)

MAX_BOXES = 16               # KB of a slot (the closing pass keeps a sample's boxes in LDS: csrc/strokes.hip)
MAX_POINTS = 256             # points of one polyline
MAX_ITER = 4096              # of the thinning (skeleton.MAX_ITER)
BOX_MODES = ("filled", "frame")
KINDS = ("disk", "gaussian")

StrokeRecord = namedtuple("StrokeRecord", "boxes box_count mask last")


def _dims(name: str, batch: int, shape) -> tuple:
    try:
        dims = tuple(shape)
    except TypeError:
        dims = ()
    if len(dims) != 3 or not all(plain_int(s) for s in dims):
        raise ValueError(f"{name}: dims must be three integers (H, W, D), got {shape!r}")
    dims = tuple(int(s) for s in dims)
    if min(dims) < 1 or max(dims) > 65535 or batch * (dims[0] + 2) * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"{name}: a batch of {batch} volumes of {dims} is outside the kernels' range "
                         "(1 <= H, W, D <= 65535, B (H + 2) W D < 2^31)")
    return dims


def _triple(name: str, v) -> Optional[tuple]:
    try:
        vals = None if isinstance(v, (str, bytes)) else tuple(v)
    except TypeError:
        vals = None
    return vals


def check_box(name: str, box, dims) -> tuple:
    """One box ``(h0, w0, d0, h1, w1, d1, channel)``: plain ints, inclusive corners inside ``dims`` with ``lo <= hi`` per axis,
    channel 0 (positive) or 1 (negative)."""
    vals = _triple(name, box)
    if vals is None or len(vals) != 7 or not all(plain_int(v) for v in vals):
        raise ValueError(f"{name} must be seven integers (h0, w0, d0, h1, w1, d1, channel), got {box!r}")
    if vals[6] not in (0, 1):
        raise ValueError(f"{name}: channel must be 0 (positive) or 1 (negative), got {vals[6]!r}")
    for a in range(3):
        for v in (vals[a], vals[3 + a]):
            if not 0 <= v < dims[a]:
                raise ValueError(f"{name}: coordinate {a} = {v} is outside 0 .. {dims[a] - 1}")
        if vals[a] > vals[3 + a]:
            raise ValueError(f"{name}: lo > hi on axis {a} ({vals[a]} > {vals[3 + a]}): corners are inclusive with lo <= hi")
    return tuple(int(v) for v in vals)


def check_points(points, dims) -> np.ndarray:
    """A polyline of 1 .. 256 integer voxel coordinates inside ``dims`` -> int32 ``[n, 3]``."""
    try:
        rows = None if isinstance(points, (str, bytes)) else [_triple("point", p) for p in points]
    except TypeError:
        rows = None
    if rows is None or any(r is None or len(r) != 3 or not all(plain_int(v) for v in r) for r in rows):
        raise ValueError(f"points must be a sequence of (h, w, d) integer triples, got {points!r}")
    if not 1 <= len(rows) <= MAX_POINTS:
        raise ValueError(f"a stroke has 1 .. {MAX_POINTS} points, got {len(rows)}")
    for i, r in enumerate(rows):
        for a in range(3):
            if not 0 <= r[a] < dims[a]:
                raise ValueError(f"point {i}: coordinate {a} = {r[a]} is outside 0 .. {dims[a] - 1}")
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def _check_channel(channel) -> int:
    if not plain_int(channel) or channel not in (0, 1):
        raise ValueError(f"channel must be 0 (positive) or 1 (negative), got {channel!r}")
    return int(channel)


class StrokeSlot:
    """Fixed device storage for the boxes and scribbles of a batch of ``dims`` = (H, W, D) volumes: up to ``max_boxes`` (<= 16)
    boxes per sample and one byte per voxel for the scribbles.  ``last[b]`` = (lo', hi', placed, 0) after ``simulate_box``,
    (voxels added to bit 0, voxels added to bit 1, converged, 0, ...) after ``simulate_scribbles``.  The host calls check every
    coordinate before anything is copied or launched."""

    def __init__(self, batch: int, dims: Sequence[int], max_boxes: int = 4, device="cuda"):
        self.batch = check_int_from("batch", batch, 1)
        self.max_boxes = check_int_from("max_boxes", max_boxes, 1)
        if self.batch > 65535:
            raise ValueError(f"batch must be at most 65535, got {batch}")
        if self.max_boxes > MAX_BOXES:
            raise ValueError(f"max_boxes must be at most {MAX_BOXES}, got {max_boxes}")
        self.dims = _dims("StrokeSlot", self.batch, dims)
        n = self.batch * self.dims[0] * self.dims[1] * self.dims[2]
        self.boxes = torch.full((self.batch, self.max_boxes, 7), -1, dtype=torch.int32, device=device)
        self.box_count = torch.zeros((self.batch,), dtype=torch.int32, device=device)
        self._bytes = torch.zeros(((n + 3) // 4 * 4,), dtype=torch.uint8, device=device)      # whole 32-bit words: draw's atomicOr
        self.mask = self._bytes[:n].view(self.batch, *self.dims)
        self.last = torch.zeros((self.batch, 8), dtype=torch.int32, device=device)
        self._scratch = torch.zeros((self.batch, 8), dtype=torch.int32, device=device)       # simulate_box: zero between calls

    @property
    def device(self):
        return self.boxes.device

    def _sample(self, b) -> int:
        if not plain_int(b) or not 0 <= b < self.batch:
            raise ValueError(f"sample index must be an integer in 0 .. {self.batch - 1}, got {b!r}")
        return int(b)

    def set_boxes(self, b: int, rows: Iterable) -> None:
        """Replace the boxes of sample ``b`` by ``[(h0, w0, d0, h1, w1, d1, channel), ...]`` (stream-ordered copies)."""
        b = self._sample(b)
        rows = [check_box(f"box {i}", r, self.dims) for i, r in enumerate(rows)]
        if len(rows) > self.max_boxes:
            raise ValueError(f"{len(rows)} boxes, the slot takes {self.max_boxes} per sample")
        table = np.full((self.max_boxes, 7), -1, dtype=np.int32)
        if rows:
            table[:len(rows)] = np.asarray(rows, dtype=np.int32)
        self.boxes[b].copy_(torch.from_numpy(table))
        self.box_count[b:b + 1].copy_(torch.tensor([len(rows)], dtype=torch.int32))

    def add_box(self, b: int, row) -> None:
        """Append one box to sample ``b``.  Reads ``box_count[b]`` back (a user's box, not part of a training step)."""
        b = self._sample(b)
        row = check_box("box", row, self.dims)
        n = int(self.box_count[b])
        if n >= self.max_boxes:
            raise ValueError(f"sample {b} is full ({self.max_boxes} boxes)")
        self.boxes[b, n].copy_(torch.tensor(row, dtype=torch.int32))
        self.box_count[b:b + 1].copy_(torch.tensor([n + 1], dtype=torch.int32))

    def draw(self, b: int, points: Iterable, channel: int) -> None:
        """Rasterise the polyline ``points`` (1 .. 256 ``(h, w, d)`` voxels inside the volume) into bit ``channel`` of sample
        ``b``'s scribble mask.  Each consecutive pair ``a -> b`` sets ``a + floor((2 i delta + n) / (2 n))`` for ``i = 0 .. n``,
        ``delta = b - a``, ``n = max |delta|`` (the floor towards minus infinity, per axis); a single point, or ``n = 0``, sets
        that voxel.  One stream-ordered copy of the points and one launch; nothing else in ``mask`` changes."""
        b = self._sample(b)
        pts = check_points(points, self.dims)
        channel = _check_channel(channel)
        check_gpu("the slot's mask", self.mask)
        steps = int(np.abs(np.diff(pts.astype(np.int64), axis=0)).max()) if len(pts) > 1 else 0
        dev = torch.from_numpy(pts).to(self.device)
        L.call("mivp_strokes_draw", L.ptr(dev), len(pts), steps, b, channel, self.batch, i3(self.dims), L.ptr(self._bytes),
               L.stream())

    def clear_scribbles(self) -> None:
        self._bytes.zero_()

    def clear(self) -> None:
        self.boxes.fill_(-1)
        self.box_count.zero_()
        self._bytes.zero_()
        self.last.zero_()
        self._scratch.zero_()

    def cpu(self) -> StrokeRecord:
        """(boxes, box_count, mask, last) as numpy arrays: the one host read."""
        return StrokeRecord(self.boxes.cpu().numpy(), self.box_count.cpu().numpy(), self.mask.cpu().numpy(),
                            self.last.cpu().numpy())


def _check_slot(slot, batch: int, dims=None) -> None:
    if not isinstance(slot, StrokeSlot):
        raise ValueError(f"slot must be a StrokeSlot, got {type(slot).__name__}")
    if slot.batch != batch:
        raise ValueError(f"the slot was built for a batch of {slot.batch}, got {batch}")
    if dims is not None and tuple(int(d) for d in dims) != slot.dims:
        raise ValueError(f"the slot holds strokes of a {slot.dims} volume, got {tuple(int(d) for d in dims)}")


def _check_encoding(box, kind, sigma, radius) -> tuple:
    """-> (frame flag, kind code, param)."""
    if box not in BOX_MODES:
        raise ValueError(f"box must be one of {BOX_MODES}, got {box!r}")
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    code, param = CK._check_kind(kind, sigma, radius)
    return int(box == "frame"), code, param


def strokes_ws(batch: int, dims: Sequence[int], device="cuda") -> torch.Tensor:
    """The uint8 workspace of ``encode_strokes`` and ``simulate_scribbles`` for ``batch`` volumes of ``dims`` (one size serves
    both; reusable by every later call)."""
    batch = check_int_from("batch", batch, 1)
    dims = _dims("strokes_ws", batch, dims)
    nbytes = int(L.lib().mivp_strokes_ws(batch, i3(dims)))
    if nbytes == 0:
        raise ValueError(f"no workspace for a batch of {batch} volumes of {dims}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _workspace(workspace, slot: StrokeSlot) -> torch.Tensor:
    need = int(L.lib().mivp_strokes_ws(slot.batch, i3(slot.dims)))
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=slot.device)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or not workspace.is_contiguous() \
            or workspace.numel() < need or workspace.device != slot.device or workspace.data_ptr() % 256:
        raise ValueError(f"workspace must be a contiguous, 256-byte aligned uint8 tensor of at least {need} bytes on the "
                         "slot's device (strokes_ws)")
    return workspace


def encode_strokes(slot: StrokeSlot, out: torch.Tensor, *, channel_offset: int, box: str = "filled", kind: str = "disk",
                   radius: float = 2.0, sigma: float = 2.0, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Write the slot's boxes and scribbles into channels ``channel_offset`` (positive) and ``channel_offset + 1`` (negative)
    of the model input ``out`` (float32 ``[B, Ctot, H, W, D]``, contiguous); every element of the two channels is stored once,
    no other byte is touched.  Per voxel and channel the value is ``max(box, stroke)``: ``box`` is 1 inside a box of the
    channel (``"filled"``) or on a box's surface (``"frame"``: inside, with a coordinate equal to the box's ``lo`` or ``hi``);
    with ``m`` the smallest squared distance in mm to a scribble voxel of the channel, ``stroke`` is ``1 if m <= radius^2 else
    0`` (``kind="disk"``) or ``exp(-m / (2 sigma^2))`` (``"gaussian"``), and ``+0`` in a channel without a scribble voxel.
    ``m`` is the exact Euclidean transform (the exact integer at unit spacing).  Four unconditional launches that read the slot
    on the device: a recording follows later slot contents.  With ``workspace=strokes_ws(B, dims)`` nothing is allocated.
    Returns ``out``."""
    if not isinstance(out, torch.Tensor) or out.dim() != 5 or out.dtype != torch.float32:
        raise ValueError("out must be a float32 [B, Ctot, H, W, D] tensor, got "
                         f"{(out.dtype, tuple(out.shape)) if isinstance(out, torch.Tensor) else type(out).__name__}")
    B, ctot = int(out.shape[0]), int(out.shape[1])
    _check_slot(slot, B, out.shape[2:])
    if not plain_int(channel_offset) or not 0 <= channel_offset <= ctot - 2:
        raise ValueError(f"channel_offset must be an integer in 0 .. {ctot - 2} (two guidance channels of {ctot}), "
                         f"got {channel_offset!r}")
    frame, code, param = _check_encoding(box, kind, sigma, radius)
    sp = check_spacing(spacing)
    check_gpu("out", out)
    if not out.is_contiguous() or out.device != slot.device:
        raise ValueError("out must be contiguous and on the slot's device")
    ws = _workspace(workspace, slot)
    L.call("mivp_strokes_encode", L.ptr(slot.boxes), L.ptr(slot.box_count), L.ptr(slot.mask), B, slot.max_boxes, ctot,
           int(channel_offset), i3(slot.dims), (C.c_float * 3)(*sp), frame, code, param, L.ptr(out), L.ptr(ws), L.stream())
    return out


def _check_ignore(ignore_index):
    if ignore_index is not None and (not plain_int(ignore_index) or not -2 ** 31 <= ignore_index < 2 ** 31):
        raise ValueError(f"ignore_index must be None or an int32, got {ignore_index!r}")
    return (0, 0) if ignore_index is None else (int(ignore_index), 1)


def draw_box_jitter(generator, batch: int, max_jitter: int) -> np.ndarray:
    """The int32 ``[B, 6]`` table (lo offsets, hi offsets) of ``simulate_box``: uniform integers in ``-max_jitter ..
    max_jitter`` from ``generator`` (a ``numpy.random.Generator`` or ``RandomState``)."""
    batch = check_int_from("batch", batch, 1)
    if not plain_int(max_jitter) or not 0 <= max_jitter <= 65535:
        raise ValueError(f"max_jitter must be an integer in 0 .. 65535, got {max_jitter!r}")
    draw = getattr(generator, "integers", None) or getattr(generator, "randint", None)
    if draw is None:
        raise ValueError(f"generator must be a numpy Generator or RandomState, got {type(generator).__name__}")
    return np.asarray(draw(-int(max_jitter), int(max_jitter) + 1, size=(batch, 6)), dtype=np.int32)


def simulate_box(target: torch.Tensor, slot: StrokeSlot, *, object_classes: Optional[Iterable[int]] = None,
                 ignore_index: Optional[int] = None, margin: Sequence[int] = (0, 0, 0), jitter=None,
                 channel: int = 0) -> StrokeSlot:
    """Append the bounding box of every sample's object to ``slot``.  ``target``: class maps ``[B, H, W, D]`` or ``[B, 1, H, W,
    D]``; the object is ``{label in object_classes}`` (default ``label > 0``) among the valid voxels (not ``ignore_index``, a
    class 0 .. 31: the rules of ``simulate_clicks``).  With ``(lo, hi)`` its tight box, the stored box is ``lo' = clamp(lo -
    margin + j_lo, 0, hi)``, ``hi' = clamp(hi + margin + j_hi, lo, dim - 1)`` per axis, ``jitter`` an optional host int32
    ``[B, 6]`` table (``draw_box_jitter``): it is never empty, lies inside the volume and meets the object.  It is appended
    with ``channel`` iff the object is not empty and the sample has room; ``last[b]`` = (lo', hi', placed, 0), or (-1 x 6, 0,
    0) for an empty object, is written either way.  Two unconditional launches, no host read."""
    target = label_batch("target", target)
    B = int(target.shape[0])
    _check_slot(slot, B, target.shape[1:])
    mask = CK.object_mask(object_classes)
    ign, has_ign = _check_ignore(ignore_index)
    m = _triple("margin", margin)
    if m is None or len(m) != 3 or not all(plain_int(v) and 0 <= v <= 65535 for v in m):
        raise ValueError(f"margin must be three integers in 0 .. 65535, got {margin!r}")
    channel = _check_channel(channel)
    table = None
    if jitter is not None:
        table = jitter.numpy() if isinstance(jitter, torch.Tensor) and not jitter.is_cuda else jitter
        if not isinstance(table, np.ndarray) or table.dtype != np.int32 or table.shape != (B, 6) \
                or int(np.abs(table.astype(np.int64)).max()) > 65535:
            raise ValueError(f"jitter must be a host int32 [{B}, 6] table with entries in -65535 .. 65535 (draw_box_jitter)")
    if target.device != slot.device:
        raise ValueError("target and the slot must be on one device")
    dev = None if table is None else torch.from_numpy(np.ascontiguousarray(table)).to(slot.device)
    L.call("mivp_strokes_box", L.ptr(target), LABEL_DTYPES[target.dtype], B, i3(slot.dims), mask, ign, has_ign,
           (C.c_int32 * 3)(*[int(v) for v in m]), L.ptr(dev), channel, slot.max_boxes, L.ptr(slot.boxes), L.ptr(slot.box_count),
           L.ptr(slot.last), L.ptr(slot._scratch), L.stream())
    return slot


def simulate_scribbles(pred: torch.Tensor, target: torch.Tensor, slot: StrokeSlot, *,
                       object_classes: Optional[Iterable[int]] = None, ignore_index: Optional[int] = None,
                       spacing: Sequence[float] = (1.0, 1.0, 1.0), min_depth: float = 1.5, max_iter: int = 32,
                       keep_endpoints: bool = True, workspace: Optional[torch.Tensor] = None) -> StrokeSlot:
    """Add the corrective scribbles of every sample to ``slot.mask``.  ``pred`` / ``target``: class maps ``[B, H, W, D]`` or
    ``[B, 1, H, W, D]``.  ``E_pos`` / ``E_neg`` are the error regions of ``simulate_clicks`` and depth is its padded transform;
    the core of a region is ``{depth^2 >= min_depth^2}`` (the boundary slivers every prediction has give no scribble) and the
    scribble is the curve skeleton of each core: per sample, exactly what ``skeleton.skeletonize(core map, 3,
    max_iter=max_iter, keep_endpoints=keep_endpoints)`` returns with ``E_pos`` as class 1 and ``E_neg`` as class 2.  Positive
    skeleton voxels set bit 0 of the mask, negative ones bit 1; bits already there stay.  ``last[b]`` = (voxels that gained
    bit 0, voxels that gained bit 1, converged, 0, ...), ``converged`` telling whether the thinning of the batch stopped by
    itself within ``max_iter`` (if not, the result is the thicker scribble of ``max_iter`` iterations).  Every launch is
    unconditional and nothing is read back; with ``workspace=strokes_ws(B, dims)`` nothing is allocated."""
    pred = label_batch("pred", pred)
    target = label_batch("target", target)
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    B = int(target.shape[0])
    _check_slot(slot, B, target.shape[1:])
    mask = CK.object_mask(object_classes)
    ign, has_ign = _check_ignore(ignore_index)
    sp = check_spacing(spacing)
    md = check_at_least("min_depth", min_depth, 0.0)
    if md * md >= 3.0e38:
        raise ValueError(f"min_depth^2 must be finite in fp32, got {min_depth!r}")
    if not plain_int(max_iter) or not 1 <= max_iter <= MAX_ITER:
        raise ValueError(f"max_iter must be an integer in 1..{MAX_ITER}, got {max_iter!r}")
    keep = check_flag("keep_endpoints", keep_endpoints)
    if pred.device != slot.device or target.device != slot.device:
        raise ValueError("pred, target and the slot must be on one device")
    ws = _workspace(workspace, slot)
    L.call("mivp_strokes_scribbles", L.ptr(pred), LABEL_DTYPES[pred.dtype], L.ptr(target), LABEL_DTYPES[target.dtype], B,
           i3(slot.dims), (C.c_float * 3)(*sp), mask, ign, has_ign, md * md, int(max_iter), int(keep), L.ptr(slot.mask),
           L.ptr(slot.last), L.ptr(ws), L.stream())
    return slot


class StrokeModel(nn.Module):
    """``forward(image) = model(cat(image, stroke guidance[, click guidance]))``: the image goes into channels ``0 .. Cimg - 1``
    of a persistent ``[B, Cimg + 2 (+ 2), H, W, D]`` buffer, the ``StrokeSlot`` is encoded into channels ``Cimg, Cimg + 1`` and
    an optional ``clicks.ClickSlot`` into ``Cimg + 2, Cimg + 3`` by ``encode_clicks`` (with this encoding's ``kind``, ``sigma``,
    ``radius`` and ``spacing``); the model reads the buffer, so a recorded step follows later slot contents.  The model must
    read that many channels (``conf.input_channels``).  Its ``named_parameters_*`` partitions are forwarded and ``conf`` is the
    model's, as with ``clicks.GuidedModel``.  With empty slots the output is the model's on the image and zero channels.
    ``encoding``: the keywords of ``encode_strokes`` (``box``, ``kind``, ``radius``, ``sigma``, ``spacing``)."""

    def __init__(self, model: nn.Module, slot: StrokeSlot, clicks: Optional[CK.ClickSlot] = None, **encoding):
        super().__init__()
        if not isinstance(model, nn.Module):
            raise ValueError(f"model must be an nn.Module, got {type(model).__name__}")
        if isinstance(model, (StrokeModel, CK.GuidedModel)):
            raise ValueError(f"model is a {type(model).__name__} already: give the ClickSlot as clicks=")
        if not isinstance(slot, StrokeSlot):
            raise ValueError(f"slot must be a StrokeSlot, got {type(slot).__name__}")
        if clicks is not None and not isinstance(clicks, CK.ClickSlot):
            raise ValueError(f"clicks must be a ClickSlot or None, got {type(clicks).__name__}")
        if clicks is not None and clicks.batch != slot.batch:
            raise ValueError(f"the ClickSlot was built for a batch of {clicks.batch}, the StrokeSlot for {slot.batch}")
        extra = 2 if clicks is None else 4
        cin = getattr(getattr(model, "conf", None), "input_channels", None)
        if cin is None or int(cin) < extra + 1:
            raise ValueError(f"the model must read the image and {extra} guidance channels (conf.input_channels >= {extra + 1}), "
                             f"got {cin!r}")
        unknown = set(encoding) - {"box", "kind", "radius", "sigma", "spacing"}
        if unknown:
            raise ValueError(f"unknown encoding keywords {sorted(unknown)}")
        enc = dict(box="filled", kind="disk", radius=2.0, sigma=2.0, spacing=(1.0, 1.0, 1.0))
        enc.update(encoding)
        _check_encoding(enc["box"], enc["kind"], enc["sigma"], enc["radius"])
        enc["spacing"] = check_spacing(enc["spacing"])
        self.model = model
        self.slot = slot
        self.clicks = clicks
        self.guidance_channels = extra
        self.image_channels = int(cin) - extra
        self.encoding = enc
        self._input = None
        self._ws = None

    @property
    def conf(self):
        return self.model.conf

    def workspace(self) -> torch.Tensor:
        """The persistent ``strokes_ws`` of the wrapper (``scribble_rounds`` simulates in it as well)."""
        if self._ws is None or self._ws.device != self.slot.device:
            self._ws = strokes_ws(self.slot.batch, self.slot.dims, self.slot.device)
        return self._ws

    def model_input(self, image: torch.Tensor) -> torch.Tensor:
        """The persistent model input, filled from ``image`` and the slots."""
        if not isinstance(image, torch.Tensor) or image.dim() != 5 or image.dtype != torch.float32:
            raise ValueError("image must be a float32 [B, Cimg, H, W, D] tensor, got "
                             f"{(image.dtype, tuple(image.shape)) if isinstance(image, torch.Tensor) else type(image).__name__}")
        g = self.guidance_channels
        if image.shape[1] != self.image_channels:
            raise ValueError(f"the model reads {self.image_channels + g} channels = {self.image_channels} image channels + {g} "
                             f"guidance channels, the image has {image.shape[1]}")
        _check_slot(self.slot, int(image.shape[0]), image.shape[2:])
        check_gpu("image", image)
        shape = (image.shape[0], self.image_channels + g, *image.shape[2:])
        if self._input is None or tuple(self._input.shape) != shape or self._input.device != image.device:
            self._input = torch.zeros(shape, dtype=torch.float32, device=image.device)
        self._input[:, :self.image_channels].copy_(image)
        enc = self.encoding
        encode_strokes(self.slot, self._input, channel_offset=self.image_channels, workspace=self.workspace(), **enc)
        if self.clicks is not None:
            CK.encode_clicks(self.clicks, self._input, channel_offset=self.image_channels + 2, sigma=enc["sigma"],
                             kind=enc["kind"], radius=enc["radius"], spacing=enc["spacing"])
        return self._input

    def forward(self, image):
        return self.model(self.model_input(image))

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name.startswith("named_parameters_"):
                return getattr(super().__getattr__("model"), name)
            raise


def scribble_rounds(guided: StrokeModel, image: torch.Tensor, target: Optional[torch.Tensor], slot: StrokeSlot, rounds: int, *,
                    key: str = "downstream", **simulate_kwargs):
    """The iterative-sampling recipe with scribbles: ``rounds`` times [forward under ``no_grad`` -> ``argmax`` over the classes
    -> ``simulate_scribbles``], so the slot's mask accumulates the corrective scribbles of every round; the caller's ordinary
    ``train_step`` on the ``StrokeModel`` then trains on them.  The model runs in the mode it is in.  ``target=None``: nothing
    is simulated, the slot keeps the caller's own strokes.  Returns the logits of the last forward (``None`` for
    ``rounds=0``); no host read."""
    rounds = check_int_from("rounds", rounds, 0)
    if not isinstance(guided, StrokeModel):
        raise ValueError(f"guided must be a StrokeModel, got {type(guided).__name__}")
    if guided.slot is not slot:
        raise ValueError("the StrokeModel reads another slot than the one given")
    logits = None
    for _ in range(rounds):
        with torch.no_grad():
            out = guided(image)
        logits = out[key] if isinstance(out, dict) else out
        if target is not None:
            simulate_scribbles(logits.argmax(dim=1), target, slot, workspace=guided.workspace(), **simulate_kwargs)
    return logits


def box_then_scribbles(guided: StrokeModel, image: torch.Tensor, target: torch.Tensor, slot: StrokeSlot, rounds: int, *,
                       key: str = "downstream", box_kwargs: Optional[dict] = None, **simulate_kwargs):
    """``simulate_box(target, slot, **box_kwargs)`` (keywords that both calls take, ``object_classes`` and ``ignore_index``, are
    passed on to it), then ``scribble_rounds``: the usual session of a box first and corrective strokes after it."""
    shared = {k: simulate_kwargs[k] for k in ("object_classes", "ignore_index") if k in simulate_kwargs}
    simulate_box(target, slot, **{**shared, **(box_kwargs or {})})
    return scribble_rounds(guided, image, target, slot, rounds, key=key, **simulate_kwargs)
