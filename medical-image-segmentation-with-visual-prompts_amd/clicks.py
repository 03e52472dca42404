"""Interactive click prompts: positive / negative clicks as two guidance channels of the model input, and the simulated
corrective click of iterative training and evaluation (RITM, DeepEdit, SAM-Med3D, nnInteractive).  DESIGN 4.46.

``ClickSlot`` is the device record of a batch (``clicks int32 [B, K, 4]`` = (h, w, d, channel), ``count int32 [B]``,
``last int32 [B, 4]``).  ``encode_clicks`` turns it into the two guidance channels of a model input in one launch;
``simulate_clicks`` / ``simulate_clicks_from_logits`` compare a prediction with the reference and append, per sample, the voxel
deepest inside the largest error -- five launches, nothing read back (csrc/clicks.hip).  ``GuidedModel`` puts the encoding in
front of a model the way ``prompting.PromptedModel`` puts a prompt there, so ``train.build_optimizer``, ``train.train_step``
and ``train.GraphedStep`` run on it unchanged; ``click_rounds`` and ``refine_volume`` are the two loops built from these calls.

Out of scope: boxes and scribbles, geodesic (image-aware) distances, random click placement weighted by depth, more than one
object per pass, clicks on a scan's native grid, any change to the predictor's kernels."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib as L
from ._host import (LABEL_DTYPES, check_at_least, check_click, check_gpu, check_int_from, check_spacing, i3, label_batch,
                    plain_int)

MAX_CLICKS = 64              # K of a slot (one wave compacts a sample's clicks: csrc/clicks.hip)
MAX_CLASSES = 32             # labels are classes 0 .. 31; the object is a 32-bit mask
KINDS = ("gaussian", "disk")
LOGITS = 4                   # pred dtype code of the fused arg-max

ClickRecord = namedtuple("ClickRecord", "clicks count last")


def _dims(name: str, shape) -> tuple:
    dims = tuple(int(s) for s in shape)
    if min(dims) < 1 or max(dims) > 65535 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"{name}: a volume of {dims} is outside the kernels' range (1 <= H, W, D <= 65535, H W D < 2^31)")
    return dims


class ClickSlot:
    """Fixed storage for up to ``max_clicks`` (<= 64) clicks per sample of a batch.  Channel 0 is a positive click, 1 a negative
    one, -1 marks an empty entry.  ``last[b]`` = (float bits of the winning depth^2, channel, raster index, placed flag) of the
    latest simulation.  ``dims``: the volume the clicks live in, when known; otherwise the first ``encode_clicks`` /
    ``simulate_clicks`` on the slot binds it.  The host calls check every coordinate before anything is copied."""

    def __init__(self, batch: int, max_clicks: int = 32, dims: Optional[Sequence[int]] = None, device="cuda"):
        self.batch = check_int_from("batch", batch, 1)
        self.max_clicks = check_int_from("max_clicks", max_clicks, 1)
        if self.batch > 65535:
            raise ValueError(f"batch must be at most 65535, got {batch}")
        if self.max_clicks > MAX_CLICKS:
            raise ValueError(f"max_clicks must be at most {MAX_CLICKS}, got {max_clicks}")
        self.dims = None if dims is None else _dims("ClickSlot", dims)
        self._reach = [0, 0, 0]                   # 1 + the largest coordinate a host call has stored, per axis
        self.clicks = torch.full((self.batch, self.max_clicks, 4), -1, dtype=torch.int32, device=device)
        self.count = torch.zeros((self.batch,), dtype=torch.int32, device=device)
        self.last = torch.zeros((self.batch, 4), dtype=torch.int32, device=device)

    @property
    def device(self):
        return self.clicks.device

    def _sample(self, b) -> int:
        if not plain_int(b) or not 0 <= b < self.batch:
            raise ValueError(f"sample index must be an integer in 0 .. {self.batch - 1}, got {b!r}")
        return int(b)

    def bind(self, dims) -> None:
        """Tie the slot to a volume: later host calls check against it, and what they stored so far must fit."""
        dims = tuple(int(d) for d in dims)
        if self.dims is not None and self.dims != dims:
            raise ValueError(f"the slot holds clicks of a {self.dims} volume, got {dims}")
        for a in range(3):
            if self._reach[a] > dims[a]:
                raise ValueError(f"the slot holds a click at coordinate {a} = {self._reach[a] - 1}, outside the volume {dims}")
        self.dims = dims

    def set(self, b: int, clicks: Iterable) -> None:
        """Replace the clicks of sample ``b`` by ``[(h, w, d, channel), ...]`` (stream-ordered copies)."""
        b = self._sample(b)
        rows = [check_click(f"click {i}", c, self.dims) for i, c in enumerate(clicks)]
        if len(rows) > self.max_clicks:
            raise ValueError(f"{len(rows)} clicks, the slot takes {self.max_clicks} per sample")
        table = np.full((self.max_clicks, 4), -1, dtype=np.int32)
        if rows:
            table[:len(rows)] = np.asarray(rows, dtype=np.int32)
            self._reach = [max(self._reach[a], int(table[:len(rows), a].max()) + 1) for a in range(3)]
        self.clicks[b].copy_(torch.from_numpy(table))
        self.count[b:b + 1].copy_(torch.tensor([len(rows)], dtype=torch.int32))

    def add(self, b: int, click) -> None:
        """Append one click to sample ``b``.  Reads ``count[b]`` back (a user's click, not part of a training step)."""
        b = self._sample(b)
        row = check_click("click", click, self.dims)
        n = int(self.count[b])
        if n >= self.max_clicks:
            raise ValueError(f"sample {b} is full ({self.max_clicks} clicks)")
        self._reach = [max(self._reach[a], row[a] + 1) for a in range(3)]
        self.clicks[b, n].copy_(torch.tensor(row, dtype=torch.int32))
        self.count[b:b + 1].copy_(torch.tensor([n + 1], dtype=torch.int32))

    def clear(self) -> None:
        self.clicks.fill_(-1)
        self.count.zero_()
        self.last.zero_()
        self._reach = [0, 0, 0]

    def cpu(self) -> ClickRecord:
        """(clicks, count, last) as numpy arrays: the one host read."""
        return ClickRecord(self.clicks.cpu().numpy(), self.count.cpu().numpy(), self.last.cpu().numpy())


def _check_slot(slot, batch: int) -> None:
    if not isinstance(slot, ClickSlot):
        raise ValueError(f"slot must be a ClickSlot, got {type(slot).__name__}")
    if slot.batch != batch:
        raise ValueError(f"the slot was built for a batch of {slot.batch}, got {batch}")


def _check_kind(kind, sigma, radius) -> tuple:
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    if kind == "gaussian":
        s = check_at_least("sigma", sigma, 0.0)
        if not 0.0 < 2.0 * s * s < 3.0e38:
            raise ValueError(f"sigma must be > 0 with 2 sigma^2 finite in fp32, got {sigma!r}")
        return 0, 2.0 * s * s
    r = check_at_least("radius", radius, 0.0)
    if r * r >= 3.0e38:
        raise ValueError(f"radius^2 must be finite in fp32, got {radius!r}")
    return 1, r * r


def encode_clicks(slot: ClickSlot, out: torch.Tensor, *, channel_offset: int, sigma: float = 2.0, kind: str = "gaussian",
                  radius: float = 2.0, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> torch.Tensor:
    """Write the slot's clicks into channels ``channel_offset`` (positive) and ``channel_offset + 1`` (negative) of the model
    input ``out`` (float32 ``[B, Ctot, H, W, D]``, contiguous); no other channel is touched.  Per voxel and channel, with
    ``m`` the smallest squared distance in mm to a click of that channel: ``exp(-m / (2 sigma^2))`` (``kind="gaussian"``: the
    maximum of the per-click Gaussians) or ``1 if m <= radius^2 else 0`` (``"disk"``); ``+0`` in a channel without clicks.  One
    unconditional launch that reads ``count`` on the device: a recording follows later slot contents.  Returns ``out``."""
    if not isinstance(out, torch.Tensor) or out.dim() != 5 or out.dtype != torch.float32:
        raise ValueError("out must be a float32 [B, Ctot, H, W, D] tensor, got "
                         f"{(out.dtype, tuple(out.shape)) if isinstance(out, torch.Tensor) else type(out).__name__}")
    B, ctot = int(out.shape[0]), int(out.shape[1])
    _check_slot(slot, B)
    if not plain_int(channel_offset) or not 0 <= channel_offset <= ctot - 2:
        raise ValueError(f"channel_offset must be an integer in 0 .. {ctot - 2} (two guidance channels of {ctot}), "
                         f"got {channel_offset!r}")
    code, param = _check_kind(kind, sigma, radius)
    sp = check_spacing(spacing)
    dims = _dims("encode_clicks", out.shape[2:])
    slot.bind(dims)
    check_gpu("out", out)
    if not out.is_contiguous() or out.device != slot.device:
        raise ValueError("out must be contiguous and on the slot's device")
    L.call("mivp_clicks_encode", L.ptr(slot.clicks), L.ptr(slot.count), B, slot.max_clicks, ctot, int(channel_offset), i3(dims),
           (C.c_float * 3)(*sp), code, param, L.ptr(out), L.stream())
    return out


def simulate_clicks_ws(batch: int, dims: Sequence[int], device="cuda") -> torch.Tensor:
    """The uint8 workspace of ``simulate_clicks`` for ``batch`` volumes of ``dims`` (reusable by every later call)."""
    batch = check_int_from("batch", batch, 1)
    dims = _dims("simulate_clicks_ws", dims)
    nbytes = int(L.lib().mivp_clicks_simulate_ws(batch, i3(dims)))
    if nbytes == 0:
        raise ValueError(f"no workspace for a batch of {batch} volumes of {dims}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def object_mask(object_classes: Optional[Iterable[int]]) -> int:
    """``object_classes`` (default: every class above 0; distinct ints in 0 .. 31) as a bit mask."""
    if object_classes is None:
        return 0xFFFFFFFE
    cls = list(object_classes)
    if not cls:
        raise ValueError("object_classes is empty")
    for c in cls:
        if not plain_int(c) or not 0 <= c < MAX_CLASSES:
            raise ValueError(f"object_classes must be ints in 0..{MAX_CLASSES - 1}, got {c!r}")
    if len(set(cls)) != len(cls):
        raise ValueError(f"object_classes has duplicates: {cls}")
    mask = 0
    for c in cls:
        mask |= 1 << int(c)
    return mask


def _simulate(pred, pdt, ncls, target, slot, dims, object_classes, ignore_index, spacing, min_depth, workspace):
    B = int(target.shape[0])
    _check_slot(slot, B)
    mask = object_mask(object_classes)
    if ignore_index is not None and (not plain_int(ignore_index) or not -2 ** 31 <= ignore_index < 2 ** 31):
        raise ValueError(f"ignore_index must be None or an int32, got {ignore_index!r}")
    sp = check_spacing(spacing)
    md = check_at_least("min_depth", min_depth, 0.0)
    if md * md >= 3.0e38:
        raise ValueError(f"min_depth^2 must be finite in fp32, got {min_depth!r}")
    slot.bind(dims)
    if pred.device != slot.device or target.device != slot.device:
        raise ValueError("pred, target and the slot must be on one device")
    need = int(L.lib().mivp_clicks_simulate_ws(B, i3(dims)))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=slot.device)
    elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or not workspace.is_contiguous() \
            or workspace.numel() < need or workspace.device != slot.device or workspace.data_ptr() % 256:
        raise ValueError(f"workspace must be a contiguous, 256-byte aligned uint8 tensor of at least {need} bytes on the "
                         "slot's device (simulate_clicks_ws)")
    L.call("mivp_clicks_simulate", L.ptr(pred), pdt, ncls, L.ptr(target), LABEL_DTYPES[target.dtype], B, i3(dims),
           (C.c_float * 3)(*sp), mask, 0 if ignore_index is None else int(ignore_index), 0 if ignore_index is None else 1,
           md * md, slot.max_clicks, L.ptr(slot.clicks), L.ptr(slot.count), L.ptr(slot.last), L.ptr(workspace), L.stream())
    return slot


def simulate_clicks(pred: torch.Tensor, target: torch.Tensor, slot: ClickSlot, *, object_classes: Optional[Iterable[int]] = None,
                    ignore_index: Optional[int] = None, spacing: Sequence[float] = (1.0, 1.0, 1.0), min_depth: float = 0.0,
                    workspace: Optional[torch.Tensor] = None) -> ClickSlot:
    """Append the next corrective click of every sample to ``slot``.  ``pred`` / ``target``: class maps ``[B, H, W, D]`` or
    ``[B, 1, H, W, D]``.  The object is ``{label in object_classes}`` (default ``label > 0``); ``E_pos`` = target in the object,
    pred not (a positive click), ``E_neg`` = pred in the object, target not (a negative click); a voxel whose target is
    ``ignore_index`` or no class 0 .. 31 is in neither.  The click is the voxel with the largest squared distance (mm) to the
    outside of its region, the outside of the volume counting as outside; ties go to ``E_pos``, then to the lowest raster
    index.  It is appended iff a region exists, its depth is at least ``min_depth`` and the sample has room; ``slot.last`` is
    written either way.  Five unconditional launches, no host read; with ``workspace=simulate_clicks_ws(B, dims)`` nothing is
    allocated."""
    pred = label_batch("pred", pred)
    target = label_batch("target", target)
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
    dims = _dims("simulate_clicks", target.shape[1:])
    return _simulate(pred, LABEL_DTYPES[pred.dtype], 0, target, slot, dims, object_classes, ignore_index, spacing, min_depth,
                     workspace)


def simulate_clicks_from_logits(logits: torch.Tensor, target: torch.Tensor, slot: ClickSlot, *,
                                object_classes: Optional[Iterable[int]] = None, ignore_index: Optional[int] = None,
                                spacing: Sequence[float] = (1.0, 1.0, 1.0), min_depth: float = 0.0,
                                workspace: Optional[torch.Tensor] = None) -> ClickSlot:
    """``simulate_clicks`` on the arg-max of ``logits [B, C, H, W, D]`` (C <= 32), fused into the first pass: no label map of
    the prediction is written; the lowest index wins among exact maxima.  The channels-last fp32 storage the model returns is
    read as it is, any other layout is copied once."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 5 or not 1 <= logits.shape[1] <= MAX_CLASSES:
        raise ValueError(f"logits must be [B, C, H, W, D] with C <= {MAX_CLASSES}, got "
                         f"{tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
    check_gpu("logits", logits)
    target = label_batch("target", target)
    if (logits.shape[0], *logits.shape[2:]) != tuple(target.shape):
        raise ValueError(f"logits {tuple(logits.shape)} and target {tuple(target.shape)} differ")
    dims = _dims("simulate_clicks_from_logits", target.shape[1:])
    z = logits.detach().permute(0, 2, 3, 4, 1).to(torch.float32).contiguous()
    return _simulate(z, LOGITS, int(logits.shape[1]), target, slot, dims, object_classes, ignore_index, spacing, min_depth,
                     workspace)


class GuidedModel(nn.Module):
    """``forward(image) = model(cat(image, guidance))``: the image goes into channels ``0 .. Cimg - 1`` of a persistent
    ``[B, Cimg + 2, H, W, D]`` buffer, the slot is encoded into the last two and the model reads the buffer, so a recorded
    step follows later slot contents.  The model must read ``Cimg + 2`` channels (``conf.input_channels``).  Its
    ``named_parameters_*`` partitions are forwarded and ``conf`` is the model's, as with ``prompting.PromptedModel``.  With
    an empty slot the output is the model's on the image and two zero channels."""

    def __init__(self, model: nn.Module, slot: ClickSlot, sigma: float = 2.0, kind: str = "gaussian", radius: float = 2.0,
                 spacing: Sequence[float] = (1.0, 1.0, 1.0)):
        super().__init__()
        if not isinstance(model, nn.Module):
            raise ValueError(f"model must be an nn.Module, got {type(model).__name__}")
        if isinstance(model, GuidedModel):
            raise ValueError("model is a GuidedModel already: one slot per model")
        if not isinstance(slot, ClickSlot):
            raise ValueError(f"slot must be a ClickSlot, got {type(slot).__name__}")
        cin = getattr(getattr(model, "conf", None), "input_channels", None)
        if cin is None or int(cin) < 3:
            raise ValueError(f"the model must read the image and two guidance channels (conf.input_channels >= 3), got {cin!r}")
        _check_kind(kind, sigma, radius)
        self.model = model
        self.slot = slot
        self.image_channels = int(cin) - 2
        self.encoding = dict(sigma=sigma, kind=kind, radius=radius, spacing=check_spacing(spacing))
        self._input = None

    @property
    def conf(self):
        return self.model.conf

    def model_input(self, image: torch.Tensor) -> torch.Tensor:
        """The persistent model input, filled from ``image`` and the slot."""
        if not isinstance(image, torch.Tensor) or image.dim() != 5 or image.dtype != torch.float32:
            raise ValueError("image must be a float32 [B, Cimg, H, W, D] tensor, got "
                             f"{(image.dtype, tuple(image.shape)) if isinstance(image, torch.Tensor) else type(image).__name__}")
        if image.shape[1] != self.image_channels:
            raise ValueError(f"the model reads {self.image_channels + 2} channels = {self.image_channels} image channels + 2 "
                             f"guidance channels, the image has {image.shape[1]}")
        _check_slot(self.slot, int(image.shape[0]))
        check_gpu("image", image)
        shape = (image.shape[0], self.image_channels + 2, *image.shape[2:])
        if self._input is None or tuple(self._input.shape) != shape or self._input.device != image.device:
            self._input = torch.zeros(shape, dtype=torch.float32, device=image.device)
        self._input[:, :self.image_channels].copy_(image)
        return encode_clicks(self.slot, self._input, channel_offset=self.image_channels, **self.encoding)

    def forward(self, image):
        return self.model(self.model_input(image))

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name.startswith("named_parameters_"):
                return getattr(super().__getattr__("model"), name)
            raise


def click_rounds(model_or_guided, image: torch.Tensor, target: Optional[torch.Tensor], slot: ClickSlot, rounds: int, *,
                 key: str = "downstream", **simulate_kwargs):
    """The iterative-sampling recipe: ``rounds`` times [forward under ``no_grad`` -> ``simulate_clicks_from_logits``], so the
    slot accumulates one corrective click per round and sample that has an error; the caller's ordinary ``train_step`` on the
    ``GuidedModel`` then trains on them.  A bare model is wrapped in a ``GuidedModel`` on ``slot`` with the default encoding.
    The model runs in the mode it is in.  ``target=None``: nothing is simulated, the slot keeps the caller's own clicks.
    Returns the logits of the last forward (``None`` for ``rounds=0``); no host read."""
    rounds = check_int_from("rounds", rounds, 0)
    guided = model_or_guided if isinstance(model_or_guided, GuidedModel) else GuidedModel(model_or_guided, slot)
    if guided.slot is not slot:
        raise ValueError("the GuidedModel reads another slot than the one given")
    logits = None
    for _ in range(rounds):
        with torch.no_grad():
            out = guided(image)
        logits = out[key] if isinstance(out, dict) else out
        if target is not None:
            simulate_clicks_from_logits(logits, target, slot, **simulate_kwargs)
    return logits


def refine_volume(predictor, image: torch.Tensor, target: Optional[torch.Tensor], slot: ClickSlot, rounds: int, *,
                  sigma: float = 2.0, kind: str = "gaussian", radius: float = 2.0, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                  **simulate_kwargs) -> List[torch.Tensor]:
    """Whole-scan refinement with a ``SlidingWindowPredictor`` whose model reads ``Cimg + 2`` channels: predict on the
    caller's clicks, then ``rounds`` times [``simulate_clicks`` against ``target`` -> ``encode_clicks`` into the whole-volume
    input -> predict].  ``image``: float32 ``[1, Cimg, H, W, D]``; the slot has batch 1.  Returns the ``rounds + 1`` label maps
    (uint8 ``[1, 1, H, W, D]``), the first from the caller's clicks alone.  ``target=None``: only that first map."""
    rounds = check_int_from("rounds", rounds, 0)
    if not isinstance(image, torch.Tensor) or image.dim() != 5 or image.shape[0] != 1 or image.dtype != torch.float32:
        raise ValueError("image must be a float32 [1, Cimg, H, W, D] tensor")
    _check_slot(slot, 1)
    check_gpu("image", image)
    cimg = int(image.shape[1])
    x = torch.zeros((1, cimg + 2, *image.shape[2:]), dtype=torch.float32, device=image.device)
    x[:, :cimg].copy_(image)
    enc = dict(channel_offset=cimg, sigma=sigma, kind=kind, radius=radius, spacing=spacing)
    maps = [predictor.predict(encode_clicks(slot, x, **enc))["labels"].clone()]      # (the predictor reuses its buffers)
    if target is None:
        return maps
    ws = simulate_clicks_ws(1, image.shape[2:], image.device)
    for _ in range(rounds):
        simulate_clicks(maps[-1], target, slot, spacing=spacing, workspace=ws, **simulate_kwargs)
        maps.append(predictor.predict(encode_clicks(slot, x, **enc))["labels"].clone())
    return maps
