"""Geodesic (image-aware) distance guidance for click and scribble prompts: the two guidance channels of ``clicks`` (DESIGN
4.46) and ``strokes`` (4.47) as a function of the geodesic distance to the prompt instead of the Euclidean one, so that a ball
around a click stops at an intensity edge (DeepIGeoS, MONAI ``GeodesicDistance`` / FastGeodis, Criminisi's generalised geodesic
transform, nnInteractive-style encodings).  DESIGN 4.48; csrc/geodesic.hip.

Per sample and plane (0 positive, 1 negative), over the 26-neighbour voxel graph: ``g(v)`` = the smallest left-to-right float32
sum of ``w(u, u') = sqrt(l^2 + (gamma (I(u) - I(u')))^2)`` over the paths from a seed, ``l^2 = (a_h |dh| + a_w |dw|) + a_d |dd|``
with ``a`` the float32 squared spacings, every operation a rounded float32 one; ``0`` at a seed, ``+inf`` in a plane without
seeds, and an edge whose weight is not finite is never taken.  The converged field equals a float32 Dijkstra's in every bit.

``seed_mask`` unites the scribble bits of a ``strokes.StrokeSlot`` and the clicks of a ``clicks.ClickSlot`` on the device (boxes
are no seeds); ``geodesic_distance`` iterates brick-wise relaxation launches to the fixed point (one int32 read every
``check_every`` launches) or issues ``max_iter`` of them blind, which is recordable; ``encode_geodesic`` runs seeds -> field ->
the two channels ``max(box, f(g))``; ``GeodesicModel`` puts that in front of a model as ``strokes.StrokeModel`` does.
``clicks.click_rounds`` and ``strokes.scribble_rounds`` accept their own wrapper only, so ``geodesic_rounds`` is the loop here;
it appends to the same slots with the same simulators.

Limits: 26-connectivity, one image channel, two planes, one ``gamma`` per call, at most 65535 iterations; the simulators keep
their Euclidean depth; no prompts on a scan's native grid."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional, Sequence

import torch
from torch import nn

from . import _lib as L
from . import clicks as CK
from . import strokes as ST
from ._host import check_at_least, check_gpu, check_image_batch, check_int_from, check_spacing, i3, plain_int

MAX_ITER = 65535             # iterations of one call (the counter words of the workspace: csrc/geodesic.hip)
BRICK = (16, 16, 32)         # the brick an iteration converges in LDS

GeodesicField = namedtuple("GeodesicField", "field info")


def _round(n: int) -> int:
    return (n + 255) // 256 * 256


def _dims(name: str, batch: int, shape) -> tuple:
    try:
        dims = tuple(shape)
    except TypeError:
        dims = ()
    if len(dims) != 3 or not all(plain_int(s) for s in dims):
        raise ValueError(f"{name}: dims must be three integers (H, W, D), got {shape!r}")
    dims = tuple(int(s) for s in dims)
    if not 1 <= batch <= 65535 or min(dims) < 1 or max(dims) > 65535 or batch * dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"{name}: a batch of {batch} volumes of {dims} is outside the kernels' range "
                         "(1 <= B, H, W, D <= 65535, B H W D < 2^31)")
    return dims


def iteration_cap(dims) -> int:
    """The most iterations a field of ``dims`` can need (a shortest path has fewer than ``H W D`` voxels and every unconverged
    iteration settles one more of them), and the most a call may issue."""
    return min(int(dims[0]) * int(dims[1]) * int(dims[2]), MAX_ITER)


def geodesic_ws(batch: int, dims: Sequence[int], device="cuda") -> torch.Tensor:
    """The uint8 workspace of ``geodesic_distance`` / ``encode_geodesic`` for ``batch`` volumes of ``dims``: room for the seed
    mask, two field buffers ``[B, 2, H, W, D]`` float32, the per-iteration counters and the ``info`` record; reusable by
    every later call."""
    batch = check_int_from("batch", batch, 1)
    dims = _dims("geodesic_ws", batch, dims)
    nbytes = int(L.lib().mivp_geodesic_ws(batch, i3(dims)))
    if nbytes == 0:
        raise ValueError(f"no workspace for a batch of {batch} volumes of {dims}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


class _Layout:
    """The parts of the workspace (include/mivp.h): byte offsets of the seed mask, the two fields, the counters, info."""

    def __init__(self, batch: int, dims):
        n = batch * dims[0] * dims[1] * dims[2]
        self.batch, self.dims, self.nvox = batch, dims, n
        self.fields = (_round(n), _round(n) + _round(8 * n))
        self.counters = self.fields[1] + _round(8 * n)
        self.info = self.counters + _round(4 * (iteration_cap(dims) + 1))
        self.size = self.info + 256

    def seeds_of(self, ws):
        return ws[:self.nvox].view(self.batch, *self.dims)

    def field_of(self, ws, n):
        at = self.fields[n & 1]
        return ws[at:at + 8 * self.nvox].view(torch.float32).view(self.batch, 2, *self.dims)

    def counter_of(self, ws, n):
        return ws[self.counters + 4 * n:self.counters + 4 * n + 4].view(torch.int32)

    def info_of(self, ws):
        return ws[self.info:self.info + 8].view(torch.int32)


def _workspace(workspace, lay: _Layout, device) -> torch.Tensor:
    need = int(L.lib().mivp_geodesic_ws(lay.batch, i3(lay.dims)))
    if need != lay.size:                                           # _Layout restates the carving of csrc/geodesic.hip
        raise RuntimeError(f"mivp_amd: the workspace layout of geodesic.py ({lay.size} bytes) is not the library's ({need})")
    if workspace is None:
        return torch.empty(lay.size, dtype=torch.uint8, device=device)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or not workspace.is_contiguous() \
            or workspace.numel() < lay.size or workspace.device != device or workspace.data_ptr() % 256:
        raise ValueError(f"workspace must be a contiguous, 256-byte aligned uint8 tensor of at least {lay.size} bytes on the "
                         "image's device (geodesic_ws)")
    return workspace


def geodesic_info(workspace: torch.Tensor, batch: int, dims: Sequence[int]) -> torch.Tensor:
    """The int32 ``[2]`` record (iterations that lowered a voxel, converged) the latest call left in ``workspace``."""
    batch = check_int_from("batch", batch, 1)
    lay = _Layout(batch, _dims("geodesic_info", batch, dims))
    if not isinstance(workspace, torch.Tensor):
        raise ValueError(f"workspace must be a tensor (geodesic_ws), got {type(workspace).__name__}")
    return lay.info_of(_workspace(workspace, lay, workspace.device))


def _check_slots(strokes, clicks, batch: int, dims) -> None:
    """Slots bound to this batch and these dims (a ``ClickSlot`` without dims is bound now)."""
    if strokes is not None:
        ST._check_slot(strokes, batch, dims)
    if clicks is not None:
        CK._check_slot(clicks, batch)
        clicks.bind(dims)
    if strokes is not None and clicks is not None and strokes.device != clicks.device:
        raise ValueError("the StrokeSlot and the ClickSlot must be on one device")


def _check_metric(gamma, spacing) -> tuple:
    g = check_at_least("gamma", gamma, 0.0)
    sp = check_spacing(spacing)
    f32 = torch.finfo(torch.float32)
    if g > f32.max or any(not f32.tiny <= s * s <= f32.max for s in sp):
        raise ValueError(f"gamma and the squared spacings must be finite (and the latter normal) in fp32, got {gamma!r}, {sp}")
    return g, sp


def _check_max_iter(max_iter, dims) -> Optional[int]:
    cap = iteration_cap(dims)
    if max_iter is not None and (not plain_int(max_iter) or not 0 <= max_iter <= cap):
        raise ValueError(f"max_iter must be None or an integer in 0 .. {cap} (min(H W D, {MAX_ITER})), got {max_iter!r}")
    return None if max_iter is None else int(max_iter)


def _launch_seed(seeds, strokes, clicks, batch, dims) -> None:
    L.call("mivp_geodesic_seed", L.ptr(None if strokes is None else strokes.mask), L.ptr(None if clicks is None else clicks.clicks),
           L.ptr(None if clicks is None else clicks.count), 1 if clicks is None else clicks.max_clicks, batch, i3(dims), L.ptr(seeds),
           L.stream())


def seed_mask(dims: Sequence[int], strokes: Optional[ST.StrokeSlot] = None, clicks: Optional[CK.ClickSlot] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The seed mask uint8 ``[B, H, W, D]`` in the bit layout of ``StrokeSlot.mask`` (bit 0 positive, bit 1 negative): the union
    of the scribble bits of ``strokes`` and of the clicks of ``clicks``, built on the device in one launch, two with clicks
    (``count`` is clamped to ``0 .. K`` there and an entry with channel -1 is skipped; boxes are no seeds).  Either slot may
    be absent; the batch is the slots', or ``out``'s.  ``out``: a contiguous, 4-byte aligned tensor whose storage goes on to
    the end of its last 32-bit word (a ``StrokeSlot.mask``, or the front of a ``geodesic_ws``)."""
    given = [s.batch for s in (strokes, clicks) if isinstance(s, (ST.StrokeSlot, CK.ClickSlot))]
    if not given and not isinstance(out, torch.Tensor):
        raise ValueError("seed_mask needs a StrokeSlot, a ClickSlot or out= to know the batch")
    batch = given[0] if given else (int(out.shape[0]) if out.dim() == 4 else 0)
    dims = _dims("seed_mask", batch, dims)
    _check_slots(strokes, clicks, batch, dims)
    n = batch * dims[0] * dims[1] * dims[2]
    slot = strokes if strokes is not None else clicks
    if out is None:
        check_gpu("the slot", slot.mask if strokes is not None else slot.clicks)
        out = torch.empty(((n + 3) // 4 * 4,), dtype=torch.uint8, device=slot.device)[:n].view(batch, *dims)
    else:
        room = out.untyped_storage().nbytes() - out.storage_offset() if isinstance(out, torch.Tensor) else 0
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (batch, *dims) \
                or not out.is_contiguous() or room < (n + 3) // 4 * 4:
            raise ValueError(f"out must be a contiguous uint8 {(batch, *dims)} tensor whose storage holds whole 32-bit words")
        if slot is not None and out.device != slot.device:
            raise ValueError("out and the slots must be on one device")
        check_gpu("out", out)
        if out.data_ptr() % 4:
            raise ValueError("out must be 4-byte aligned")
    _launch_seed(out, strokes, clicks, batch, dims)
    return out


def _iterate(image, channel, lay: _Layout, sp, gamma, max_iter, check_every, ws) -> int:
    """begin was issued: the iterations and end.  Returns the number of iterations issued."""
    B, dims = lay.batch, lay.dims
    spacing = (C.c_float * 3)(*sp)
    d3 = i3(dims)

    def launch(it):
        L.call("mivp_geodesic_iter", it, L.ptr(image), int(image.shape[1]), channel, B, d3, spacing, gamma, L.ptr(ws), L.stream())

    n = 0
    if max_iter is not None:
        for n in range(1, max_iter + 1):
            launch(n)
    else:
        cap = iteration_cap(dims)
        while True:
            if n >= cap:
                raise RuntimeError(f"the geodesic field did not converge in {cap} iterations (min(H W D, {MAX_ITER}))")
            for _ in range(min(check_every, cap - n)):
                n += 1
                launch(n)
            if int(lay.counter_of(ws, n)) == 0:                    # the one int32 read: iteration n lowered nothing
                break
    L.call("mivp_geodesic_end", n, B, d3, L.ptr(ws), L.ptr(lay.info_of(ws)), L.stream())
    return n


def geodesic_distance(image: torch.Tensor, seeds: torch.Tensor, *, image_channel: int = 0,
                      spacing: Sequence[float] = (1.0, 1.0, 1.0), gamma: float = 1.0, max_iter: Optional[int] = None,
                      check_every: int = 4, workspace: Optional[torch.Tensor] = None) -> GeodesicField:
    """The geodesic distance fields of ``seeds`` (uint8 ``[B, H, W, D]``, ``seed_mask``) on channel ``image_channel`` of
    ``image`` (float32 ``[B, C, H, W, D]``, contiguous) -> ``GeodesicField(field float32 [B, 2, H, W, D], info int32 [2])``,
    both views into the workspace (valid until its next use).  ``max_iter=None``: iterate on the host, reading one int32 every
    ``check_every`` launches, until a launch lowered nothing; more than ``min(H W D, 65535)`` launches raise.  ``max_iter=n``:
    exactly ``n`` launches, nothing read, recordable; launches behind the fixed point return at once.  ``info`` = (iterations
    that lowered a voxel, 1 if the field is the fixed point else 0).  Equal calls give equal bits, converged or not, and an
    unconverged field is nowhere below the converged one."""
    image = check_image_batch("image", image)
    B, cimg = int(image.shape[0]), int(image.shape[1])
    dims = _dims("geodesic_distance", B, image.shape[2:])
    if not plain_int(image_channel) or not 0 <= image_channel < cimg:
        raise ValueError(f"image_channel must be an integer in 0 .. {cimg - 1}, got {image_channel!r}")
    if not isinstance(seeds, torch.Tensor) or seeds.dtype != torch.uint8 or tuple(seeds.shape) != (B, *dims) \
            or not seeds.is_contiguous() or seeds.device != image.device:
        raise ValueError(f"seeds must be a contiguous uint8 {(B, *dims)} tensor on the image's device (seed_mask), got "
                         f"{(seeds.dtype, tuple(seeds.shape)) if isinstance(seeds, torch.Tensor) else type(seeds).__name__}")
    g, sp = _check_metric(gamma, spacing)
    max_iter = _check_max_iter(max_iter, dims)
    check_every = check_int_from("check_every", check_every, 1)
    lay = _Layout(B, dims)
    if workspace is not None:
        _workspace(workspace, lay, image.device)
    check_gpu("image", image)
    ws = _workspace(workspace, lay, image.device)
    L.call("mivp_geodesic_begin", L.ptr(seeds), B, i3(dims), L.ptr(ws), L.stream())
    n = _iterate(image, int(image_channel), lay, sp, g, max_iter, check_every, ws)
    return GeodesicField(lay.field_of(ws, n), lay.info_of(ws))


def encode_geodesic(image: torch.Tensor, out: torch.Tensor, *, strokes: Optional[ST.StrokeSlot] = None,
                    clicks: Optional[CK.ClickSlot] = None, channel_offset: int, image_channel: int = 0, gamma: float,
                    spacing: Sequence[float], kind: str = "gaussian", sigma: float = 2.0, radius: float = 2.0,
                    box: str = "filled", max_iter: Optional[int] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Write the geodesic guidance of the slots into channels ``channel_offset`` (positive) and ``channel_offset + 1``
    (negative) of the model input ``out`` (float32 ``[B, Ctot, H, W, D]``, contiguous); every element of the two channels is
    stored once, no other byte is touched.  Per voxel and channel the value is ``max(box, f(g))``: ``box`` the rule of
    ``encode_strokes`` on the boxes of ``strokes``; ``g`` the geodesic distance (``geodesic_distance``) to the scribble voxels
    and clicks of the channel on channel ``image_channel`` of ``image`` (float32 ``[B, C, H, W, D]``; it may be ``out`` itself
    when the image channel is none of the two written; any other tensor that shares memory with ``out`` is refused); with ``m = g g`` in float32, ``f = exp(-m / (2 sigma^2))``
    (``"gaussian"``) or ``1 if m <= radius^2 else 0`` (``"disk"``), ``+0`` in a channel without seeds.  seed -> begin ->
    iterations -> end -> encode; with ``max_iter=n`` every launch is unconditional and reads the slots on the device, so a
    recording follows later slot contents and images.  ``geodesic_info(workspace, B, dims)`` is the record of the call.
    Returns ``out``."""
    image = check_image_batch("image", image)
    if not isinstance(out, torch.Tensor) or out.dim() != 5 or out.dtype != torch.float32:
        raise ValueError("out must be a float32 [B, Ctot, H, W, D] tensor, got "
                         f"{(out.dtype, tuple(out.shape)) if isinstance(out, torch.Tensor) else type(out).__name__}")
    B, cimg, ctot = int(image.shape[0]), int(image.shape[1]), int(out.shape[1])
    dims = _dims("encode_geodesic", B, image.shape[2:])
    if (int(out.shape[0]), *out.shape[2:]) != (B, *dims):
        raise ValueError(f"image {tuple(image.shape)} and out {tuple(out.shape)} differ in batch or volume")
    if not plain_int(image_channel) or not 0 <= image_channel < cimg:
        raise ValueError(f"image_channel must be an integer in 0 .. {cimg - 1}, got {image_channel!r}")
    if not plain_int(channel_offset) or not 0 <= channel_offset <= ctot - 2:
        raise ValueError(f"channel_offset must be an integer in 0 .. {ctot - 2} (two guidance channels of {ctot}), "
                         f"got {channel_offset!r}")
    if strokes is not None and not isinstance(strokes, ST.StrokeSlot):
        raise ValueError(f"strokes must be a StrokeSlot or None, got {type(strokes).__name__}")
    if clicks is not None and not isinstance(clicks, CK.ClickSlot):
        raise ValueError(f"clicks must be a ClickSlot or None, got {type(clicks).__name__}")
    _check_slots(strokes, clicks, B, dims)
    frame, code, param = ST._check_encoding(box, kind, sigma, radius)
    g, sp = _check_metric(gamma, spacing)
    max_iter = _check_max_iter(max_iter, dims)
    if not out.is_contiguous() or out.device != image.device or any(s is not None and s.device != image.device
                                                                    for s in (strokes, clicks)):
        raise ValueError("out must be contiguous, and out, the image and the slots on one device")
    if image.data_ptr() == out.data_ptr() and cimg == ctot:
        if channel_offset <= image_channel <= channel_offset + 1:
            raise ValueError("image is out: the image channel must be none of the two guidance channels")
    elif image.device == out.device and image.data_ptr() < out.data_ptr() + 4 * out.numel() \
            and out.data_ptr() < image.data_ptr() + 4 * image.numel():
        raise ValueError("image overlaps out without being out itself: give out as the image, or a tensor of its own")
    lay = _Layout(B, dims)
    if workspace is not None:
        _workspace(workspace, lay, image.device)
    check_gpu("image", image)
    check_gpu("out", out)
    ws = _workspace(workspace, lay, image.device)
    seeds = lay.seeds_of(ws)
    _launch_seed(seeds, strokes, clicks, B, dims)
    L.call("mivp_geodesic_begin", L.ptr(seeds), B, i3(dims), L.ptr(ws), L.stream())
    n = _iterate(image, int(image_channel), lay, sp, g, max_iter, 4, ws)
    L.call("mivp_geodesic_encode", L.ptr(None if strokes is None else strokes.boxes),
           L.ptr(None if strokes is None else strokes.box_count), 1 if strokes is None else strokes.max_boxes, n, B, ctot,
           int(channel_offset), i3(dims), frame, code, param, L.ptr(out), L.ptr(ws), L.stream())
    return out


class GeodesicModel(nn.Module):
    """``forward(image) = model(cat(image, geodesic guidance))``: the image goes into channels ``0 .. Cimg - 1`` of a persistent
    ``[B, Cimg + 2, H, W, D]`` buffer and ``encode_geodesic`` writes the guidance of the ``StrokeSlot`` and / or ``ClickSlot``
    into the last two, reading the image from the buffer, in a persistent workspace; the model reads the buffer, so a recorded
    step follows later slot contents.  The model must read ``Cimg + 2`` channels (``conf.input_channels``); ``conf`` is the
    model's and its ``named_parameters_*`` partitions are forwarded, so ``train.build_optimizer``, ``train.train_step`` and
    ``train.GraphedStep`` run on it unchanged -- with ``max_iter`` an integer there (``None`` reads back; a forward issues
    ``min(max_iter, H W D)`` iterations, which is enough for any field of the volume).  With empty slots
    the output is the model's on the image and two zero channels.  ``encoding``: ``box``, ``kind``, ``radius``, ``sigma``,
    ``spacing``, ``image_channel``.  ``info`` is the record of the latest forward."""

    def __init__(self, model: nn.Module, *, strokes: Optional[ST.StrokeSlot] = None, clicks: Optional[CK.ClickSlot] = None,
                 gamma: float, max_iter: Optional[int], **encoding):
        super().__init__()
        if not isinstance(model, nn.Module):
            raise ValueError(f"model must be an nn.Module, got {type(model).__name__}")
        if isinstance(model, (GeodesicModel, ST.StrokeModel, CK.GuidedModel)):
            raise ValueError(f"model is a {type(model).__name__} already: give the slots as strokes= and clicks=")
        if strokes is not None and not isinstance(strokes, ST.StrokeSlot):
            raise ValueError(f"strokes must be a StrokeSlot or None, got {type(strokes).__name__}")
        if clicks is not None and not isinstance(clicks, CK.ClickSlot):
            raise ValueError(f"clicks must be a ClickSlot or None, got {type(clicks).__name__}")
        if strokes is not None and clicks is not None and clicks.batch != strokes.batch:
            raise ValueError(f"the ClickSlot was built for a batch of {clicks.batch}, the StrokeSlot for {strokes.batch}")
        cin = getattr(getattr(model, "conf", None), "input_channels", None)
        if cin is None or int(cin) < 3:
            raise ValueError(f"the model must read the image and two guidance channels (conf.input_channels >= 3), got {cin!r}")
        unknown = set(encoding) - {"box", "kind", "radius", "sigma", "spacing", "image_channel"}
        if unknown:
            raise ValueError(f"unknown encoding keywords {sorted(unknown)}")
        enc = dict(box="filled", kind="gaussian", radius=2.0, sigma=2.0, spacing=(1.0, 1.0, 1.0), image_channel=0)
        enc.update(encoding)
        ST._check_encoding(enc["box"], enc["kind"], enc["sigma"], enc["radius"])
        gamma, enc["spacing"] = _check_metric(gamma, enc["spacing"])
        if max_iter is not None and (not plain_int(max_iter) or not 0 <= max_iter <= MAX_ITER):
            raise ValueError(f"max_iter must be None or an integer in 0 .. {MAX_ITER}, got {max_iter!r}")
        self.image_channels = int(cin) - 2
        if not plain_int(enc["image_channel"]) or not 0 <= enc["image_channel"] < self.image_channels:
            raise ValueError(f"image_channel must be an integer in 0 .. {self.image_channels - 1}, got {enc['image_channel']!r}")
        self.model = model
        self.strokes = strokes
        self.clicks = clicks
        self.gamma = gamma
        self.max_iter = max_iter
        self.encoding = enc
        self._input = None
        self._ws = None

    @property
    def conf(self):
        return self.model.conf

    @property
    def info(self) -> Optional[torch.Tensor]:
        if self._input is None:
            return None
        return geodesic_info(self._ws, int(self._input.shape[0]), self._input.shape[2:])

    def model_input(self, image: torch.Tensor) -> torch.Tensor:
        """The persistent model input, filled from ``image`` and the slots."""
        image = check_image_batch("image", image, contiguous=False)
        if image.shape[1] != self.image_channels:
            raise ValueError(f"the model reads {self.image_channels + 2} channels = {self.image_channels} image channels + 2 "
                             f"guidance channels, the image has {image.shape[1]}")
        B = int(image.shape[0])
        dims = _dims("GeodesicModel", B, image.shape[2:])
        _check_slots(self.strokes, self.clicks, B, dims)
        check_gpu("image", image)
        shape = (B, self.image_channels + 2, *dims)
        if self._input is None or tuple(self._input.shape) != shape or self._input.device != image.device:
            self._input = torch.zeros(shape, dtype=torch.float32, device=image.device)
            self._ws = geodesic_ws(B, dims, image.device)
        self._input[:, :self.image_channels].copy_(image)
        # launches behind the fixed point return at once, so the volume's cap loses nothing
        max_iter = None if self.max_iter is None else min(self.max_iter, iteration_cap(dims))
        return encode_geodesic(self._input, self._input, strokes=self.strokes, clicks=self.clicks,
                               channel_offset=self.image_channels, gamma=self.gamma, max_iter=max_iter,
                               workspace=self._ws, **self.encoding)

    def forward(self, image):
        return self.model(self.model_input(image))

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name.startswith("named_parameters_"):
                return getattr(super().__getattr__("model"), name)
            raise


def geodesic_rounds(guided: GeodesicModel, image: torch.Tensor, target: Optional[torch.Tensor], rounds: int, *,
                    key: str = "downstream", click_kwargs: Optional[dict] = None, scribble_kwargs: Optional[dict] = None):
    """The iterative-sampling recipe on a ``GeodesicModel`` (``clicks.click_rounds`` and ``strokes.scribble_rounds`` take
    their own wrappers only): ``rounds`` times [forward under ``no_grad`` -> ``simulate_clicks_from_logits`` into the wrapper's
    ``ClickSlot`` (``click_kwargs``) and / or ``simulate_scribbles`` of the arg-max into its ``StrokeSlot``
    (``scribble_kwargs``)], the simulators and slots of the Euclidean encodings as they stand (their depth stays Euclidean).
    The model runs in the mode it is in.  ``target=None``: nothing is simulated.  Returns the logits of the last forward
    (``None`` for ``rounds=0``); no host read when the wrapper's ``max_iter`` is an integer."""
    rounds = check_int_from("rounds", rounds, 0)
    if not isinstance(guided, GeodesicModel):
        raise ValueError(f"guided must be a GeodesicModel, got {type(guided).__name__}")
    logits = None
    for _ in range(rounds):
        with torch.no_grad():
            out = guided(image)
        logits = out[key] if isinstance(out, dict) else out
        if target is None:
            continue
        if guided.clicks is not None:
            CK.simulate_clicks_from_logits(logits, target, guided.clicks, **(click_kwargs or {}))
        if guided.strokes is not None:
            ST.simulate_scribbles(logits.argmax(dim=1), target, guided.strokes, **(scribble_kwargs or {}))
    return logits
