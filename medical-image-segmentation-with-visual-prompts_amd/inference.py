"""Evaluation side of the reference's ``SegmentationTrainer.test`` on the device (segmentation.py:204-300):
the fixed sliding windows, sub-batches of ten, per-volume MeanIoU / DiceCoefficient -- with the windows cut on the device
and the metric counts accumulated by one kernel per sub-batch (no ``.item()`` inside the loop; the reference syncs
2 x classes times per update, utils.py:26-35,52-62)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import (ImmutableValue, channels_last_or_copy, check_classes, check_fill_logit, check_finite, check_flag,
                    check_gpu, check_int_from, check_region_mask, i3, iou_dice)
from .multilabel import GroupEvaluation, evaluate_volume_groups  # noqa: F401  (inference.evaluate_volume_groups)
from .skeleton import CenterlineEvaluation, evaluate_volume_centerline  # noqa: F401  (inference.evaluate_volume_centerline)
from .window_fit import WindowFit, foreground_box


def window_grid(image_size: Sequence[int], roi: Sequence[int]) -> Tuple[List[slice], List[int], List[int]]:
    """segmentation.py:232-241: stride = roi // 2, the volume is centre-cropped to the largest size the stride grid covers.
    Returns (crop slices, stride, windows per axis)."""
    stride = [r // 2 for r in roi]
    slc, count = [], []
    for n, w, s in zip(image_size, roi, stride):
        adjusted = (n - w) // s * s + w
        start = (n - adjusted) // 2
        slc.append(slice(start, start + adjusted))
        count.append((adjusted - w) // s + 1)
    return slc, stride, count


def sliding_window_view(x: torch.Tensor, roi: Sequence[int]) -> torch.Tensor:
    """``x [1, C, H, W, D]`` -> ``[N, C, r0, r1, r2]`` in the reference's window order (segmentation.py:242-253)."""
    if x.shape[0] != 1:
        raise ValueError("the reference's test() unfolds one volume at a time (it squeezes the batch axis)")
    slc, stride, _ = window_grid(x.shape[2:], roi)
    a = x[:, :, slc[0], slc[1], slc[2]]
    u = a.unfold(2, roi[0], stride[0]).unfold(3, roi[1], stride[1]).unfold(4, roi[2], stride[2])
    # a VIEW over the volume ([n0, n1, n2] windows of [C, roi]): with stride roi / 2 the materialised windows are ~8x the
    # volume (the reference keeps them on the CPU and moves ten at a time); ``window_batch`` copies one sub-batch
    return u.squeeze(0).permute(1, 2, 3, 0, 4, 5, 6)


def sliding_windows(x: torch.Tensor, roi: Sequence[int]) -> torch.Tensor:
    """All windows materialised, ``[N, C, roi]`` in the reference's flatten order (tests; small volumes)."""
    v = sliding_window_view(x, roi)
    return v.reshape(-1, *v.shape[3:]).contiguous()


def window_batch(win_view: torch.Tensor, begin: int, end: int) -> torch.Tensor:
    """Windows ``begin .. end`` (row-major over the window grid, the reference's flatten order) as one contiguous batch."""
    flat = win_view.reshape(-1, *win_view.shape[3:]) if win_view.is_contiguous() else None
    if flat is not None:
        return flat[begin:end]
    n0, n1, n2 = win_view.shape[:3]
    idx = torch.arange(begin, min(end, n0 * n1 * n2), device=win_view.device)
    return win_view[idx // (n1 * n2), (idx // n2) % n1, idx % n2].contiguous()


class SegMetrics:
    """MeanIoU and DiceCoefficient (utils.py:14-64) from device-resident counts."""

    def __init__(self, num_classes: int, device):
        self.num_classes = num_classes
        self.counts = torch.zeros((num_classes, 3), dtype=torch.int64, device=device)

    def reset(self):
        self.counts.zero_()

    def update(self, preds: torch.Tensor, target: torch.Tensor):
        """preds [B, C, ...] float logits (the model's channels-first view of channels-last storage, or contiguous);
        target [B, 1, ...] float class indices."""
        if not preds.is_cuda:
            raise RuntimeError("SegMetrics runs on the GPU (the CPU restatement is oracle/loss_ref.py)")
        Cn = preds.shape[1]
        if Cn != self.num_classes:
            raise ValueError("class count mismatch")
        src, clast = channels_last_or_copy(preds)
        tgt = target.float().contiguous()
        vol = 1
        for n in preds.shape[2:]:
            vol *= int(n)
        L.call("mivp_seg_counts", L.ptr(src), L.ptr(tgt), preds.shape[0] * vol, Cn, clast, vol, L.ptr(self.counts), L.stream())

    def compute(self) -> Tuple[float, float]:
        """(mean IoU, mean Dice) -- the one host read."""
        return iou_dice(self.counts)


@torch.no_grad()
def test_volume(model, x: torch.Tensor, seg: torch.Tensor, roi: Sequence[int], num_classes: int, sub_batch: int = 10):
    """One volume of segmentation.py:225-286: windows, sub-batches of ten through ``model`` (eval mode), metrics over all of
    the volume's windows.  ``x [1, C, H, W, D]``, ``seg [1, 1, H, W, D]`` (already mapped to class indices).  Returns
    (mean IoU, mean Dice) of this volume."""
    dev = x.device
    xw = sliding_window_view(x, roi)
    sw = sliding_window_view(seg, roi)
    m = SegMetrics(num_classes, dev)
    n = xw.shape[0] * xw.shape[1] * xw.shape[2]
    for i in range(0, n, sub_batch):
        out = model(window_batch(xw, i, i + sub_batch))["downstream"]
        m.update(out, window_batch(sw, i, i + sub_batch))
    return m.compute()


def summarize(values: List[float]) -> Tuple[float, float]:
    """mean and (population) standard deviation over the volumes, as logged by segmentation.py:297-300."""
    mean = sum(values) / len(values)
    return mean, (sum((v - mean) ** 2 for v in values) / len(values)) ** 0.5



# ---------------------------------------------------------------------------------------------------------------------
# Whole-volume prediction: every voxel predicted, overlapping windows blended on the device (csrc/stitch.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _check_overlap(overlap: float):
    if not (0.0 <= float(overlap) < 1.0):
        raise ValueError(f"overlap must be in [0, 1), got {overlap}")


# truncates non-integer sizes, unlike scan._shape3, which rejects them
def _check_shape3(name: str, v: Sequence[int]) -> Tuple[int, int, int]:
    t = tuple(int(a) for a in v)
    if len(t) != 3 or min(t) < 1:
        raise ValueError(f"{name} must be three positive sizes, got {tuple(v)}")
    return t


def _check_sub_batch(sub_batch) -> int:
    if int(sub_batch) < 1:
        raise ValueError("sub_batch must be >= 1")
    return int(sub_batch)


def window_padding(image_size: Sequence[int], roi: Sequence[int]) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """(zeros in front per axis, padded size per axis): an axis shorter than the roi is padded to the roi, (r - n) // 2
    in front and the rest behind; other axes are not padded."""
    n, r = _check_shape3("image_size", image_size), _check_shape3("roi", roi)
    pad = tuple((ri - ni) // 2 if ni < ri else 0 for ni, ri in zip(n, r))
    return pad, tuple(max(ni, ri) for ni, ri in zip(n, r))


def _fit_intervals(roi: Sequence[int], overlap: float) -> Tuple[int, int, int]:
    """Per axis ``max(int(r * (1 - overlap)), 1)``, the window step of ``window_origins`` (and of the fitted tiling,
    which takes it from the host so that the float arithmetic is done once)."""
    _check_overlap(overlap)
    return tuple(max(int(r * (1.0 - float(overlap))), 1) for r in _check_shape3("roi", roi))


def window_origins(image_size: Sequence[int], roi: Sequence[int], overlap: float) -> np.ndarray:
    """Window origins int32 [N, 3] in padded-volume coordinates (``window_padding``), row-major over the per-axis counts.

    The placement follows MONAI ``sliding_window_inference``'s conventions, written out here (MONAI is not a dependency,
    so parity with it is not pinned by a test): per axis, on the padded size n and roi r,
    ``interval = max(int(r * (1 - overlap)), 1)``, ``count = ceil((n - r) / interval) + 1`` and window i starts at
    ``min(i * interval, n - r)``, so the last window is flush with the end."""
    _check_overlap(overlap)                                      # (refused before a bad shape, as always)
    _, p = window_padding(image_size, roi)
    axes = []
    for n, r, interval in zip(p, roi, _fit_intervals(roi, overlap)):
        count = int(math.ceil((n - r) / interval)) + 1
        axes.append([min(i * interval, n - r) for i in range(count)])
    g = np.stack(np.meshgrid(*[np.asarray(a, dtype=np.int32) for a in axes], indexing="ij"), axis=-1)
    return g.reshape(-1, 3).astype(np.int32)


def window_table(origins: np.ndarray, sub_batch: int) -> np.ndarray:
    """The device table: int32 [ceil(N / sub_batch) * sub_batch, 4] = (o0, o1, o2, valid); padding entries are invalid."""
    return tta_table(origins, sub_batch, (0,))


def flip_codes(mirror_axes: Sequence[int] = ()) -> Tuple[int, ...]:
    """The flip codes of mirror test-time augmentation: every subset of ``mirror_axes`` (distinct spatial axes out of
    0 = H, 1 = W, 2 = D) as a 3-bit mask, bit ``a`` set = axis ``a`` flipped, in increasing numeric order from 0."""
    try:
        axes = [int(a) for a in mirror_axes]
        exact = all(int(a) == a for a in mirror_axes)
    except (TypeError, ValueError):
        raise ValueError(f"mirror_axes must be a sequence of axes out of 0, 1, 2, got {mirror_axes!r}") from None
    if not exact or any(a < 0 or a > 2 for a in axes):
        raise ValueError(f"mirror_axes must be spatial axes out of 0 (H), 1 (W), 2 (D), got {tuple(mirror_axes)}")
    if len(set(axes)) != len(axes):
        raise ValueError(f"mirror_axes must be distinct, got {tuple(mirror_axes)}")
    mask = sum(1 << a for a in axes)
    return tuple(m for m in range(8) if m & ~mask == 0)


def tta_table(origins: np.ndarray, sub_batch: int, codes: Sequence[int]) -> np.ndarray:
    """The device work list under mirror augmentation: int32 [ceil(N F / sub_batch) * sub_batch, 4] =
    (o0, o1, o2, valid | code << 1), entry ``w * F + j`` = window ``w`` under ``codes[j]`` (window-major, flip-minor);
    padding entries are invalid.  ``codes == (0,)`` gives ``window_table(origins, sub_batch)``."""
    _check_sub_batch(sub_batch)
    codes = [int(m) for m in codes]
    if not codes or any(m < 0 or m > 7 for m in codes) or len(set(codes)) != len(codes):
        raise ValueError(f"codes must be distinct 3-bit flip masks, got {codes}")
    f = len(codes)
    n = origins.shape[0] * f
    total = -(-n // int(sub_batch)) * int(sub_batch)
    t = np.zeros((total, 4), dtype=np.int32)
    t[:n, :3] = np.repeat(origins, f, axis=0)
    t[:n, 3] = 1 + 2 * np.tile(np.asarray(codes, dtype=np.int32), origins.shape[0])
    return t


def importance_tables(roi: Sequence[int], mode: str = "gaussian", sigma_scale: float = 0.125):
    """The separable importance map as three 1-D float64 tables and the floor it is clamped at from below:
    w(i, j, k) = max(t0[i] * t1[j] * t2[k], floor).  ``"constant"``: all ones.  ``"gaussian"``:
    t_d(i) = exp(-(i - r_d // 2)^2 / (2 sigma_d^2)), sigma_d = sigma_scale * r_d, floor = max(min(map), 1e-3)."""
    r = _check_shape3("roi", roi)
    if mode == "constant":
        return [np.ones(n, dtype=np.float64) for n in r], 1.0
    if mode != "gaussian":
        raise ValueError(f"mode must be 'gaussian' or 'constant', got {mode!r}")
    if not float(sigma_scale) > 0:
        raise ValueError("sigma_scale must be > 0")
    tabs = []
    for n in r:
        sigma = float(sigma_scale) * n
        i = np.arange(n, dtype=np.float64)
        tabs.append(np.exp(-((i - n // 2) ** 2) / (2.0 * sigma * sigma)))
    floor = max(float(np.prod([t.min() for t in tabs])), 1e-3)
    return tabs, floor


class WindowSkip(ImmutableValue):
    """Which windows a ``SlidingWindowPredictor(skip=...)`` leaves out.  A voxel of the prepared volume is
    foreground iff ``vol[channel] > threshold`` (strict fp32: NaN is not foreground; the default threshold is the
    reference's ``LoadPseudoBgMaskd`` rule, transforms.py:363); a window is kept iff it holds at least ``min_voxels``
    foreground voxels.  Voxels no kept window covers get the label ``fill_class`` and the blended logits ``+fill_logit``
    at ``fill_class``, ``-fill_logit`` elsewhere.  ``channel`` and ``fill_class`` are checked against the predictor's
    channel and class counts when it is built.  Immutable."""

    __slots__ = ("threshold", "channel", "min_voxels", "fill_class", "fill_logit")

    def __init__(self, threshold: float = 0.0025, channel: int = 0, min_voxels: int = 1, fill_class: int = 0,
                 fill_logit: float = 10.0):
        check_finite("threshold", threshold)
        check_fill_logit(fill_logit)
        for name, v, lo in (("channel", channel, 0), ("min_voxels", min_voxels, 1), ("fill_class", fill_class, 0)):
            check_int_from(name, v, lo)
        self._set(threshold=float(threshold), channel=int(channel), min_voxels=int(min_voxels), fill_class=int(fill_class),
                  fill_logit=float(fill_logit))


class AutoForeground:
    """Foreground of a raw scan from its own histogram, for ``predict_scan(..., foreground=AutoForeground())`` on a
    predictor built with ``skip=`` or ``fit=``: the voxels of ``raw[channel]`` above the Otsu threshold of
    the scan's histogram (``mivp_amd.scanstats``; ``above``: count only voxels with a value greater than it, so that
    ``above=0`` on MR separates tissue from the dark rim) take the place of the rule's fixed threshold on the prepared
    volume, which means nothing for a z-scored scan.  A plain spec.  Like ``IntensityWindow`` it keeps the buffers its
    calls work in -- histogram, Otsu record, the mask on the native grid and the mask on the model grid -- one set per
    (device, channels, native shape, model grid), made at the first call, so **a spec serves one stream at a time**."""

    def __init__(self, channel: int = 0, above: Optional[int] = None):
        from . import scanstats
        check_int_from("channel", channel, 0)
        self.channel, self.above = int(channel), scanstats._check_above(above)
        self._buffers: Dict[tuple, tuple] = {}

    def buffers(self, channels: int, shape: Sequence[int], size: Sequence[int], device) -> tuple:
        """(ScanHistogram, OtsuSlot, uint8 ``shape`` native-grid mask, uint8 ``[1, 1] + size`` model-grid mask) for scans
        of ``channels`` channels and native ``shape`` on ``device``, predicted on the model grid ``size``."""
        from . import scanstats
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (str(dev), int(channels), tuple(int(n) for n in shape), tuple(int(n) for n in size))
        if key not in self._buffers:
            self._buffers[key] = (scanstats.ScanHistogram(channels, dev), scanstats.OtsuSlot(channels, dev),
                                  torch.zeros(key[2], dtype=torch.uint8, device=dev),
                                  torch.zeros((1, 1) + key[3], dtype=torch.uint8, device=dev))
        return self._buffers[key]

    def __repr__(self):
        return f"AutoForeground(channel={self.channel}, above={self.above})"


def _model_factor(conf) -> Tuple[int, int, int]:
    """Per-axis size multiple the SwinUnetR accepts: the patch embedding times the encoder's patch mergings (every stage
    halves H and W, only the first one D: swin_unetr.py merge_last_dim)."""
    depth = int(conf.depth_unet)
    ps = [int(a) for a in conf.input_patch_size]
    return ps[0] * 2 ** depth, ps[1] * 2 ** depth, ps[2] * 2 ** min(depth, 1)


class SlidingWindowPredictor(CenterlineEvaluation, GroupEvaluation):
    """Whole-volume sliding-window prediction of a ``downstream`` model on the GPU.

    For one image size it owns the window table, the device sub-batch index, the model's input batch, the blend
    accumulators and the Dice / IoU count table; ``predict`` / ``evaluate`` can be called for any number of volumes of
    that size.  Per sub-batch: one gather launch cuts the windows out of the volume into the input batch, the model runs,
    one blend launch adds ``w * logits`` and ``w`` into the accumulators (gather form, no float atomics: bitwise
    independent of ``sub_batch``), one launch advances the index.  One finalize launch writes the labels.

    ``mirror_axes`` (distinct axes out of 0 = H, 1 = W, 2 = D) turns on mirror test-time augmentation: every window is
    predicted under each of the ``2 ** len(mirror_axes)`` combinations of flips (``flip_codes``), the logits are flipped back
    and all of them take part in the same weighted mean (logits are averaged, not probabilities; the importance map is
    not flipped).  The work list is window-major, flip-minor (``tta_table``), its sub-batches are ``sub_batch`` consecutive
    entries, and every voxel still sums in increasing entry index (with compensated fp32 sums, whose state is kept per
    voxel between launches), so the result stays bitwise independent of ``sub_batch`` and of the graph form.

    ``graph=True`` records gather -> model -> blend -> advance once (after two eager sub-batches that pack the weight
    caches) and replays it ``ceil(N F / sub_batch)`` times with no host work in between: bitwise equal to eager.  The graph
    holds the model's weights as they were when it was recorded; build a new predictor after changing them.

    ``skip`` (a ``WindowSkip``; ``None``, the default, launches what the predictor always launched and reads nothing
    back) leaves the windows without foreground out.  Per volume: reset -> one occupancy launch (foreground voxels per
    window, ``self.occupancy``) -> one compact launch that writes the kept entries of the immutable full work list
    (``self.table_full``), in their original order, into ``self.table`` -- the buffer the gather, the blend and the
    recorded graph read -- and zeroes the rest -> ``ceil(n_kept F / sub_batch)`` sub-batches -> one fill launch (voxels no
    kept window covered get the fill logits) -> finalize.  The number of sub-batches is ONE 8-BYTE HOST READ of the
    compact launch's (kept windows, kept entries) word, the only synchronisation ``skip`` adds: without it the empty
    sub-batches would still run the model.  Entry order is preserved, so every voxel still sums in increasing entry
    index: the result stays bitwise independent of ``sub_batch`` and of the graph form, a voxel all of whose covering
    windows are kept (with ``min_voxels=1``: every foreground voxel) gets the logits of the unfiltered prediction bit
    for bit, and the graph is recorded once (with the full table) and replayed for every volume whatever its kept set.
    A compacted sub-batch can span any union box, so the blend is then ``mivp_window_blend_any``: the unfiltered launch
    grid, walked with a stride over a larger box (the same sums per voxel).  After a run
    ``n_kept`` is the number of windows kept and ``n_sub_run`` the number of sub-batches run.  ``set_region(mask)``
    replaces the threshold rule by a resident uint8 ``[H, W, D]`` mask (foreground: ``mask != 0``);
    ``predict_scan(..., foreground=AutoForeground())`` computes such a mask per scan from the raw scan's own Otsu
    threshold (for ``skip`` and ``fit`` alike).

    ``fit`` (a ``WindowFit``; ``None``, the default, launches what the predictor always launched and reads nothing back;
    not together with ``skip``) tiles the foreground's bounding box instead of the whole volume, so windows are removed
    where ``skip`` could only drop the ones that hold no foreground at all.  Per volume: reset -> the box
    (``foreground_box`` into ``self.box``; of ``mask != 0`` after ``set_region(mask)``) -> one plan launch that writes
    the fitted work list into ``self.table`` and its origins into ``self.fit_origins`` -> the one 8-byte host read of
    (windows, entries) -> ``ceil(entries / sub_batch)`` sub-batches -> the fill launch -> finalize.  Per axis on the
    padded volume (p = padded size, r = roi, m = margin, [lo, hi] the box): ``b0 = max(lo + pad - m, 0)``,
    ``b1 = min(hi + pad + m + 1, p)``, ``n = b1 - b0``; if ``n < r`` then ``b0 = clamp(b0 - (r - n) // 2, 0, p - r)`` and
    ``n = r``; ``count = ceil((n - r) / interval) + 1`` with ``window_origins``' interval, window i starts at
    ``b0 + min(i * interval, n - r)``.  ``n <= p``, so no axis has more windows than the full tiling: the table, the
    input batch, the accumulators and the graph (recorded once with the full table) are reused as built, and a box that
    is the whole volume gives the full tiling and the prediction without ``fit`` bit for bit.  After a run ``n_kept`` is
    the number of fitted windows and ``n_sub_run`` the number of sub-batches run."""

    def __init__(self, model, image_size: Sequence[int], in_channels: int, num_classes: int, roi: Sequence[int],
                 overlap: float = 0.5, mode: str = "gaussian", sigma_scale: float = 0.125, sub_batch: int = 10,
                 graph: bool = False, mirror_axes: Sequence[int] = (), skip: Optional[WindowSkip] = None, *,
                 fit: Optional[WindowFit] = None):
        """The class docstring describes the arguments; ``fit`` is keyword-only."""
        self.image_size = _check_shape3("image_size", image_size)
        self.roi = _check_shape3("roi", roi)
        _check_overlap(overlap)
        self.flip_codes = flip_codes(mirror_axes)
        self.mirror_axes = tuple(int(a) for a in mirror_axes)
        self.n_flips = len(self.flip_codes)
        _check_sub_batch(sub_batch)
        if not 1 <= int(in_channels) <= 4:
            raise ValueError("in_channels must be in 1..4")
        check_classes(num_classes)
        for name, rule, cls in (("skip", skip, WindowSkip), ("fit", fit, WindowFit)):
            if rule is None:
                continue
            if not isinstance(rule, cls):
                raise ValueError(f"{name} must be a {cls.__name__} or None, got {type(rule).__name__}")
            if name == "fit" and skip is not None:
                raise ValueError("fit and skip cannot be combined: build the predictor with one of them")
            if rule.channel >= int(in_channels):
                raise ValueError(f"{name}.channel {rule.channel} is not a channel of a {int(in_channels)}-channel volume")
            if rule.fill_class >= int(num_classes):
                raise ValueError(f"{name}.fill_class {rule.fill_class} is not one of {int(num_classes)} classes")
        # the active selection rule, if any: it writes the volume's work list into self.table, then one 8-byte read
        self.skip, self.fit, self._rule = skip, fit, skip if skip is not None else fit
        conf = getattr(model, "conf", None)
        if conf is not None:
            if getattr(conf, "training_mode", "downstream") != "downstream":
                raise ValueError("SlidingWindowPredictor needs a 'downstream' model (its output is out['downstream'])")
            if int(conf.input_channels) != int(in_channels):
                raise ValueError(f"in_channels {in_channels} does not match the model's input_channels {conf.input_channels}")
            if int(conf.output_channels_downstream) != int(num_classes):
                raise ValueError(f"num_classes {num_classes} does not match the model's output_channels_downstream "
                                 f"{conf.output_channels_downstream}")
            f = _model_factor(conf)
            if any(r % m for r, m in zip(self.roi, f)):
                raise ValueError(f"roi {self.roi} is not a multiple of {f}, the input size multiple of this model")
        dev = next(iter(model.parameters()), None)
        dev = dev.device if dev is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise RuntimeError("SlidingWindowPredictor runs on the GPU: move the model to the device (no CPU fallback)")
        self.model, self.dev = model, dev
        self.cin, self.ncls = int(in_channels), int(num_classes)
        self.sub_batch, self.graph_mode = int(sub_batch), bool(graph)
        self.overlap, self.mode = float(overlap), mode
        self.pad, self.pdims = window_padding(self.image_size, self.roi)
        self.origins = window_origins(self.image_size, self.roi, overlap)
        self.n_windows = int(self.origins.shape[0])
        self.n_entries = self.n_windows * self.n_flips
        table = tta_table(self.origins, self.sub_batch, self.flip_codes)
        self.n_sub = table.shape[0] // self.sub_batch
        # the flip-aware kernels run when there is a flip; a plain predictor keeps the plain entry points
        self._tta_kernels = self.n_flips > 1
        # grid of the blend: the largest union box of one sub-batch's entries (the flips of a window share its box)
        ubox = [0, 0, 0]
        for s in range(self.n_sub):
            o = table[s * self.sub_batch:min((s + 1) * self.sub_batch, self.n_entries), :3]
            for a in range(3):
                ubox[a] = max(ubox[a], int(o[:, a].max() - o[:, a].min()) + self.roi[a])
        # (with skip a compacted sub-batch can have any union box: the grid stays this one, mivp_window_blend_any strides)
        self.ubox = tuple(ubox)
        tabs, self.w_floor = importance_tables(self.roi, mode, sigma_scale)
        self.w = [torch.tensor(t, dtype=torch.float32, device=dev) for t in tabs]
        self.table = torch.from_numpy(table).to(dev)
        self.sub_idx = torch.zeros(1, dtype=torch.int32, device=dev)
        self.xb = torch.zeros((self.sub_batch, self.cin) + self.roi, dtype=torch.float32, device=dev)
        self.acc = torch.zeros(self.pdims + (self.ncls,), dtype=torch.float32, device=dev)
        self.wsum = torch.zeros(self.pdims, dtype=torch.float32, device=dev)
        self.counts = torch.zeros((self.ncls, 3), dtype=torch.int64, device=dev)
        # under augmentation a voxel adds F times as many contributions: the blend then carries the rounding error of acc
        # and wsum along (compensated sums, in the same order), so that they round like the plain prediction's
        self.comp = (torch.zeros(self.pdims + (self.ncls + 1,), dtype=torch.float32, device=dev)
                     if self.n_flips > 1 else None)
        self._a = dict(dims=i3(self.image_size), pad=i3(self.pad), pdims=i3(self.pdims), roi=i3(self.roi),
                       ubox=i3(self.ubox))
        self.vol = None          # graph mode: the resident volume the recorded gather reads
        self.graph = None
        self.cc_ws = None        # post-processing workspace (8 bytes per voxel), allocated on first use
        # window skipping: the full work list stays as built; self.table is the active (compacted) list of the volume
        self.occupancy, self.region = None, None
        self._auto_mask = None   # graph mode: the model-grid mask predict_scan(foreground=...) writes
        self.n_kept, self.n_sub_run = self.n_windows, self.n_sub
        self.box = None
        if self._rule is not None:
            self.table_full = self.table.clone()
            self.meta = torch.zeros(2, dtype=torch.int32, device=dev)
        if fit is not None:
            # the fitted tiling never has more windows per axis than the full one: table, xb, accumulators, graph as built
            self.box = torch.zeros(6, dtype=torch.int32, device=dev)
            self.fit_origins = torch.zeros((self.n_windows, 3), dtype=torch.int32, device=dev)
            self._fit_args = (i3(_fit_intervals(self.roi, overlap)), i3([min(m, 2 ** 30) for m in fit.margin]),
                              (C.c_int32 * self.n_flips)(*self.flip_codes))
        if skip is not None:
            self.origins_dev = torch.from_numpy(np.ascontiguousarray(self.origins)).to(dev)
            self.occupancy = torch.zeros(self.n_windows, dtype=torch.int32, device=dev)

    # ------------------------------------------------------------------ per sub-batch launches
    def _gather(self, vol):
        a = self._a
        L.call("mivp_window_gather_tta" if self._tta_kernels else "mivp_window_gather", L.ptr(vol), self.cin, a["dims"],
               a["pad"], a["pdims"], a["roi"], L.ptr(self.table), self.table.shape[0], L.ptr(self.sub_idx), self.sub_batch,
               L.ptr(self.xb), L.stream())

    def _blend(self, out):
        if tuple(out.shape) != (self.sub_batch, self.ncls) + self.roi:
            raise ValueError(f"the model returned {tuple(out.shape)}, expected {(self.sub_batch, self.ncls) + self.roi}")
        src, clast = channels_last_or_copy(out)
        a = self._a
        args = (L.ptr(src), clast, self.ncls, a["pdims"], a["roi"], L.ptr(self.table), self.table.shape[0],
                L.ptr(self.sub_idx), self.sub_batch, a["ubox"], L.ptr(self.w[0]), L.ptr(self.w[1]), L.ptr(self.w[2]),
                self.w_floor, L.ptr(self.acc), L.ptr(self.wsum))
        if self._rule is not None:                               # any union box on the unfiltered grid (comp None: plain sums)
            L.call("mivp_window_blend_any", *args, L.ptr(self.comp), L.stream())
        elif self._tta_kernels:
            L.call("mivp_window_blend_tta", *args, L.ptr(self.comp), L.stream())
        else:
            L.call("mivp_window_blend", *args, L.stream())

    def _step(self, vol):
        self._gather(vol)
        out = self.model(self.xb)["downstream"]
        self._blend(out)
        L.call("mivp_window_advance", L.ptr(self.sub_idx), L.stream())
        return out

    def _reset(self):
        self.acc.zero_()
        self.wsum.zero_()
        if self.comp is not None:
            self.comp.zero_()
        self.sub_idx.zero_()

    # ------------------------------------------------------------------ window skipping (csrc/window_skip.hip)
    def set_region(self, mask: Optional[torch.Tensor]):
        """While a resident uint8 ``[H, W, D]`` GPU tensor is set, foreground means ``mask != 0`` (a body or lung mask
        from ``mivp_amd.components``) and the threshold is ignored; ``None`` returns to the threshold rule.  The tensor
        is read at every run, not copied."""
        if self._rule is None:
            raise ValueError("set_region needs a predictor built with skip=WindowSkip(...)")
        if mask is not None:
            check_region_mask(mask, self.image_size, self.dev)
        self.region = mask

    def _select(self, vol):
        """occupancy -> compact into ``self.table``; no host read."""
        a, k = self._a, self.skip
        src = (L.ptr(vol), self.cin, k.channel, k.threshold, None) if self.region is None else \
            (None, 0, 0, 0.0, L.ptr(self.region))
        L.call("mivp_window_occupancy", *src, a["dims"], a["pad"], a["pdims"], a["roi"], L.ptr(self.origins_dev), 3,
               self.n_windows, L.ptr(self.occupancy), L.stream())
        L.call("mivp_window_compact", L.ptr(self.table_full), self.table.shape[0], self.n_windows, self.n_flips,
               L.ptr(self.occupancy), k.min_voxels, L.ptr(self.table), L.ptr(self.meta), L.stream())

    def _plan(self, vol):
        """box -> the fitted work list into ``self.table`` (csrc/window_fit.hip); no host read."""
        a, k = self._a, self.fit
        src = self.region if self.region is not None else vol
        foreground_box(src, k.channel, k.threshold, out=self.box)
        step, margin, codes = self._fit_args
        L.call("mivp_window_fit_plan", L.ptr(self.box), a["dims"], a["pad"], a["pdims"], a["roi"], step, margin, codes,
               self.n_flips, L.ptr(self.table), self.table.shape[0], L.ptr(self.fit_origins), self.n_windows, L.ptr(self.meta),
               L.stream())

    def _kept(self) -> int:
        """The one host read of a skipping or fitting run: (windows, entries) of the volume's work list -> the number of
        sub-batches to run."""
        kept_windows, kept_entries = self.meta.tolist()
        if kept_entries < 0:
            raise RuntimeError("mivp_amd: the fitted tiling does not fit the predictor's work list")
        self.n_kept = int(kept_windows)
        self.n_sub_run = min(-(-int(kept_entries) // self.sub_batch), self.n_sub)
        return self.n_sub_run

    def _fill(self):
        k = self._rule
        L.call("mivp_stitch_fill", L.ptr(self.acc), L.ptr(self.wsum), self.ncls, self._a["pdims"], k.fill_class, k.fill_logit,
               L.stream())

    def _record(self):
        """Warm up two sub-batches eagerly on a side stream, then record one sub-batch step."""
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._reset()
            for _ in range(min(2, self.n_sub)):
                self._step(self.vol)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._out = self._step(self.vol)

    # ------------------------------------------------------------------ whole volume
    def _check_input(self, x, name="x", channels=None):
        check_gpu(name, x)
        if x.dim() != 5 or x.shape[0] != 1:
            raise ValueError(f"{name} must be [1, C, H, W, D] (one volume at a time), got {tuple(x.shape)}")
        ch = self.cin if channels is None else channels
        if tuple(x.shape[1:]) != (ch,) + self.image_size:
            raise ValueError(f"{name} has shape {tuple(x.shape)}, the predictor was built for {(1, ch) + self.image_size}")
        if x.device != self.dev:
            raise ValueError(f"{name} is on {x.device}, the model on {self.dev}")

    @torch.no_grad()
    def _run(self, x, want_logits, seg, post=None, maps=()):
        """-> (labels, logits or None, {name: map} for the names in ``maps`` out of probs / confidence / entropy)."""
        self._check_input(x)
        if self.graph_mode and self.model.training:
            raise RuntimeError("graph=True needs the model in eval() mode")
        vol = x.float().contiguous()
        if self.graph_mode:
            if self.vol is None:
                self.vol = torch.empty_like(vol)
            if vol.data_ptr() != self.vol.data_ptr():            # predict_scan prepares straight into the resident volume
                self.vol.copy_(vol)
            if self.graph is None:
                if self._rule is not None:                       # warm up and record with the full work list
                    self.table.copy_(self.table_full)
                self._record()
            vol = self.vol                                       # what the launches below and the recorded gather read
        self._reset()
        n_sub = self.n_sub
        if self._rule is not None:
            (self._select if self.skip is not None else self._plan)(vol)
            n_sub = self._kept()
        if self.graph_mode:
            for _ in range(n_sub):
                self.graph.replay()
        else:
            for _ in range(n_sub):
                self._step(vol)
        if self._rule is not None:
            self._fill()
        labels = torch.empty((1, 1) + self.image_size, dtype=torch.uint8, device=self.dev)
        logits = torch.empty((1, self.ncls) + self.image_size, dtype=torch.float32, device=self.dev) if want_logits else None
        tgt = None
        if seg is not None:
            tgt = seg.float().contiguous()
            self.counts.zero_()
        a = self._a
        counts = self.counts if seg is not None else None
        extra = {k: torch.empty((1, self.ncls if k == "probs" else 1) + self.image_size, dtype=torch.float32,
                                device=self.dev) for k in maps}
        # the post-processing rewrites the labels in place; its filter pass, not the finalize, counts them against seg
        f_tgt, f_counts = (tgt, counts) if post is None else (None, None)
        # a call that asks for no maps keeps the plain finalize; the probability one takes the three maps in the middle
        if extra:
            L.call("mivp_stitch_finalize_probs", L.ptr(self.acc), L.ptr(self.wsum), self.ncls, a["dims"], a["pad"], a["pdims"],
                   L.ptr(labels), L.ptr(logits), L.ptr(extra.get("probs")), L.ptr(extra.get("confidence")),
                   L.ptr(extra.get("entropy")), L.ptr(f_tgt), L.ptr(f_counts), L.stream())
        else:
            L.call("mivp_stitch_finalize", L.ptr(self.acc), L.ptr(self.wsum), self.ncls, a["dims"], a["pad"], a["pdims"],
                   L.ptr(labels), L.ptr(logits), L.ptr(f_tgt), L.ptr(f_counts), L.stream())
        if post is not None:
            from . import components
            lab = labels[0, 0]
            self.cc_ws = components._postprocess_launch(lab, lab, post, self.cc_ws,
                                                        tgt[0, 0] if tgt is not None else None, counts)
        return labels, logits, extra

    def _post(self, postprocess):
        from . import components
        return components.postprocess_kwargs(postprocess, self.ncls)

    def predict(self, x: torch.Tensor, return_logits: bool = False, postprocess: Optional[Dict] = None,
                return_probs: bool = False, return_confidence: bool = False,
                return_entropy: bool = False) -> Dict[str, torch.Tensor]:
        """``x [1, Cin, H, W, D]`` -> ``{"labels": uint8 [1, 1, H, W, D]}`` (+ ``"logits"``: the blended fp32 logits
        ``[1, C, H, W, D]``).  ``postprocess``: a dict of ``mivp_amd.components.postprocess_labels`` keyword arguments
        (``largest``, ``min_size``, ``classes``, ``connectivity``) applied to the labels on the device; ``"logits"``
        stays the blend before post-processing.  On request, from the same finalize launch and like ``"logits"`` of the
        blend before post-processing: ``"probs"`` fp32 ``[1, C, H, W, D]``, the softmax of the blended logits over the
        classes; ``"confidence"`` fp32 ``[1, 1, H, W, D]``, the maximum probability; ``"entropy"`` fp32
        ``[1, 1, H, W, D]``, ``-sum p ln p / ln C`` in [0, 1] (0 for one class)."""
        post = self._post(postprocess)
        maps = [k for k, on in (("probs", return_probs), ("confidence", return_confidence), ("entropy", return_entropy))
                if on]
        labels, logits, extra = self._run(x, return_logits, None, post, maps)
        out = {"labels": labels}
        if return_logits:
            out["logits"] = logits
        out.update(extra)
        return out

    def predict_regions(self, x: torch.Tensor, return_logits: bool = False, postprocess: Optional[Dict] = None,
                        return_probs: bool = False, return_confidence: bool = False, return_entropy: bool = False,
                        spacing: Sequence[float] = (1.0, 1.0, 1.0), **region_kwargs) -> Dict[str, object]:
        """``predict(x, ...)`` plus ``"regions"``: the ``mivp_amd.regions.RegionTable`` of the returned labels
        (``region_kwargs``: ``connectivity``, ``classes``, ``max_regions`` of ``region_stats``), with the confidence map
        as its image when ``return_confidence`` is set (``vmean`` is then the mean confidence per lesion).  No host read."""
        from . import regions
        regions.check_region_kwargs(self.ncls, spacing, **region_kwargs)
        out = self.predict(x, return_logits, postprocess, return_probs, return_confidence, return_entropy)
        out["regions"] = regions.region_stats(out["labels"], self.ncls, image=out.get("confidence"), spacing=spacing,
                                              **region_kwargs)
        return out

    def evaluate_lesions(self, x: torch.Tensor, seg: torch.Tensor, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                         postprocess: Optional[Dict] = None, with_scores: bool = False, **lesion_kwargs):
        """Lesion-wise detection metrics of the whole-volume prediction against ``seg [1, 1, H, W, D]``: the
        ``mivp_amd.regions.LesionReport`` of ``lesion_metrics(predict(x, postprocess=postprocess)["labels"], seg,
        num_classes, spacing, **lesion_kwargs)`` (``connectivity``, ``iou_threshold``, ``min_size``, ``classes``,
        ``max_regions``, ``max_pairs``).  ``with_scores``: the prediction also writes its confidence map and the report is
        built with it as ``pred_image`` (lesion scores, ``froc()``).  Prediction, post-processing and the metrics run with
        no host read in between; ``LesionReport.cpu()`` synchronises."""
        from . import regions
        post = self._post(postprocess)
        self._check_input(seg, "seg", channels=1)
        regions.check_lesion_kwargs(self.ncls, spacing, **lesion_kwargs)
        if not with_scores:
            labels, _, _ = self._run(x, False, None, post)
            return regions.lesion_metrics(labels, seg, self.ncls, spacing, **lesion_kwargs)
        labels, _, extra = self._run(x, False, None, post, ["confidence"])
        return regions.lesion_score_metrics(labels, seg, self.ncls, extra["confidence"], spacing, **lesion_kwargs)

    def evaluate_calibration(self, x: torch.Tensor, seg: torch.Tensor, n_bins: int = 15, out=None):
        """Calibration and threshold-sweep tables of the whole-volume prediction against ``seg [1, 1, H, W, D]``: the
        ``mivp_amd.calibration.CalibrationReport`` of ``calibration_tables(predict(x, return_probs=True)["probs"], seg,
        num_classes, n_bins, out)``.  ``out``: an earlier report to pool into.  No host read;
        ``CalibrationReport.cpu()`` synchronises."""
        from . import calibration
        self._check_input(seg, "seg", channels=1)
        shape = (1, self.ncls) + self.image_size
        calibration._check_calibration_args(torch.empty(shape, dtype=torch.float32, device="meta"), seg, self.ncls, n_bins,
                                            out)
        _, _, extra = self._run(x, False, None, None, ["probs"])
        return calibration.calibration_tables(extra["probs"], seg, self.ncls, n_bins, out)

    def evaluate(self, x: torch.Tensor, seg: torch.Tensor, postprocess: Optional[Dict] = None) -> Tuple[float, float]:
        """(mean IoU, mean Dice) of the whole-volume prediction against ``seg [1, 1, H, W, D]`` (class indices), with the
        formulas of ``SegMetrics.compute``; the per-class counts stay in ``self.counts``.  One host read.  With
        ``postprocess`` (as in ``predict``) the counts are those of the post-processed labels."""
        post = self._post(postprocess)
        self._check_input(seg, "seg", channels=1)
        self._run(x, False, seg, post)
        return iou_dice(self.counts)

    def evaluate_surface(self, x: torch.Tensor, seg: torch.Tensor, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                         percentile: float = 95.0, tolerance: float = 1.0, include_background: bool = False,
                         postprocess: Optional[Dict] = None) -> Dict[str, object]:
        """Surface-distance metrics of the whole-volume prediction against ``seg [1, 1, H, W, D]``: the dict of
        ``mivp_amd.surface.surface_metrics(predict(x)["labels"], seg, ...)`` plus ``"iou"`` / ``"dice"``, the values
        ``evaluate`` returns, from the same finalize launch.  One host read for all of them.  With ``postprocess`` (as in
        ``predict``) every value describes the post-processed labels."""
        from . import surface as S
        post = self._post(postprocess)
        self._check_input(seg, "seg", channels=1)
        ncls, sp, pc, tol = S._check_metric_args(self.ncls, spacing, percentile, tolerance)
        labels, _, _ = self._run(x, False, seg, post)
        scount, recs = S._metrics_launch(labels, seg, ncls, sp, pc, tol, include_background)
        host = torch.cat([self.counts.reshape(-1), scount.reshape(-1), recs.reshape(-1)]).cpu()
        rest = host[3 * ncls:].numpy()
        out = S._metrics_finish(rest[:2 * ncls].reshape(ncls, 2), rest[2 * ncls:].reshape(ncls, 2, S._REC), ncls, pc,
                                include_background)
        out["iou"], out["dice"] = iou_dice(host[:3 * ncls].reshape(ncls, 3))
        return out

    # ------------------------------------------------------------------ raw scans (mivp_amd.scan)
    def _prepare_scan(self, raw, geom, restore, postprocess, intensity):
        """Checked raw scan -> the model's input on the device: the predictor's resident volume in graph mode, so that the
        recorded gather reads what the prepare launch wrote (with ``window=`` the histogram and plan launches run eagerly
        in front of it, like the prepare launch itself)."""
        from . import scan
        unknown = set(intensity) - {"a_min", "a_max", "b_min", "b_max", "clip", "window", "mask", "antialias"}
        if unknown:
            raise ValueError(f"unknown intensity arguments {sorted(unknown)}")
        r = scan.check_predict_args(self.image_size, self.cin, raw, geom, restore, postprocess)
        intensity = dict(intensity)
        if check_flag("antialias", intensity.pop("antialias", False)):
            intensity["flags"] = scan.FLAG_ANTIALIAS
        out = None
        if self.graph_mode and isinstance(r, torch.Tensor) and r.is_cuda:
            if self.vol is None:
                self.vol = torch.empty((1, self.cin) + self.image_size, dtype=torch.float32, device=self.dev)
            out = self.vol
        return scan.prepare_scan(r, geom, out=out, **intensity)

    def _check_foreground(self, foreground, raw, geom):
        """The host-side checks of ``foreground=`` (no device work)."""
        from . import scan, scanstats
        if foreground is None:
            return
        if self._rule is None:
            raise ValueError("foreground= needs a predictor built with skip=WindowSkip(...) or fit=WindowFit(...)")
        if not isinstance(foreground, AutoForeground):
            raise ValueError(f"foreground must be an AutoForeground or None, got {type(foreground).__name__}")
        if foreground.channel >= self.cin:
            raise ValueError(f"foreground.channel {foreground.channel} is not a channel of a {self.cin}-channel scan")
        r = scan._raw_view(raw, scan._check_geom(geom))
        if r.dtype not in scanstats._DTYPES:
            raise ValueError(f"foreground= takes int16 or uint8 scans, got {r.dtype}")

    def _auto_region(self, foreground: AutoForeground, raw, geom) -> torch.Tensor:
        """histogram -> Otsu plan -> mask on the native grid -> nearest to the model grid: four launches on the current
        stream, no host read.  In graph mode the model-grid mask is the predictor's own buffer."""
        from . import scan, scanstats
        r = scan._raw_view(raw, geom)
        hist, otsu, native, region = foreground.buffers(r.shape[0], geom.shape, self.image_size, r.device)
        if self.graph_mode:
            if self._auto_mask is None:
                self._auto_mask = torch.zeros((1, 1) + self.image_size, dtype=torch.uint8, device=self.dev)
            region = self._auto_mask
        scanstats.scan_histogram(r, above=foreground.above, out=hist.zero_())
        scanstats.otsu_slot(hist, out=otsu)
        scanstats.foreground_mask(r, otsu, foreground.channel, out=native)
        return scan.prepare_labels(native, geom, out=region, check=False)[0, 0]

    def _with_foreground(self, foreground, raw, geom, run):
        """``run()`` with the region of ``foreground`` (if given) in place of the one ``set_region`` holds."""
        if foreground is None:
            return run()
        held = self.region
        self.region = self._auto_region(foreground, raw, geom)
        try:
            return run()
        finally:
            self.region = held

    def predict_scan(self, raw: torch.Tensor, geom, restore: str = "labels", postprocess: Optional[Dict] = None,
                     **intensity) -> Dict[str, torch.Tensor]:
        """A raw scan on its native grid (``[C, H, W, D]`` int16 / uint8 / int32 / float32, ``geom`` a
        ``mivp_amd.scan.ScanGeometry`` whose model grid is this predictor's image size) -> ``{"labels": uint8
        [H, W, D]`` on the native grid, ``"labels_oriented"``: uint8 ``[1, 1, H', W', D']`` on the model grid``}``:
        ``prepare_scan`` -> the sliding-window prediction -> optional post-processing on the model grid -> restore, with
        no host read.  ``restore="labels"`` resizes the label map back (nearest); ``restore="logits"`` interpolates the
        blended logits on the native grid and takes the arg-max there (``restore_labels_from_logits``).  ``intensity``:
        ``a_min``, ``a_max``, ``b_min``, ``b_max``, ``clip``, ``antialias`` of ``prepare_scan``, or its ``window`` (and ``mask``): a
        data-driven window (``mivp_amd.scanstats``) adds two launches in front of the prepare launch and no host read,
        in graph mode too, where the prepare launch writes the predictor's resident volume as before.

        ``foreground`` (one more keyword of ``intensity``: an ``AutoForeground``, on a predictor built with ``skip=`` or
        ``fit=``; int16 / uint8 scans): for this call foreground is where the raw scan lies above its own Otsu threshold, in place of the
        rule's threshold on the prepared volume.  Histogram -> Otsu plan -> ``foreground_mask`` -> ``prepare_labels``
        (nearest, to the model grid) run in front of the occupancy / box launch with no host read, and the result equals
        ``set_region(prepare_labels(foreground_mask(...))[0, 0])`` followed by ``predict_scan`` bit for bit.  A region
        set with ``set_region`` is kept and holds again afterwards."""
        from . import scan
        post = self._post(postprocess)
        foreground = intensity.pop("foreground", None)
        self._check_foreground(foreground, raw, geom)
        x = self._prepare_scan(raw, geom, restore, postprocess, intensity)
        labels, logits, _ = self._with_foreground(foreground, raw, geom,
                                                  lambda: self._run(x, restore == "logits", None, post))
        native = scan.restore_labels(labels, geom) if restore == "labels" else scan.restore_labels_from_logits(logits, geom)
        return {"labels": native, "labels_oriented": labels}

    def evaluate_scan(self, raw: torch.Tensor, seg_native: torch.Tensor, geom, postprocess: Optional[Dict] = None,
                      **intensity) -> Tuple[float, float]:
        """``evaluate`` for a raw scan and a ground truth stored on the scan's native grid: ``prepare_labels`` takes the
        ground truth to the model grid and the scoring happens there, on the grid the model saw (as the reference's
        ``test()`` does).  Returns (mean IoU, mean Dice).  ``intensity`` as in ``predict_scan``, its ``foreground`` included."""
        from . import scan
        self._post(postprocess)
        foreground = intensity.pop("foreground", None)
        self._check_foreground(foreground, raw, geom)
        x = self._prepare_scan(raw, geom, "labels", postprocess, intensity)
        seg = scan.prepare_labels(seg_native, geom)
        return self._with_foreground(foreground, raw, geom, lambda: self.evaluate(x, seg, postprocess))


def _one_shot(model, x_or_shape, cin, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph, mirror_axes, skip,
              fit=None):
    """The predictor behind a one-shot wrapper: built for the volume ``x [1, Cin, H, W, D]`` (``cin`` None), or for an
    image size and its ``cin``."""
    if cin is None:
        if not isinstance(x_or_shape, torch.Tensor) or x_or_shape.dim() != 5:
            raise ValueError("x must be a [1, C, H, W, D] tensor")
        x_or_shape, cin = x_or_shape.shape[2:], x_or_shape.shape[1]
    return SlidingWindowPredictor(model, x_or_shape, cin, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph,
                                  mirror_axes, skip, fit=fit)


def predict_scan_volume(model, raw: torch.Tensor, affine, roi: Sequence[int], num_classes: int, out_size=None,
                        axcodes: str = "RAS", overlap: float = 0.5, mode: str = "gaussian", sigma_scale: float = 0.125,
                        sub_batch: int = 10, graph: bool = False, restore: str = "labels",
                        postprocess: Optional[Dict] = None, mirror_axes: Sequence[int] = (),
                        skip: Optional[WindowSkip] = None, *, fit: Optional[WindowFit] = None,
                        **intensity) -> Dict[str, torch.Tensor]:
    """One-shot ``SlidingWindowPredictor(...).predict_scan(raw, geom, restore, postprocess, **intensity)`` with
    ``geom = ScanGeometry.from_affine(raw's spatial shape, affine, axcodes, out_size, out_spacing)``; also returns
    ``"geometry"``.  Keyword-only ``fit``: the predictor's ``fit=``.  ``intensity`` may carry ``predict_scan``'s
    ``foreground=`` and ``antialias=``, and ``out_spacing=``: the model grid from a target spacing in place of ``out_size``."""
    from . import scan
    if not isinstance(raw, torch.Tensor) or raw.dim() not in (3, 4, 5):
        raise ValueError("raw must be a [C, H, W, D] (or [H, W, D] / [1, C, H, W, D]) tensor")
    geom = scan.ScanGeometry.from_affine(tuple(raw.shape[-3:]), affine, axcodes, out_size,
                                         intensity.pop("out_spacing", None))
    cin = 1 if raw.dim() == 3 else int(raw.shape[-4])
    out = _one_shot(model, geom.size, cin, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph, mirror_axes,
                    skip, fit).predict_scan(raw, geom, restore, postprocess, **intensity)
    out["geometry"] = geom
    return out


def predict_volume(model, x: torch.Tensor, roi: Sequence[int], num_classes: int, overlap: float = 0.5,
                   mode: str = "gaussian", sigma_scale: float = 0.125, sub_batch: int = 10, graph: bool = False,
                   return_logits: bool = False, postprocess: Optional[Dict] = None, mirror_axes: Sequence[int] = (),
                   return_probs: bool = False, return_confidence: bool = False,
                   return_entropy: bool = False, skip: Optional[WindowSkip] = None, *,
                   fit: Optional[WindowFit] = None) -> Dict[str, torch.Tensor]:
    """One-shot ``SlidingWindowPredictor(..., mirror_axes=mirror_axes, skip=skip).predict(x, return_logits, postprocess, ...)`` for
    ``x [1, Cin, H, W, D]``.
    Keyword-only ``fit``: the predictor's ``fit=``."""
    return _one_shot(model, x, None, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph, mirror_axes,
                     skip, fit).predict(x, return_logits, postprocess, return_probs, return_confidence, return_entropy)


def evaluate_volume(model, x: torch.Tensor, seg: torch.Tensor, roi: Sequence[int], num_classes: int, overlap: float = 0.5,
                    mode: str = "gaussian", sigma_scale: float = 0.125, sub_batch: int = 10,
                    graph: bool = False, postprocess: Optional[Dict] = None,
                    mirror_axes: Sequence[int] = (), skip: Optional[WindowSkip] = None, *,
                    fit: Optional[WindowFit] = None) -> Tuple[float, float]:
    """One-shot ``SlidingWindowPredictor(...).evaluate(x, seg, postprocess)``: whole-volume (mean IoU, mean Dice).
    Keyword-only ``fit``: the predictor's ``fit=``."""
    return _one_shot(model, x, None, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph, mirror_axes,
                     skip, fit).evaluate(x, seg, postprocess)


def evaluate_volume_surface(model, x: torch.Tensor, seg: torch.Tensor, roi: Sequence[int], num_classes: int,
                            overlap: float = 0.5, mode: str = "gaussian", sigma_scale: float = 0.125, sub_batch: int = 10,
                            graph: bool = False, spacing: Sequence[float] = (1.0, 1.0, 1.0), percentile: float = 95.0,
                            tolerance: float = 1.0, include_background: bool = False,
                            postprocess: Optional[Dict] = None, mirror_axes: Sequence[int] = (),
                            skip: Optional[WindowSkip] = None, *, fit: Optional[WindowFit] = None) -> Dict[str, object]:
    """One-shot ``SlidingWindowPredictor(...).evaluate_surface(x, seg, ...)``: whole-volume surface metrics + IoU / Dice.
    Keyword-only ``fit``: the predictor's ``fit=``."""
    return _one_shot(model, x, None, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph, mirror_axes,
                     skip, fit).evaluate_surface(x, seg, spacing, percentile, tolerance, include_background, postprocess)


def evaluate_volume_lesions(model, x: torch.Tensor, seg: torch.Tensor, roi: Sequence[int], num_classes: int,
                            overlap: float = 0.5, mode: str = "gaussian", sigma_scale: float = 0.125, sub_batch: int = 10,
                            graph: bool = False, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                            postprocess: Optional[Dict] = None, mirror_axes: Sequence[int] = (),
                            with_scores: bool = False, skip: Optional[WindowSkip] = None, *,
                            fit: Optional[WindowFit] = None, **lesion_kwargs):
    """One-shot ``SlidingWindowPredictor(...).evaluate_lesions(x, seg, spacing, postprocess, with_scores,
    **lesion_kwargs)``: the lesion-wise ``mivp_amd.regions.LesionReport`` of the whole-volume prediction.
    Keyword-only ``fit``: the predictor's ``fit=``."""
    return _one_shot(model, x, None, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph, mirror_axes,
                     skip, fit).evaluate_lesions(x, seg, spacing, postprocess, with_scores, **lesion_kwargs)


def evaluate_volume_calibration(model, x: torch.Tensor, seg: torch.Tensor, roi: Sequence[int], num_classes: int,
                                overlap: float = 0.5, mode: str = "gaussian", sigma_scale: float = 0.125,
                                sub_batch: int = 10, graph: bool = False, mirror_axes: Sequence[int] = (),
                                n_bins: int = 15, out=None, skip: Optional[WindowSkip] = None, *,
                                fit: Optional[WindowFit] = None):
    """One-shot ``SlidingWindowPredictor(...).evaluate_calibration(x, seg, n_bins, out)``: the
    ``mivp_amd.calibration.CalibrationReport`` of the whole-volume prediction.
    Keyword-only ``fit``: the predictor's ``fit=``."""
    return _one_shot(model, x, None, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph, mirror_axes,
                     skip, fit).evaluate_calibration(x, seg, n_bins, out)
