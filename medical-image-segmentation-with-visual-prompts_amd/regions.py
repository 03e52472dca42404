"""Per-lesion region statistics and lesion-wise detection metrics on the GPU (csrc/regions.hip).

Definitions (written out, as in ``mivp_amd.components``; ``tests/regions_ref.py`` restates them in numpy / scipy):

- **Layout.**  Class maps are ``[1, 1, H, W, D]`` or ``[H, W, D]`` GPU tensors, uint8, int32, int64, float32 or bool, with
  the layout and class rules of ``mivp_amd.components`` (a value outside ``[0, C)`` or a non-integer float belongs to no
  class).  ``image`` has the same spatial shape and is int16, uint8, int32 or float32 (finite values).
- **Regions.**  The voxels whose class is in ``classes`` (default ``1..C-1``) are labelled per class value with the
  adjacency rule and numbering of ``components.label_components``: 1..n in the raster order of each region's first voxel,
  over all listed classes together.  Regions of other classes are not listed and take no number.
- **RegionTable.**  Device tensors of ``max_regions`` entries, entry ``r`` describing the region labelled ``r + 1``:
  ``cls`` int32, ``size`` int64 (voxels), ``first`` int64 (linear index of the first voxel), ``bbox`` int32 ``[6]`` (minimum
  h, w, d then maximum h, w, d, inclusive), ``coord_sum`` int64 ``[3]``; with an image ``vmin`` / ``vmax`` (int32, or
  float32 for a float image) and ``vsum`` / ``vsqsum`` (int64, or float64 for a float image; the int64 sums are exact
  while they fit: only the squares of an int32 image with values beyond about 2^31 / sqrt(voxels) can wrap).  ``n`` (device int32) is the
  number of regions, ``overflow`` (device int32) says that it exceeds ``max_regions``; ``labels`` is the dense int32 label
  map.  Derived values are properties computed with torch in float64 from the integer fields: ``volume_mm3`` = size *
  prod(spacing); ``centroid`` = coord_sum / size; ``centroid_mm`` = centroid * spacing; ``extent`` = bbox max - min + 1;
  ``vmean`` = vsum / size; ``vstd`` = sqrt(max(vsqsum / size - vmean^2, 0)) (the population deviation).
- **Lesion matching.**  Prediction and reference are both labelled as above.  Regions smaller than ``min_size`` voxels are
  ignored on both sides.  For a predicted region p and a reference region t of the same class n_pt = |p and t|.  The pair is
  a *match* when n_pt > 0 and IoU(p, t) = n_pt / (|p| + |t| - n_pt) meets the threshold: ``> 0`` when ``iou_threshold ==
  0``, else ``>= iou_threshold``, the division being one float64 division.  t is *detected* iff it has a match; p is a
  *true positive* iff it has a match, else a false positive.  ``counts`` int64 ``[C, 4]`` = (n_ref, n_pred, detected,
  true-positive predictions) per class; ``sensitivity`` = detected / n_ref, ``precision`` = tp / n_pred, ``f1`` =
  2 tp' / (2 tp' + fn + fp) with tp' = detected, fn = n_ref - detected, fp = n_pred - tp; each NaN where its denominator
  is 0.  Per reference lesion: ``size``, ``overlap`` = sum_p n_pt, ``touching`` = sum of |p| over the p with n_pt > 0,
  ``best_pred`` = the p with the largest n_pt (ties to the smaller label, 0 when none), ``best_overlap`` its n_pt,
  ``best_iou``, ``dice_t`` = 2 overlap / (size + touching), ``detected``; ``valid`` marks the lesions of at least
  ``min_size`` voxels (the others hold zeros).  ``lesion_dice[c]`` = sum_t dice_t / (n_ref + false positives), NaN when
  that is 0: the lesion-wise Dice of the multi-lesion benchmarks **without their dilation of the reference** (they
  dilate the reference before the components are taken, so that nearby lesions merge; here they do not).
- **Lesion scores and FROC** (``lesion_score_metrics``, a float32 image such as the confidence map).
  ``score[p]`` = the predicted region's ``vmax``; ``best_score[t]`` = the largest score over the predictions that match t
  (the match rule above), ``-inf`` where there is none.  Per class the thresholds are the distinct scores of the valid
  predictions (at least ``min_size`` voxels), descending; at tau: det = #{valid t : best_score >= tau}, fp = #{valid p :
  not matched, score >= tau}, tp_pred = #{valid p : matched, score >= tau}; ``sensitivity`` = det / n_ref, ``precision``
  = tp_pred / (tp_pred + fp), ``average_precision`` = sum_i (S_i - S_{i-1}) P_i along the thresholds; ``froc_score`` =
  the mean over the fp levels of the largest sensitivity among the thresholds with fp <= level, 0 where none.  ``vmax`` is
  exact, so all of this is bitwise reproducible (``vmean`` comes from float64 atomics and is not the score).
- **Shape descriptors** (``region_shape(table)``, csrc/region_shape.hip; ``tests/shape_ref.py`` restates them
  with Python sets and integers).  ``RegionShape`` holds device tensors of ``max_regions`` entries: ``moment2`` int64
  ``[6]`` = the sums of h*h, w*w, d*d, h*w, h*d, w*d over the region's voxel indices; ``faces`` int64 ``[3]`` = the
  exposed voxel faces normal to h, w, d (the voxel across does not carry the region's label or lies outside the volume;
  an isolated voxel has (2, 2, 2)); ``cells`` int64 ``[2]`` = the distinct vertices V and edges E of the union of the
  region's closed unit cubes; ``covariance_mm2`` float64 ``[3, 3]`` = (n M_ab - S_a S_b) / n^2 * spacing_a * spacing_b with
  the numerator formed exactly (the covariance of the voxel centres, **without the 1/12 voxel-extent term**: the
  pyradiomics convention); ``eigenvalues`` float64 ``[3]`` of it, descending, clamped at 0; ``axes`` float64 ``[3, 3]``,
  row i the unit eigenvector of eigenvalue i in (h, w, d) order with its largest-magnitude component positive.  Derived,
  in float64: ``euler`` (int64) = V - E + F - size with F = (6 size + sum(faces)) / 2; ``major_axis_length``,
  ``minor_axis_length``, ``least_axis_length`` = 4 sqrt(lambda_i); ``elongation`` = sqrt(lambda_1 / lambda_0) and
  ``flatness`` = sqrt(lambda_2 / lambda_0), NaN where lambda_0 is 0; ``surface_area_mm2`` = faces_h sw sd + faces_w sh sd +
  faces_d sh sw; ``surface_to_volume`` = surface_area_mm2 / volume_mm3; ``sphericity`` = (36 pi V^2)^(1/3) / A with V the
  volume and A the surface area.  Three conventions:

  - The Euler number is that of the **union of closed voxels**: the 26-connectivity convention (voxels that share only a
    vertex or an edge are joined), whatever connectivity labelled the map.  It equals components - tunnels + cavities.
  - The surface area is the **voxel-face area**.  It overestimates a smooth surface: a digital ball tends to 1.5 times its
    true area, so its sphericity tends to 2/3.  A weighted (Lindblad) or mesh estimator is out of scope.
  - The maximum Feret diameter, convex hulls and shape on the scan's native grid are out of scope.

  The integer fields and ``euler`` are exact and bitwise reproducible; the float64 fields are a fixed sequence of
  operations on them and reproducible too.  No dimension may exceed 65535 (the int64 moments then cannot overflow).

Numerics: every integer field is exact and bitwise reproducible, and so is everything derived from integers.  For float32
images ``vmin`` / ``vmax`` are exact, and ``vsum`` / ``vsqsum`` are float64 sums added with hardware atomics: **these two
(and ``vmean`` / ``vstd`` from them) are the one pair of fields that is not bitwise reproducible**; their error is within
``size * 2^-53 * sum|x|`` (``sum x^2``) of any other float64 summation order.

Nothing here reads back to the host, so ``region_stats``, ``region_shape`` and ``lesion_metrics`` can be recorded in a
``torch.cuda.graph``.  ``RegionTable.cpu()``, ``RegionShape.cpu()`` and ``LesionReport.cpu()`` are the synchronising calls;
they raise ``RuntimeError`` on overflow.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import RegionTable as _CTable
from ._host import (LABEL_DTYPES, check_classes, check_connectivity, check_gpu, check_min_size, check_spacing, class_mask,
                    i3, label_volume, workspace)
from .shape import MAX_SHAPE_DIM, RegionShape, _check_shape_table, region_shape  # noqa: F401  (regions.region_shape)

_IMAGE_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.float32: 3, torch.int16: 4}


def _check_region_args(num_classes, connectivity=26, classes: Optional[Iterable[int]] = None, max_regions=4096,
                       spacing=(1.0, 1.0, 1.0)):
    """-> (num_classes, class bit mask, connectivity, max_regions, spacing)."""
    ncls = check_classes(num_classes)
    conn = check_connectivity(connectivity)
    mask = class_mask(ncls, classes)
    if isinstance(max_regions, bool) or not isinstance(max_regions, numbers.Integral) or not 1 <= max_regions <= 2 ** 24:
        raise ValueError(f"max_regions must be an int in 1..2^24, got {max_regions!r}")
    return ncls, mask, conn, int(max_regions), check_spacing(spacing)


def _check_lesion_args(iou_threshold=0.0, min_size=0, max_regions=4096, max_pairs=None):
    """-> (iou_threshold, min_size, max_pairs)."""
    if isinstance(iou_threshold, bool) or not isinstance(iou_threshold, numbers.Real) or \
            not (math.isfinite(iou_threshold) and 0.0 <= iou_threshold <= 1.0):
        raise ValueError(f"iou_threshold must be in [0, 1], got {iou_threshold!r}")
    min_size = check_min_size(min_size)
    if max_pairs is None:
        max_pairs = 4 * int(max_regions)
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, numbers.Integral) or not 1 <= max_pairs <= 2 ** 28:
        raise ValueError(f"max_pairs must be an int in 1..2^28, got {max_pairs!r}")
    return float(iou_threshold), min_size, int(max_pairs)


REGION_KWARGS = ("connectivity", "classes", "max_regions")
LESION_KWARGS = ("connectivity", "iou_threshold", "min_size", "classes", "max_regions", "max_pairs")


def check_region_kwargs(num_classes, spacing=(1.0, 1.0, 1.0), **kwargs):
    """Validate the keyword arguments a caller will forward to ``region_stats`` (``REGION_KWARGS``), before it spends
    time on anything else; raises ``ValueError`` like ``region_stats`` would."""
    unknown = set(kwargs) - set(REGION_KWARGS)
    if unknown:
        raise ValueError(f"unknown region_stats arguments {sorted(unknown)}")
    _check_region_args(num_classes, spacing=spacing, **kwargs)


def check_lesion_kwargs(num_classes, spacing=(1.0, 1.0, 1.0), **kwargs):
    """The same for ``lesion_metrics`` (``LESION_KWARGS``)."""
    unknown = set(kwargs) - set(LESION_KWARGS)
    if unknown:
        raise ValueError(f"unknown lesion_metrics arguments {sorted(unknown)}")
    r = _check_region_args(num_classes, spacing=spacing, **{k: v for k, v in kwargs.items() if k in REGION_KWARGS})
    _check_lesion_args(kwargs.get("iou_threshold", 0.0), kwargs.get("min_size", 0), r[3], kwargs.get("max_pairs"))


def _check_image(image, dims, device) -> torch.Tensor:
    check_gpu("image", image)
    if image.device != device:
        raise ValueError(f"image is on {image.device}, labels on {device}")
    if image.dim() == 5 and image.shape[0] == 1 and image.shape[1] == 1:
        image = image[0, 0]
    if image.dim() != 3 or tuple(image.shape) != tuple(dims):
        raise ValueError(f"image must have the labels' spatial shape {tuple(dims)}, got {tuple(image.shape)}")
    if image.dtype not in _IMAGE_DTYPES:
        raise ValueError(f"image must be int16, uint8, int32 or float32, got {image.dtype}")
    return image.contiguous()


class RegionTable:
    """The regions of one class map (the module docstring has every field).  All tensors live on the device."""

    _FIELDS = ("cls", "size", "first", "bbox", "coord_sum")
    _IMAGE_FIELDS = ("vmin", "vmax", "vsum", "vsqsum")

    def __init__(self, dims, max_regions: int, spacing, device, image_dtype: Optional[torch.dtype]):
        m = int(max_regions)
        self.dims, self.max_regions, self.spacing = tuple(int(d) for d in dims), m, tuple(spacing)
        self.n = torch.empty(1, dtype=torch.int32, device=device)
        self.overflow = torch.empty(1, dtype=torch.int32, device=device)
        self.labels = torch.empty(self.dims, dtype=torch.int32, device=device)
        self.cls = torch.empty(m, dtype=torch.int32, device=device)
        self.size = torch.empty(m, dtype=torch.int64, device=device)
        self.first = torch.empty(m, dtype=torch.int64, device=device)
        self.bbox = torch.empty((m, 6), dtype=torch.int32, device=device)
        self.coord_sum = torch.empty((m, 3), dtype=torch.int64, device=device)
        self.image_dtype = image_dtype
        self.vmin = self.vmax = self.vsum = self.vsqsum = None
        if image_dtype is not None:
            isf = image_dtype == torch.float32
            self.vmin = torch.empty(m, dtype=torch.float32 if isf else torch.int32, device=device)
            self.vmax = torch.empty_like(self.vmin)
            self.vsum = torch.empty(m, dtype=torch.float64 if isf else torch.int64, device=device)
            self.vsqsum = torch.empty_like(self.vsum)
        self._c = _CTable(m, -1 if image_dtype is None else _IMAGE_DTYPES[image_dtype],
                          *[None if t is None else t.data_ptr()
                            for t in (self.n, self.overflow, self.cls, self.size, self.first, self.bbox, self.coord_sum,
                                      self.vmin, self.vmax, self.vsum, self.vsqsum)])

    # ---- derived, float64, from the integer fields
    def _per(self, a: torch.Tensor) -> torch.Tensor:
        size = self.size.to(torch.float64)
        return a.to(torch.float64) / (size if a.dim() == 1 else size[:, None])

    @property
    def volume_mm3(self) -> torch.Tensor:
        return self.size.to(torch.float64) * (self.spacing[0] * self.spacing[1] * self.spacing[2])

    @property
    def centroid(self) -> torch.Tensor:
        return self._per(self.coord_sum)

    @property
    def centroid_mm(self) -> torch.Tensor:
        return self.centroid * torch.tensor(self.spacing, dtype=torch.float64, device=self.size.device)

    @property
    def extent(self) -> torch.Tensor:
        return self.bbox[:, 3:] - self.bbox[:, :3] + (self.size > 0).to(torch.int32)[:, None]

    def _need_image(self):
        if self.vsum is None:
            raise RuntimeError("this RegionTable was computed without an image")

    @property
    def vmean(self) -> torch.Tensor:
        self._need_image()
        return self._per(self.vsum)

    @property
    def vstd(self) -> torch.Tensor:
        self._need_image()
        m = self.vmean
        return torch.sqrt(torch.clamp(self._per(self.vsqsum) - m * m, min=0.0))

    def _device_fields(self) -> Dict[str, torch.Tensor]:
        out = {k: getattr(self, k) for k in self._FIELDS}
        out.update(volume_mm3=self.volume_mm3, centroid=self.centroid, centroid_mm=self.centroid_mm, extent=self.extent)
        if self.vsum is not None:
            out.update({k: getattr(self, k) for k in self._IMAGE_FIELDS})
            out.update(vmean=self.vmean, vstd=self.vstd)
        return out

    def check_overflow(self, n: int, overflow: int, what: str = "region table"):
        if overflow:
            raise RuntimeError(f"{what} overflow: {n} components, capacity {self.max_regions} (raise max_regions)")

    def cpu(self) -> Dict[str, np.ndarray]:
        """The one synchronising call: every field and derived value as a numpy array trimmed to ``n`` (plus ``"n"``).
        Raises ``RuntimeError`` when the map has more regions than ``max_regions``."""
        fields = self._device_fields()
        head = torch.stack([self.n[0], self.overflow[0]]).cpu()
        n, overflow = int(head[0]), int(head[1])
        self.check_overflow(n, overflow)
        out = {k: v[:n].cpu().numpy() for k, v in fields.items()}
        out["n"] = n
        return out


def _stats_launch(v: torch.Tensor, args, image: Optional[torch.Tensor], ws: Optional[torch.Tensor] = None) -> RegionTable:
    ncls, mask, conn, max_regions, spacing = args
    dims = tuple(v.shape)
    tab = RegionTable(dims, max_regions, spacing, v.device, None if image is None else image.dtype)
    if ws is None:
        ws = workspace("region_stats", dims, v.device)
    L.call("mivp_region_stats", L.ptr(v), LABEL_DTYPES[v.dtype], i3(dims), ncls, mask, conn, L.ptr(image), L.ptr(tab.labels),
           C.byref(tab._c), L.ptr(ws), L.stream())
    return tab


def region_stats(labels: torch.Tensor, num_classes: int, image: Optional[torch.Tensor] = None,
                 spacing: Sequence[float] = (1.0, 1.0, 1.0), connectivity: int = 26,
                 classes: Optional[Iterable[int]] = None, max_regions: int = 4096) -> RegionTable:
    """The connected regions of the class map ``labels`` with their size, first voxel, bounding box and coordinate sums,
    and with ``image`` their minimum, maximum, sum and sum of squares (the module docstring has the definitions).  No host
    read: ``RegionTable.cpu()`` synchronises."""
    check_gpu("labels", labels)
    args = _check_region_args(num_classes, connectivity, classes, max_regions, spacing)
    v = label_volume("labels", labels)
    img = None if image is None else _check_image(image, v.shape, v.device)
    return _stats_launch(v, args, img)


class LesionReport:
    """Lesion-wise detection metrics of a prediction against a reference (the module docstring has every field)."""

    def __init__(self, pred_regions: RegionTable, target_regions: RegionTable, num_classes: int, min_size: int,
                 iou_threshold: float, max_pairs: int):
        dev = pred_regions.size.device
        self.pred_regions, self.target_regions = pred_regions, target_regions
        self.num_classes, self.min_size, self.iou_threshold, self.max_pairs = num_classes, min_size, iou_threshold, max_pairs
        mt, mp = target_regions.max_regions, pred_regions.max_regions
        self.pairs = torch.empty(int(L.lib().mivp_region_overlap_ws(max_pairs)) // 8, dtype=torch.int64, device=dev)
        self.counts = torch.empty((num_classes, 4), dtype=torch.int64, device=dev)
        self.overlap = torch.empty(mt, dtype=torch.int64, device=dev)
        self.touching = torch.empty(mt, dtype=torch.int64, device=dev)
        self.best_overlap = torch.empty(mt, dtype=torch.int64, device=dev)
        self.best_pred = torch.empty(mt, dtype=torch.int32, device=dev)
        self.detected = torch.empty(mt, dtype=torch.int32, device=dev)
        self.matched = torch.empty(mp, dtype=torch.int32, device=dev)
        self.score = self.best_score = None                 # float32, with lesion_score_metrics only

    @property
    def size(self) -> torch.Tensor:
        return self.target_regions.size

    @property
    def valid(self) -> torch.Tensor:
        t = self.target_regions
        return (torch.arange(t.max_regions, device=t.size.device) < t.n) & (t.size >= self.min_size) & (t.size > 0)

    @property
    def n_pairs(self) -> torch.Tensor:
        return self.pairs[0]

    @property
    def pair_overflow(self) -> torch.Tensor:
        return self.pairs[1]

    @property
    def best_iou(self) -> torch.Tensor:
        n = self.best_overlap.to(torch.float64)
        sp = self.pred_regions.size[(self.best_pred.long() - 1).clamp(min=0)].to(torch.float64)
        iou = n / (sp + self.size.to(torch.float64) - n)
        return torch.where(self.best_pred > 0, iou, torch.zeros_like(iou))

    @property
    def dice_t(self) -> torch.Tensor:
        d = 2.0 * self.overlap.to(torch.float64) / (self.size + self.touching).to(torch.float64)
        return torch.where(self.valid, d, torch.zeros_like(d))

    def _ratio(self, num, den):
        num, den = num.to(torch.float64), den.to(torch.float64)
        return torch.where(den > 0, num / den, torch.full_like(den, float("nan")))

    @property
    def sensitivity(self) -> torch.Tensor:
        return self._ratio(self.counts[:, 2], self.counts[:, 0])

    @property
    def precision(self) -> torch.Tensor:
        return self._ratio(self.counts[:, 3], self.counts[:, 1])

    @property
    def f1(self) -> torch.Tensor:
        c = self.counts
        det, fn, fp = c[:, 2], c[:, 0] - c[:, 2], c[:, 1] - c[:, 3]
        return self._ratio(2 * det, 2 * det + fn + fp)

    @property
    def lesion_dice(self) -> torch.Tensor:
        cls = self.target_regions.cls
        onehot = cls[None, :] == torch.arange(self.num_classes, device=cls.device, dtype=cls.dtype)[:, None]
        total = torch.where(onehot, self.dice_t[None, :], torch.zeros((), dtype=torch.float64, device=cls.device)).sum(1)
        c = self.counts
        return self._ratio(total, c[:, 0] + c[:, 1] - c[:, 3])

    # ---- FROC (with lesion_score_metrics)
    def _need_scores(self):
        if self.score is None:
            raise RuntimeError("this LesionReport was computed without pred_image (lesion_score_metrics): it has no lesion scores")

    @property
    def valid_pred(self) -> torch.Tensor:
        p = self.pred_regions
        return (torch.arange(p.max_regions, device=p.size.device) < p.n) & (p.size >= self.min_size) & (p.size > 0)

    def froc(self) -> Dict[str, torch.Tensor]:
        """The free-response curve per class, on the device and with no host read: ``thresholds`` float32 ``[C, M]``
        (``M`` = the prediction table's ``max_regions``; the first ``n_thresholds[c]`` entries of a row are the distinct
        scores of the class's valid predictions, descending, the rest NaN) and, at each of them, ``sensitivity`` =
        det / n_ref, ``fp`` (int64, -1 in the padding), ``precision`` = tp_pred / (tp_pred + fp); ``average_precision``
        ``[C]`` = sum_i (S_i - S_{i-1}) P_i over the thresholds in that order, S_{-1} = 0 (0 without predictions).
        Values with n_ref = 0 are NaN."""
        self._need_scores()
        p, t = self.pred_regions, self.target_regions
        dev, ncls, mp, mt = p.size.device, self.num_classes, p.max_regions, t.max_regions
        classes = torch.arange(ncls, device=dev, dtype=p.cls.dtype)[:, None]
        vp = self.valid_pred[None, :] & (p.cls[None, :] == classes)
        vt = self.valid[None, :] & (t.cls[None, :] == classes)
        ninf = torch.full((), float("-inf"), dtype=torch.float32, device=dev)
        idx = torch.arange(mp, device=dev)[None, :]
        srt = torch.where(vp, self.score[None, :], ninf).sort(1, descending=True).values
        first = (idx < vp.sum(1)[:, None]) & ((idx == 0) | (srt != srt.roll(1, 1)))
        k = first.sum(1)
        live = idx < k[:, None]
        thr = torch.where(first, srt, ninf).sort(1, descending=True).values
        probe = torch.where(live, thr, -ninf).contiguous()          # +inf in the padding: nothing reaches it

        def at_least(values, mask):                                  # per class and threshold: #{mask : value >= tau}
            asc = torch.where(mask, values[None, :], ninf).sort(1).values.contiguous()
            return asc.shape[1] - torch.searchsorted(asc, probe)

        hit = self.matched[None, :] > 0
        det = at_least(self.best_score, vt)
        fp = at_least(self.score, vp & ~hit)
        tpp = at_least(self.score, vp & hit)
        n_ref = self.counts[:, 0]
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        sens = torch.where(live, self._ratio(det, n_ref[:, None].expand_as(det)), nan)
        prec = torch.where(live, self._ratio(tpp, tpp + fp), nan)
        step = det - torch.cat([torch.zeros_like(det[:, :1]), det[:, :-1]], 1)
        term = torch.where(live, step.to(torch.float64) * prec, torch.zeros((), dtype=torch.float64, device=dev))
        return dict(thresholds=torch.where(live, thr, torch.full_like(thr, float("nan"))), n_thresholds=k,
                    sensitivity=sens, fp=torch.where(live, fp, torch.full_like(fp, -1)), precision=prec,
                    average_precision=self._ratio(term.sum(1), n_ref))

    def froc_score(self, fp_levels: Sequence[float] = (0.125, 0.25, 0.5, 1, 2, 4, 8)) -> torch.Tensor:
        """Per class, the mean over ``fp_levels`` of the largest sensitivity among the thresholds with ``fp <= level``
        (0 where there is none); NaN for a class without reference lesions.  No host read."""
        levels = [float(a) for a in fp_levels]
        if not levels or not all(math.isfinite(a) and a >= 0 for a in levels):
            raise ValueError(f"fp_levels must be a non-empty sequence of non-negative numbers, got {fp_levels!r}")
        f = self.froc()
        sens, fp = f["sensitivity"], f["fp"]
        zero = torch.zeros((), dtype=torch.float64, device=sens.device)
        total = torch.zeros(self.num_classes, dtype=torch.float64, device=sens.device)
        for a in levels:
            total = total + torch.where((fp >= 0) & (fp <= a), sens, zero).max(1).values
        return torch.where(self.counts[:, 0] > 0, total / len(levels), torch.full_like(total, float("nan")))

    def cpu(self) -> Dict[str, object]:
        """The one synchronising call: ``counts`` and the per-class values, the per-lesion arrays trimmed to the number
        of reference lesions, ``pairs`` (int64 ``[K, 3]`` rows (p, t, n_pt) sorted by p then t) and the two region tables
        (``pred_regions`` / ``target_regions``, as ``RegionTable.cpu()``).  With lesion scores also ``score`` (per
        prediction), ``best_score`` (per reference lesion), ``froc`` (the arrays of ``froc()``, trimmed to the longest
        curve) and ``froc_score``.  Raises ``RuntimeError`` when either region table or the pair table overflowed."""
        curve = None if self.score is None else dict(self.froc(), froc_score=self.froc_score())
        per_class = dict(counts=self.counts, sensitivity=self.sensitivity, precision=self.precision, f1=self.f1,
                         lesion_dice=self.lesion_dice)
        per_lesion = dict(size=self.size, valid=self.valid, overlap=self.overlap, touching=self.touching,
                          best_pred=self.best_pred, best_overlap=self.best_overlap, best_iou=self.best_iou,
                          dice_t=self.dice_t, detected=self.detected)
        matched = self.matched
        pred, target = self.pred_regions, self.target_regions
        pf, tf = pred._device_fields(), target._device_fields()
        head = torch.stack([pred.n[0].long(), pred.overflow[0].long(), target.n[0].long(), target.overflow[0].long(),
                            self.pairs[0], self.pairs[1]]).cpu()
        np_, po, nt, to, nk, ko = (int(a) for a in head)
        pred.check_overflow(np_, po, "predicted region table")
        target.check_overflow(nt, to, "reference region table")
        if ko:
            raise RuntimeError(f"pair table overflow: more than {self.max_pairs} distinct (prediction, reference) pairs "
                               f"(raise max_pairs)")
        out = {k: v.cpu().numpy() for k, v in per_class.items()}
        out.update({k: v[:nt].cpu().numpy() for k, v in per_lesion.items()})
        out["matched"] = matched[:np_].cpu().numpy()
        if curve is not None:
            out["score"] = self.score[:np_].cpu().numpy()
            out["best_score"] = self.best_score[:nt].cpu().numpy()
            out["froc_score"] = curve.pop("froc_score").cpu().numpy()
            host = {k: v.cpu().numpy() for k, v in curve.items()}
            kmax = int(host["n_thresholds"].max()) if host["n_thresholds"].size else 0
            out["froc"] = {k: (v[:, :kmax] if v.ndim == 2 else v) for k, v in host.items()}
        slots = (self.pairs.numel() - 2) // 2
        keys, cnt = self.pairs[2:2 + slots], self.pairs[2 + slots:]
        used = keys != 0
        keys, cnt = keys[used], cnt[used]
        order = torch.argsort(keys)
        keys, cnt = keys[order], cnt[order]
        out["pairs"] = torch.stack([keys >> 32, keys & 0xFFFFFFFF, cnt], 1).cpu().numpy()
        out["pred_regions"] = {**{k: v[:np_].cpu().numpy() for k, v in pf.items()}, "n": np_}
        out["target_regions"] = {**{k: v[:nt].cpu().numpy() for k, v in tf.items()}, "n": nt}
        return out


def _lesion_launch(pv: torch.Tensor, tv: torch.Tensor, rargs, largs, pred_image: Optional[torch.Tensor] = None) -> LesionReport:
    ncls = rargs[0]
    thr, min_size, max_pairs = largs
    pred = _stats_launch(pv, rargs, pred_image)
    target = _stats_launch(tv, rargs, None)
    rep = LesionReport(pred, target, ncls, min_size, thr, max_pairs)
    L.call("mivp_region_overlap", L.ptr(pred.labels), L.ptr(target.labels), i3(pv.shape), C.byref(pred._c), C.byref(target._c),
           max_pairs, L.ptr(rep.pairs), L.stream())
    L.call("mivp_lesion_match", C.byref(pred._c), C.byref(target._c), L.ptr(rep.pairs), max_pairs, ncls, min_size, thr,
           L.ptr(rep.counts), L.ptr(rep.overlap), L.ptr(rep.touching), L.ptr(rep.best_overlap), L.ptr(rep.best_pred),
           L.ptr(rep.detected), L.ptr(rep.matched), L.stream())
    if pred_image is not None:
        rep.score = torch.empty(pred.max_regions, dtype=torch.float32, device=pv.device)
        rep.best_score = torch.empty(target.max_regions, dtype=torch.float32, device=pv.device)
        L.call("mivp_lesion_best_score", C.byref(pred._c), C.byref(target._c), L.ptr(rep.pairs), max_pairs, min_size, thr,
               L.ptr(rep.best_score), L.ptr(rep.score), L.stream())
    return rep


def lesion_metrics(pred: torch.Tensor, target: torch.Tensor, num_classes: int,
                   spacing: Sequence[float] = (1.0, 1.0, 1.0), connectivity: int = 26, iou_threshold: float = 0.0,
                   min_size: int = 0, classes: Optional[Iterable[int]] = None, max_regions: int = 4096,
                   max_pairs: Optional[int] = None) -> LesionReport:
    """Lesion-wise detection metrics of the class map ``pred`` against the class map ``target`` (the module docstring has
    the definitions): per-class counts, sensitivity, precision, F1 and lesion-wise Dice, the per-lesion table and both
    ``RegionTable``s.  ``max_pairs`` defaults to ``4 * max_regions``.  No host read: ``LesionReport.cpu()`` synchronises.
    ``lesion_score_metrics`` is the same with a score per lesion."""
    return lesion_score_metrics(pred, target, num_classes, None, spacing, connectivity, iou_threshold, min_size, classes,
                                max_regions, max_pairs)


def lesion_score_metrics(pred: torch.Tensor, target: torch.Tensor, num_classes: int, pred_image: Optional[torch.Tensor],
                         spacing: Sequence[float] = (1.0, 1.0, 1.0), connectivity: int = 26, iou_threshold: float = 0.0,
                         min_size: int = 0, classes: Optional[Iterable[int]] = None, max_regions: int = 4096,
                         max_pairs: Optional[int] = None) -> LesionReport:
    """``lesion_metrics`` with lesion scores: ``pred_image`` (float32, the spatial shape of ``pred``; a confidence map) is
    the image of the predicted ``RegionTable``, and the report carries ``score`` / ``best_score``, ``froc()`` and
    ``froc_score()`` (the module docstring has the definitions).  ``pred_image=None`` is ``lesion_metrics``."""
    check_gpu("pred", pred)
    check_gpu("target", target)
    rargs = _check_region_args(num_classes, connectivity, classes, max_regions, spacing)
    largs = _check_lesion_args(iou_threshold, min_size, max_regions, max_pairs)
    pv, tv = label_volume("pred", pred), label_volume("target", target)
    if pv.shape != tv.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if pv.device != tv.device:
        raise ValueError(f"pred is on {pv.device}, target on {tv.device}")
    img = None
    if pred_image is not None:
        img = _check_image(pred_image, pv.shape, pv.device)
        if img.dtype != torch.float32:
            raise ValueError(f"pred_image must be float32, got {img.dtype}")
    return _lesion_launch(pv, tv, rargs, largs, img)
