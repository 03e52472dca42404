"""Centreline extraction (3-D thinning), the clDice metric and centreline statistics on the GPU (csrc/skeleton.hip, DESIGN
4.38).

Definitions (written out, as in ``mivp_amd.components``; ``tests/skeleton_ref.py`` restates them in numpy and Python):

- **Layout.**  A volume is ``[1, 1, H, W, D]`` or ``[H, W, D]``, contiguous ``[H][W][D]`` with D fastest, fewer than 2^31
  voxels, with the dtypes of ``mivp_amd.components``.  ``num_classes`` C is 1..16, ``classes`` defaults to ``1..C-1`` and
  0 is rejected.
- **Object and background.**  The object of a voxel ``v`` is the set of voxels that hold the same selected class as ``v``.
  Everything else is background for it: other classes, classes not in ``classes``, values outside ``[0, C)``, non-integer
  floats and everything outside the volume.
- **Simple point, (26, 6) topology.**  With ``obj`` the object voxels among the 26 neighbours of ``v``, ``v`` is simple
  iff (a) ``obj`` is not empty and is one component under 26-adjacency within the neighbourhood, and (b) the background
  voxels among the 18-neighbours contain a 6-neighbour of ``v`` and all background 6-neighbours of ``v`` lie in one
  component of that set under 6-adjacency.  Deleting a simple point changes neither the components of the object nor
  its tunnels and cavities.
- **End point.**  At most one object neighbour.
- **Iteration.**  (1) Mark the border: the object voxels with a face neighbour that is not in their object, on the state
  the iteration starts from.  (2) Eight sub-passes, one per subfield ``s = (h&1)<<2 | (w&1)<<1 | (d&1)``, ``s = 0..7``: a
  sub-pass deletes every marked voxel of its subfield that is simple **on the current state** and, with
  ``keep_endpoints``, is no end point on it.  (3) Stop after an iteration that deletes nothing.  Two voxels of one
  subfield are never 26-adjacent, so the result depends on no thread order and is the same bits on every run.

  The skeletons are defined by this algorithm, not by scikit-image's (Lee94 deletes in another order).
  ``keep_endpoints=False`` gives the ultimate topological kernel: a component without tunnels and cavities becomes one
  voxel, a ring stays a closed curve.
- **clDice** (Shit et al., CVPR 2021) per class ``c``, with ``V`` the voxels of the class and ``S`` its skeleton, P the
  prediction and L the reference: ``Tprec = |S_P and V_L| / |S_P|``, ``Tsens = |S_L and V_P| / |S_L|``, ``clDice = 2 Tprec
  Tsens / (Tprec + Tsens)``, in float64 from integer counts.  **Empty sets** follow ``SegMetrics``, where a class without
  voxels scores 0 rather than NaN: a ratio with a zero denominator is 0, so a class that is absent on either side (or on
  both) has clDice 0 and pulls the mean down.  The means are taken over ``classes``.
- **Centreline statistics** per class of one skeleton: the voxels; those with 0, 1, 2 and >= 3 same-class 26-neighbours
  (isolated, end points, interior, branch points); 13 edge counts, one per forward offset (the offsets ``(dh, dw, dd)``
  whose first non-zero component is positive, in lexicographic order), an edge being a pair of voxels that far apart that
  hold the same class.  ``length_mm = sum_k edges_k * |offset_k * spacing|``, added in that order in float64: this is the
  length of the **26-adjacency graph** of the skeleton.  Where three skeleton voxels are mutually adjacent (a corner, a
  branch point) the graph has the diagonal as well as the two legs, so it is an upper estimate of the curve length.

Everything runs on the device in integer arithmetic with integer atomics.  ``skeletonize(max_iter=None)`` reads one int32
per iteration; ``skeletonize(max_iter=n)``, ``centerline_metrics(max_iter=n)`` and ``skeleton_stats`` read nothing back
and can be recorded in a ``torch.cuda.graph``.  ``SkeletonStats.cpu()`` and ``CenterlineReport.cpu()`` synchronise.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from ._host import (LABEL_DTYPES, check_classes, check_flag, check_gpu, check_spacing, class_mask, i3, label_volume,
                    plain_int, workspace)

MAX_ITER = 4096
FORWARD_OFFSETS = tuple((a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) > (0, 0, 0))
CL_WORDS, ST_WORDS = 4, 18
assert len(FORWARD_OFFSETS) == 13


class SkeletonResult(NamedTuple):
    """``skeleton``: uint8 of the input's shape, a voxel keeps its class if it survives and is 0 otherwise.  ``iterations``:
    the iterations that ran, the last one that deleted nothing included; ``converged``: whether one deleted nothing.  Both
    are a Python int and a bool after ``max_iter=None`` and device int32 scalars after ``max_iter=n``."""
    skeleton: torch.Tensor
    iterations: Union[int, torch.Tensor]
    converged: Union[bool, torch.Tensor]


def _check_skeleton_args(num_classes, classes: Optional[Iterable[int]] = None, keep_endpoints=True,
                         max_iter=None) -> Tuple[int, int, Tuple[int, ...], bool, Optional[int]]:
    """-> (num_classes, class bit mask, the classes in ascending order, keep_endpoints, max_iter)."""
    ncls = check_classes(num_classes)
    mask = class_mask(ncls, classes)
    keep = check_flag("keep_endpoints", keep_endpoints)
    if max_iter is not None and (not plain_int(max_iter) or not 1 <= int(max_iter) <= MAX_ITER):
        raise ValueError(f"max_iter must be None or an integer in 1..{MAX_ITER}, got {max_iter!r}")
    return ncls, mask, tuple(c for c in range(1, ncls) if (mask >> c) & 1), keep, None if max_iter is None else int(max_iter)


def _thin(v: torch.Tensor, args) -> SkeletonResult:
    """Thin the prepared ``[H, W, D]`` map ``v``; ``args`` from ``_check_skeleton_args``."""
    ncls, mask, _, keep, max_iter = args
    dims = tuple(v.shape)
    skel = torch.empty(dims, dtype=torch.uint8, device=v.device)
    ws = workspace("skeleton", dims, v.device)
    L.call("mivp_skeleton_begin", L.ptr(v), LABEL_DTYPES[v.dtype], i3(dims), ncls, mask, L.ptr(skel), L.ptr(ws), L.stream())
    if max_iter is None:
        deleted = ws[:8].view(torch.int32)
        it = 0
        while True:
            it += 1
            L.call("mivp_skeleton_iter", L.ptr(skel), i3(dims), int(keep), it, L.ptr(ws), L.stream())
            if int(deleted[it & 1].item()) == 0:           # the one host read of this iteration
                return SkeletonResult(skel, it, True)
    for it in range(1, max_iter + 1):
        L.call("mivp_skeleton_iter", L.ptr(skel), i3(dims), int(keep), it, L.ptr(ws), L.stream())
    state = torch.empty(2, dtype=torch.int32, device=v.device)
    L.call("mivp_skeleton_end", L.ptr(ws), max_iter, L.ptr(state[:1]), L.ptr(state[1:]), L.stream())
    return SkeletonResult(skel, state[0], state[1])


def skeletonize(labels: torch.Tensor, num_classes: int, classes: Optional[Iterable[int]] = None, keep_endpoints: bool = True,
                max_iter: Optional[int] = None) -> SkeletonResult:
    """The skeleton of every class in ``classes`` of the GPU class map ``labels`` (``[1, 1, H, W, D]`` or ``[H, W, D]``) by
    the thinning of the module docstring; each class is thinned on its own, with every other voxel as background.  The
    input is not modified.  ``max_iter=None`` iterates until nothing is deleted and reads one int32 per iteration;
    ``max_iter=n`` (1..4096) issues exactly ``n`` iterations' launches with no host read (each returns at once after an
    iteration that deleted nothing), which can be recorded in a ``torch.cuda.graph``."""
    args = _check_skeleton_args(num_classes, classes, keep_endpoints, max_iter)
    v = label_volume("labels", labels)
    skel, iterations, converged = _thin(v, args)
    return SkeletonResult(skel.reshape(labels.shape), iterations, converged)


def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den in float64, 0 where den is 0 (the module docstring: empty sets)."""
    num, den = num.to(torch.float64), den.to(torch.float64)
    return torch.where(den > 0, num / den.clamp(min=1.0), torch.zeros_like(den))


def _seq_sum(terms: Sequence[torch.Tensor]) -> torch.Tensor:
    """The terms added one after the other (a fixed order, so the float64 result is the same bits everywhere)."""
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def _check_out(out, kind, ncls: int, classes: Tuple[int, ...], spacing=None):
    if not isinstance(out, kind):
        raise TypeError(f"out must be a {kind.__name__}")
    if (out.num_classes, out.classes) != (ncls, classes):
        raise ValueError(f"out was made for (num_classes, classes) = {(out.num_classes, out.classes)}, this call has "
                         f"{(ncls, classes)}")
    if spacing is not None and out.spacing != spacing:
        raise ValueError(f"out was made for spacing {out.spacing}, this call has {spacing}")


class SkeletonStats:
    """The centreline statistics of one or more skeletons (the module docstring has every field): ``counts`` is the int64
    ``[C, 18]`` device table behind them, row ``c`` for class ``c`` (rows of classes outside ``classes`` stay zero)."""

    INT_FIELDS = ("voxels", "isolated", "end_points", "interior", "branch_points", "edges")

    def __init__(self, num_classes: int, classes: Sequence[int], spacing: Sequence[float], device):
        self.num_classes, self.classes, self.spacing = int(num_classes), tuple(classes), tuple(spacing)
        self.counts = torch.zeros((self.num_classes, ST_WORDS), dtype=torch.int64, device=device)

    voxels = property(lambda self: self.counts[:, 0])
    isolated = property(lambda self: self.counts[:, 1])
    end_points = property(lambda self: self.counts[:, 2])
    interior = property(lambda self: self.counts[:, 3])
    branch_points = property(lambda self: self.counts[:, 4])
    edges = property(lambda self: self.counts[:, 5:])

    @property
    def edge_lengths_mm(self) -> Tuple[float, ...]:
        return tuple(math.sqrt(sum((o * s) ** 2 for o, s in zip(off, self.spacing))) for off in FORWARD_OFFSETS)

    @property
    def length_mm(self) -> torch.Tensor:
        """float64 ``[C]``: the length of the 26-adjacency graph of each class's skeleton."""
        e = self.edges.to(torch.float64)
        return _seq_sum([e[:, k] * w for k, w in enumerate(self.edge_lengths_mm)])

    def zero_(self) -> "SkeletonStats":
        self.counts.zero_()
        return self

    def cpu(self) -> Dict[str, object]:
        """The synchronising call: every field as a numpy array ``[C]`` (``edges`` ``[C, 13]``), plus ``length_mm``,
        ``classes``, ``num_classes`` and ``spacing``."""
        out = {k: getattr(self, k).cpu().numpy() for k in self.INT_FIELDS}
        out.update(length_mm=self.length_mm.cpu().numpy(), classes=self.classes, num_classes=self.num_classes,
                   spacing=self.spacing)
        return out


def _stats_launch(skel: torch.Tensor, ncls: int, mask: int, stats: SkeletonStats):
    L.call("mivp_skeleton_stats", L.ptr(skel), i3(tuple(skel.shape)), ncls, mask, L.ptr(stats.counts), L.stream())


def skeleton_stats(skeleton: torch.Tensor, num_classes: int, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                   classes: Optional[Iterable[int]] = None, out: Optional[SkeletonStats] = None) -> SkeletonStats:
    """The centreline statistics of ``skeleton`` (what ``skeletonize`` returned; any class map of the module's layouts is
    taken as it is): one counting pass, no host read.  With ``out=`` the counts are added to that object, which is how
    scans are pooled."""
    ncls, mask, cls, _, _ = _check_skeleton_args(num_classes, classes)
    sp = check_spacing(spacing)
    v = label_volume("skeleton", skeleton)
    if out is not None:
        _check_out(out, SkeletonStats, ncls, cls, sp)
    if v.dtype != torch.uint8:
        u = torch.empty(tuple(v.shape), dtype=torch.uint8, device=v.device)
        L.call("mivp_skeleton_begin", L.ptr(v), LABEL_DTYPES[v.dtype], i3(tuple(v.shape)), ncls, mask, L.ptr(u), None,
               L.stream())
        v = u
    stats = SkeletonStats(ncls, cls, sp, v.device) if out is None else out
    _stats_launch(v, ncls, mask, stats)
    return stats


class CenterlineReport:
    """The clDice counts of one or more (prediction, reference) pairs and the metrics derived from them (the module
    docstring has the definitions).  ``counts``: int64 ``[C, 4]`` on the device, per class ``|S_P|``, ``|S_P and V_L|``,
    ``|S_L|``, ``|S_L and V_P|``.  ``pred_stats`` / ``target_stats``: the ``SkeletonStats`` of the two skeletons.
    ``pred_skeleton`` / ``target_skeleton`` and ``iterations`` / ``converged`` (pairs: prediction, reference) describe the
    last pair that was added."""

    def __init__(self, num_classes: int, classes: Sequence[int], spacing: Sequence[float], device):
        self.num_classes, self.classes, self.spacing = int(num_classes), tuple(classes), tuple(spacing)
        self.counts = torch.zeros((self.num_classes, CL_WORDS), dtype=torch.int64, device=device)
        self.pred_stats = SkeletonStats(num_classes, classes, spacing, device)
        self.target_stats = SkeletonStats(num_classes, classes, spacing, device)
        self.pred_skeleton = self.target_skeleton = None
        self.iterations = self.converged = None

    skeleton_pred = property(lambda self: self.counts[:, 0])
    skeleton_pred_in_target = property(lambda self: self.counts[:, 1])
    skeleton_target = property(lambda self: self.counts[:, 2])
    skeleton_target_in_pred = property(lambda self: self.counts[:, 3])

    @property
    def tprec(self) -> torch.Tensor:
        return _ratio(self.counts[:, 1], self.counts[:, 0])

    @property
    def tsens(self) -> torch.Tensor:
        return _ratio(self.counts[:, 3], self.counts[:, 2])

    @property
    def cldice(self) -> torch.Tensor:
        p, s = self.tprec, self.tsens
        den = p + s
        return torch.where(den > 0, 2.0 * p * s / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))

    def _mean(self, per_class: torch.Tensor) -> torch.Tensor:
        return _seq_sum([per_class[c] for c in self.classes]) / float(len(self.classes))

    mean_tprec = property(lambda self: self._mean(self.tprec))
    mean_tsens = property(lambda self: self._mean(self.tsens))
    mean_cldice = property(lambda self: self._mean(self.cldice))

    def zero_(self) -> "CenterlineReport":
        self.counts.zero_()
        self.pred_stats.zero_()
        self.target_stats.zero_()
        return self

    def cpu(self) -> Dict[str, object]:
        """The synchronising call: ``counts`` ``[C, 4]``, ``tprec`` / ``tsens`` / ``cldice`` ``[C]`` and their means over
        ``classes`` as floats, ``pred`` / ``target`` (the dicts of ``SkeletonStats.cpu()``), ``iterations`` / ``converged``
        (pairs: prediction, reference), ``classes``, ``num_classes`` and ``spacing``."""
        out = {k: getattr(self, k).cpu().numpy() for k in ("counts", "tprec", "tsens", "cldice")}
        out.update({k: float(getattr(self, k).cpu()) for k in ("mean_tprec", "mean_tsens", "mean_cldice")})
        out.update(pred=self.pred_stats.cpu(), target=self.target_stats.cpu(), classes=self.classes,
                   num_classes=self.num_classes, spacing=self.spacing)
        if self.iterations is not None:
            out["iterations"] = tuple(int(a) for a in self.iterations)
            out["converged"] = tuple(bool(a) for a in self.converged)
        return out


def check_centerline_kwargs(num_classes, spacing=(1.0, 1.0, 1.0), classes=None, keep_endpoints=True, max_iter=None):
    """Validate the arguments of ``centerline_metrics`` that need no tensor -> (checked ``_check_skeleton_args`` tuple,
    spacing)."""
    return _check_skeleton_args(num_classes, classes, keep_endpoints, max_iter), check_spacing(spacing)


def centerline_metrics(pred: torch.Tensor, target: torch.Tensor, num_classes: int,
                       spacing: Sequence[float] = (1.0, 1.0, 1.0), classes: Optional[Iterable[int]] = None,
                       keep_endpoints: bool = True, max_iter: Optional[int] = None,
                       out: Optional[CenterlineReport] = None) -> CenterlineReport:
    """clDice of the class map ``pred`` against the reference ``target`` (both ``[1, 1, H, W, D]`` or ``[H, W, D]`` on the
    GPU, the same spatial shape): both are thinned with ``skeletonize(..., classes, keep_endpoints, max_iter)``, one fused
    pass counts the four sets of the module docstring and one pass per skeleton its ``SkeletonStats``.  With ``out=`` the
    counts are added to that report, which is how scans are pooled.  With ``max_iter=n`` nothing is read back."""
    cls = None if classes is None else list(classes)
    args, sp = check_centerline_kwargs(num_classes, spacing, cls, keep_endpoints, max_iter)
    ncls, mask, sel = args[:3]
    check_gpu("pred", pred)
    check_gpu("target", target)
    p, t = label_volume("pred", pred), label_volume("target", target)
    if p.shape != t.shape:
        raise ValueError(f"pred and target must have the same spatial shape, got {tuple(p.shape)} and {tuple(t.shape)}")
    if p.device != t.device:
        raise ValueError(f"pred is on {p.device}, target on {t.device}")
    if out is not None:
        _check_out(out, CenterlineReport, ncls, sel, sp)
        if out.counts.device != p.device:
            raise ValueError(f"out is on {out.counts.device}, pred on {p.device}")
    rep = CenterlineReport(ncls, sel, sp, p.device) if out is None else out
    sp_res, sl_res = _thin(p, args), _thin(t, args)
    L.call("mivp_centerline_counts", L.ptr(p), LABEL_DTYPES[p.dtype], L.ptr(t), LABEL_DTYPES[t.dtype],
           L.ptr(sp_res.skeleton), L.ptr(sl_res.skeleton), i3(tuple(p.shape)), ncls, L.ptr(rep.counts), L.stream())
    _stats_launch(sp_res.skeleton, ncls, mask, rep.pred_stats)
    _stats_launch(sl_res.skeleton, ncls, mask, rep.target_stats)
    rep.pred_skeleton, rep.target_skeleton = sp_res.skeleton, sl_res.skeleton
    rep.iterations = (sp_res.iterations, sl_res.iterations)
    rep.converged = (sp_res.converged, sl_res.converged)
    return rep


class CenterlineEvaluation:
    """The centreline evaluation of ``SlidingWindowPredictor`` (its base class, so that the predictor's own body keeps the
    methods it had)."""

    def evaluate_centerline(self, x: torch.Tensor, seg: torch.Tensor, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                            classes: Optional[Iterable[int]] = None, postprocess: Optional[Dict] = None,
                            keep_endpoints: bool = True, max_iter: Optional[int] = None) -> CenterlineReport:
        """clDice and centreline statistics of the whole-volume prediction against ``seg [1, 1, H, W, D]``: the
        ``CenterlineReport`` of ``centerline_metrics(predict(x, postprocess=postprocess)["labels"], seg, num_classes,
        spacing, classes, keep_endpoints, max_iter)``.  With ``max_iter=n`` prediction, post-processing, thinning and
        counting run with no host read in between; ``CenterlineReport.cpu()`` synchronises."""
        post = self._post(postprocess)
        self._check_input(seg, "seg", channels=1)
        cls = None if classes is None else list(classes)
        check_centerline_kwargs(self.ncls, spacing, cls, keep_endpoints, max_iter)
        labels, _, _ = self._run(x, False, None, post)
        return centerline_metrics(labels, seg, self.ncls, spacing, cls, keep_endpoints, max_iter)


def evaluate_volume_centerline(model, x: torch.Tensor, seg: torch.Tensor, roi: Sequence[int], num_classes: int,
                               overlap: float = 0.5, mode: str = "gaussian", sigma_scale: float = 0.125, sub_batch: int = 10,
                               graph: bool = False, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                               classes: Optional[Iterable[int]] = None, postprocess: Optional[Dict] = None,
                               mirror_axes: Sequence[int] = (), keep_endpoints: bool = True, max_iter: Optional[int] = None,
                               skip=None, *, fit=None) -> CenterlineReport:
    """One-shot ``SlidingWindowPredictor(...).evaluate_centerline(x, seg, spacing, classes, postprocess, keep_endpoints,
    max_iter)``: the ``CenterlineReport`` of the whole-volume prediction.  Keyword-only ``fit``: the predictor's ``fit=``."""
    from . import inference
    return inference._one_shot(model, x, None, num_classes, roi, overlap, mode, sigma_scale, sub_batch, graph, mirror_axes,
                               skip, fit).evaluate_centerline(x, seg, spacing, classes, postprocess, keep_endpoints, max_iter)
