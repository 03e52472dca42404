"""Surface-distance metrics of a label map against a reference on the GPU (csrc/surface.hip).

Definitions (MONAI is not a dependency here, so the conventions are written out rather than pinned to it):

- **Surface of a class.**  For a binary mask M (label == c), a voxel is a surface voxel if it is in M and at least one of
  its 6 face neighbours is outside M or outside the volume:
  ``M & ~scipy.ndimage.binary_erosion(M, generate_binary_structure(3, 1), border_value=0)``.  Values outside
  ``[0, num_classes)`` (and non-integer floats) belong to no class.
- **Distances.**  ``spacing = (s0, s1, s2)`` is in mm per voxel along H, W, D; the distance between voxels is
  ``sqrt(sum_a (s_a * delta_a)^2)``.  The directed surface distances from A to B are, for every surface voxel of A, the
  distance to the nearest surface voxel of B: ``distance_transform_edt(~surf_B, sampling=spacing)`` sampled at ``surf_A``.
- **Per class c** (pred = A, target = B), both directions:
  ``hd`` = the maximum over both directed sets; ``hd_p`` = ``max(P_p(d_AB), P_p(d_BA))`` with
  ``P_p = numpy.percentile(..., method="linear")``; ``assd`` = ``(sum d_AB + sum d_BA) / (|dA| + |dB|)``;
  ``nsd`` at tolerance tau mm = ``(#{d_AB <= tau} + #{d_BA <= tau}) / (|dA| + |dB|)`` (voxel counts, no surface-element
  area weighting).
- **Empty classes.**  Both surfaces empty: every value is ``nan``.  One empty: ``hd``, ``hd_p`` and ``assd`` are ``inf``
  and ``nsd`` is 0.  The background class (0) is skipped unless ``include_background``; skipped entries are ``nan``.

Everything up to the final read runs on the device with no host synchronisation: one surface-map launch, then per
(class, direction) one exact EDT (three separable passes) and one statistics chain (an exact radix select of the two
ranks P_p reads, the maximum, the count within tau and a fixed-order float64 sum).  The host does the closing float64
arithmetic: ``sqrt``, the percentile interpolation and the ratios.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Sequence

import numpy as np
import torch

from . import _lib as L
from ._host import LABEL_DTYPES, check_classes, check_gpu, check_spacing, i3, label_volume, workspace

_REC = 8          # record int64 [8] per (class, direction): see include/mivp.h, mivp_surface_stats


def _surface_launch(pred: torch.Tensor, target, num_classes: int):
    """Launch the surface map of pred (and target): (surf_pred, surf_target or None, counts int64 [C, 2] on device)."""
    dims = tuple(pred.shape)
    sp = torch.empty(dims, dtype=torch.uint8, device=pred.device)
    st = torch.empty(dims, dtype=torch.uint8, device=pred.device) if target is not None else None
    counts = torch.zeros((num_classes, 2), dtype=torch.int64, device=pred.device)
    L.call("mivp_surface_map", L.ptr(pred), L.ptr(target), LABEL_DTYPES[pred.dtype], num_classes, i3(dims), L.ptr(sp),
           L.ptr(st), L.ptr(counts), L.stream())
    return sp, st, counts


def surface_map(labels: torch.Tensor, num_classes: int) -> torch.Tensor:
    """``labels [1, 1, H, W, D]`` (uint8, int32, int64 or float class indices) -> uint8 ``[1, 1, H, W, D]``: the class on
    its surface voxels, 255 elsewhere."""
    ncls = check_classes(num_classes)
    lab = label_volume("labels", labels)
    sp, _, _ = _surface_launch(lab, None, ncls)
    return sp.reshape((1, 1) + tuple(lab.shape))


def _edt_launch(seeds: torch.Tensor, cls: int, spacing, out: torch.Tensor, ws: torch.Tensor):
    L.call("mivp_edt_sq", L.ptr(seeds), cls, i3(seeds.shape), (C.c_float * 3)(*spacing), L.ptr(out), L.ptr(ws), L.stream())


def distance_transform_sq(seeds: torch.Tensor, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> torch.Tensor:
    """Exact squared Euclidean distance transform: ``seeds [H, W, D]`` (or ``[1, 1, H, W, D]``; non-zero = seed) ->
    float32 ``[H, W, D]``, the squared distance in mm^2 from every voxel to the nearest seed, ``inf`` where there is no
    seed.  With ``spacing == (1, 1, 1)`` the values are the exact integers ``rint(distance_transform_edt(~seeds)^2)``."""
    sp = check_spacing(spacing)
    check_gpu("seeds", seeds)
    s = seeds[0, 0] if seeds.dim() == 5 and seeds.shape[:2] == (1, 1) else seeds
    if s.dim() != 3:
        raise ValueError(f"seeds must be [H, W, D] or [1, 1, H, W, D], got {tuple(seeds.shape)}")
    if s.shape[0] > 65535 or s.shape[1] > 65535 or s.numel() >= 2 ** 31:
        raise ValueError(f"seeds of shape {tuple(s.shape)}: H and W must be <= 65535 and the volume < 2^31 voxels")
    s = (s != 0).to(torch.uint8).contiguous()
    out = torch.empty(tuple(s.shape), dtype=torch.float32, device=s.device)
    _edt_launch(s, 1, sp, out, workspace("edt", s.shape, s.device))
    return out


def _check_metric_args(num_classes, spacing, percentile, tolerance):
    ncls = check_classes(num_classes)
    sp = check_spacing(spacing)
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError(f"percentile must be in [0, 100], got {percentile}")
    if not float(tolerance) >= 0.0 or not math.isfinite(float(tolerance)):
        raise ValueError(f"tolerance must be a non-negative number of mm, got {tolerance}")
    return ncls, sp, float(percentile), float(tolerance)


def _metrics_launch(pred, target, ncls, spacing, percentile, tolerance, include_background):
    """All device work of ``surface_metrics``; returns (counts int64 [C, 2], records int64 [C, 2, 8]) on the device."""
    p, t = label_volume("pred", pred), label_volume("target", target)
    if p.shape != t.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if p.device != t.device:
        raise ValueError(f"pred is on {p.device}, target on {t.device}")
    if p.shape[0] > 65535 or p.shape[1] > 65535:
        raise ValueError(f"volume {tuple(p.shape)}: H and W must be <= 65535")
    if t.dtype != p.dtype:
        p, t = p.float(), t.float()
    dims = tuple(p.shape)
    sp, st, counts = _surface_launch(p, t, ncls)
    recs = torch.zeros((ncls, 2, _REC), dtype=torch.int64, device=p.device)
    dist = torch.empty(dims, dtype=torch.float32, device=p.device)
    ews = workspace("edt", dims, p.device)
    sws = workspace("surface_stats", dims, p.device)
    q, a = percentile / 100.0, i3(dims)
    for c in range(0 if include_background else 1, ncls):
        # direction 0: pred's surface sampled in the EDT of target's; direction 1: the other way round
        for m, (seeds, sampled) in enumerate(((st, sp), (sp, st))):
            _edt_launch(seeds, c, spacing, dist, ews)
            L.call("mivp_surface_stats", L.ptr(sampled), c, L.ptr(dist), a, C.c_void_p(counts.data_ptr() + 8 * (2 * c + m)), q,
                   tolerance, L.ptr(sws), C.c_void_p(recs.data_ptr() + 8 * _REC * (2 * c + m)), L.stream())
    return counts, recs


def _key_dist(key) -> float:
    """sqrt of the float32 squared distance whose bits are ``key``, in float64."""
    return math.sqrt(float(np.array([int(key)], dtype=np.uint32).view(np.float32)[0]))


def _percentile(rec, q: float) -> float:
    """numpy.percentile(method="linear") from the two order statistics the device selected."""
    n = int(rec[0])
    vi = (n - 1) * q
    lo, hi = int(rec[6]), int(rec[7])
    a, b = _key_dist(rec[4]), _key_dist(rec[5])
    if lo == hi:
        return a
    g = vi - math.floor(vi)
    diff = b - a
    return b - diff * (1 - g) if g >= 0.5 else a + diff * g


def _metrics_finish(counts: np.ndarray, recs: np.ndarray, ncls, percentile, include_background) -> Dict[str, torch.Tensor]:
    q = percentile / 100.0
    out = {k: np.full(ncls, np.nan) for k in ("hd", "hd_p", "assd", "nsd")}
    for c in range(0 if include_background else 1, ncls):
        na, nb = int(counts[c, 0]), int(counts[c, 1])
        if na == 0 and nb == 0:
            continue
        if na == 0 or nb == 0:
            out["hd"][c] = out["hd_p"][c] = out["assd"][c] = math.inf
            out["nsd"][c] = 0.0
            continue
        r = recs[c]
        out["hd"][c] = max(_key_dist(r[0, 1]), _key_dist(r[1, 1]))
        out["hd_p"][c] = max(_percentile(r[0], q), _percentile(r[1], q))
        sums = r[:, 3].copy().view(np.float64)
        out["assd"][c] = (float(sums[0]) + float(sums[1])) / (na + nb)
        out["nsd"][c] = (int(r[0, 2]) + int(r[1, 2])) / (na + nb)
    res = {k: torch.from_numpy(v) for k, v in out.items()}
    res["surface_voxels"] = torch.from_numpy(counts.astype(np.int64))
    return res


def surface_metrics(pred: torch.Tensor, target: torch.Tensor, num_classes: int, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                    percentile: float = 95.0, tolerance: float = 1.0,
                    include_background: bool = False) -> Dict[str, torch.Tensor]:
    """Per-class surface-distance metrics of ``pred`` against ``target`` (``[1, 1, H, W, D]`` GPU class maps, e.g.
    ``predict(x)["labels"]`` and the ``seg`` that ``evaluate`` takes); definitions in the module docstring.

    Returns float64 CPU tensors ``[num_classes]`` ``hd``, ``hd_p``, ``assd``, ``nsd`` and int64 ``surface_voxels
    [num_classes, 2]`` (pred, target).  One host read."""
    check_gpu("pred", pred)
    check_gpu("target", target)
    ncls, sp, pc, tol = _check_metric_args(num_classes, spacing, percentile, tolerance)
    counts, recs = _metrics_launch(pred, target, ncls, sp, pc, tol, include_background)
    host = torch.cat([counts.reshape(-1), recs.reshape(-1)]).cpu().numpy()
    return _metrics_finish(host[:2 * ncls].reshape(ncls, 2), host[2 * ncls:].reshape(ncls, 2, _REC), ncls, pc,
                           include_background)
