"""Connected-component labelling and label-map post-processing on the GPU (csrc/components.hip).

Definitions (MONAI is not a dependency here, so the conventions are written out rather than pinned to it):

- **Layout.**  A volume is ``[1, 1, H, W, D]`` or ``[H, W, D]``, contiguous ``[H][W][D]`` with D fastest (the layout of
  ``mivp_amd.surface``), with fewer than 2^31 voxels.  uint8, int32, int64 and float32 are read as they are, bool as
  uint8; other dtypes are converted to float32 first.
- **Adjacency.**  ``connectivity`` 6, 18 or 26 is ``scipy.ndimage.generate_binary_structure(3, k)`` for k = 1, 2, 3.  Two
  adjacent voxels are joined when they hold the **same nonzero value** (for a 0/1 mask this is exactly
  ``scipy.ndimage.label(mask, structure)``; a float NaN equals nothing, so each NaN voxel is a component of its own).
- **Numbering.**  Components are numbered 1..n in the raster (C) order of each component's first voxel; 0 is
  background.  This is scipy's numbering, so labels compare with ``scipy.ndimage.label`` bit for bit.
- **Post-processing** of a class map with ``num_classes`` C (1..16), ``classes`` (default ``1..C-1``; 0 is rejected),
  ``min_size >= 0``, ``largest`` and ``connectivity`` (default 26): a component of a class in ``classes`` is kept iff its
  size is ``>= min_size`` and, when ``largest``, it is that class's largest component, ties going to the component whose
  first voxel comes first in raster order.  Removed voxels become 0.  Voxels of other classes, values outside
  ``[0, C)`` and non-integer floats are never changed.  The output has the input's dtype and shape; the input is not
  modified.

Everything runs on the device in integer arithmetic (bitwise reproducible): a union-find whose roots are always the
minimum linear index of their component (tile-local unions in LDS, lock-free atomicMin unions across tile faces, one
compression pass), then either a device-wide scan that ranks the roots (labelling) or per-root sizes, a per-class best
root and one filter pass (post-processing).  ``postprocess_labels`` makes no host read and can be recorded in a
``torch.cuda.graph``.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Tuple

import torch

from . import _lib as L
from ._host import CONNECTIVITY  # noqa: F401  (public here since the module was written)
from ._host import (LABEL_DTYPES, check_classes, check_connectivity, check_gpu, check_min_size, class_mask, i3,
                    label_volume, workspace)

_check_connectivity = check_connectivity      # the name tests/test_components_host.py imports


def _check_post_args(num_classes, largest=True, min_size=0, classes: Optional[Iterable[int]] = None,
                     connectivity=26) -> Tuple[int, int, int, bool, int]:
    """Validate the post-processing arguments -> (num_classes, class bit mask, min_size, largest, connectivity)."""
    ncls = check_classes(num_classes)
    min_size = check_min_size(min_size)
    if not isinstance(largest, bool):
        raise ValueError(f"largest must be a bool, got {largest!r}")
    if not largest and min_size == 0:
        raise ValueError("largest=False with min_size=0 keeps every component: nothing to do")
    conn = check_connectivity(connectivity)
    return ncls, class_mask(ncls, classes), min_size, largest, conn


def label_components(x: torch.Tensor, connectivity: int = 6) -> Tuple[torch.Tensor, int]:
    """Label the connected components of ``x`` (``[1, 1, H, W, D]`` or ``[H, W, D]`` GPU tensor; voxels holding the same
    nonzero value are joined): ``(labels, n)`` with ``labels`` int32 of x's shape numbered 1..n as
    ``scipy.ndimage.label`` numbers them (the module docstring), 0 on background.  ``n`` is a Python int: reading it is
    the one host synchronisation of this call."""
    conn = check_connectivity(connectivity)
    v = label_volume("x", x)
    dims = tuple(v.shape)
    labels = torch.empty(dims, dtype=torch.int32, device=v.device)
    n = torch.empty(1, dtype=torch.int32, device=v.device)
    ws = workspace("label", dims, v.device)
    L.call("mivp_label_components", L.ptr(v), LABEL_DTYPES[v.dtype], i3(dims), conn, L.ptr(labels), L.ptr(n), L.ptr(ws),
           L.stream())
    return labels.reshape(x.shape), int(n.item())


def _postprocess_launch(v: torch.Tensor, out: torch.Tensor, args, ws: Optional[torch.Tensor] = None,
                        target: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Launch the post-processing of the prepared ``[H, W, D]`` map ``v`` into ``out`` (may be ``v``); ``args`` from
    ``_check_post_args``; ``target`` float32 ``[H, W, D]`` with ``counts`` int64 ``[C, 3]`` adds the Dice / IoU counts of
    ``out``.  Returns the workspace (reusable for the same shape)."""
    ncls, mask, min_size, largest, conn = args
    dims = tuple(v.shape)
    if ws is None:
        ws = workspace("postprocess", dims, v.device)
    L.call("mivp_postprocess_labels", L.ptr(v), LABEL_DTYPES[v.dtype], i3(dims), ncls, mask, min_size, int(largest), conn,
           L.ptr(out), L.ptr(target), L.ptr(counts), L.ptr(ws), L.stream())
    return ws


def postprocess_labels(labels: torch.Tensor, num_classes: int, largest: bool = True, min_size: int = 0,
                       classes: Optional[Iterable[int]] = None, connectivity: int = 26) -> torch.Tensor:
    """Keep the largest connected component of each class in ``classes`` and / or remove its components smaller than
    ``min_size`` voxels (the module docstring has the exact rule).  ``labels`` is a ``[1, 1, H, W, D]`` or ``[H, W, D]``
    GPU class map; the result is a new tensor of its dtype and shape.  No host synchronisation (graph-capturable)."""
    check_gpu("labels", labels)
    args = _check_post_args(num_classes, largest, min_size, classes, connectivity)
    v = label_volume("labels", labels)
    out = torch.empty_like(v)
    _postprocess_launch(v, out, args)
    if labels.dtype == torch.bool:
        out = out.view(torch.bool)
    elif out.dtype != labels.dtype:
        out = out.to(labels.dtype)
    return out.reshape(labels.shape)


def postprocess_kwargs(postprocess: Optional[Dict], num_classes: int):
    """The predictor's ``postprocess`` dict (``postprocess_labels`` keyword arguments) -> checked ``_check_post_args``
    tuple for its ``num_classes``, or None."""
    if postprocess is None:
        return None
    if not isinstance(postprocess, dict):
        raise ValueError(f"postprocess must be a dict of postprocess_labels keyword arguments or None, got "
                         f"{type(postprocess).__name__}")
    kw = dict(postprocess)
    if "num_classes" in kw:
        if kw.pop("num_classes") != num_classes:
            raise ValueError(f"postprocess num_classes {postprocess['num_classes']} differs from the predictor's "
                             f"{num_classes}")
    unknown = set(kw) - {"largest", "min_size", "classes", "connectivity"}
    if unknown:
        raise ValueError(f"postprocess has unknown keys {sorted(unknown)}")
    return _check_post_args(num_classes, **kw)
