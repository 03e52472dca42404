"""Fitting the prediction windows to the foreground bounding box: the ``WindowFit`` value object of
``SlidingWindowPredictor(fit=...)`` and ``foreground_box`` (csrc/window_fit.hip).  ``mivp_amd.inference`` re-exports both."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._host import ImmutableValue, check_fill_logit, check_finite, check_gpu, check_int_from, i3, plain_int


class WindowFit(ImmutableValue):
    """How a ``SlidingWindowPredictor(fit=...)`` fits its windows to the foreground.  A voxel of the
    prepared volume is foreground iff ``vol[channel] > threshold`` (strict fp32: NaN is not foreground; the default is
    ``WindowSkip``'s).  The windows tile the foreground's bounding box, grown by ``margin`` voxels per axis (an integer
    or three of them), instead of the whole volume.  Voxels no fitted window covers get the label ``fill_class`` and the
    blended logits ``+fill_logit`` at ``fill_class``, ``-fill_logit`` elsewhere.  ``channel`` and ``fill_class`` are
    checked against the predictor's channel and class counts when it is built.  Immutable."""

    __slots__ = ("threshold", "channel", "margin", "fill_class", "fill_logit")

    def __init__(self, threshold: float = 0.0025, channel: int = 0, margin=0, fill_class: int = 0,
                 fill_logit: float = 10.0):
        check_finite("threshold", threshold)
        check_fill_logit(fill_logit)
        check_int_from("channel", channel, 0)
        check_int_from("fill_class", fill_class, 0)
        if plain_int(margin):
            m = (margin,) * 3
        elif isinstance(margin, (tuple, list, np.ndarray)) and len(margin) == 3:
            m = tuple(margin)
        else:
            raise ValueError(f"margin must be a non-negative integer or three of them, got {margin!r}")
        self._set(threshold=float(threshold), channel=int(channel), margin=tuple(check_int_from("margin", v, 0) for v in m),
                  fill_class=int(fill_class), fill_logit=float(fill_logit))


def foreground_box(vol_or_mask: torch.Tensor, channel: int = 0, threshold: float = 0.0025,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The inclusive bounding box of the foreground as a device int32 ``[6]`` tensor ``(lo0, lo1, lo2, hi0, hi1, hi2)``
    in image coordinates; no foreground gives ``lo = (H, W, D)`` and ``hi = -1``.  An fp32 ``[1, C, H, W, D]`` or
    ``[C, H, W, D]`` volume: foreground is ``vol[channel] > threshold`` (strict fp32, NaN is not foreground).  A uint8
    ``[H, W, D]`` mask: foreground is ``mask != 0`` (``channel`` and ``threshold`` are not used).  ``out``: an int32
    ``[6]`` tensor on the same device to write.  Two launches (csrc/window_fit.hip), no host read: records in a graph."""
    t = vol_or_mask
    check_gpu("vol_or_mask", t)
    if t.dtype == torch.uint8 and t.dim() == 3:
        vol, mask, cin = None, t, 0
    elif t.dtype == torch.float32 and (t.dim() == 4 or (t.dim() == 5 and t.shape[0] == 1)):
        vol, mask = (t[0] if t.dim() == 5 else t), None
        cin = int(vol.shape[0])
        check_finite("threshold", threshold)
        if check_int_from("channel", channel, 0) >= cin:
            raise ValueError(f"channel {channel} is not a channel of a {cin}-channel volume")
    else:
        raise ValueError("foreground_box takes an fp32 [1, C, H, W, D] / [C, H, W, D] volume or a uint8 [H, W, D] mask, "
                         f"got {t.dtype} {tuple(t.shape)}")
    dims = tuple(int(n) for n in t.shape[-3:])
    if min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"the volume must hold 1 .. 2^31 - 1 voxels, got {dims}")
    if not t.is_contiguous():
        raise ValueError("vol_or_mask must be contiguous")
    if out is None:
        out = torch.empty(6, dtype=torch.int32, device=t.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != (6,) \
            or out.device != t.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous int32 [6] tensor on the input's device")
    L.call("mivp_foreground_box", L.ptr(vol), cin, int(channel) if vol is not None else 0,
           float(threshold) if vol is not None else 0.0, L.ptr(mask), i3(dims), L.ptr(out), L.stream())
    return out
