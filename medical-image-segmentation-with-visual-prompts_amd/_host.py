"""Host-side argument checks and small helpers shared by the evaluation modules (``inference``, ``surface``,
``components``, ``regions``, ``calibration``, ``scan``, ``scanstats``, ``skeleton``, ``clicks``, ``geodesic``).  One definition each: a module that needs one
imports it from here, not from a sibling.  Also the two things the predictor's pieces share that are not checks: the
``ImmutableValue`` base of ``WindowSkip`` / ``WindowFit`` and ``channels_last_or_copy``, the layout in which the kernels
read a model's logits.  Nothing here launches a kernel except ``workspace``'s size query."""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

LABEL_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}    # dtype codes of the label kernels
CONNECTIVITY = (6, 18, 26)


def channels_last_or_copy(t: torch.Tensor):
    """``[B, C, ...]`` logits as the kernels read them -> (tensor, channels_last flag): the channels-last view when the
    storage is fp32 channels-last (what the model returns), else an fp32 contiguous channels-first copy."""
    base = t.permute(0, *range(2, t.dim()), 1)
    if base.is_contiguous() and t.dtype == torch.float32:
        return base, 1
    return t.float().contiguous(), 0


def i3(v):
    """Three sizes as the ``int32[3]`` the C ABI takes."""
    return (C.c_int32 * 3)(*[int(a) for a in v])


def plain_int(v) -> bool:
    """An int or a numpy integer, but not a bool."""
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


class ImmutableValue:
    """Base of the small value objects (``WindowSkip``, ``WindowFit``): the fields are the subclass's ``__slots__``, set
    once by ``_set`` in its ``__init__``; immutability, ``repr``, equality and hashing follow from them."""

    __slots__ = ()

    def _set(self, **fields):
        for k in self.__slots__:
            object.__setattr__(self, k, fields[k])

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is immutable")

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={getattr(self, k)}' for k in self.__slots__)})"

    def __eq__(self, other):
        return isinstance(other, type(self)) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))


def check_finite(name: str, v) -> float:
    """A finite int or float (numpy scalars included), but not a bool."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(v)):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def check_at_least(name: str, v, lo: float) -> float:
    """A ``check_finite`` number >= ``lo``."""
    if check_finite(name, v) < lo:
        raise ValueError(f"{name} must be >= {lo:g}, got {v!r}")
    return float(v)


def check_flag(name: str, v) -> bool:
    """A bool (numpy bools included), nothing that merely converts to one."""
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} must be a bool, got {v!r}")
    return bool(v)


def check_int_from(name: str, v, lo: int) -> int:
    """A ``plain_int`` in ``lo .. 2^31 - 1``."""
    if not plain_int(v) or int(v) < lo or int(v) >= 2 ** 31:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return int(v)


def check_fill_logit(v) -> float:
    """The logit magnitude of filled voxels: finite, > 0 and finite in fp32."""
    check_finite("fill_logit", v)
    if not 0 < float(v) <= float(np.finfo(np.float32).max):
        raise ValueError(f"fill_logit must be > 0 and finite in fp32, got {v!r}")
    return float(v)


def check_region_mask(mask, image_size, device):
    """A resident foreground mask of the predictors: a contiguous uint8 ``[H, W, D]`` GPU tensor on ``device``."""
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise ValueError("the region mask must be a GPU tensor (no CPU fallback)")
    if mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(image_size):
        raise ValueError(f"the region mask must be uint8 {tuple(image_size)}, got {mask.dtype} {tuple(mask.shape)}")
    if mask.device != device or not mask.is_contiguous():
        raise ValueError("the region mask must be contiguous and on the model's device")


def check_gpu(name: str, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (no CPU fallback)")


def check_classes(num_classes: int) -> int:
    if not 1 <= int(num_classes) <= 16:
        raise ValueError(f"num_classes must be in 1..16, got {num_classes}")
    return int(num_classes)


def check_spacing(spacing: Sequence[float], name: str = "spacing") -> Tuple[float, float, float]:
    s = tuple(float(a) for a in spacing)
    if len(s) != 3 or not all(math.isfinite(a) and a > 0 for a in s):
        raise ValueError(f"{name} must be three positive sizes in mm, got {tuple(spacing)}")
    return s


def check_connectivity(connectivity) -> int:
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITY:
        raise ValueError(f"connectivity must be one of {CONNECTIVITY}, got {connectivity!r}")
    return int(connectivity)


def class_mask(ncls: int, classes: Optional[Iterable[int]]) -> int:
    """``classes`` (default ``1..ncls-1``; distinct ints, 0 is rejected) as a bit mask."""
    cls = list(range(1, ncls)) if classes is None else list(classes)
    if not cls:
        raise ValueError("classes is empty" + (" (num_classes=1 has no foreground class)" if classes is None else ""))
    for c in cls:
        if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 1 <= c < ncls:
            raise ValueError(f"classes must be ints in 1..{ncls - 1}, got {c!r}")
    if len(set(cls)) != len(cls):
        raise ValueError(f"classes has duplicates: {cls}")
    mask = 0
    for c in cls:
        mask |= 1 << int(c)
    return mask


def check_min_size(min_size) -> int:
    """Component sizes are below 2^31: a larger ``min_size`` removes every component, as 2^31 - 1 does."""
    if isinstance(min_size, bool) or not isinstance(min_size, numbers.Integral) or min_size < 0:
        raise ValueError(f"min_size must be a non-negative int, got {min_size!r}")
    return min(int(min_size), 2 ** 31 - 1)


def label_volume(name: str, t: torch.Tensor) -> torch.Tensor:
    """``[1, 1, H, W, D]`` (or ``[H, W, D]``) GPU class map -> contiguous ``[H, W, D]`` of a dtype in ``LABEL_DTYPES``
    (bool is read as uint8, any other dtype is converted to float32)."""
    check_gpu(name, t)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dim() == 5:
        if t.shape[0] != 1 or t.shape[1] != 1:
            raise ValueError(f"{name} must be [1, 1, H, W, D] (one volume of class indices), got {tuple(t.shape)}")
        t = t[0, 0]
    elif t.dim() != 3:
        raise ValueError(f"{name} must be [1, 1, H, W, D] or [H, W, D], got {tuple(t.shape)}")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{name} has {t.numel()} voxels, the kernels take fewer than 2^31")
    if t.dtype not in LABEL_DTYPES:
        t = t.float()
    return t.contiguous()


def label_batch(name: str, t: torch.Tensor) -> torch.Tensor:
    """``[B, 1, H, W, D]`` (or ``[B, H, W, D]``) GPU class maps -> contiguous ``[B, H, W, D]`` of a dtype in ``LABEL_DTYPES``
    (the conversions of ``label_volume``; fewer than 2^31 voxels per sample)."""
    if not isinstance(t, torch.Tensor) or t.dim() not in (4, 5) or (t.dim() == 5 and t.shape[1] != 1):
        raise ValueError(f"{name} must be [B, 1, H, W, D] or [B, H, W, D] class indices, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    check_gpu(name, t)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dim() == 5:
        t = t[:, 0]
    if t.shape[0] < 1 or min(t.shape[1:]) < 1 or t[0].numel() >= 2 ** 31:
        raise ValueError(f"{name}: {tuple(t.shape)} must hold at least one voxel and fewer than 2^31 per sample")
    if t.dtype not in LABEL_DTYPES:
        t = t.float()
    return t.contiguous()


def check_image_batch(name: str, t, contiguous: bool = True) -> torch.Tensor:
    """A float32 ``[B, C, H, W, D]`` image batch of the prompt encodings (``contiguous``: as the kernels read it)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 5 or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 [B, C, H, W, D] tensor, got "
                         f"{(t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def check_click(name: str, click, dims=None) -> Tuple[int, int, int, int]:
    """One click ``(h, w, d, channel)``: plain ints, coordinates in ``0 .. 65534`` (and inside ``dims`` when given), channel 0
    (positive) or 1 (negative)."""
    try:
        vals = None if isinstance(click, (str, bytes)) else tuple(click)
    except TypeError:
        vals = None
    if vals is None or len(vals) != 4 or not all(plain_int(v) for v in vals):
        raise ValueError(f"{name} must be four integers (h, w, d, channel), got {click!r}")
    if vals[3] not in (0, 1):
        raise ValueError(f"{name}: channel must be 0 (positive) or 1 (negative), got {vals[3]!r}")
    for a in range(3):
        hi = 65535 if dims is None else int(dims[a])
        if not 0 <= vals[a] < hi:
            raise ValueError(f"{name}: coordinate {a} = {vals[a]} is outside 0 .. {hi - 1}")
    return tuple(int(v) for v in vals)


def workspace(kind: str, dims, device) -> torch.Tensor:
    """The uint8 workspace ``mivp_<kind>_ws(dims)`` asks for (at least one byte)."""
    nbytes = int(getattr(L.lib(), f"mivp_{kind}_ws")(i3(dims)))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def iou_dice(counts: torch.Tensor) -> Tuple[float, float]:
    """(mean IoU, mean Dice) in float64 from a ``[C, 3]`` table of (intersection, predicted, target) counts (utils.py:14-64);
    a device table costs the one host read."""
    c = counts.to(torch.float64).cpu()
    inter, psum, tsum = c[:, 0], c[:, 1], c[:, 2]
    iou = (inter / (psum + tsum - inter + 1e-6)).mean()
    dice = (2 * inter / (psum + tsum + 1e-6)).mean()
    return float(iou), float(dice)
