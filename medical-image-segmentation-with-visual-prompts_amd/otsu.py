"""Otsu foreground thresholds from the device scan histogram (csrc/scanstats.hip): the launches behind
``scanstats.otsu_slot`` / ``foreground_mask`` / ``window_slot_above``.  ``mivp_amd.scanstats`` has the definitions, the
``OtsuSlot`` record and the window specs that use them (``IntensityWindow(..., foreground="otsu")``); the three calls are
reachable from there as well.  Nothing here reads back to the host."""
from __future__ import annotations

import numbers
from typing import Optional

import torch

from . import _lib as L
from ._host import check_gpu, i3
from .scanstats import (_DTYPES, IntensityWindow, OtsuSlot, ScanHistogram, WindowSlot, _check_hist, _check_otsu, _check_raw,
                        _plan)


def otsu_slot(hist: ScanHistogram, out: Optional[OtsuSlot] = None) -> OtsuSlot:
    """A histogram (of one scan, or pooled) -> the device record ``(t, n_le, n_gt, valid)`` of its Otsu threshold per
    channel (``mivp_amd.scanstats`` has the definition), in one launch with no host read."""
    _check_hist(hist)
    if out is not None:
        if not isinstance(out, OtsuSlot) or out.channels != hist.channels:
            raise ValueError(f"out must be an OtsuSlot of {hist.channels} channels")
        if out.words.device != hist.table.device:
            raise ValueError(f"out is on {out.words.device}, hist on {hist.table.device}")
    if not hist.table.is_cuda:
        raise RuntimeError("hist must live on the GPU (no CPU fallback)")
    slot = OtsuSlot(hist.channels, hist.table.device) if out is None else out
    L.call("mivp_scan_otsu_plan", L.ptr(hist.table), hist.channels, L.ptr(slot.words), L.stream())
    return slot


def foreground_mask(raw: torch.Tensor, otsu: OtsuSlot, channel: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 ``[H, W, D]`` on the scan's native grid: ``raw[channel] > t`` with ``t`` read from the device record (all
    ones where the record is not valid), in one launch with no host read.  ``raw`` as in ``scan_histogram``."""
    channels, shape = _check_raw(raw)
    if isinstance(channel, bool) or not isinstance(channel, numbers.Integral) or not 0 <= channel < channels:
        raise ValueError(f"channel must be one of the scan's {channels} channels, got {channel!r}")
    _check_otsu(otsu, channels, raw.device, "raw")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape:
            raise ValueError(f"out must be a uint8 tensor of shape {shape}")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
        if out.device != raw.device:
            raise ValueError(f"out is on {out.device}, raw on {raw.device}")
    check_gpu("raw", raw)
    r = raw.contiguous()
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=r.device)
    L.call("mivp_scan_threshold_mask", L.ptr(r), _DTYPES[r.dtype], channels, i3(shape), int(channel), L.ptr(otsu.words),
           L.ptr(out), L.stream())
    return out


def window_slot_above(hist: ScanHistogram, spec: IntensityWindow, otsu: OtsuSlot,
                      out: Optional[WindowSlot] = None) -> WindowSlot:
    """``window_slot(hist, spec, out)`` taken over the counted values above the threshold of ``otsu`` (the record of
    ``otsu_slot(hist)``, of this histogram or of a pooled one) where it is valid, and over all of them where it is not:
    one launch, no host read."""
    if otsu is None:
        raise ValueError("otsu must be an OtsuSlot, got None")
    return _plan(hist, spec, out, otsu)
