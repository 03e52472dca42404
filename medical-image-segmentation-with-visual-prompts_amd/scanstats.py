"""Scan statistics and data-driven intensity windows on the GPU (csrc/scanstats.hip).

``scan.prepare_scan`` maps intensities through a window the caller must know.  A CT from the reference's data set has one
(-1000..1000); an MR volume, a cone-beam CT or a CT with another rescale intercept does not: its window is a property of its
own histogram, or of its data set's.  This module computes that on the device, with no host read, so that
``prepare -> predict -> post-process -> restore`` stays one recordable sequence.

Definitions (``tests/scanstats_ref.py`` restates them in numpy):

- **Histogram.**  ``raw`` is an int16 or uint8 scan ``[C, H, W, D]``.  ``table[c, v + 32768]`` counts the voxels of channel
  ``c`` with value ``v`` (the same layout for both dtypes) that are *selected*: where ``mask`` (uint8 ``[H, W, D]`` on the
  native grid, shared by the channels; a label map works) is non-zero, and, with ``above``, where ``v > above``
  (``above=0`` is the usual non-zero MR foreground).  The kernel adds to the table, so scans pool into one data-set
  histogram through ``out=``.  Counts are int64, exact and bitwise reproducible.
- **Order statistics.**  ``N`` is the count.  For ``q`` in ``[0, 1]`` the statistic is the ``k``-th smallest selected value
  with ``k = max(1, ceil(q * N))`` (one float64 multiply): ``np.sort(v)[k - 1]``, the *nearest-rank* percentile.  It is
  always a value of the scan.  It is **not** numpy's default ``np.percentile``, which interpolates between neighbours.
- **Moments.**  ``S1 = sum v n_v`` and ``S2 = sum v^2 n_v`` in int64 (exact while ``S2 < 2^63``, which holds for every
  histogram of fewer than 2^33 voxels); ``mean = S1 / N`` and the population ``std = sqrt(max(0, S2 / N - mean^2))`` in
  float64.
- **Window slot.**  Eight fp32 words per channel, ``(s, t, lo, hi, a_lo, a_hi, mean, std)``, each rounded from float64
  once; ``prepare_scan`` applies ``v = clamp(fma(x, s, t), lo, hi)`` per source voxel.

  - ``IntensityWindow.percentile``: ``scan.intensity_map(a_lo, a_hi, b_min, b_max)`` bit for bit, with ``a_lo`` / ``a_hi``
    the order statistics of ``q_lo`` / ``q_hi``.  ``a_hi == a_lo`` (a constant scan, nothing selected): ``s = 0``,
    ``t = b_min``.
  - ``IntensityWindow.zscore``: ``s = 1 / std``, ``t = -mean / std``; ``std == 0`` or ``N == 0``: ``s = 1``, ``t = -mean``
    (``mean = 0`` when ``N == 0``).  With ``clip=(q_lo, q_hi)`` the result is clamped to the images of the two order
    statistics, ``lo = fma(a_lo, s, t)`` and ``hi = fma(a_hi, s, t)`` in fp32; without it ``lo, hi = -FLT_MAX, FLT_MAX``
    and ``a_lo`` / ``a_hi`` are the minimum and the maximum.

The LDS window.  A workgroup counts 16384 consecutive values in LDS and sends any other value to the global table, so the
table is the same for every ``base`` (the lowest value counted in LDS) and only the speed depends on it.  The defaults,
-4096 for int16 (CT in Hounsfield units with its usual padding values, and MR up to 12287) and 0 for uint8, cover real
scans; pass ``base=`` for data that sits elsewhere.

Otsu foreground thresholds (``tests/otsu_ref.py`` restates them in Python integers).  Per channel, with
``N = sum n_v`` and ``S = sum v n_v`` over the table: a candidate ``t`` is a counted value that is not the largest counted
value; ``n0 = sum_{v<=t} n_v``, ``A = sum_{v<=t} v n_v``, ``P = A N - S n0``, ``q = n0 (N - n0)``.  Otsu's between-class
variance is ``P^2 / (N^2 q)``; the threshold is the candidate that maximises ``P^2 / q``, compared in exact integers
(``P_a^2 q_b`` against ``P_b^2 q_a``, 256-bit on the device), equal values picking the lower ``t``.  It is always a value of
the scan, and foreground is ``v > t``.  The record is int64 ``(t, n_le, n_gt, valid)``; fewer than two distinct counted
values, ``N == 0`` or ``N >= 2^33`` give ``valid = 0`` (``t`` = the largest counted value, 0 if none; ``n_le = N``), and
every consumer then applies no restriction: the mask is all ones, the restricted plan is the unrestricted one.
``otsu_slot`` computes the record from a histogram, ``foreground_mask`` the uint8 mask on the native grid,
``window_slot_above`` the plan of a (pooled) histogram over the bins above the threshold (the three live in
``mivp_amd/otsu.py`` and are reachable through this module too), and ``foreground="otsu"`` on a window spec
restricts its statistics the same way -- a restriction on bins, not a second pass over voxels.  ``above=`` still selects what is counted; Otsu acts on what was counted.

Nothing here reads back to the host; ``ScanHistogram.cpu()``, ``WindowSlot.cpu()`` and ``OtsuSlot.cpu()`` are the
synchronising calls.
"""
from __future__ import annotations

import math
import numbers
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import check_gpu, i3

NBINS = 65536
OFFSET = 32768                # bin of value 0
LDS_WINDOW = 16384            # consecutive values a workgroup counts in LDS
FLAG_PER_VALUE = 1            # one atomic per value instead of one per run of equal values (tools/bench_scanstats.py)
MODE_PERCENTILE, MODE_ZSCORE = 0, 1
_DTYPES = {torch.uint8: 0, torch.int16: 4}
_BASE = {torch.uint8: 0, torch.int16: -4096}


def _check_q(name: str, q) -> float:
    if isinstance(q, bool) or not isinstance(q, numbers.Real) or not 0.0 <= float(q) <= 1.0:
        raise ValueError(f"{name} must be a number in [0, 1], got {q!r}")
    return float(q)


def _check_foreground(foreground) -> Optional[str]:
    if foreground is not None and foreground != "otsu":
        raise ValueError(f"foreground must be None or 'otsu', got {foreground!r}")
    return foreground


def _check_channels(channels) -> int:
    if isinstance(channels, bool) or not isinstance(channels, numbers.Integral) or not 1 <= channels <= 4:
        raise ValueError(f"channels must be 1..4, got {channels!r}")
    return int(channels)


def _check_above(above) -> Optional[int]:
    if above is None:
        return None
    if isinstance(above, bool) or not isinstance(above, numbers.Integral) or not -2 ** 31 <= above < 2 ** 31:
        raise ValueError(f"above must be an integer (or None), got {above!r}")
    return int(above)


class ScanReport:
    """Host-side statistics of a ``ScanHistogram``, computed from the exact table: per channel ``count``, ``min``,
    ``max`` (0 where nothing was counted), ``mean``, ``std`` (float64, the module's definitions), ``percentile(q)`` (the
    nearest-rank order statistic) and ``counts`` / ``values``: the dense counts of the occupied range ``min..max``."""

    def __init__(self, table: np.ndarray):
        self.table = np.ascontiguousarray(table, dtype=np.int64)
        self.channels = self.table.shape[0]
        v = np.arange(NBINS, dtype=np.int64) - OFFSET
        self.count = self.table.sum(axis=1)
        self.min = np.zeros(self.channels, dtype=np.int64)
        self.max = np.zeros(self.channels, dtype=np.int64)
        self.mean = np.zeros(self.channels, dtype=np.float64)
        self.std = np.zeros(self.channels, dtype=np.float64)
        self.values: List[np.ndarray] = []
        self.counts: List[np.ndarray] = []
        for c in range(self.channels):
            occ = np.flatnonzero(self.table[c])
            if occ.size == 0:
                self.values.append(np.zeros(0, dtype=np.int64))
                self.counts.append(np.zeros(0, dtype=np.int64))
                continue
            self.min[c], self.max[c] = v[occ[0]], v[occ[-1]]
            self.values.append(v[occ[0]:occ[-1] + 1].copy())
            self.counts.append(self.table[c, occ[0]:occ[-1] + 1].copy())
            n = int(self.count[c])
            s1 = sum(int(a) * int(k) for a, k in zip(v[occ], self.table[c, occ]))      # Python integers: exact
            s2 = sum(int(a) * int(a) * int(k) for a, k in zip(v[occ], self.table[c, occ]))
            self.mean[c] = s1 / n
            self.std[c] = math.sqrt(max(0.0, s2 / n - self.mean[c] * self.mean[c]))

    def percentile(self, q: float) -> np.ndarray:
        """int64 ``[C]``: the ``max(1, ceil(q * N))``-th smallest counted value per channel (0 where ``N == 0``)."""
        q = _check_q("q", q)
        out = np.zeros(self.channels, dtype=np.int64)
        for c in range(self.channels):
            n = int(self.count[c])
            if n:
                k = max(1, int(math.ceil(q * float(n))))
                out[c] = int(np.searchsorted(np.cumsum(self.table[c]), k, side="left")) - OFFSET
        return out

    def otsu(self) -> Dict[str, np.ndarray]:
        """Otsu's threshold per channel from the exact table, in Python integers (the module docstring has the
        definition): ``{"t", "n_le", "n_gt", "valid"}`` int64 ``[C]``, what ``otsu_slot`` writes on the device, and
        ``"eta"`` float64 ``[C]``: the separability ``sigma_b^2 / sigma_total^2`` of the chosen threshold (0 where
        ``valid`` is 0), for reporting."""
        out = {k: np.zeros(self.channels, dtype=np.int64) for k in ("t", "n_le", "n_gt", "valid")}
        out["eta"] = np.zeros(self.channels, dtype=np.float64)
        for c in range(self.channels):
            occ = [(int(b) - OFFSET, int(self.table[c, b])) for b in np.flatnonzero(self.table[c])]
            N = sum(k for _, k in occ)
            S = sum(v * k for v, k in occ)
            out["t"][c], out["n_le"][c] = (occ[-1][0] if occ else 0), N
            if len(occ) < 2 or N >= 2 ** 33:
                continue
            n0, A, best = 0, 0, None                                             # best = (P^2, q, t, n0)
            for v, k in occ[:-1]:
                n0, A = n0 + k, A + v * k
                P, q = A * N - S * n0, n0 * (N - n0)
                if best is None or P * P * best[1] > best[0] * q:               # equal: the lower t stays
                    best = (P * P, q, v, n0)
            S2 = sum(v * v * k for v, k in occ)
            out["t"][c], out["n_le"][c], out["n_gt"][c], out["valid"][c] = best[2], best[3], N - best[3], 1
            out["eta"][c] = float(Fraction(best[0], best[1] * (S2 * N - S * S)))
        return out


class ScanHistogram:
    """The device table int64 ``[C, 65536]`` of one or more scans (``table[c, v + 32768]``)."""

    def __init__(self, channels: int, device):
        self.channels = _check_channels(channels)
        self.table = torch.zeros((self.channels, NBINS), dtype=torch.int64, device=device)

    def zero_(self) -> "ScanHistogram":
        self.table.zero_()
        return self

    def cpu(self) -> ScanReport:
        """The one synchronising call: the table on the host with the statistics derived from it."""
        return ScanReport(self.table.cpu().numpy())


class WindowSlot:
    """The device plan fp32 ``[C, 8]`` of ``window_slot``: ``(s, t, lo, hi, a_lo, a_hi, mean, std)`` per channel."""

    def __init__(self, channels: int, device, mode: int = MODE_PERCENTILE):
        self.channels, self.mode = _check_channels(channels), int(mode)
        self.words = torch.zeros((self.channels, 8), dtype=torch.float32, device=device)

    def cpu(self) -> np.ndarray:
        """The synchronising call: the words as a numpy fp32 ``[C, 8]`` array."""
        return self.words.cpu().numpy()


class OtsuSlot:
    """The device record int64 ``[C, 4]`` of ``otsu_slot``: ``(t, n_le, n_gt, valid)`` per channel."""

    def __init__(self, channels: int, device):
        self.channels = _check_channels(channels)
        self.words = torch.zeros((self.channels, 4), dtype=torch.int64, device=device)

    def cpu(self) -> np.ndarray:
        """The synchronising call: the record as a numpy int64 ``[C, 4]`` array."""
        return self.words.cpu().numpy()


class IntensityWindow:
    """How a scan's window follows from its histogram (the module docstring has the formulas).  A plain spec, built
    through ``IntensityWindow.percentile(...)`` or ``IntensityWindow.zscore(...)``.  It also keeps the histogram and slot
    buffers ``prepare_scan(window=spec)`` works in, one pair per (device, channels), made at the first call: a later
    call, and a graph recording after an eager warm-up, allocates nothing.  Every call with the spec writes those
    buffers, so **a spec serves one stream at a time**: calls that may overlap on different streams need a spec each (or
    their own ``ScanHistogram`` / ``WindowSlot`` through ``scan_histogram`` and ``window_slot``).  ``foreground="otsu"``
    takes the statistics over the counted values above the histogram's own Otsu threshold (one more plan launch; the
    buffers then hold an ``OtsuSlot`` as well)."""

    def __init__(self, mode: int, q_lo: float, q_hi: float, b_min: float, b_max: float, above: Optional[int], clip: bool,
                 foreground: Optional[str] = None):
        self.mode = int(mode)
        self.q_lo, self.q_hi = _check_q("q_lo", q_lo), _check_q("q_hi", q_hi)
        if self.q_lo > self.q_hi:
            raise ValueError(f"q_lo must not exceed q_hi, got q_lo={q_lo}, q_hi={q_hi}")
        self.b_min, self.b_max = float(b_min), float(b_max)
        if not (math.isfinite(self.b_min) and math.isfinite(self.b_max)):
            raise ValueError(f"b_min and b_max must be finite, got {b_min}, {b_max}")
        if self.b_max < self.b_min:
            raise ValueError(f"b_max must not be below b_min, got b_min={b_min}, b_max={b_max}")
        self.above = _check_above(above)
        self.clip = bool(clip)
        self.foreground = _check_foreground(foreground)
        self._buffers: Dict[Tuple[str, int], tuple] = {}

    @classmethod
    def percentile(cls, q_lo: float = 0.005, q_hi: float = 0.995, b_min: float = 0.0, b_max: float = 1.0,
                   above: Optional[int] = None, foreground: Optional[str] = None) -> "IntensityWindow":
        """``[a_lo, a_hi]``, the nearest-rank order statistics of ``q_lo`` and ``q_hi`` over the selected voxels, maps
        linearly to ``[b_min, b_max]``.  ``above``: count only voxels with a value greater than it.  ``foreground``:
        ``None``, or ``"otsu"`` for the counted voxels above their Otsu threshold."""
        return cls(MODE_PERCENTILE, q_lo, q_hi, b_min, b_max, above, True, foreground)

    @classmethod
    def zscore(cls, above: Optional[int] = None, clip: Optional[Tuple[float, float]] = None,
               foreground: Optional[str] = None) -> "IntensityWindow":
        """``(x - mean) / std`` of the selected voxels, with ``clip=(q_lo, q_hi)`` clamped to the images of those two
        order statistics.  ``foreground`` as in ``percentile``."""
        if clip is None:
            return cls(MODE_ZSCORE, 0.0, 1.0, 0.0, 1.0, above, False, foreground)
        try:
            q_lo, q_hi = clip
        except (TypeError, ValueError):
            raise ValueError(f"clip must be (q_lo, q_hi) or None, got {clip!r}") from None
        return cls(MODE_ZSCORE, q_lo, q_hi, 0.0, 1.0, above, True, foreground)

    def buffers(self, channels: int, device) -> tuple:
        """The (histogram, slot) pair ``prepare_scan(window=self)`` uses for scans of ``channels`` channels on
        ``device`` -- (histogram, slot, Otsu record) with ``foreground="otsu"``; call it ahead of a graph recording to
        keep the allocation out of it."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:                              # "cuda" and "cuda:0" are one device
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (str(dev), int(channels))
        if key not in self._buffers:
            bufs = (ScanHistogram(channels, device), WindowSlot(channels, device, self.mode))
            self._buffers[key] = bufs + (OtsuSlot(channels, device),) if self.foreground else bufs
        return self._buffers[key]

    def __repr__(self):
        fg = "" if self.foreground is None else f", foreground={self.foreground!r}"
        if self.mode == MODE_PERCENTILE:
            return (f"IntensityWindow.percentile(q_lo={self.q_lo}, q_hi={self.q_hi}, b_min={self.b_min}, "
                    f"b_max={self.b_max}, above={self.above}{fg})")
        return f"IntensityWindow.zscore(above={self.above}, clip={(self.q_lo, self.q_hi) if self.clip else None}{fg})"


def _check_raw(raw) -> Tuple[int, Tuple[int, int, int]]:
    """[H, W, D], [C, H, W, D] or [1, C, H, W, D], int16 or uint8 -> (channels, spatial shape)."""
    if not isinstance(raw, torch.Tensor):
        raise ValueError(f"raw must be a torch.Tensor, got {type(raw).__name__}")
    if raw.dtype not in _DTYPES:
        raise ValueError(f"a scan histogram takes int16 or uint8 scans, got {raw.dtype}")
    if raw.dim() == 5 and raw.shape[0] != 1 or raw.dim() not in (3, 4, 5):
        raise ValueError(f"raw must be [C, H, W, D] (or [H, W, D] / [1, C, H, W, D]), got {tuple(raw.shape)}")
    shape = tuple(int(s) for s in raw.shape[-3:])
    channels = 1 if raw.dim() == 3 else int(raw.shape[-4])
    if not 1 <= channels <= 4:
        raise ValueError(f"raw must have 1..4 channels, got {channels}")
    if min(shape) < 1 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError(f"a channel must have between 1 and 2^31 - 1 voxels, got {shape}")
    return channels, shape


def _check_mask(mask, shape) -> None:
    if mask is None:
        return
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8:
        raise ValueError("mask must be a uint8 tensor on the scan's native grid")
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"mask has shape {tuple(mask.shape)}, the scan's native grid is {tuple(shape)}")


def scan_histogram(raw: torch.Tensor, mask: Optional[torch.Tensor] = None, above: Optional[int] = None,
                   out: Optional[ScanHistogram] = None, base: Optional[int] = None, flags: int = 0) -> ScanHistogram:
    """The exact histogram of an int16 or uint8 scan (``[C, H, W, D]``, ``[H, W, D]`` or ``[1, C, H, W, D]``, C <= 4) in
    one launch: see the module docstring.  ``mask``: uint8 ``[H, W, D]``, count where non-zero; ``above``: count where
    ``v > above``; both may be given.  ``out=``: add to an earlier histogram (pooling); else a zeroed one is made.
    ``base``: the lowest value of the LDS window (speed only).  No host read."""
    channels, shape = _check_raw(raw)
    _check_mask(mask, shape)
    above = _check_above(above)
    if base is not None and (isinstance(base, bool) or not isinstance(base, numbers.Integral)
                             or not -2 ** 31 <= base < 2 ** 31):
        raise ValueError(f"base must be an integer (or None), got {base!r}")
    if out is not None:
        if not isinstance(out, ScanHistogram):
            raise ValueError(f"out must be a ScanHistogram, got {type(out).__name__}")
        if out.channels != channels:
            raise ValueError(f"out was made for {out.channels} channels, raw has {channels}")
    check_gpu("raw", raw)
    if mask is not None and mask.device != raw.device:
        raise ValueError(f"mask is on {mask.device}, raw on {raw.device}")
    if out is not None and out.table.device != raw.device:
        raise ValueError(f"out is on {out.table.device}, raw on {raw.device}")
    r = raw.contiguous()
    m = None if mask is None else mask.contiguous()
    hist = ScanHistogram(channels, r.device) if out is None else out
    L.call("mivp_scan_hist", L.ptr(r), _DTYPES[r.dtype], channels, i3(shape), L.ptr(m), int(above is not None), above or 0,
           _BASE[r.dtype] if base is None else int(base), int(flags), L.ptr(hist.table), L.stream())
    return hist


def _check_hist(hist) -> ScanHistogram:
    if not isinstance(hist, ScanHistogram):
        raise ValueError(f"hist must be a ScanHistogram, got {type(hist).__name__}")
    return hist


def _check_otsu(otsu, channels: int, device, like: str) -> None:
    if not isinstance(otsu, OtsuSlot):
        raise ValueError(f"otsu must be an OtsuSlot, got {type(otsu).__name__}")
    if otsu.channels != channels:
        raise ValueError(f"otsu was made for {otsu.channels} channels, {like} has {channels}")
    if otsu.words.device != device:
        raise ValueError(f"otsu is on {otsu.words.device}, {like} on {device}")


def window_slot(hist: ScanHistogram, spec: IntensityWindow, out: Optional[WindowSlot] = None) -> WindowSlot:
    """A histogram (of one scan, or pooled over a data set) -> the device plan of ``spec``, in one launch with no host
    read.  ``prepare_scan(window=slot)`` applies it to any scan of that many channels.  (``window_slot_above`` takes
    the plan over the counted values above an Otsu threshold.)"""
    return _plan(hist, spec, out, None)


def _plan(hist, spec, out, otsu) -> WindowSlot:
    """``window_slot`` (``otsu`` None) and ``otsu.window_slot_above``: the checks and the one plan launch."""
    _check_hist(hist)
    if not isinstance(spec, IntensityWindow):
        raise ValueError(f"spec must be an IntensityWindow, got {type(spec).__name__}")
    if out is not None:
        if not isinstance(out, WindowSlot) or out.channels != hist.channels:
            raise ValueError(f"out must be a WindowSlot of {hist.channels} channels")
        if out.words.device != hist.table.device:
            raise ValueError(f"out is on {out.words.device}, hist on {hist.table.device}")
    if otsu is not None:
        _check_otsu(otsu, hist.channels, hist.table.device, "hist")
    if not hist.table.is_cuda:
        raise RuntimeError("hist must live on the GPU (no CPU fallback)")
    slot = WindowSlot(hist.channels, hist.table.device) if out is None else out
    slot.mode = spec.mode
    if otsu is not None:
        L.call("mivp_scan_window_plan_above", L.ptr(hist.table), hist.channels, spec.mode, spec.q_lo, spec.q_hi, spec.b_min,
               spec.b_max, int(spec.clip), L.ptr(otsu.words), L.ptr(slot.words), L.stream())
        return slot
    L.call("mivp_scan_window_plan", L.ptr(hist.table), hist.channels, spec.mode, spec.q_lo, spec.q_hi, spec.b_min, spec.b_max,
           int(spec.clip), L.ptr(slot.words), L.stream())
    return slot


def _is_transfer(window) -> bool:
    """``window=`` is a transfer table or its spec (``mivp_amd.transfer``), not a linear window."""
    from . import transfer
    return isinstance(window, (transfer.IntensityTransfer, transfer.TransferTable))


def check_window_args(window, raw: torch.Tensor, mask, shape) -> None:
    """The host-side checks of ``prepare_scan(window=...)`` (``raw`` already ``[C, H, W, D]``)."""
    if _is_transfer(window):
        from . import transfer
        return transfer.check_transfer_args(window, raw, mask, shape)
    if not isinstance(window, (IntensityWindow, WindowSlot)):
        raise ValueError("window must be an IntensityWindow, a WindowSlot, an IntensityTransfer or a TransferTable, got "
                         f"{type(window).__name__}")
    if raw.dtype not in _DTYPES:
        raise ValueError(f"a data-driven window takes int16 or uint8 scans, got {raw.dtype}")
    if isinstance(window, WindowSlot):
        if mask is not None:
            raise ValueError("mask selects the voxels of a histogram: a WindowSlot is already computed")
        if window.channels != raw.shape[0]:
            raise ValueError(f"window was made for {window.channels} channels, raw has {raw.shape[0]}")
    _check_mask(mask, shape)


def resolve_window(window, raw: torch.Tensor, mask) -> WindowSlot:
    """``prepare_scan``'s device side of ``window=``: a ``WindowSlot`` as it is; an ``IntensityWindow`` runs histogram ->
    plan on ``raw`` itself in the spec's own buffers (a clear and two launches, no host read); with
    ``foreground="otsu"`` histogram -> Otsu plan -> restricted plan (a clear and three launches).  (The transfer types
    of ``_is_transfer`` resolve to a table, not a slot: ``transfer.resolve_table``.)"""
    if isinstance(window, WindowSlot):
        if window.words.device != raw.device:
            raise ValueError(f"window is on {window.words.device}, raw on {raw.device}")
        return window
    hist, slot, *rest = window.buffers(raw.shape[0], raw.device)
    scan_histogram(raw, mask=mask, above=window.above, out=hist.zero_())
    if window.foreground is None:
        return window_slot(hist, window, out=slot)
    from . import otsu
    return otsu.window_slot_above(hist, window, otsu.otsu_slot(hist, out=rest[0]), out=slot)


def __getattr__(name):
    # the Otsu calls live in mivp_amd/otsu.py (which imports this module) and are reachable from here as well
    if name in ("otsu_slot", "foreground_mask", "window_slot_above"):
        from . import otsu
        return getattr(otsu, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
