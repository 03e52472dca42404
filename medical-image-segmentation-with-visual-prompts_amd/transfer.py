"""Intensity transfer tables on the GPU: histogram equalisation, histogram matching and Nyul-Udupa landmark
standardisation (csrc/scan_transfer.hip).

``mivp_amd.scanstats`` derives a *window* from a scan's histogram: one linear map per channel.  MR volumes, cone-beam CT and
multi-site sets need more: the same tissue sits at different, non-linearly related intensities from scanner to scanner.
What runs in front of a segmentation model for such data is a per-value, monotone, non-linear map taken from the histogram.
This module builds that map as a table on the device, from the exact histogram that is already there, and applies it with
one streaming launch, so that ``prepare -> predict -> post-process -> restore`` stays one recordable, read-free sequence.

Definitions (``tests/transfer_ref.py`` restates them in numpy and Python integers).  A histogram is a ``ScanHistogram``
(int64 ``[C, 65536]``, the bin of value ``v`` at ``v + 32768``); ``n_v`` is the count of ``v``, ``C(v) = sum_{w <= v} n_w``,
``N = C(32767)``, a *counted* value has ``n_v > 0``.  With an ``OtsuSlot`` whose valid word is set the bins at or below its
threshold read as zero everywhere below (the rule of ``window_slot_above``).  A **table** is fp32 ``[C, 65536]``:
``table[c, v + 32768]`` is the model-input intensity of raw value ``v``, defined for every ``v``.  It carries the int32
``[C, 4]`` **meta** record (lowest counted value, highest counted value, valid, 0), both values 0 when nothing is counted.
Every float64 operation below rounds on its own; the result rounds to float32 once.

- **Equalise** ``(b_min, b_max)``.  ``v0`` the lowest counted value, ``c0 = n_v0``, ``d = N - c0``;
  ``r = max(C(v) - c0, 0) / d`` (0 when ``d == 0``); ``y = r * (b_max - b_min) + b_min``.
- **Match** (reference histogram, reference ``WindowSlot``, ``clip``).  ``u(v)`` is the smallest value ``u`` with
  ``C_ref(u) * N_src >= max(C_src(v), 1) * N_ref``, compared in integers; ``N_src == 0`` or ``N_ref == 0``: ``u(v) = v``; a
  histogram with ``N >= 2^33``: the same and ``valid = 0``.  Then the prepare launch's own map, ``y = fmaf((float)u, s, t)``
  clamped to ``[lo, hi]`` with ``clip``, from the words of the reference slot: matching a scan to its own histogram
  reproduces ``prepare_scan(window=slot)`` bit for bit.
- **Landmarks** (Nyul-Udupa).  Quantiles ``q_0 < ... < q_{n-1}`` in ``[0, 1]``, ``2 <= n <= 16``; ``m_i`` is the
  nearest-rank order statistic of ``q_i`` (``k = max(1, ceil(q * N))``, this package's rank rule).  A scan's record is int64
  ``[C, 17]`` = (valid, ``m_0 .. m_{n-1}``, zero padded), valid when ``N > 0`` and ``m_{n-1} > m_0``.  A ``LandmarkBank``
  (float64 ``[C, 17]`` = (count, sums)) learns the standard scale: a valid record adds 1 and
  ``s_lo + (m_i - m_0) / (m_{n-1} - m_0) * (s_hi - s_lo)``; ``S_i = sum_i / count``.  The knots are the distinct ``m_i`` in
  increasing order, a knot's standard value the mean of the ``S_i`` that share it.  With knots ``(M_j, T_j)``, ``j < K``,
  segment ``j`` serves ``M_j <= v < M_{j+1}``, segment 0 everything below and segment ``K - 2`` everything from ``M_{K-1}``
  on (both ends extrapolate): ``y = T_j + (v - M_j) / (M_{j+1} - M_j) * (T_{j+1} - T_j)``, with ``clip`` clamped to
  ``[T_0, T_{K-1}]``.  ``K < 2``: the single knot's value everywhere (0 when ``N == 0``); an empty bank: 0 everywhere and
  ``valid = 0``.
- **Apply.**  ``out[c][e] = table[c][raw[c][e] + 32768]``: int16 or uint8 ``[C, H, W, D]`` in, fp32 on the same grid out.

``prepare_scan(raw, geom, window=X)`` takes an ``IntensityTransfer`` spec or a ``TransferTable`` as ``X``: clear, histogram,
[Otsu plan], [landmarks], table plan, apply into an fp32 workspace the geometry keeps, then the existing float32 prepare
launch with the identity map.  Nothing reads back to the host; ``TransferTable.cpu()``, ``LandmarkSlot.cpu()`` and
``LandmarkBank.cpu()`` are the synchronising calls.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import scanstats as S
from ._host import check_gpu, i3

DEFAULT_Q = (0.01, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.99)
MAX_LANDMARKS = 16
LM_WORDS = 1 + MAX_LANDMARKS
FLAG_GLOBAL = 1               # apply_table: gather every value from the table in global memory (tools/bench_transfer.py)
MODE_EQUALIZE, MODE_MATCH, MODE_LANDMARKS = 0, 1, 2


def _check_quantiles(quantiles) -> Tuple[float, ...]:
    try:
        q = tuple(quantiles)
    except TypeError:
        raise ValueError(f"quantiles must be 2..{MAX_LANDMARKS} numbers, got {quantiles!r}") from None
    if not 2 <= len(q) <= MAX_LANDMARKS:
        raise ValueError(f"quantiles must be 2..{MAX_LANDMARKS} numbers, got {len(q)}")
    q = tuple(S._check_q("a quantile", x) for x in q)
    if any(b <= a for a, b in zip(q, q[1:])):
        raise ValueError(f"quantiles must be strictly increasing, got {q}")
    return q


def _check_range(lo_name: str, lo, hi_name: str, hi) -> Tuple[float, float]:
    for name, x in ((lo_name, lo), (hi_name, hi)):
        if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(float(x)):
            raise ValueError(f"{lo_name} and {hi_name} must be finite numbers, got {name}={x!r}")
    if float(hi) < float(lo):
        raise ValueError(f"{hi_name} must not be below {lo_name}, got {lo_name}={lo}, {hi_name}={hi}")
    return float(lo), float(hi)


def _same_device(name: str, t: torch.Tensor, like_name: str, like: torch.Tensor) -> None:
    if t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, {like_name} on {like.device}")


def _need_gpu(name: str, t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (no CPU fallback)")


class TransferTable:
    """A device table fp32 ``[C, 65536]`` (``table[c, v + 32768]``) with its meta record int32 ``[C, 4]`` = (lowest counted
    value, highest counted value, valid, 0)."""

    def __init__(self, channels: int, device):
        self.channels = S._check_channels(channels)
        self.table = torch.zeros((self.channels, S.NBINS), dtype=torch.float32, device=device)
        self.meta = torch.zeros((self.channels, 4), dtype=torch.int32, device=device)

    def cpu(self) -> Tuple[np.ndarray, np.ndarray]:
        """The synchronising call: (table fp32 ``[C, 65536]``, meta int32 ``[C, 4]``) as numpy arrays."""
        return self.table.cpu().numpy(), self.meta.cpu().numpy()


class LandmarkSlot:
    """One scan's landmark record on the device: int64 ``[C, 17]`` = (valid, ``m_0 .. m_{n-1}``, zero padded), for the
    ``quantiles`` it was taken at.  ``hist`` / ``otsu`` are the histogram (and the Otsu record) ``scan_landmarks`` read:
    ``landmark_table`` takes ``N`` and the two values of the table's meta record from them, so they must still hold that
    scan when it runs."""

    def __init__(self, channels: int, device, quantiles=DEFAULT_Q):
        self.channels = S._check_channels(channels)
        self.quantiles = _check_quantiles(quantiles)
        self.words = torch.zeros((self.channels, LM_WORDS), dtype=torch.int64, device=device)
        self.hist: Optional[S.ScanHistogram] = None
        self.otsu: Optional[S.OtsuSlot] = None

    def cpu(self) -> np.ndarray:
        """The synchronising call: the record as a numpy int64 ``[C, 17]`` array."""
        return self.words.cpu().numpy()


class LandmarkBank:
    """The standard scale of the landmark method, learnt on the device: float64 ``[C, 17]`` = (count, ``sum_0 ..
    sum_{n-1}``, zero padded); the standard landmarks are ``sum_i / count``.  ``words`` is a plain tensor: save it, and hand
    it back through ``words=`` (it is used as it is, not copied).  ``add_scan`` works in buffers the bank keeps, so a bank
    serves one stream at a time."""

    def __init__(self, channels: int, quantiles=DEFAULT_Q, s_lo: float = 0.0, s_hi: float = 1.0, device="cuda",
                 words: Optional[torch.Tensor] = None):
        self.channels = S._check_channels(channels)
        self.quantiles = _check_quantiles(quantiles)
        self.s_lo, self.s_hi = _check_range("s_lo", s_lo, "s_hi", s_hi)
        if words is None:
            words = torch.zeros((self.channels, LM_WORDS), dtype=torch.float64, device=device)
        elif (not isinstance(words, torch.Tensor) or words.dtype != torch.float64
              or tuple(words.shape) != (self.channels, LM_WORDS) or not words.is_contiguous()):
            raise ValueError(f"words must be a contiguous float64 tensor of shape {(self.channels, LM_WORDS)}")
        self.words = words
        self._work: Optional[tuple] = None

    def zero_(self) -> "LandmarkBank":
        self.words.zero_()
        return self

    def cpu(self) -> np.ndarray:
        """The synchronising call: the words as a numpy float64 ``[C, 17]`` array (``[:, 0]`` is the number of scans)."""
        return self.words.cpu().numpy()

    def add(self, landmarks: LandmarkSlot) -> "LandmarkBank":
        """Add one scan's record (an invalid one adds nothing): one tiny launch, no host read."""
        _check_landmarks(landmarks, self)
        _need_gpu("the bank", self.words)
        L.call("mivp_scan_landmark_bank_add", L.ptr(landmarks.words), self.channels, len(self.quantiles), self.s_lo,
               self.s_hi, L.ptr(self.words), L.stream())
        return self

    def add_scan(self, raw: torch.Tensor, mask: Optional[torch.Tensor] = None, above: Optional[int] = None,
                 foreground: Optional[str] = None) -> "LandmarkBank":
        """histogram -> [Otsu plan] -> landmarks -> add, with no host read.  ``raw``, ``mask``, ``above`` as in
        ``scan_histogram``; ``foreground``: ``None`` or ``"otsu"``."""
        channels, _ = S._check_raw(raw)
        if channels != self.channels:
            raise ValueError(f"the bank was made for {self.channels} channels, raw has {channels}")
        S._check_foreground(foreground)
        check_gpu("raw", raw)
        _same_device("the bank", self.words, "raw", raw)
        if self._work is None:
            self._work = (S.ScanHistogram(channels, raw.device), S.OtsuSlot(channels, raw.device),
                          LandmarkSlot(channels, raw.device, self.quantiles))
        hist, otsu, lm = self._work
        S.scan_histogram(raw, mask=mask, above=above, out=hist.zero_())
        rec = None
        if foreground:
            from . import otsu as O
            rec = O.otsu_slot(hist, out=otsu)
        return self.add(scan_landmarks(hist, self.quantiles, otsu=rec, out=lm))


def _check_landmarks(landmarks, bank: LandmarkBank) -> None:
    if not isinstance(landmarks, LandmarkSlot):
        raise ValueError(f"landmarks must be a LandmarkSlot, got {type(landmarks).__name__}")
    if not isinstance(bank, LandmarkBank):
        raise ValueError(f"bank must be a LandmarkBank, got {type(bank).__name__}")
    if landmarks.channels != bank.channels:
        raise ValueError(f"landmarks were made for {landmarks.channels} channels, the bank for {bank.channels}")
    if landmarks.quantiles != bank.quantiles:
        raise ValueError(f"landmarks were taken at quantiles {landmarks.quantiles}, the bank holds {bank.quantiles}")
    _same_device("landmarks", landmarks.words, "the bank", bank.words)


def _check_table_out(out, hist: S.ScanHistogram) -> None:
    if out is None:
        return
    if not isinstance(out, TransferTable) or out.channels != hist.channels:
        raise ValueError(f"out must be a TransferTable of {hist.channels} channels")
    _same_device("out", out.table, "hist", hist.table)


def _check_otsu(otsu, hist: S.ScanHistogram) -> None:
    if otsu is not None:
        S._check_otsu(otsu, hist.channels, hist.table.device, "hist")


def equalize_table(hist: S.ScanHistogram, b_min: float = 0.0, b_max: float = 1.0, otsu: Optional[S.OtsuSlot] = None,
                   out: Optional[TransferTable] = None) -> TransferTable:
    """A histogram (of one scan, or pooled) -> the equalisation table onto ``[b_min, b_max]`` (the module docstring), in
    one launch with no host read.  ``otsu``: restrict to the counted values above its threshold."""
    S._check_hist(hist)
    b_min, b_max = _check_range("b_min", b_min, "b_max", b_max)
    _check_otsu(otsu, hist)
    _check_table_out(out, hist)
    _need_gpu("hist", hist.table)
    tab = TransferTable(hist.channels, hist.table.device) if out is None else out
    L.call("mivp_scan_transfer_equalize", L.ptr(hist.table), hist.channels, b_min, b_max,
           None if otsu is None else L.ptr(otsu.words), L.ptr(tab.table), L.ptr(tab.meta), L.stream())
    return tab


def match_table(hist: S.ScanHistogram, ref_hist: S.ScanHistogram, ref_slot: S.WindowSlot, clip: bool = True,
                otsu: Optional[S.OtsuSlot] = None, out: Optional[TransferTable] = None) -> TransferTable:
    """The table that matches ``hist`` to the reference histogram ``ref_hist`` and then applies the window ``ref_slot``
    (``window_slot`` of ``ref_hist``), in one launch with no host read.  ``otsu`` restricts ``hist``."""
    S._check_hist(hist)
    if not isinstance(ref_hist, S.ScanHistogram):
        raise ValueError(f"ref_hist must be a ScanHistogram, got {type(ref_hist).__name__}")
    if not isinstance(ref_slot, S.WindowSlot):
        raise ValueError(f"ref_slot must be a WindowSlot, got {type(ref_slot).__name__}")
    if ref_hist.channels != hist.channels or ref_slot.channels != hist.channels:
        raise ValueError(f"hist has {hist.channels} channels, ref_hist {ref_hist.channels}, ref_slot {ref_slot.channels}")
    _same_device("ref_hist", ref_hist.table, "hist", hist.table)
    _same_device("ref_slot", ref_slot.words, "hist", hist.table)
    _check_otsu(otsu, hist)
    _check_table_out(out, hist)
    _need_gpu("hist", hist.table)
    tab = TransferTable(hist.channels, hist.table.device) if out is None else out
    L.call("mivp_scan_transfer_match", L.ptr(hist.table), L.ptr(ref_hist.table), L.ptr(ref_slot.words), hist.channels,
           int(bool(clip)), None if otsu is None else L.ptr(otsu.words), L.ptr(tab.table), L.ptr(tab.meta), L.stream())
    return tab


def scan_landmarks(hist: S.ScanHistogram, quantiles=DEFAULT_Q, otsu: Optional[S.OtsuSlot] = None,
                   out: Optional[LandmarkSlot] = None) -> LandmarkSlot:
    """A histogram -> its landmark record at ``quantiles`` (nearest-rank order statistics), in one launch with no host
    read.  The slot remembers ``hist`` and ``otsu`` for ``landmark_table``."""
    S._check_hist(hist)
    q = _check_quantiles(quantiles)
    _check_otsu(otsu, hist)
    if out is not None:
        if not isinstance(out, LandmarkSlot) or out.channels != hist.channels:
            raise ValueError(f"out must be a LandmarkSlot of {hist.channels} channels")
        _same_device("out", out.words, "hist", hist.table)
    _need_gpu("hist", hist.table)
    lm = LandmarkSlot(hist.channels, hist.table.device, q) if out is None else out
    lm.quantiles, lm.hist, lm.otsu = q, hist, otsu
    qs = (C.c_double * len(q))(*q)
    L.call("mivp_scan_landmarks", L.ptr(hist.table), hist.channels, qs, len(q), None if otsu is None else L.ptr(otsu.words),
           L.ptr(lm.words), L.stream())
    return lm


def landmark_table(landmarks: LandmarkSlot, bank: LandmarkBank, clip: bool = False,
                   out: Optional[TransferTable] = None) -> TransferTable:
    """A scan's landmark record and the learnt standard scale -> the piecewise-linear table, in one launch with no host
    read.  ``clip``: clamp to the standard values of the outer knots instead of extrapolating."""
    _check_landmarks(landmarks, bank)
    hist = landmarks.hist
    if hist is None:
        raise ValueError("landmarks hold no record yet: they come from scan_landmarks")
    _check_table_out(out, hist)
    _need_gpu("landmarks", landmarks.words)
    tab = TransferTable(hist.channels, hist.table.device) if out is None else out
    L.call("mivp_scan_transfer_landmarks", L.ptr(hist.table), L.ptr(landmarks.words), L.ptr(bank.words), hist.channels,
           len(bank.quantiles), int(bool(clip)), None if landmarks.otsu is None else L.ptr(landmarks.otsu.words),
           L.ptr(tab.table), L.ptr(tab.meta), L.stream())
    return tab


def apply_table(raw: torch.Tensor, table: TransferTable, out: Optional[torch.Tensor] = None, flags: int = 0) -> torch.Tensor:
    """``out[c] = table[c][raw[c] + 32768]``: an int16 or uint8 scan (``[C, H, W, D]``, ``[H, W, D]`` or
    ``[1, C, H, W, D]``, C <= 4) -> fp32 ``[C, H, W, D]`` on the same grid, in one streaming launch.  ``flags``: 0 gathers
    from an LDS copy of the counted range of the table, ``FLAG_GLOBAL`` from the table in global memory; the same bits."""
    channels, shape = S._check_raw(raw)
    if not isinstance(table, TransferTable):
        raise ValueError(f"table must be a TransferTable, got {type(table).__name__}")
    if table.channels != channels:
        raise ValueError(f"table was made for {table.channels} channels, raw has {channels}")
    if isinstance(flags, bool) or not isinstance(flags, numbers.Integral) or flags & ~FLAG_GLOBAL:
        raise ValueError(f"flags must be 0 or FLAG_GLOBAL, got {flags!r}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (channels,) + shape:
            raise ValueError(f"out must be a float32 tensor of shape {(channels,) + shape}")
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
        _same_device("out", out, "raw", raw)
    check_gpu("raw", raw)
    _same_device("table", table.table, "raw", raw)
    r = raw.contiguous()
    if out is None:
        out = torch.empty((channels,) + shape, dtype=torch.float32, device=r.device)
    L.call("mivp_scan_transfer_apply", L.ptr(r), S._DTYPES[r.dtype], channels, i3(shape), L.ptr(table.table),
           L.ptr(table.meta), int(flags), L.ptr(out), L.stream())
    return out


class IntensityTransfer:
    """How a scan's transfer table follows from its histogram: a plain spec, built through ``IntensityTransfer.equalize``,
    ``.match`` or ``.landmarks``, for ``prepare_scan(window=spec)`` (and ``predict_scan`` / ``evaluate_scan`` /
    ``predict_scan_volume`` through their intensity keywords).  Like ``IntensityWindow`` it keeps the device buffers it
    works in, one set per (device, channels), made at the first call: a later call, and a graph recording after an eager
    warm-up, allocates nothing.  Every call writes those buffers, so **a spec serves one stream at a time**."""

    def __init__(self, mode: int, above: Optional[int], foreground: Optional[str], clip: bool = False, b_min: float = 0.0,
                 b_max: float = 1.0, ref_hist=None, ref_window=None, bank=None):
        self.mode = int(mode)
        self.above = S._check_above(above)
        self.foreground = S._check_foreground(foreground)
        self.clip = bool(clip)
        self.b_min, self.b_max = b_min, b_max
        self.ref_hist, self.ref_window, self.bank = ref_hist, ref_window, bank
        self._ref_slot: Optional[S.WindowSlot] = ref_window if isinstance(ref_window, S.WindowSlot) else None
        self._buffers: Dict[Tuple[str, int], tuple] = {}

    @classmethod
    def equalize(cls, b_min: float = 0.0, b_max: float = 1.0, above: Optional[int] = None,
                 foreground: Optional[str] = None) -> "IntensityTransfer":
        """Histogram equalisation of the selected voxels onto ``[b_min, b_max]``.  ``above``: count only voxels with a
        value greater than it; ``foreground``: ``None``, or ``"otsu"`` for the counted voxels above their Otsu threshold."""
        b_min, b_max = _check_range("b_min", b_min, "b_max", b_max)
        return cls(MODE_EQUALIZE, above, foreground, b_min=b_min, b_max=b_max)

    @classmethod
    def match(cls, ref_hist: S.ScanHistogram, ref_window, clip: bool = True, above: Optional[int] = None,
              foreground: Optional[str] = None) -> "IntensityTransfer":
        """Histogram matching to ``ref_hist`` (a template's or a data set's histogram), followed by the window
        ``ref_window`` of the reference: an ``IntensityWindow`` spec, planned on ``ref_hist`` once at the first call, or a
        ``WindowSlot``.  ``clip`` as in ``prepare_scan``; ``above`` / ``foreground`` select what the scan counts."""
        if not isinstance(ref_hist, S.ScanHistogram):
            raise ValueError(f"ref_hist must be a ScanHistogram, got {type(ref_hist).__name__}")
        if not isinstance(ref_window, (S.IntensityWindow, S.WindowSlot)):
            raise ValueError(f"ref_window must be an IntensityWindow or a WindowSlot, got {type(ref_window).__name__}")
        if isinstance(ref_window, S.WindowSlot):
            if ref_window.channels != ref_hist.channels:
                raise ValueError(f"ref_window was made for {ref_window.channels} channels, ref_hist for {ref_hist.channels}")
            _same_device("ref_window", ref_window.words, "ref_hist", ref_hist.table)
        return cls(MODE_MATCH, above, foreground, clip=clip, ref_hist=ref_hist, ref_window=ref_window)

    @classmethod
    def landmarks(cls, bank: LandmarkBank, clip: bool = False, above: Optional[int] = None,
                  foreground: Optional[str] = None) -> "IntensityTransfer":
        """Nyul-Udupa standardisation onto the scale ``bank`` has learnt, at the bank's quantiles.  ``clip``: clamp to the
        outer standard landmarks instead of extrapolating (the method extrapolates)."""
        if not isinstance(bank, LandmarkBank):
            raise ValueError(f"bank must be a LandmarkBank, got {type(bank).__name__}")
        return cls(MODE_LANDMARKS, above, foreground, clip=clip, bank=bank)

    @property
    def channels(self) -> Optional[int]:
        """The number of channels the spec is bound to by its reference histogram or bank (None for equalisation)."""
        if self.mode == MODE_MATCH:
            return self.ref_hist.channels
        return self.bank.channels if self.mode == MODE_LANDMARKS else None

    def buffers(self, channels: int, device) -> tuple:
        """(histogram, table, Otsu record or None, landmark slot or None) that ``prepare_scan(window=self)`` uses for
        scans of ``channels`` channels on ``device``; call it ahead of a graph recording to keep the allocation out."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:                              # "cuda" and "cuda:0" are one device
            dev = torch.device("cuda", torch.cuda.current_device())
        key = (str(dev), int(channels))
        if key not in self._buffers:
            self._buffers[key] = (S.ScanHistogram(channels, device), TransferTable(channels, device),
                                  S.OtsuSlot(channels, device) if self.foreground else None,
                                  LandmarkSlot(channels, device, self.bank.quantiles) if self.mode == MODE_LANDMARKS else None)
        return self._buffers[key]

    def ref_slot(self) -> S.WindowSlot:
        """The reference's window on the device (match): planned from the ``IntensityWindow`` once and kept."""
        if self._ref_slot is None:
            from . import otsu as O
            w = self.ref_window
            if w.foreground is None:
                self._ref_slot = S.window_slot(self.ref_hist, w)
            else:
                self._ref_slot = O.window_slot_above(self.ref_hist, w, O.otsu_slot(self.ref_hist))
        return self._ref_slot

    def plan(self, raw: torch.Tensor, mask: Optional[torch.Tensor] = None) -> TransferTable:
        """The table of ``raw`` (``[C, H, W, D]`` on the device) in the spec's own buffers: a clear, the histogram,
        [the Otsu plan], [the landmarks] and the table plan, with no host read."""
        hist, tab, otsu, lm = self.buffers(raw.shape[0], raw.device)
        S.scan_histogram(raw, mask=mask, above=self.above, out=hist.zero_())
        if otsu is not None:
            from . import otsu as O
            O.otsu_slot(hist, out=otsu)
        if self.mode == MODE_EQUALIZE:
            return equalize_table(hist, self.b_min, self.b_max, otsu=otsu, out=tab)
        if self.mode == MODE_MATCH:
            return match_table(hist, self.ref_hist, self.ref_slot(), self.clip, otsu=otsu, out=tab)
        return landmark_table(scan_landmarks(hist, self.bank.quantiles, otsu=otsu, out=lm), self.bank, self.clip, out=tab)

    def __repr__(self):
        sel = f"above={self.above}" + ("" if self.foreground is None else f", foreground={self.foreground!r}")
        if self.mode == MODE_EQUALIZE:
            return f"IntensityTransfer.equalize(b_min={self.b_min}, b_max={self.b_max}, {sel})"
        if self.mode == MODE_MATCH:
            return f"IntensityTransfer.match(ref_window={self.ref_window!r}, clip={self.clip}, {sel})"
        return f"IntensityTransfer.landmarks(quantiles={self.bank.quantiles}, clip={self.clip}, {sel})"


def check_transfer_args(window, raw: torch.Tensor, mask, shape) -> None:
    """The host-side checks of ``prepare_scan(window=<IntensityTransfer or TransferTable>)`` (``raw`` already
    ``[C, H, W, D]``); ``scanstats.check_window_args`` sends these two types here."""
    if raw.dtype not in S._DTYPES:
        raise ValueError(f"an intensity transfer takes int16 or uint8 scans, got {raw.dtype}")
    if isinstance(window, TransferTable):
        if mask is not None:
            raise ValueError("mask selects the voxels of a histogram: a TransferTable is already computed")
        if window.channels != raw.shape[0]:
            raise ValueError(f"window was made for {window.channels} channels, raw has {raw.shape[0]}")
    elif window.channels is not None and window.channels != raw.shape[0]:
        raise ValueError(f"window was made for {window.channels} channels, raw has {raw.shape[0]}")
    S._check_mask(mask, shape)


def resolve_table(window, raw: torch.Tensor, mask) -> TransferTable:
    """``prepare_scan``'s device side of these two types: a ``TransferTable`` as it is, an ``IntensityTransfer`` planned
    on ``raw`` itself in the spec's own buffers."""
    if isinstance(window, TransferTable):
        _same_device("window", window.table, "raw", raw)
        return window
    return window.plan(raw, mask)
