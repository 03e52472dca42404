"""Calibration and threshold-sweep metrics of a probability volume on the GPU (csrc/calibration.hip).

Definitions (written out, as in ``mivp_amd.regions``; ``tests/calibration_ref.py`` restates them in numpy):

- **Inputs.**  ``probs`` is fp32 ``[C, H, W, D]`` or ``[1, C, H, W, D]`` on the GPU, what
  ``SlidingWindowPredictor.predict(return_probs=True)`` returns; ``target`` is a class map with the layouts and dtypes of
  ``mivp_amd.regions``.  ``num_classes == C``, ``1 <= C <= 16``, ``1 <= n_bins <= 1024``.
- **Quantised probability.**  ``Q = 2^20`` and ``q = int(rint(p * Q))``, in fp32 with round-half-even.  The product is
  exact, so ``np.rint(p32 * np.float32(Q))`` is the same integer on every voxel.
- **Valid voxel.**  Each of its ``C`` probabilities is finite and in ``[0, 1]`` and its reference value is an integer in
  ``[0, C)``.  A voxel with a bad probability adds 1 to ``n_invalid``; otherwise one with an out-of-range reference value
  adds 1 to ``n_ignored`` (this is how an ignore label such as 255 is masked).  Neither contributes anywhere else.
- **Bin.**  ``b = min(n_bins - 1, (q * n_bins) >> 20)`` in integer arithmetic.
- **Rows.**  ``C + 1`` of them.  Rows ``0..C-1`` are one-vs-rest: ``p = p_c``, ``y = [target == c]``.  Row ``C`` is
  top-label: ``p = max_c p_c``, ``y = [argmax == target]``, the arg-max taking the lowest index among equals.
- **Tables**, int64 and exact: ``count[r, b]``, ``pos[r, b]`` (sum of y), ``qsum[r, b]`` (sum of q); per row ``n``,
  ``n_pos`` and the squared error ``e = |q - y Q|`` split so that it cannot overflow, ``sq_hi`` = sum of ``e^2 >> 20`` and
  ``sq_lo`` = sum of ``e^2 & (Q - 1)``; ``n_ignored`` and ``n_invalid``.
- **Derived values**, properties of a ``CalibrationReport`` computed with torch in float64 from the integer tables:

  - ``bin_confidence = qsum / (count Q)`` and ``bin_accuracy = pos / count`` (the reliability diagram), NaN in empty bins.
  - ``ece[r] = sum_b (count / n) |pos / count - qsum / (count Q)|`` over the non-empty bins.  A term equals
    ``|pos Q - qsum| / (n Q)`` and the numerators are integers, so the sum is taken exactly in int64 and divided once.
    ``mce[r]`` is the largest gap ``|pos / count - qsum / (count Q)| = |pos Q - qsum| / (count Q)`` of a non-empty bin.
  - ``brier[r] = (sq_hi 2^20 + sq_lo) / (Q^2 n)``.
  - Threshold ``k`` (``0..n_bins-1``) means "positive where ``b >= k``": ``tp[r, k] = sum_{b>=k} pos``, ``fp[r, k] =
    sum_{b>=k} (count - pos)``, ``fn = n_pos - tp``; ``dice_curve = 2 tp / (2 tp + fp + fn)``; ``best_threshold`` = the
    first maximum of ``dice_curve`` (over the entries that are defined) as ``k / n_bins``, with its Dice.
  - ``roc_auc``: the trapezoid over the points ``(fp / (n - n_pos), tp / n_pos)``, closed with ``(0, 0)``.
  - ``average_precision = sum_k (R_k - R_{k+1}) P_k``, ``R_k = tp_k / n_pos``, ``R_{n_bins} = 0``, ``P_k = tp_k /
    (tp_k + fp_k)``; a threshold above which there is no voxel adds nothing.
  - Each is NaN where its denominator is 0.

Numerics: the kernel adds integers with integer atomics, which commute, so **every table is exact and bitwise reproducible**
whatever the order of arrival, and so is everything derived from them.

``calibration_tables`` reads nothing back to the host, so it can be recorded in a ``torch.cuda.graph``;
``CalibrationReport.cpu()`` is the synchronising call.  The tables add: pass ``out=`` an earlier report of the same
``(C, n_bins)`` to pool scans.
"""
from __future__ import annotations

import numbers
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import LABEL_DTYPES, check_classes, check_gpu, i3, label_volume

QBITS = 20
Q = 1 << QBITS
MAX_BINS = 1024
FLAG_COMBINE = 1        # sum same-cell lanes within a wave before the atomic (slower: tools/bench_calibration.py)


def table_words(num_classes: int, n_bins: int) -> int:
    """int64 words of the table block of ``mivp_calibration_hist`` (``mivp_calibration_ws`` / 8)."""
    r = num_classes + 1
    return 3 * r * n_bins + 4 * r + 2


def _nan_ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    num, den = num.to(torch.float64), den.to(torch.float64)
    return torch.where(den > 0, num / den, torch.full_like(den, float("nan")))


class CalibrationReport:
    """The integer tables of one or more (probability volume, reference) pairs and the metrics derived from them (the
    module docstring has every field).  All tensors live on the device; ``tables`` is the one int64 block behind them."""

    INT_FIELDS = ("count", "pos", "qsum", "n", "n_pos", "sq_hi", "sq_lo", "n_ignored", "n_invalid")
    DERIVED = ("bin_confidence", "bin_accuracy", "ece", "mce", "brier", "tp", "fp", "fn", "dice_curve", "roc_auc",
               "average_precision")

    def __init__(self, num_classes: int, n_bins: int, device):
        self.num_classes, self.n_bins = int(num_classes), int(n_bins)
        self.tables = torch.zeros(table_words(self.num_classes, self.n_bins), dtype=torch.int64, device=device)

    # ---- the integer tables
    def _block(self, i: int) -> torch.Tensor:
        r, b = self.num_classes + 1, self.n_bins
        return self.tables[i * r * b:(i + 1) * r * b].view(r, b)

    def _row(self, i: int) -> torch.Tensor:
        r, b = self.num_classes + 1, self.n_bins
        return self.tables[3 * r * b + i * r:3 * r * b + (i + 1) * r]

    count = property(lambda self: self._block(0))
    pos = property(lambda self: self._block(1))
    qsum = property(lambda self: self._block(2))
    n = property(lambda self: self._row(0))
    n_pos = property(lambda self: self._row(1))
    sq_hi = property(lambda self: self._row(2))
    sq_lo = property(lambda self: self._row(3))
    n_ignored = property(lambda self: self.tables[-2])
    n_invalid = property(lambda self: self.tables[-1])

    def zero_(self) -> "CalibrationReport":
        self.tables.zero_()
        return self

    # ---- calibration
    @property
    def bin_confidence(self) -> torch.Tensor:
        return _nan_ratio(self.qsum, self.count * Q)

    @property
    def bin_accuracy(self) -> torch.Tensor:
        return _nan_ratio(self.pos, self.count)

    def _gap(self) -> torch.Tensor:
        return (self.pos * Q - self.qsum).abs()

    @property
    def ece(self) -> torch.Tensor:
        return _nan_ratio(self._gap().sum(1), self.n * Q)

    @property
    def mce(self) -> torch.Tensor:
        gap = _nan_ratio(self._gap(), self.count * Q)
        m = torch.where(torch.isnan(gap), torch.full_like(gap, -1.0), gap).max(1).values
        return torch.where(self.n > 0, m, torch.full_like(m, float("nan")))

    @property
    def brier(self) -> torch.Tensor:
        num = self.sq_hi.to(torch.float64) * float(Q) + self.sq_lo.to(torch.float64)
        return _nan_ratio(num, self.n.to(torch.float64) * float(Q) * float(Q))

    # ---- threshold sweep
    @staticmethod
    def _tail(a: torch.Tensor) -> torch.Tensor:
        return a.flip(1).cumsum(1).flip(1)

    @property
    def tp(self) -> torch.Tensor:
        return self._tail(self.pos)

    @property
    def fp(self) -> torch.Tensor:
        return self._tail(self.count - self.pos)

    @property
    def fn(self) -> torch.Tensor:
        return self.n_pos[:, None] - self.tp

    @property
    def dice_curve(self) -> torch.Tensor:
        tp = self.tp
        return _nan_ratio(2 * tp, 2 * tp + self.fp + self.fn)

    @property
    def best_threshold(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(threshold ``k / n_bins``, its Dice) per row; NaN where no entry of the curve is defined."""
        d = self.dice_curve
        bad = torch.isnan(d)
        k = torch.where(bad, torch.full_like(d, -1.0), d).argmax(1)
        none = bad.all(1)
        nan = torch.full((d.shape[0],), float("nan"), dtype=torch.float64, device=d.device)
        return (torch.where(none, nan, k.to(torch.float64) / float(self.n_bins)),
                torch.where(none, nan, d.gather(1, k[:, None])[:, 0]))

    @property
    def roc_auc(self) -> torch.Tensor:
        tp, fp = self.tp, self.fp
        zero = torch.zeros_like(tp[:, :1])
        tp1, fp1 = torch.cat([tp[:, 1:], zero], 1), torch.cat([fp[:, 1:], zero], 1)
        area = ((fp - fp1).to(torch.float64) * (tp + tp1).to(torch.float64)).sum(1)
        neg = (self.n - self.n_pos).to(torch.float64)
        return _nan_ratio(area, 2.0 * neg * self.n_pos.to(torch.float64))

    @property
    def average_precision(self) -> torch.Tensor:
        tp, fp = self.tp, self.fp
        tp1 = torch.cat([tp[:, 1:], torch.zeros_like(tp[:, :1])], 1)
        prec = _nan_ratio(tp, tp + fp)
        term = (tp - tp1).to(torch.float64) * torch.where(torch.isnan(prec), torch.zeros_like(prec), prec)
        return _nan_ratio(term.sum(1), self.n_pos)

    def cpu(self) -> Dict[str, object]:
        """The one synchronising call: every table and derived value as a numpy array (``n_ignored`` / ``n_invalid`` as
        ints), plus ``best_threshold`` / ``best_dice``, ``num_classes`` and ``n_bins``."""
        thr, dice = self.best_threshold
        dev = {k: getattr(self, k) for k in self.INT_FIELDS[:7] + self.DERIVED}
        dev.update(best_threshold=thr, best_dice=dice)
        out = {k: v.cpu().numpy() for k, v in dev.items()}
        tail = self.tables[-2:].cpu()
        out.update(n_ignored=int(tail[0]), n_invalid=int(tail[1]), num_classes=self.num_classes, n_bins=self.n_bins)
        return out


def _check_calibration_args(probs, target, num_classes, n_bins=15, out=None) -> Tuple[int, int, Tuple[int, int, int]]:
    """Everything that can be checked without the GPU -> (num_classes, n_bins, spatial shape)."""
    if not isinstance(probs, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("probs and target must be torch tensors")
    if probs.dtype != torch.float32:
        raise TypeError(f"probs must be float32, got {probs.dtype}")
    ncls = check_classes(num_classes)
    if isinstance(n_bins, bool) or not isinstance(n_bins, numbers.Integral) or not 1 <= n_bins <= MAX_BINS:
        raise ValueError(f"n_bins must be an int in 1..{MAX_BINS}, got {n_bins!r}")
    if probs.dim() == 5 and probs.shape[0] == 1:
        shape = tuple(probs.shape[1:])
    elif probs.dim() == 4:
        shape = tuple(probs.shape)
    else:
        raise ValueError(f"probs must be [C, H, W, D] or [1, C, H, W, D], got {tuple(probs.shape)}")
    if shape[0] != ncls:
        raise ValueError(f"probs has {shape[0]} class planes, num_classes is {ncls}")
    tshape = tuple(target.shape[2:]) if target.dim() == 5 and tuple(target.shape[:2]) == (1, 1) else tuple(target.shape)
    if len(tshape) != 3 or tshape != shape[1:]:
        raise ValueError(f"target must be [1, 1, H, W, D] or [H, W, D] with probs' spatial shape {shape[1:]}, "
                         f"got {tuple(target.shape)}")
    if min(shape) < 1 or shape[1] * shape[2] * shape[3] >= 2 ** 31:
        raise ValueError(f"the volume must have between 1 and 2^31 - 1 voxels, got {shape[1:]}")
    if out is not None:
        if not isinstance(out, CalibrationReport):
            raise TypeError("out must be a CalibrationReport")
        if (out.num_classes, out.n_bins) != (ncls, int(n_bins)):
            raise ValueError(f"out was made for (num_classes, n_bins) = {(out.num_classes, out.n_bins)}, "
                             f"this call has {(ncls, int(n_bins))}")
    return ncls, int(n_bins), shape[1:]


def calibration_tables(probs: torch.Tensor, target: torch.Tensor, num_classes: int, n_bins: int = 15,
                       out: Optional[CalibrationReport] = None, flags: int = 0) -> CalibrationReport:
    """One fused pass over the probability volume ``probs`` and the class map ``target`` (the module docstring has the
    definitions): the ``CalibrationReport`` of their tables.  With ``out=`` the counts are added to that report, which is
    how scans are pooled.  No host read: ``CalibrationReport.cpu()`` synchronises."""
    ncls, nb, dims = _check_calibration_args(probs, target, num_classes, n_bins, out)
    check_gpu("probs", probs)
    check_gpu("target", target)
    if probs.device != target.device:
        raise ValueError(f"probs is on {probs.device}, target on {target.device}")
    if out is not None and out.tables.device != probs.device:
        raise ValueError(f"out is on {out.tables.device}, probs on {probs.device}")
    p = (probs[0] if probs.dim() == 5 else probs).contiguous()
    t = label_volume("target", target)
    rep = CalibrationReport(ncls, nb, p.device) if out is None else out
    assert rep.tables.numel() * 8 == int(L.lib().mivp_calibration_ws(ncls, nb))
    L.call("mivp_calibration_hist", L.ptr(p), L.ptr(t), LABEL_DTYPES[t.dtype], i3(dims), ncls, nb, int(flags),
           L.ptr(rep.tables), L.stream())
    return rep
