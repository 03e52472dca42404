"""Random intensity augmentation of a batch that is resident on the device: the reference's ``basic_rand_ts`` chain
(datasets/transforms.py:222-243, ``random_transforms: true``) -- RandBiasField, RandStdShiftIntensity, RandAdjustContrast,
RandScaleIntensity, RandHistogramShift, each per sample with probability 0.05 -- for the two pre-training steps.

It follows ``multiview.draw_views`` / ``ViewSlot``: the draws are made on the host (``draw_intensity``), a fixed device slot
holds them (``IntensitySlot``), two launches of csrc/intensity.hip read the slot (``augment_intensity``: statistics, then
apply), nothing is read back, and both launches record into a step's graph.  The formulas are MONAI's as documented
(DESIGN.md 4.21); MONAI's own draw streams are not reproduced (``Compose`` reseeds every child transform), so parity is
unpinned at that boundary."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib as L

FLAG_BIAS, FLAG_SHIFT, FLAG_CONTRAST, FLAG_SCALE, FLAG_HIST = 1, 2, 4, 8, 16
FLAG_ALL = 31
N_COEFF = 20                    # Legendre degree 3: c[i][j][k], i + j + k <= 3, i outer, k inner
MAX_POINTS = 12
RECORD = 40                     # int32 words per sample in the slot (mivp.h)
_R_NCP, _R_SHIFT, _R_GAMMA, _R_SCALE, _R_COEF, _R_FLOAT = 1, 2, 3, 4, 5, 25


@dataclass
class IntensityDraws:
    """What one step draws on the host, one entry per sample.  A step whose flag is off keeps neutral parameters
    (coefficients 0, factors 0, gamma 1, the reference control points).  Values are float32: what the kernels read."""
    flags: np.ndarray               # int32 [B], FLAG_* bits
    coeffs: np.ndarray              # float32 [B, 20]
    shift: np.ndarray               # float32 [B]: the std-shift factor
    gamma: np.ndarray               # float32 [B]
    scale: np.ndarray               # float32 [B]: the scale factor f of v * (1 + f)
    n_points: np.ndarray            # int32 [B], 2..12 (the draws give 8..12)
    floating: np.ndarray            # float32 [B, 12]: the first n_points are used, the rest are 1

    @property
    def batch(self) -> int:
        return int(self.flags.shape[0])

    def pack(self) -> np.ndarray:
        """int32 [B, RECORD]: the slot's records (float32 values as their bits)."""
        B = self.batch
        f = np.zeros((B, RECORD), dtype=np.float32)
        f[:, _R_SHIFT], f[:, _R_GAMMA], f[:, _R_SCALE] = self.shift, self.gamma, self.scale
        f[:, _R_COEF:_R_COEF + N_COEFF] = self.coeffs
        f[:, _R_FLOAT:_R_FLOAT + MAX_POINTS] = self.floating
        w = f.view(np.int32)
        w[:, 0] = self.flags
        w[:, _R_NCP] = self.n_points
        return w

    @classmethod
    def unpack(cls, words: np.ndarray) -> "IntensityDraws":
        w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, RECORD)
        f = w.view(np.float32)
        return cls(w[:, 0].copy(), f[:, _R_COEF:_R_COEF + N_COEFF].copy(), f[:, _R_SHIFT].copy(), f[:, _R_GAMMA].copy(),
                   f[:, _R_SCALE].copy(), w[:, _R_NCP].copy(), f[:, _R_FLOAT:_R_FLOAT + MAX_POINTS].copy())

    def check(self):
        B = self.batch
        shapes = [(self.coeffs, (B, N_COEFF)), (self.shift, (B,)), (self.gamma, (B,)), (self.scale, (B,)),
                  (self.n_points, (B,)), (self.floating, (B, MAX_POINTS))]
        if self.flags.ndim != 1 or any(tuple(a.shape) != s for a, s in shapes):
            raise ValueError("IntensityDraws: arrays of one batch size expected (coeffs [B, 20], floating [B, 12])")
        if np.any(self.flags & ~FLAG_ALL) or np.any(self.n_points < 2) or np.any(self.n_points > MAX_POINTS):
            raise ValueError("IntensityDraws: flags outside the five steps, or a control-point count outside 2..12")
        return self


def draw_intensity(rs: np.random.RandomState, B: int, prob: float = 0.05, coeff_range=(0.0, 0.1), std_factors=(0.0, 0.1),
                   gamma=(0.5, 4.5), scale: float = 2.0, control_points=(8, 12)) -> IntensityDraws:
    """The host draws of one batch from ONE RandomState: per sample, in chain order, ``rand() < prob`` and then -- only if
    the step fired -- its parameters: 20 x uniform(coeff_range); uniform(std_factors); uniform(gamma); uniform(-scale, scale);
    randint(lo, hi + 1) control points and floating[i] = uniform(floating[i-1], floating[i+1]) for i = 1..n-2 on
    linspace(0, 1, n).  The defaults are the reference's ``basic_rand_ts`` values."""
    lo, hi = int(control_points[0]), int(control_points[1])
    if not (2 <= lo <= hi <= MAX_POINTS):
        raise ValueError(f"draw_intensity: control_points {control_points} outside 2..{MAX_POINTS}")
    if B < 1:
        raise ValueError("draw_intensity: B >= 1 expected")
    d = IntensityDraws(np.zeros(B, np.int32), np.zeros((B, N_COEFF), np.float32), np.zeros(B, np.float32),
                       np.ones(B, np.float32), np.zeros(B, np.float32), np.full(B, lo, np.int32),
                       np.ones((B, MAX_POINTS), np.float32))
    d.floating[:, :lo] = np.linspace(0.0, 1.0, lo)
    for b in range(B):
        if rs.rand() < prob:
            d.flags[b] |= FLAG_BIAS
            d.coeffs[b] = rs.uniform(coeff_range[0], coeff_range[1], N_COEFF)
        if rs.rand() < prob:
            d.flags[b] |= FLAG_SHIFT
            d.shift[b] = rs.uniform(std_factors[0], std_factors[1])
        if rs.rand() < prob:
            d.flags[b] |= FLAG_CONTRAST
            d.gamma[b] = rs.uniform(gamma[0], gamma[1])
        if rs.rand() < prob:
            d.flags[b] |= FLAG_SCALE
            d.scale[b] = rs.uniform(-scale, scale)
        if rs.rand() < prob:
            d.flags[b] |= FLAG_HIST
            n = int(rs.randint(lo, hi + 1))
            fl = np.linspace(0.0, 1.0, n)
            for i in range(1, n - 1):
                fl[i] = rs.uniform(fl[i - 1], fl[i + 1])
            d.n_points[b] = n
            d.floating[b] = 1.0
            d.floating[b, :n] = fl
    return d


class IntensitySlot:
    """Fixed device memory of one batch's draws -- int32 [B][RECORD] records -- and the statistics partials the two
    launches hand over, in ONE allocation whose pointer a recorded graph keeps.  The workspace is sized for any volume (the
    kernels cap the workgroups per sample).  ``load`` refreshes the records from a new pinned staging buffer without
    blocking and does nothing while a graph is being recorded, exactly as ``multiview.ViewSlot.load``."""

    def __init__(self, B: int, device):
        self.B = int(B)
        if self.B < 1:
            raise ValueError("IntensitySlot: B >= 1 expected")
        self.ws_bytes = int(L.lib().mivp_intensity_ws(self.B, 1 << 40))
        self.buf = torch.zeros(self.B * RECORD + self.ws_bytes // 4, dtype=torch.int32, device=device)
        self.records = self.buf[:self.B * RECORD]
        self.ws = self.buf[self.B * RECORD:]
        self.draws = None

    def load(self, draws: IntensityDraws):
        if draws.check().batch != self.B:
            raise ValueError(f"IntensitySlot: draws of batch {draws.batch} do not match the slot's batch {self.B}")
        if torch.cuda.is_current_stream_capturing():
            return
        self.records.copy_(torch.from_numpy(draws.pack().reshape(-1)).pin_memory(), non_blocking=True)
        self.draws = draws


def _check_input(x: torch.Tensor, slot: IntensitySlot, out: Optional[torch.Tensor]):
    if not isinstance(slot, IntensitySlot):
        raise ValueError("intensity augmentation: an IntensitySlot expected")
    if x.dim() != 5 or x.shape[0] != slot.B:
        raise ValueError(f"intensity augmentation: input of shape {tuple(x.shape)} does not match a [B, C, H, W, D] batch of "
                         f"{slot.B} samples")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("intensity augmentation: the input must be a contiguous fp32 [B, C, H, W, D] tensor")
    if x.numel() == 0 or x[0].numel() >= 2 ** 31:
        raise ValueError("intensity augmentation: between 1 and 2^31 - 1 voxels per sample expected")
    if slot.draws is None:
        raise ValueError("intensity augmentation: the slot holds no draws (IntensitySlot.load)")
    if out is not None and (out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != x.device):
        raise ValueError("intensity augmentation: out must be a contiguous fp32 tensor of the input's shape and device")


@torch.no_grad()
def augment_intensity(x: torch.Tensor, slot: IntensitySlot, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The chain of the draws loaded in ``slot`` applied to ``x`` [B, C, H, W, D]: two launches on the current stream
    (statistics, apply), no host read between them.  ``out`` may be ``x`` (in place); a sample without flags is copied bit
    for bit.  Detached, like the views the steps build from it."""
    _check_input(x, slot, out)
    if out is None:
        out = torch.empty_like(x)
    B, Cn = x.shape[0], x.shape[1]
    dims = (C.c_int32 * 3)(*x.shape[2:])
    L.call("mivp_intensity_stats", L.ptr(x), B, Cn, dims, L.ptr(slot.records), L.ptr(slot.ws), slot.ws_bytes, L.stream())
    L.call("mivp_intensity_apply", L.ptr(x), B, Cn, dims, L.ptr(slot.records), L.ptr(slot.ws), slot.ws_bytes, L.ptr(out),
           L.stream())
    return out


def as_slot(augment, x: torch.Tensor) -> IntensitySlot:
    """The ``augment=`` argument of the step functions: draws (a slot is made and loaded) or a slot with draws loaded."""
    if isinstance(augment, IntensitySlot):
        return augment
    if isinstance(augment, IntensityDraws):
        if x.dim() != 5 or augment.batch != x.shape[0]:
            raise ValueError(f"intensity augmentation: draws of batch {augment.batch} for an input of shape {tuple(x.shape)}")
        slot = IntensitySlot(augment.batch, x.device)
        slot.load(augment)
        return slot
    raise ValueError("augment= takes IntensityDraws or an IntensitySlot with draws loaded")
