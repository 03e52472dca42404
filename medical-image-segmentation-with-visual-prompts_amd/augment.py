"""Random intensity augmentation of a batch that is resident on the device: the reference's ``basic_rand_ts`` chain
(datasets/transforms.py:222-243, ``random_transforms: true``) -- RandBiasField, RandStdShiftIntensity, RandAdjustContrast,
RandScaleIntensity, RandHistogramShift, each per sample with probability 0.05 -- for the two pre-training steps.

It follows ``multiview.draw_views`` / ``ViewSlot``: the draws are made on the host (``draw_intensity``), a fixed device slot
holds them (``IntensitySlot``), two launches of csrc/intensity.hip read the slot (``augment_intensity``: statistics, then
apply), nothing is read back, and both launches record into a step's graph.  The formulas are MONAI's as documented
(DESIGN.md 4.21); MONAI's own draw streams are not reproduced (``Compose`` reseeds every child transform), so parity is
unpinned at that boundary.

The neighbourhood-based augmentations -- additive Gaussian noise, Gaussian blur, low-resolution simulation (MONAI's
``RandGaussianNoise``, ``RandGaussianSmooth``, ``RandSimulateLowResolution``; nnU-Net's default pipeline carries all three)
-- follow the same shape: ``draw_filters`` -> ``FilterSlot`` -> ``augment_filters`` (csrc/filters.hip)."""
from __future__ import annotations

import ctypes as C
import math
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


# ------------------------------------------------------------------------------------------------------------------
# neighbourhood-based augmentation: Gaussian noise, Gaussian blur, low-resolution simulation (csrc/filters.hip)
# ------------------------------------------------------------------------------------------------------------------
FLAG_NOISE, FLAG_SMOOTH, FLAG_LOWRES = 1, 2, 4
FLAG_FILTERS = 7
MAX_RADIUS = 8
N_TAPS = 2 * MAX_RADIUS + 1
FILTER_RECORD = 64              # int32 words per sample in the slot (MIVP_FILTER_RECORD_WORDS of mivp.h)
_F_KEY, _F_MEAN, _F_STD, _F_RADIUS, _F_LOW, _F_TAPS = 1, 2, 3, 4, 7, 10


def gaussian_taps(sigma: float):
    """MONAI's ``gaussian_1d(sigma, truncated=4.0, approx="erf")`` as documented: ``(r, centred float32 [17])`` with
    r = int(max(4 sigma, 0.5) + 0.5) and tap[k] = 0.5 (erf((k + 0.5) / (sigma sqrt 2)) - erf((k - 0.5) / (sigma sqrt 2))),
    clamped at 0, for k = -r..r at index 8 + k; computed in float64, not normalised."""
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"gaussian_taps: sigma {sigma} is not positive and finite")
    r = int(max(4.0 * sigma, 0.5) + 0.5)
    if r > MAX_RADIUS:
        raise ValueError(f"gaussian_taps: sigma {sigma} gives radius {r}, above {MAX_RADIUS}")
    taps = np.zeros(N_TAPS, np.float32)
    t = 1.0 / (sigma * math.sqrt(2.0))
    for k in range(-r, r + 1):
        taps[MAX_RADIUS + k] = max(0.5 * (math.erf((k + 0.5) * t) - math.erf((k - 0.5) * t)), 0.0)
    return r, taps


@dataclass
class FilterDraws:
    """What one step draws on the host for the noise / smooth / low-res chain, one entry per sample.  A step whose flag is
    off keeps neutral parameters (std 0, radius 0, the full grid).  Values are float32: what the kernels read."""
    flags: np.ndarray               # int32 [B], FLAG_NOISE | FLAG_SMOOTH | FLAG_LOWRES
    noise_key: np.ndarray           # uint32 [B]
    noise_mean: np.ndarray          # float32 [B]
    noise_std: np.ndarray           # float32 [B]
    radius: np.ndarray              # int32 [B, 3], 0..8 per axis H, W, D; 0: the axis is not filtered
    taps: np.ndarray                # float32 [B, 3, 17], tap k of axis a at [b, a, 8 + k] for k = -r..r, the rest 0
    low_size: np.ndarray            # int32 [B, 3]: the low-resolution grid

    @property
    def batch(self) -> int:
        return int(self.flags.shape[0])

    def pack(self) -> np.ndarray:
        """int32 [B, FILTER_RECORD]: the slot's records (float32 values as their bits)."""
        B = self.batch
        f = np.zeros((B, FILTER_RECORD), dtype=np.float32)
        f[:, _F_MEAN], f[:, _F_STD] = self.noise_mean, self.noise_std
        f[:, _F_TAPS:_F_TAPS + 3 * N_TAPS] = np.asarray(self.taps, np.float32).reshape(B, 3 * N_TAPS)
        w = f.view(np.int32)
        w[:, 0] = self.flags
        w[:, _F_KEY] = np.asarray(self.noise_key, np.uint32).view(np.int32)
        w[:, _F_RADIUS:_F_RADIUS + 3] = self.radius
        w[:, _F_LOW:_F_LOW + 3] = self.low_size
        return w

    @classmethod
    def unpack(cls, words: np.ndarray) -> "FilterDraws":
        w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1, FILTER_RECORD)
        f = w.view(np.float32)
        return cls(w[:, 0].copy(), w[:, _F_KEY].copy().view(np.uint32), f[:, _F_MEAN].copy(), f[:, _F_STD].copy(),
                   w[:, _F_RADIUS:_F_RADIUS + 3].copy(), f[:, _F_TAPS:_F_TAPS + 3 * N_TAPS].copy().reshape(-1, 3, N_TAPS),
                   w[:, _F_LOW:_F_LOW + 3].copy())

    def check(self):
        B = self.batch
        shapes = [(self.noise_key, (B,)), (self.noise_mean, (B,)), (self.noise_std, (B,)), (self.radius, (B, 3)),
                  (self.taps, (B, 3, N_TAPS)), (self.low_size, (B, 3))]
        if self.flags.ndim != 1 or any(tuple(a.shape) != s for a, s in shapes):
            raise ValueError("FilterDraws: arrays of one batch size expected (radius [B, 3], taps [B, 3, 17], low_size [B, 3])")
        with np.errstate(invalid="ignore"):
            tests = (((self.flags & ~FLAG_FILTERS) != 0, "flags outside the three steps"),
                     (((self.radius < 0) | (self.radius > MAX_RADIUS)).any(axis=1), f"a radius outside 0..{MAX_RADIUS}"),
                     (~(np.isfinite(self.taps) & (self.taps >= 0)).all(axis=(1, 2)), "a tap that is negative or not finite"),
                     (~(np.isfinite(self.noise_std) & (self.noise_std >= 0)), "a noise_std that is negative or not finite"),
                     (~np.isfinite(self.noise_mean), "a noise_mean that is not finite"),
                     ((self.low_size < 1).any(axis=1), "a low_size below 1"))
        for bad, what in tests:
            if bad.any():
                raise ValueError(f"FilterDraws: sample {int(np.flatnonzero(bad)[0])}: {what}")
        return self


def neutral_filters(B: int, dims) -> FilterDraws:
    """Draws with every step off."""
    if B < 1 or len(dims) != 3 or min(int(n) for n in dims) < 1:
        raise ValueError("FilterDraws: B >= 1 and three extents >= 1 expected")
    return FilterDraws(np.zeros(B, np.int32), np.zeros(B, np.uint32), np.zeros(B, np.float32), np.zeros(B, np.float32),
                       np.zeros((B, 3), np.int32), np.zeros((B, 3, N_TAPS), np.float32),
                       np.tile(np.asarray(dims, np.int32), (B, 1)))


def draw_filters(rs: np.random.RandomState, B: int, dims, prob: float = 0.1, noise_std=(0.0, 0.1), sigma=(0.25, 1.5),
                 zoom=(0.5, 1.0)) -> FilterDraws:
    """The host draws of one batch from ONE RandomState: per sample, in the order noise, smooth, low-res, ``rand() < prob``
    and then -- only if the step fired -- its parameters: randint(2^32) for the noise key and uniform(noise_std) for its
    std (the mean is 0); one uniform(sigma) per axis H, W, D, turned into taps by ``gaussian_taps``; one uniform(zoom)
    and low_size[a] = max(1, int(dims[a] z + 0.5)).  The formulas are MONAI's as documented (RandGaussianNoise,
    RandGaussianSmooth with one sigma per axis, RandSimulateLowResolution); MONAI's own draw streams are not reproduced
    (DESIGN.md 8)."""
    d = neutral_filters(B, dims)
    dims = [int(n) for n in dims]
    if not (0.0 < float(sigma[0]) <= float(sigma[1])) or int(max(4.0 * float(sigma[1]), 0.5) + 0.5) > MAX_RADIUS:
        raise ValueError(f"draw_filters: sigma range {tuple(sigma)} is not positive or gives a radius above {MAX_RADIUS}")
    if not (0.0 <= float(noise_std[0]) <= float(noise_std[1])):
        raise ValueError(f"draw_filters: noise_std range {tuple(noise_std)} is negative or reversed")
    if not (0.0 < float(zoom[0]) <= float(zoom[1]) <= 1.0):
        raise ValueError(f"draw_filters: zoom range {tuple(zoom)} outside (0, 1]")
    for b in range(B):
        if rs.rand() < prob:
            d.flags[b] |= FLAG_NOISE
            d.noise_key[b] = rs.randint(0, 2 ** 32, dtype=np.uint32)
            d.noise_std[b] = rs.uniform(noise_std[0], noise_std[1])
        if rs.rand() < prob:
            d.flags[b] |= FLAG_SMOOTH
            for a in range(3):
                d.radius[b, a], d.taps[b, a] = gaussian_taps(rs.uniform(sigma[0], sigma[1]))
        if rs.rand() < prob:
            d.flags[b] |= FLAG_LOWRES
            z = rs.uniform(zoom[0], zoom[1])
            d.low_size[b] = [max(1, int(n * z + 0.5)) for n in dims]
    return d


class FilterSlot:
    """Fixed device memory of one batch's filter draws -- int32 [B][FILTER_RECORD] records -- and the two batch-sized
    temporaries the launches pass the stages through (the low-res pass cannot run in place), in ONE allocation whose
    pointer a recorded graph keeps.  ``load`` works as ``IntensitySlot.load`` does and also refuses a low grid larger
    than the volume."""

    def __init__(self, B: int, C_: int, dims, device):
        self.B, self.C, self.dims = int(B), int(C_), tuple(int(n) for n in dims)
        if self.B < 1 or self.C < 1 or len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError("FilterSlot: B >= 1, C >= 1 and three extents >= 1 expected")
        self.ws_bytes = int(L.lib().mivp_filter_ws(self.B, self.C, (C.c_int32 * 3)(*self.dims)))
        if self.ws_bytes == 0:
            raise ValueError(f"FilterSlot: a batch of {self.B} x {self.C} x {self.dims} is outside what the kernels take "
                             "(fewer than 2^31 elements per sample, at most 65535 samples)")
        self.buf = torch.zeros(self.B * FILTER_RECORD + self.ws_bytes // 4, dtype=torch.int32, device=device)
        self.records = self.buf[:self.B * FILTER_RECORD]
        self.ws = self.buf[self.B * FILTER_RECORD:]
        self.draws = None

    def load(self, draws: FilterDraws):
        if draws.check().batch != self.B:
            raise ValueError(f"FilterSlot: draws of batch {draws.batch} do not match the slot's batch {self.B}")
        bad = (draws.low_size > np.asarray(self.dims)).any(axis=1)
        if bad.any():
            b = int(np.flatnonzero(bad)[0])
            raise ValueError(f"FilterSlot: sample {b}: low_size {draws.low_size[b].tolist()} exceeds the volume "
                             f"{list(self.dims)}")
        if torch.cuda.is_current_stream_capturing():
            return
        self.records.copy_(torch.from_numpy(draws.pack().reshape(-1)).pin_memory(), non_blocking=True)
        self.draws = draws


@torch.no_grad()
def augment_filters(x: torch.Tensor, slot: FilterSlot, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Noise, then blur, then low-resolution simulation of the draws loaded in ``slot`` applied to ``x`` [B, C, H, W, D]:
    three launches on the current stream whatever the draws hold, nothing allocated beyond ``out``, nothing read back.
    ``out`` may be ``x`` (in place); a sample without flags is copied bit for bit (in place: not written).  Detached."""
    if not isinstance(slot, FilterSlot):
        raise ValueError("filter augmentation: a FilterSlot expected")
    if x.dim() != 5 or x.shape[0] != slot.B or x.shape[1] != slot.C or tuple(x.shape[2:]) != slot.dims:
        raise ValueError(f"filter augmentation: input of shape {tuple(x.shape)} does not match the slot's batch "
                         f"[{slot.B}, {slot.C}, {', '.join(map(str, slot.dims))}]")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("filter augmentation: the input must be a contiguous fp32 [B, C, H, W, D] tensor")
    if x.numel() == 0 or x[0].numel() >= 2 ** 31:
        raise ValueError("filter augmentation: between 1 and 2^31 - 1 elements per sample expected")
    if slot.draws is None:
        raise ValueError("filter augmentation: the slot holds no draws (FilterSlot.load)")
    if out is not None and (out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != x.device):
        raise ValueError("filter augmentation: out must be a contiguous fp32 tensor of the input's shape and device")
    if out is None:
        out = torch.empty_like(x)
    L.call("mivp_filter_apply", L.ptr(x), slot.B, slot.C, (C.c_int32 * 3)(*slot.dims), L.ptr(slot.records), L.ptr(slot.ws),
           slot.ws_bytes, L.ptr(out), L.stream())
    return out

def as_slot(augment, x: torch.Tensor):
    """The ``augment=`` argument of the step functions: draws (a slot is made and loaded) or a slot with draws loaded, of
    the intensity chain or of the filters."""
    if isinstance(augment, (IntensitySlot, FilterSlot)):
        return augment
    if isinstance(augment, (IntensityDraws, FilterDraws)):
        if x.dim() != 5 or augment.batch != x.shape[0]:
            raise ValueError(f"{_kind(augment)} augmentation: draws of batch {augment.batch} for an input of shape "
                             f"{tuple(x.shape)}")
        slot = (IntensitySlot(augment.batch, x.device) if isinstance(augment, IntensityDraws)
                else FilterSlot(augment.batch, x.shape[1], tuple(x.shape[2:]), x.device))
        slot.load(augment)
        return slot
    raise ValueError("augment= takes IntensityDraws, FilterDraws, a slot of either kind with draws loaded, or a list of them")


def _kind(a) -> str:
    return "intensity" if isinstance(a, (IntensityDraws, IntensitySlot)) else "filter"


def as_slots(augment, x: torch.Tensor) -> list:
    """``as_slot`` for the list form of ``augment=``: one entry or a list / tuple of them, in the order they are applied."""
    return [as_slot(a, x) for a in (augment if isinstance(augment, (list, tuple)) else [augment])]


@torch.no_grad()
def apply_slots(x: torch.Tensor, slots) -> torch.Tensor:
    """``x`` through the slots in order, out of place (``x`` is left as it is)."""
    for slot in slots:
        x = augment_intensity(x, slot) if isinstance(slot, IntensitySlot) else augment_filters(x, slot)
    return x


class AugmentChain:
    """The ``augment=`` argument of a recorded step: one entry or a list / tuple of them, each a slot the caller reloads,
    draws used for every step, or a callable returning the next step's draws.  ``refresh`` -- before every warm-up step
    and replay -- loads the next draws of every entry that is not a caller's slot; the slot of such an entry is made at the
    first refresh, of the kind of the draws it meets (the warm-up steps run before anything is recorded)."""

    def __init__(self, augment, x: torch.Tensor):
        self.listed = isinstance(augment, (list, tuple))
        self.entries = list(augment) if self.listed else [augment]
        self.slots = [a if isinstance(a, (IntensitySlot, FilterSlot)) else None for a in self.entries]
        self.x = x

    def refresh(self):
        for i, a in enumerate(self.entries):
            if self.slots[i] is a:
                continue
            d = a() if callable(a) else a
            if self.slots[i] is None:
                self.slots[i] = as_slot(d, self.x)
            else:
                self.slots[i].load(d)

    def apply(self, x: torch.Tensor) -> torch.Tensor:
        return apply_slots(x, self.slots)

    @property
    def augment_slot(self):
        """What a recorded step shows as ``step.augment_slot``: the slot, or the list of them for the list form."""
        return list(self.slots) if self.listed else self.slots[0]
