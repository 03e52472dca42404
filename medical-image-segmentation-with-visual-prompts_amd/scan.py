"""Scan preparation and native-grid restore around whole-volume prediction on the GPU (csrc/scan.hip).

The reference prepares a scan on CPU workers with MONAI (src/datasets/transforms.py): ``ScaleIntensityRanged(clip=True)``
-> ``Orientationd('RAS')`` -> optionally ``Resized`` (trilinear for the image, nearest for the mask).  MONAI and nibabel
are not dependencies here, so the conventions are written out rather than pinned to them:

- **Grids.**  The *native* grid is the scan as stored, ``[H, W, D]`` contiguous with D fastest, with a 4 x 4 affine from
  voxel indices to world millimetres (RAS+: x to the right, y to anterior, z to superior).  The *oriented* grid is
  ``flip(transpose(native, perm), flipped axes)``; the *model* grid is the oriented grid resized to ``out_size`` (or the
  oriented grid itself).
- **Orientation rule.**  The columns of the affine's 3 x 3 block are normalised by their norms (the voxel spacing).
  Native axes are assigned to world axes greedily by decreasing absolute entry (always a permutation); an axis is flipped
  where the chosen entry's sign disagrees with the requested code (``R``, ``A``, ``S`` are the positive directions).
- **Intensity map.**  ``v = fma(x, s, t)`` in fp32 with ``s = fp32((b_max - b_min) / (a_max - a_min))`` and
  ``t = fp32(b_min - a_min * (b_max - b_min) / (a_max - a_min))``, then, with ``clip``, clamped to ``[b_min, b_max]``.
  It is applied to every source voxel *before* the resize, which is the reference's order.
- **Resize.**  ``torch.nn.functional.interpolate``: ``mode='trilinear', align_corners=False`` without antialiasing for
  images and logits, ``mode='nearest'`` for label maps, as per-axis tables (``linear_taps``, ``nearest_indices``).
  ``prepare_scan(flags=FLAG_ANTIALIAS)`` filters the minified axes of the image instead (``aa_taps``).

Four launches, all GPU tensors in and out with no CPU fallback: ``prepare_scan``, ``prepare_labels``, ``restore_labels``
and ``restore_labels_from_logits``.  ``ScanGeometry`` holds what both directions need and is plain numpy.
``prepare_scan(window=...)`` takes the window from the scan's own histogram instead (``mivp_amd.scanstats``).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import check_gpu, i3
from .resample import aa_pass_order, aa_taps, spacing_size  # noqa: F401  (public here, next to linear_taps)

_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.float32: 3, torch.int16: 4}
_CODES = {"L": (0, -1), "R": (0, 1), "P": (1, -1), "A": (1, 1), "I": (2, -1), "S": (2, 1)}
FLAG_DIRECT = 1          # read the source directly even when the innermost axis moves (tools/bench_scan.py)
FLAG_STAGED = 2          # stage tiles through LDS where the default reads directly (labels, arg-max)
FLAG_ANTIALIAS = 4       # prepare_scan: filter every minified axis (csrc/scan_aa.hip); not a bit of the C entries
AA_MAX_TAPS = 32         # taps per output the anti-aliased kernels take on a minified axis (csrc/scan_aa.hip)


# rejects non-integer sizes, unlike inference._check_shape3, which truncates them
def _shape3(name: str, v) -> Tuple[int, int, int]:
    try:
        t = tuple(int(a) for a in v)
    except TypeError:
        raise ValueError(f"{name} must be three positive sizes, got {v!r}") from None
    if len(t) != 3 or min(t) < 1 or any(int(a) != a for a in v):
        raise ValueError(f"{name} must be three positive sizes, got {tuple(v)}")
    return t


def nearest_indices(n_in: int, n_out: int) -> np.ndarray:
    """The source index ``F.interpolate(mode='nearest')`` reads for each of ``n_out`` outputs over ``n_in`` inputs:
    ``min(floor(dst * (n_in / n_out)), n_in - 1)`` with the scale and the product in fp32, as torch computes them."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_in - 1).astype(np.int32)


def linear_taps(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``F.interpolate(mode='linear', align_corners=False)`` along one axis as (lower index int32, upper index int32,
    weight of the upper one float64): ``src = max((dst + 0.5) * n_in / n_out - 0.5, 0)``, ``lo = floor(src)``,
    ``hi = min(lo + 1, n_in - 1)``, ``w = src - lo``.  Equal sizes give ``lo = dst`` and ``w = 0`` exactly."""
    src = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5, 0.0)
    lo = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo.astype(np.int32), hi.astype(np.int32), src - lo


def intensity_map(a_min: float = -1000.0, a_max: float = 1000.0, b_min: float = 0.0, b_max: float = 1.0):
    """(s, t, lo, hi) as fp32 values: ``v = clamp(fma(x, s, t), lo, hi)`` (the module docstring)."""
    vals = [float(a_min), float(a_max), float(b_min), float(b_max)]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"a_min, a_max, b_min, b_max must be finite, got {vals}")
    if not vals[1] > vals[0]:
        raise ValueError(f"a_max must be greater than a_min, got a_min={a_min}, a_max={a_max}")
    if vals[3] < vals[2]:
        raise ValueError(f"b_max must not be below b_min, got b_min={b_min}, b_max={b_max}")
    s = (vals[3] - vals[2]) / (vals[1] - vals[0])
    return tuple(float(np.float32(v)) for v in (s, vals[2] - vals[0] * s, vals[2], vals[3]))


class ScanGeometry:
    """How one scan's native grid maps to the grid the model sees, and back.

    ``shape``: native ``(H, W, D)``.  ``perm`` / ``flip``: oriented axis ``a`` is native axis ``perm[a]``, reversed where
    ``flip[a]``.  ``oriented_shape``, ``spacing`` (mm per voxel along the oriented axes: the ``spacing=`` of
    ``surface_metrics`` / ``evaluate_surface`` when there is no resize; ``model_spacing`` after one), ``out_size`` (the
    resize target or None) and ``size`` (the model grid: ``out_size`` or ``oriented_shape``)."""

    def __init__(self, shape, perm, flip, spacing=(1.0, 1.0, 1.0), out_size=None, axcodes: str = "RAS"):
        self.shape = _shape3("shape", shape)
        self.perm = tuple(int(p) for p in perm)
        if sorted(self.perm) != [0, 1, 2]:
            raise ValueError(f"perm must be a permutation of (0, 1, 2), got {tuple(perm)}")
        self.flip = tuple(bool(f) for f in flip)
        if len(self.flip) != 3:
            raise ValueError(f"flip must have three entries, got {tuple(flip)}")
        self.spacing = tuple(float(s) for s in spacing)
        if len(self.spacing) != 3 or not all(math.isfinite(s) and s > 0 for s in self.spacing):
            raise ValueError(f"spacing must be three positive sizes in mm, got {tuple(spacing)}")
        self.oriented_shape = tuple(self.shape[p] for p in self.perm)
        self.out_size = None if out_size is None else _shape3("out_size", out_size)
        self.size = self.out_size or self.oriented_shape
        self.resized = self.size != self.oriented_shape
        self.inverse = tuple(self.perm.index(j) for j in range(3))
        self.axcodes = axcodes
        self.minified = any(n < m for n, m in zip(self.size, self.oriented_shape))
        self._np: Dict[str, tuple] = {}
        self._dev: Dict[tuple, torch.Tensor] = {}

    @property
    def model_spacing(self) -> Tuple[float, float, float]:
        """mm per voxel of the model grid (``spacing`` scaled by the resize)."""
        return tuple(s * n / m for s, n, m in zip(self.spacing, self.oriented_shape, self.size))

    @classmethod
    def identity(cls, shape, spacing=(1.0, 1.0, 1.0), out_size=None, out_spacing=None) -> "ScanGeometry":
        """A tensor that is already oriented.  ``out_spacing`` as in ``from_affine``."""
        return cls._resampled(shape, (0, 1, 2), (False, False, False), spacing, out_size, out_spacing, "RAS")

    @classmethod
    def _resampled(cls, shape, perm, flip, spacing, out_size, out_spacing, axcodes) -> "ScanGeometry":
        if out_spacing is None:
            return cls(shape, perm, flip, spacing, out_size, axcodes)
        if out_size is not None:
            raise ValueError("out_size and out_spacing both fix the model grid: pass one or the other")
        g = cls(shape, perm, flip, spacing, None, axcodes)
        return cls(shape, perm, flip, spacing, spacing_size(g.oriented_shape, g.spacing, out_spacing), axcodes)

    @classmethod
    def from_affine(cls, shape, affine, axcodes: str = "RAS", out_size=None, out_spacing=None) -> "ScanGeometry":
        """From the native shape and the scan's 4 x 4 (or 3 x 3) voxel-to-world affine (RAS+ world).  ``out_spacing``
        (mm per voxel along the oriented axes, in place of ``out_size``) resamples to a target spacing: the model grid is
        ``spacing_size(oriented_shape, spacing, out_spacing)`` and ``model_spacing`` reports what results."""
        shape = _shape3("shape", shape)
        if not isinstance(axcodes, str) or len(axcodes) != 3 or any(ch not in _CODES for ch in axcodes.upper()):
            raise ValueError(f"axcodes must be three letters, one per axis from L/R, P/A, I/S, got {axcodes!r}")
        want = [_CODES[ch] for ch in axcodes.upper()]
        if sorted(w[0] for w in want) != [0, 1, 2]:
            raise ValueError(f"axcodes must name each of L/R, P/A, I/S once, got {axcodes!r}")
        a = np.asarray(affine, dtype=np.float64)
        if a.shape not in ((4, 4), (3, 3)) or not np.all(np.isfinite(a)):
            raise ValueError(f"affine must be a finite 4 x 4 (or 3 x 3) matrix, got shape {a.shape}")
        m = a[:3, :3]
        norms = np.sqrt((m * m).sum(axis=0))
        if not np.all(norms > 0):
            raise ValueError("affine is singular: a voxel axis has zero length")
        r = m / norms
        if abs(np.linalg.det(r)) < 1e-6:
            raise ValueError("affine is singular: its voxel axes are linearly dependent")
        # greedy assignment by decreasing |entry|: r[world, native]
        native_of_world, sign_of_world = [None] * 3, [1.0] * 3
        free_w, free_n = {0, 1, 2}, {0, 1, 2}
        for idx in np.argsort(-np.abs(r), axis=None, kind="stable"):
            w, n = divmod(int(idx), 3)
            if w in free_w and n in free_n:
                native_of_world[w], sign_of_world[w] = n, (1.0 if r[w, n] >= 0 else -1.0)
                free_w.discard(w)
                free_n.discard(n)
        perm = tuple(native_of_world[w] for w, _ in want)
        flip = tuple(sign_of_world[w] != float(s) for w, s in want)
        return cls._resampled(shape, perm, flip, tuple(float(norms[p]) for p in perm), out_size, out_spacing,
                              axcodes.upper())

    # ------------------------------------------------------------------ per-axis tables (host)
    def _to_native(self, a: int, idx: np.ndarray) -> np.ndarray:
        return (self.oriented_shape[a] - 1 - idx) if self.flip[a] else idx

    def tables(self, kind: str):
        """``(src_dims, out_dims, axes, interp, int32 table)`` of one launch (include/mivp.h, ABI 17).  ``kind``:
        ``"image"`` / ``"labels"`` native -> model grid, ``"restore_labels"`` / ``"restore_logits"`` model -> native."""
        if kind in self._np:
            return self._np[kind]
        if kind == "image_aa":
            self._np[kind] = self._aa_tables()
            return self._np[kind]
        if kind not in ("image", "labels", "restore_labels", "restore_logits"):
            raise ValueError(f"unknown table kind {kind!r}")
        interp = self.resized and kind in ("image", "restore_logits")
        lo, hi, w = [], [], []
        if kind in ("image", "labels"):
            src_dims, out_dims, axes = self.shape, self.size, self.perm
            for a in range(3):
                n_in, n_out = self.oriented_shape[a], self.size[a]
                if interp:
                    l, h, wt = linear_taps(n_in, n_out)
                else:
                    l = nearest_indices(n_in, n_out) if n_in != n_out else np.arange(n_out, dtype=np.int32)
                    h, wt = l, np.zeros(n_out)
                lo.append(self._to_native(a, l))
                hi.append(self._to_native(a, h))
                w.append(wt)
        else:
            src_dims, out_dims, axes = self.size, self.shape, self.inverse
            for j in range(3):
                a = self.inverse[j]
                n_in, n_out = self.size[a], self.oriented_shape[a]
                d = self._to_native(a, np.arange(n_out))          # native index -> oriented index (its own inverse)
                if interp:
                    l, h, wt = linear_taps(n_in, n_out)
                else:
                    l = nearest_indices(n_in, n_out) if n_in != n_out else np.arange(n_out, dtype=np.int32)
                    h, wt = l, np.zeros(n_out)
                lo.append(l[d])
                hi.append(h[d])
                w.append(wt[d])
        sections = [np.concatenate(lo).astype(np.int32)]
        if interp:
            sections += [np.concatenate(hi).astype(np.int32), np.concatenate(w).astype(np.float32).view(np.int32)]
        self._np[kind] = (tuple(src_dims), tuple(out_dims), tuple(axes), bool(interp), np.concatenate(sections))
        return self._np[kind]

    def _aa_tables(self):
        """``(src_dims, out_dims, axes, (flips, tmax), int32 table)`` of the anti-aliased launches (include/mivp.h): per
        oriented axis, in oriented coordinates, ``first | count | w[n_out][Tmax]`` where the axis is minified (``aa_taps``,
        weights rounded to fp32 once), ``lo | hi | w`` where it is up-sampled (``linear_taps``), nothing where it stays."""
        parts, tmax = [], [1, 1, 1]
        for a in range(3):
            n_in, n_out = self.oriented_shape[a], self.size[a]
            if n_out < n_in:
                x0, count, w = aa_taps(n_in, n_out)
                tmax[a] = int(w.shape[1])
                if tmax[a] > AA_MAX_TAPS:
                    raise ValueError(f"antialias: oriented axis {a} shrinks {n_in} -> {n_out} and needs {tmax[a]} taps per "
                                     f"output, the kernels take at most {AA_MAX_TAPS} (a minification up to about 15)")
                parts += [x0, count, np.ascontiguousarray(w, dtype=np.float32).reshape(-1).view(np.int32)]
            elif n_out > n_in:
                lo, hi, w = linear_taps(n_in, n_out)
                parts += [lo, hi, w.astype(np.float32).view(np.int32)]
        table = np.concatenate(parts).astype(np.int32) if parts else np.zeros(1, dtype=np.int32)
        return (self.shape, self.size, self.perm, (tuple(int(f) for f in self.flip), tuple(tmax)), table)

    def aa_workspace(self, device, channels: int) -> torch.Tensor:
        """The workspace of the anti-aliased launches for ``channels`` channels on ``device``, allocated once."""
        key = ("aa_ws", str(device), int(channels))
        if key not in self._dev:
            nbytes = int(L.lib().mivp_scan_prepare_aa_ws(int(channels), i3(self.shape), i3(self.size), i3(self.perm)))
            self._dev[key] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        return self._dev[key]

    def transfer_workspace(self, device, channels: int) -> torch.Tensor:
        """fp32 ``[C, H, W, D]`` on the native grid for ``channels`` channels on ``device``, allocated once: what a
        transfer table's apply launch writes and the prepare launch reads (``prepare_scan(window=IntensityTransfer)``)."""
        key = ("transfer_ws", str(device), int(channels))
        if key not in self._dev:
            self._dev[key] = torch.empty((int(channels),) + self.shape, dtype=torch.float32, device=device)
        return self._dev[key]

    def device_tables(self, kind: str, device) -> torch.Tensor:
        key = (kind, str(device))
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.tables(kind)[4]).to(device)
        return self._dev[key]

    def __repr__(self):
        return (f"ScanGeometry(shape={self.shape}, perm={self.perm}, flip={self.flip}, spacing={self.spacing}, "
                f"out_size={self.out_size})")


# ---------------------------------------------------------------------------------------------------------------------
def _check_geom(geom) -> ScanGeometry:
    if not isinstance(geom, ScanGeometry):
        raise ValueError(f"geom must be a ScanGeometry, got {type(geom).__name__}")
    return geom


def _check_tensor(name: str, t, dims: Sequence[int], dtypes) -> None:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dim() not in dims:
        raise ValueError(f"{name} must have {' or '.join(str(d) for d in dims)} dimensions, got shape {tuple(t.shape)}")
    if dtypes is not None and t.dtype not in dtypes:
        raise ValueError(f"{name} must be one of {[str(d).replace('torch.', '') for d in dtypes]}, got {t.dtype}")


def _check_out(out, shape, dtype, like: torch.Tensor):
    if out is None:
        return None
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype:
        raise ValueError(f"out must be a {str(dtype).replace('torch.', '')} tensor of shape {tuple(shape)}")
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")
    if out.device != like.device:
        raise ValueError(f"out is on {out.device}, the input on {like.device}")
    return out


def _volume3(name: str, t: torch.Tensor, want: Tuple[int, int, int]) -> torch.Tensor:
    """``[H, W, D]`` or ``[1, 1, H, W, D]`` -> ``[H, W, D]`` of the expected size."""
    if t.dim() == 5:
        if tuple(t.shape[:2]) != (1, 1):
            raise ValueError(f"{name} must be [1, 1, H, W, D] or [H, W, D], got {tuple(t.shape)}")
        t = t[0, 0]
    if tuple(t.shape) != tuple(want):
        raise ValueError(f"{name} has spatial size {tuple(t.shape)}, the geometry expects {tuple(want)}")
    return t


def _raw_view(raw, geom: ScanGeometry) -> torch.Tensor:
    """``[H, W, D]``, ``[C, H, W, D]`` or ``[1, C, H, W, D]`` -> ``[C, H, W, D]`` (checked, still on its device)."""
    _check_tensor("raw", raw, (3, 4, 5), tuple(_DTYPES))
    if raw.dim() == 5:
        if raw.shape[0] != 1:
            raise ValueError(f"raw must hold one scan ([1, C, H, W, D]), got {tuple(raw.shape)}")
        raw = raw[0]
    elif raw.dim() == 3:
        raw = raw[None]
    if not 1 <= raw.shape[0] <= 4:
        raise ValueError(f"raw must have 1..4 channels, got {raw.shape[0]}")
    if tuple(raw.shape[1:]) != geom.shape:
        raise ValueError(f"raw has spatial size {tuple(raw.shape[1:])}, the geometry's native shape is {geom.shape}")
    return raw


def prepare_scan(raw: torch.Tensor, geom: ScanGeometry, a_min: Optional[float] = None, a_max: Optional[float] = None,
                 b_min: float = 0.0, b_max: float = 1.0, clip: bool = True, out: Optional[torch.Tensor] = None, flags: int = 0,
                 window=None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A raw scan on its native grid -> the model's input, in one launch: intensity map (with clip), orientation and,
    when ``geom.out_size`` is set, the trilinear resize.  ``raw``: ``[C, H, W, D]`` (or ``[H, W, D]`` /
    ``[1, C, H, W, D]``), C <= 4, int16, uint8, int32 or float32.  Returns fp32 ``[1, C, H', W', D']`` (``out`` when
    given).  Without a resize the result is bit-equal to the intensity map of the transposed and flipped scan.
    ``a_min`` / ``a_max`` default to the reference's CT window, -1000 and 1000.

    ``window=`` replaces the fixed window by one that follows from the data (``mivp_amd.scanstats``, int16 / uint8 scans
    only), per channel and with no host read.  An ``IntensityWindow`` is computed on the scan itself: histogram -> plan ->
    this launch reading the plan from the device, three launches that record into a graph (the spec keeps the buffers:
    after one eager call nothing is allocated); ``mask`` (uint8 on the native grid) and the spec's ``above`` select the
    voxels it counts.  A ``WindowSlot`` -- ``window_slot`` of a histogram pooled over a data set -- is applied as it is.
    ``a_min`` / ``a_max`` must then be left out, and so must ``b_min`` / ``b_max``, which belong to the spec
    (``ValueError`` otherwise); ``clip`` holds for a percentile window (a z-score window clamps by its own ``clip=``
    percentiles).  An ``IntensityTransfer`` or a ``TransferTable`` (``mivp_amd.transfer``, DESIGN 4.44: equalisation,
    histogram matching, landmark standardisation) maps every value through a table instead: histogram -> table plan ->
    one streaming launch that writes the table's values on the native grid into a workspace the geometry keeps -> the
    float32 launch of this function with the identity map.  ``clip`` then belongs to the spec; ``mask`` goes with a spec only.

    ``flags=FLAG_ANTIALIAS`` (``antialias=True`` of ``predict_scan`` / ``evaluate_scan`` / ``predict_scan_volume``; a flag
    bit because this function's signature is frozen) filters every minified axis with the normalised triangle filter of support ``n_in / n_out``
    (``aa_taps``: the separable filter of torch's 2-D ``antialias=True``, here for a resident 3-D scan), one launch per
    minified axis through a workspace the geometry keeps (csrc/scan_aa.hip); up-sampled axes keep the
    two-tap form.  A geometry with no minified axis takes the launch it takes without the flag: the same bits.  The other
    flag bits select read paths of that launch only."""
    geom = _check_geom(geom)
    r = _raw_view(raw, geom)
    flags = int(flags)
    aa = bool(flags & FLAG_ANTIALIAS) and geom.minified
    flags &= ~FLAG_ANTIALIAS                                      # the C entries see their own bits only
    if aa:
        aa_src, aa_dst, aa_axes, (aa_flips, aa_tmax), _ = geom.tables("image_aa")      # refuses too many taps
    if window is None:
        if mask is not None:
            raise ValueError("mask selects the voxels a data-driven window counts: it needs window=")
        mp = intensity_map(-1000.0 if a_min is None else a_min, 1000.0 if a_max is None else a_max, b_min, b_max)
    else:
        from . import scanstats
        if a_min is not None or a_max is not None:
            raise ValueError("window= takes the place of a_min / a_max: pass one or the other")
        if (b_min, b_max) != (0.0, 1.0):
            raise ValueError("with window= the output range belongs to the window: pass b_min / b_max to "
                             "IntensityWindow.percentile, not to prepare_scan")
        scanstats.check_window_args(window, r, mask, geom.shape)
    shape = (1, r.shape[0]) + geom.size
    out = _check_out(out, shape, torch.float32, r)
    check_gpu("raw", r)
    r = r.contiguous()
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=r.device)
    src, dst, axes, interp, _ = geom.tables("image")
    if aa:
        aa_tab, ws = L.ptr(geom.device_tables("image_aa", r.device)), L.ptr(geom.aa_workspace(r.device, r.shape[0]))
    if window is not None and scanstats._is_transfer(window):
        # the table's values on the native grid, then the float32 launches below with the identity map and no clip
        from . import transfer
        r = transfer.apply_table(r, transfer.resolve_table(window, r, mask), out=geom.transfer_workspace(r.device, r.shape[0]))
        window, mp, clip = None, (1.0, 0.0, 0.0, 1.0), False
    if window is not None:
        slot = scanstats.resolve_window(window, r, mask)
        dev_clip = bool(clip) if slot.mode == scanstats.MODE_PERCENTILE else True
        if aa:
            L.call("mivp_scan_prepare_aa_dev", L.ptr(r), _DTYPES[r.dtype], r.shape[0], i3(aa_src), i3(aa_dst),
                   i3(aa_axes), i3(aa_flips), i3(aa_tmax), aa_tab, L.ptr(slot.words), int(dev_clip), L.ptr(out), ws,
                   L.stream())
            return out
        L.call("mivp_scan_prepare_dev", L.ptr(r), _DTYPES[r.dtype], r.shape[0], i3(src), i3(dst), i3(axes),
               L.ptr(geom.device_tables("image", r.device)), int(interp), L.ptr(slot.words), int(dev_clip), int(flags),
               L.ptr(out), L.stream())
        return out
    if aa:
        L.call("mivp_scan_prepare_aa", L.ptr(r), _DTYPES[r.dtype], r.shape[0], i3(aa_src), i3(aa_dst), i3(aa_axes),
               i3(aa_flips), i3(aa_tmax), aa_tab, (C.c_float * 4)(*mp), int(bool(clip)), L.ptr(out), ws, L.stream())
        return out
    L.call("mivp_scan_prepare", L.ptr(r), _DTYPES[r.dtype], r.shape[0], i3(src), i3(dst), i3(axes),
           L.ptr(geom.device_tables("image", r.device)), int(interp), (C.c_float * 4)(*mp), int(bool(clip)), int(flags),
           L.ptr(out), L.stream())
    return out


def prepare_labels(seg: torch.Tensor, geom: ScanGeometry, out: Optional[torch.Tensor] = None, check: bool = True,
                   flags: int = 0) -> torch.Tensor:
    """A label map on the native grid (``[H, W, D]`` or ``[1, 1, H, W, D]``; int16, uint8, int32 or float32 class
    indices) -> uint8 ``[1, 1, H', W', D']`` on the model grid: orientation and nearest resize.  A value outside 0..255
    (or a non-integer float) raises ``ValueError``: the kernel sets a device flag, read once here (the one host
    synchronisation; ``check=False`` skips the read and leaves such voxels 0)."""
    geom = _check_geom(geom)
    _check_tensor("seg", seg, (3, 5), tuple(_DTYPES))
    s = _volume3("seg", seg, geom.shape)
    shape = (1, 1) + geom.size
    out = _check_out(out, shape, torch.uint8, s)
    check_gpu("seg", s)
    s = s.contiguous()
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=s.device)
    bad = torch.zeros(1, dtype=torch.int32, device=s.device)
    src, dst, axes, _, _ = geom.tables("labels")
    L.call("mivp_scan_prepare_labels", L.ptr(s), _DTYPES[s.dtype], i3(src), i3(dst), i3(axes),
           L.ptr(geom.device_tables("labels", s.device)), int(flags), L.ptr(out), L.ptr(bad), L.stream())
    if check and int(bad.item()) != 0:
        raise ValueError("seg holds values outside 0..255 (or non-integer values): they do not fit a uint8 label map")
    return out


def restore_labels(labels: torch.Tensor, geom: ScanGeometry, out: Optional[torch.Tensor] = None,
                   flags: int = 0) -> torch.Tensor:
    """uint8 labels on the model grid (``[1, 1, H', W', D']`` or ``[H', W', D']``, e.g. ``predict(x)["labels"]``) -> uint8
    ``[H, W, D]`` on the scan's native grid: nearest resize back to the oriented size, inverse flip and permutation.
    No host synchronisation."""
    geom = _check_geom(geom)
    _check_tensor("labels", labels, (3, 5), (torch.uint8,))
    v = _volume3("labels", labels, geom.size)
    out = _check_out(out, geom.shape, torch.uint8, v)
    check_gpu("labels", v)
    v = v.contiguous()
    if out is None:
        out = torch.empty(geom.shape, dtype=torch.uint8, device=v.device)
    src, dst, axes, _, _ = geom.tables("restore_labels")
    L.call("mivp_scan_restore_labels", L.ptr(v), i3(src), i3(dst), i3(axes),
           L.ptr(geom.device_tables("restore_labels", v.device)), int(flags), L.ptr(out), L.stream())
    return out


def restore_labels_from_logits(logits: torch.Tensor, geom: ScanGeometry, out: Optional[torch.Tensor] = None,
                               flags: int = 0) -> torch.Tensor:
    """Blended fp32 logits on the model grid (``[1, C, H', W', D']`` or ``[C, H', W', D']``, C <= 16, what
    ``predict(x, return_logits=True)["logits"]`` holds) -> uint8 labels ``[H, W, D]`` on the native grid: per native voxel
    the trilinear interpolation of every class and the arg-max (the lowest class wins a tie).  The native-size logits are
    never stored.  No host synchronisation."""
    geom = _check_geom(geom)
    _check_tensor("logits", logits, (4, 5), (torch.float32,))
    v = logits
    if v.dim() == 5:
        if v.shape[0] != 1:
            raise ValueError(f"logits must hold one volume ([1, C, H, W, D]), got {tuple(v.shape)}")
        v = v[0]
    if not 1 <= v.shape[0] <= 16:
        raise ValueError(f"logits must have 1..16 classes, got {v.shape[0]}")
    if tuple(v.shape[1:]) != geom.size:
        raise ValueError(f"logits have spatial size {tuple(v.shape[1:])}, the geometry's model grid is {geom.size}")
    out = _check_out(out, geom.shape, torch.uint8, v)
    check_gpu("logits", v)
    v = v.contiguous()
    if out is None:
        out = torch.empty(geom.shape, dtype=torch.uint8, device=v.device)
    src, dst, axes, interp, _ = geom.tables("restore_logits")
    L.call("mivp_scan_restore_argmax", L.ptr(v), v.shape[0], i3(src), i3(dst), i3(axes),
           L.ptr(geom.device_tables("restore_logits", v.device)), int(interp), int(flags), L.ptr(out), L.stream())
    return out


def check_predict_args(image_size, in_channels: int, raw, geom, restore: str, postprocess=None) -> torch.Tensor:
    """The argument checks of ``SlidingWindowPredictor.predict_scan`` (no device work): returns raw as ``[C, H, W, D]``."""
    geom = _check_geom(geom)
    if restore not in ("labels", "logits"):
        raise ValueError(f"restore must be 'labels' or 'logits', got {restore!r}")
    if restore == "logits" and postprocess is not None:
        raise ValueError("postprocess works on the label map: use restore='labels' with it")
    r = _raw_view(raw, geom)
    if geom.size != tuple(image_size):
        raise ValueError(f"the geometry's model grid is {geom.size}, the predictor was built for {tuple(image_size)}")
    if r.shape[0] != int(in_channels):
        raise ValueError(f"raw has {r.shape[0]} channels, the predictor was built for {in_channels}")
    return r
