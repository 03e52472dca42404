"""Objectives of the reference's trainers on the device.

* ``ClusteredPrototypeLoss``  -- drop-in for losses/clustered_prototype_loss.py:13-206 (same constructor and ``forward``
  signature).  The point sampling of the full-resolution latents (the only part that touches big tensors: the model's
  channels-last bf16 ``latent_outputs``) is a pair of HIP kernels (csrc/proto.hip: forward gather, backward as a gather over
  voxels -- no atomics); the soft k-means / assignment algebra runs on the sampled points ([B, N / r^3, C] f32, a few
  hundred rows at the reference's sizes) with stock PyTorch GPU tensor ops.
* ``dice_focal_loss``         -- lives in train.py (fused HIP kernel, csrc/loss.hip).
* ``dice_loss``               -- MONAI ``DiceLoss(include_background, to_onehot_y=True, softmax=True)`` as documented
  (students_teacher.py:96-100); the Dice-focal kernels without the focal term; MONAI is absent from the image: parity
  unpinned, restated in oracle/loss_ref.py::dice_loss.
* ``SegLossSpec`` / ``seg_loss`` / ``SegLoss`` -- Tversky region term + weighted (focal) softmax cross-entropy with an
  ignore label (csrc/segloss.hip): not in the reference; ``train.step_loss`` uses it when ``conf.seg_loss`` is set.
  ``SegLossSpec(top_k=...)`` averages the cross-entropy over the hardest k % of the batch's voxels only (nnU-Net's
  ``DC_and_topk_loss``; csrc/segtopk.hip).
* ``signed_distance_maps`` / ``boundary_loss`` / ``SegLossSpec(lambda_boundary=...)`` -- the boundary loss of Kervadec et al.
  (MIDL 2019): softmax probabilities integrated against the signed distance maps of the labels, the maps built on the device
  per step by a batched exact distance transform (csrc/distmap.hip).
* ``soft_skeleton`` / ``cldice_loss`` / ``SegLossSpec(lambda_cldice=...)`` -- the clDice topology term of Shit et al. (CVPR
  2021): each mask against the other one's soft skeleton, skeletons and their backward as 3-D min / max brick kernels
  (csrc/cldice.hip).
* ``hausdorff_weight_maps`` / ``hausdorff_dt_loss`` / ``HausdorffDTLoss`` -- the Hausdorff distance-transform loss of Karimi &
  Salcudean (IEEE TMI 2019): the squared error weighted by the distance fields of the hard prediction and of the labels, both
  built on the device per step by the batched transform (csrc/hausdorff.hip); a module around an optional base
  loss, not a field of ``SegLossSpec``.
* ``lovasz_softmax_loss`` / ``LovaszSoftmaxLoss`` -- the Lovasz-Softmax loss of Berman, Triki & Blaschko (CVPR 2018), the
  convex surrogate of the per-class Jaccard index: one 32-bit key per (segment, voxel), an exact device-wide radix sort, a
  prefix pass and a gradient pass with an order-independent tie rule (csrc/lovasz.hip, csrc/sort_common.hpp); a
  module around an optional base loss like ``HausdorffDTLoss``.
"""
from __future__ import annotations

import ctypes as C
import math
from functools import lru_cache
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from ._host import (ImmutableValue, check_at_least, check_classes, check_finite, check_flag, check_gpu, check_spacing, i3,
                    plain_int)


def reduced_size(dims: Sequence[int], reduction_factor: float) -> List[int]:
    return [max(int(n // reduction_factor), 1) for n in dims]


@lru_cache(maxsize=2048)
def _axis_np(n_full: int, lo_crop: int, n_crop: int, n_out: int):
    """Interpolation taps of one axis: forward (lo, hi, w) per output index (absolute voxel coordinates) and backward
    (i1, w1, i2, w2) per voxel coordinate.  Sample i sits at x = ((2 i + 1) n_crop / n_out - 1) / 2 of the cropped axis
    (grid_sample with align_corners = False on an identity grid)."""
    lo = np.zeros(n_out, np.int32); hi = np.zeros(n_out, np.int32); w = np.zeros(n_out, np.float32)
    i1 = np.full(n_full, -1, np.int32); i2 = np.full(n_full, -1, np.int32)
    w1 = np.zeros(n_full, np.float32); w2 = np.zeros(n_full, np.float32)

    def add(c, i, wt):
        if wt == 0.0:
            return
        if i1[c] == i or i1[c] < 0:
            i1[c] = i; w1[c] += wt
        elif i2[c] == i or i2[c] < 0:
            i2[c] = i; w2[c] += wt
        else:
            raise RuntimeError("sample spacing below one voxel: more than two samples touch a voxel")

    for i in range(n_out):
        x = ((2 * i + 1) * n_crop / n_out - 1.0) / 2.0
        x = min(max(x, 0.0), n_crop - 1.0)
        l = min(int(math.floor(x)), n_crop - 1)
        h = min(l + 1, n_crop - 1)
        ww = np.float32(x - l)
        lo[i], hi[i], w[i] = lo_crop + l, lo_crop + h, ww
        add(lo_crop + l, i, float(np.float32(1.0) - ww))
        add(lo_crop + h, i, float(ww))
    return lo, hi, w, i1, w1, i2, w2


@lru_cache(maxsize=512)
def _axis_tables(n_full: int, lo_crop: int, n_crop: int, n_out: int, device_str: str):
    dev = torch.device(device_str)
    return tuple(torch.from_numpy(a).to(dev) for a in _axis_np(n_full, lo_crop, n_crop, n_out))


@lru_cache(maxsize=2048)
def _axis_packed_pinned(n_full: int, lo_crop: int, n_crop: int, n_out: int):
    """The seven tables of one axis as ONE pinned 4-byte-word buffer [3 n_out + 4 n_full] (lo | hi | w | i1 | w1 | i2 | w2):
    the source of a JitterSlot refresh (one asynchronous copy per axis; the buffer is never written again)."""
    words = np.concatenate([a.view(np.int32) for a in _axis_np(n_full, lo_crop, n_crop, n_out)])
    return torch.from_numpy(words).pin_memory()


class JitterSlot:
    """Persistent device tables of ONE student's jittered sampling grid.  ``_SamplePointsFn`` normally takes its tables from
    a cache keyed by the jitter, i.e. the table POINTERS change with the jitter; a recorded graph holds pointers, so in
    graph mode (``ClusteredPrototypeLoss(static_jitter=True)``) the kernels read these fixed buffers and a new jitter is
    a refresh of their CONTENT (``load``, three small host-to-device copies, stream-ordered before the replay)."""

    def __init__(self):
        self.geo = None
        self.bufs = None

    def load(self, dims, out_dims, jitter, device):
        geo = (tuple(int(v) for v in dims), tuple(int(v) for v in out_dims), str(device))
        capturing = torch.cuda.is_current_stream_capturing()
        if self.geo != geo:
            if capturing:
                raise RuntimeError("JitterSlot: the sampling geometry changed between the eager warm-up and the recording")
            self.bufs = [torch.zeros(3 * od + 4 * n, dtype=torch.int32, device=device) for n, od in zip(geo[0], geo[1])]
            self.geo = geo
        if capturing:
            return                                              # a recording must not freeze today's content into the graph
        j = [int(v) for v in jitter] if jitter is not None else [0] * 6
        for a, (n, od) in enumerate(zip(geo[0], geo[1])):
            lo, nc = j[2 * a], n - j[2 * a] - j[2 * a + 1]
            if nc < 1:
                raise ValueError("jitter crop leaves an empty volume")
            self.bufs[a].copy_(_axis_packed_pinned(n, lo, nc, od), non_blocking=True)

    def reload(self, jitter):
        if self.geo is None:
            raise RuntimeError("JitterSlot.reload before the first load")
        self.load(self.geo[0], self.geo[1], jitter, torch.device(self.geo[2]))

    def tables(self, dims, out_dims):
        if self.geo is None or self.geo[0] != tuple(int(v) for v in dims) or self.geo[1] != tuple(int(v) for v in out_dims):
            raise RuntimeError("JitterSlot: volume / grid size differs from the loaded tables")
        out = []
        for buf, n, od in zip(self.bufs, self.geo[0], self.geo[1]):
            f = buf.view(torch.float32)
            out.append((buf[:od], buf[od:2 * od], f[2 * od:3 * od], buf[3 * od:3 * od + n], f[3 * od + n:3 * od + 2 * n],
                        buf[3 * od + 2 * n:3 * od + 3 * n], f[3 * od + 3 * n:3 * od + 4 * n]))
        return out


def _ptr3(ts, ctype):
    return (C.POINTER(ctype) * 3)(*[C.cast(t.data_ptr(), C.POINTER(ctype)) for t in ts])


class _SamplePointsFn(torch.autograd.Function):
    """vol [B, C, H, W, D] (the model's channels-first VIEW of channels-last bf16 storage, or a contiguous f32 channels-first
    tensor) -> f32 [B, N, C] at the reduced grid's cell centres of the (jitter-cropped) volume."""

    @staticmethod
    def forward(ctx, vol, out_dims, jitter, slot=None):
        B, Cc, H, W, D = vol.shape
        if slot is not None:
            tabs = slot.tables((H, W, D), out_dims)             # content = the jitter last loaded into the slot
        else:
            j = [int(v) for v in jitter] if jitter is not None else [0] * 6
            crop = [(j[0], H - j[0] - j[1]), (j[2], W - j[2] - j[3]), (j[4], D - j[4] - j[5])]
            if min(c[1] for c in crop) < 1:
                raise ValueError("jitter crop leaves an empty volume")
            tabs = [_axis_tables(n, lo, nc, int(od), str(vol.device)) for n, (lo, nc), od in zip((H, W, D), crop, out_dims)]
        base = vol.permute(0, 2, 3, 4, 1)
        if base.is_contiguous():
            src, clast = base, 1
        elif vol.is_contiguous():
            src, clast = vol, 0
        else:
            src, clast = vol.contiguous(), 0
        if src.dtype not in (torch.bfloat16, torch.float32):
            src = src.float()
        od = (C.c_int32 * 3)(*[int(v) for v in out_dims])
        N = int(out_dims[0]) * int(out_dims[1]) * int(out_dims[2])
        out = torch.empty((B, N, Cc), dtype=torch.float32, device=vol.device)
        L.call("mivp_sample_points_fwd", L.ptr(src), 1 if src.dtype == torch.bfloat16 else 0, clast, B, H, W, D, Cc, od,
               _ptr3([t[0] for t in tabs], C.c_int32), _ptr3([t[1] for t in tabs], C.c_int32),
               _ptr3([t[2] for t in tabs], C.c_float), L.ptr(out), L.stream())
        ctx.tabs = tabs
        ctx.meta = (B, Cc, H, W, D, tuple(int(v) for v in out_dims), clast, src.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        B, Cc, H, W, D, out_dims, clast, dtype = ctx.meta
        tabs = ctx.tabs
        if Cc % 8 != 0:
            raise NotImplementedError("sample_points backward needs a channel count that is a multiple of 8")
        g = torch.empty((B, H, W, D, Cc), dtype=torch.bfloat16, device=gout.device)
        od = (C.c_int32 * 3)(*out_dims)
        L.call("mivp_sample_points_bwd", L.ptr(gout.contiguous().float()), B, H, W, D, Cc, od,
               _ptr3([t[3] for t in tabs], C.c_int32), _ptr3([t[5] for t in tabs], C.c_int32),
               _ptr3([t[4] for t in tabs], C.c_float), _ptr3([t[6] for t in tabs], C.c_float), L.ptr(g), L.stream())
        g = g.permute(0, 4, 1, 2, 3)                            # channels-first view, like the forward's input
        return (g if dtype == torch.bfloat16 else g.float()), None, None, None


def sample_points(vol: torch.Tensor, out_dims: Sequence[int], jitter=None, slot: Optional["JitterSlot"] = None) -> torch.Tensor:
    if not vol.is_cuda:
        raise RuntimeError("mivp_amd.losses runs on the GPU only (the CPU oracle lives in oracle/proto_ref.py)")
    return _SamplePointsFn.apply(vol, tuple(int(v) for v in out_dims), None if jitter is None else tuple(int(v) for v in jitter), slot)


def _pair_dist(cx: torch.Tensor, cy: torch.Tensor) -> torch.Tensor:
    # [B, Nx, 3] x [B, Ny, 3] -> [B, Nx, Ny]; the exact difference form (the matmul form loses the digits that decide the
    # nearest-point argmin and the max_dist threshold)
    return torch.cdist(cx, cy, compute_mode="donot_use_mm_for_euclid_dist")


class ClusteredPrototypeLoss(torch.nn.Module):
    """losses/clustered_prototype_loss.py:13-60.  ``forward`` draws the spatial jitter of each student exactly like the
    reference (``torch.randint(0, ceil(reduction_factor), (6,))`` from the global CPU generator, :173-178); pass ``jitters``
    to fix it (parity tests).  ``detach_teacher`` (default True) treats the teacher-side quantities as constants: the
    reference builds an autograd graph through the teacher forward although no optimizer ever reads the teacher's
    gradients (students_teacher.py:150-207, momentum_model.py:24) -- student gradients and the loss value are identical."""

    def __init__(self, reduction_factor: float = 8.0, k_means_iterations: int = 3, fwhm: float = 128.0,
                 detach_teacher: bool = True, static_jitter: bool = False):
        super().__init__()
        self.reduction_factor = reduction_factor
        self.k_means_iterations = k_means_iterations
        self.fwhm = fwhm
        self.detach_teacher = detach_teacher
        # graph mode (train.GraphedStep): the students' sampling tables live in fixed buffers (JitterSlot)
        self.static_jitter = static_jitter
        self._slots: List[JitterSlot] = []

    def draw_jitters(self, n_students: int):
        """The reference's draw (clustered_prototype_loss.py:173-178): six integers per student from the global CPU generator."""
        return [torch.randint(low=0, high=int(math.ceil(self.reduction_factor)), size=(6,)).tolist() for _ in range(n_students)]

    def load_jitters(self, jitters):
        """Graph mode: refresh the recorded step's sampling tables (call before each replay)."""
        for slot, j in zip(self._slots, jitters):
            slot.reload(j)

    def forward(self, emb_s: List[torch.Tensor], emb_t: torch.Tensor, coord_s: List[torch.Tensor], coord_t: torch.Tensor,
                temp_s: float = 0.066, temp_t: float = 0.033, jitters: Optional[List[Sequence[int]]] = None,
                max_dist: float = 4.0) -> torch.Tensor:
        rf = self.reduction_factor
        sigma2 = (self.fwhm / 2.355) ** 2
        if jitters is None:
            jitters = self.draw_jitters(len(emb_s))
        if self.detach_teacher:
            emb_t = emb_t.detach()
        rs_t = reduced_size(emb_t.shape[2:], rf)
        rs_p = reduced_size(emb_t.shape[2:], rf * 2)
        coord_t = coord_t.float()
        e_p, c_p = sample_points(emb_t, rs_p), sample_points(coord_t, rs_p)          # [B, P, C], [B, P, 3]
        e_t, c_t = sample_points(emb_t, rs_t), sample_points(coord_t, rs_t)
        e_t_n = F.normalize(e_t, dim=-1)
        e_p_n = F.normalize(e_p, dim=-1)

        def soft_assign():
            sim = torch.softmax(e_t_n @ e_p_n.transpose(1, 2) / temp_t, dim=-1)
            return sim * torch.exp(-_pair_dist(c_t, c_p) ** 2 / (2 * sigma2))

        for _ in range(self.k_means_iterations):
            w = soft_assign()
            den = w.sum(dim=1).unsqueeze(-1)
            e_p = (w.transpose(1, 2) @ e_t) / den
            e_p_n = F.normalize(e_p, dim=-1)
            c_p = (w.transpose(1, 2) @ c_t) / den
        sim_t_p = soft_assign()

        total = torch.zeros((), dtype=torch.float32, device=emb_t.device)
        for i in range(len(emb_s)):
            rs_s = reduced_size(emb_s[i].shape[2:], rf)
            slot = None
            if self.static_jitter:
                while len(self._slots) <= i:
                    self._slots.append(JitterSlot())
                slot = self._slots[i]
                slot.load(emb_s[i].shape[2:], rs_s, jitters[i], emb_s[i].device)
            e_z = sample_points(emb_s[i], rs_s, jitters[i], slot)
            c_z = sample_points(coord_s[i].float(), rs_s, jitters[i], slot)
            dmin, idx = _pair_dist(c_z, c_t).min(dim=-1)
            keep = (dmin <= max_dist).float()
            sim = torch.softmax(F.normalize(e_z, dim=-1) @ e_p_n.transpose(1, 2) / temp_s, dim=-1)
            target = torch.gather(sim_t_p, 1, idx.unsqueeze(-1).expand(-1, -1, sim_t_p.shape[-1]))
            logp = torch.clamp(torch.log(sim + 1e-16), min=-1e3, max=-0.0)
            ce = -(target * logp).sum(dim=-1)                   # [B, Ns]
            # mean over the kept points of every batch element (an element without kept points is NaN, as in the reference)
            total = total + ((ce * keep).sum(dim=1) / keep.sum(dim=1)).mean()
        return total


def dice_loss(logits: torch.Tensor, target: torch.Tensor, include_background: bool = True) -> torch.Tensor:
    """MONAI ``DiceLoss(include_background, to_onehot_y=True, softmax=True)`` (students_teacher.py:96-100, used at :190-197):
    per (batch, class) ``1 - (2 sum(p t) + 1e-5) / (sum(p) + sum(t) + 1e-5)``, mean.  Parity unpinned (MONAI absent; restated
    in oracle/loss_ref.py::dice_loss).  On the device this is the Dice-focal statistics / gradient kernel pair without the
    focal term (csrc/loss.hip, ``gamma < 0``): two streaming passes over the logits, no softmax / one-hot tensors."""
    from .train import _DiceFocalFn
    if not logits.is_cuda:
        raise RuntimeError("mivp_amd.losses.dice_loss runs on the GPU (the CPU restatement is oracle/loss_ref.py)")
    if logits.shape[1] > 8:
        raise RuntimeError("dice_loss: at most 8 classes (csrc/loss.hip)")
    base = logits.permute(0, 2, 3, 4, 1)
    if base.dtype != torch.float32 or not base.is_contiguous():
        base = base.float().contiguous()                    # (the HIP model's logits already are channels-last f32 storage)
    tgt = target.to(torch.float32).contiguous()
    return _DiceFocalFn.apply(base, tgt, include_background, -1.0)


# ---------------------------------------------------------------------------------------------
# Tversky region term + weighted (focal) softmax cross-entropy with an ignore label (csrc/segloss.hip)
# ---------------------------------------------------------------------------------------------
SEG_LOSS_MAX_CLASSES = 8
SEG_LOSS_SMOOTH = 1e-5


CLDICE_MAX_ITERATIONS = 16


def _check_iterations(n, name="iterations") -> int:
    if not plain_int(n) or not 1 <= int(n) <= CLDICE_MAX_ITERATIONS:
        raise ValueError(f"{name} must be an int in 1..{CLDICE_MAX_ITERATIONS}, got {n!r}")
    return int(n)


def _check_smooth(v, name="smooth") -> float:
    s = check_finite(name, v)
    if not s > 0.0 or s > float(np.finfo(np.float32).max) or float(np.float32(s)) == 0.0:
        raise ValueError(f"{name} must be > 0 and finite in fp32, got {v!r}")
    return s


class SegLossSpec(ImmutableValue):
    """Options of ``seg_loss`` (an immutable value; the formulas are in the docstring of ``seg_loss``).

    ``alpha``, ``beta`` >= 0: the Tversky weights of false positives / false negatives (0.5, 0.5: the project's Dice);
    ``batch``: region sums over the whole batch instead of per sample; ``include_background``: class 0 in the region term;
    ``focal_gamma``: 0 (plain cross-entropy) or >= 1 (an exponent in (0, 1) has an unbounded gradient at p -> 1);
    ``class_weights``: one weight >= 0 per class, or None (all ones); ``ignore_index``: the label of voxels that take no part,
    or None; ``lambda_region``, ``lambda_voxel``, ``lambda_boundary`` >= 0, not all three 0; ``top_k``: None, or the fraction
    in (0, 1] of the batch's valid voxels -- the hardest ones -- that the cross-entropy is averaged over (needs
    ``lambda_voxel`` > 0); ``lambda_boundary``: the weight of the boundary term (``boundary_loss``; not together with
    ``top_k``), ``boundary_spacing``: the voxel size (mm along H, W, D) its distance maps are measured in;
    ``lambda_cldice`` >= 0: the weight of the clDice term (``cldice_loss``; not together with ``top_k``; the four lambdas
    must not all be 0), ``cldice_iterations``: its skeleton iterations, an int in 1..16, ``cldice_smooth`` > 0."""

    __slots__ = ("alpha", "beta", "batch", "include_background", "focal_gamma", "class_weights", "ignore_index",
                 "lambda_region", "lambda_voxel", "top_k", "lambda_boundary", "boundary_spacing", "lambda_cldice",
                 "cldice_iterations", "cldice_smooth")

    def __init__(self, alpha: float = 0.5, beta: float = 0.5, batch: bool = False, include_background: bool = True,
                 focal_gamma: float = 0.0, class_weights: Optional[Sequence[float]] = None,
                 ignore_index: Optional[int] = None, lambda_region: float = 1.0, lambda_voxel: float = 1.0,
                 top_k: Optional[float] = None, lambda_boundary: float = 0.0,
                 boundary_spacing: Sequence[float] = (1.0, 1.0, 1.0), lambda_cldice: float = 0.0,
                 cldice_iterations: int = 3, cldice_smooth: float = 1.0):
        f32_max = float(np.finfo(np.float32).max)
        for name, v in (("alpha", alpha), ("beta", beta), ("lambda_region", lambda_region), ("lambda_voxel", lambda_voxel),
                        ("lambda_boundary", lambda_boundary), ("lambda_cldice", lambda_cldice)):
            if check_at_least(name, v, 0.0) > f32_max:
                raise ValueError(f"{name} must be finite in fp32, got {v!r}")
        gamma = check_at_least("focal_gamma", focal_gamma, 0.0)
        if 0.0 < gamma < 1.0 or gamma > f32_max:
            raise ValueError(f"focal_gamma must be 0 or >= 1 (its gradient is unbounded at p -> 1 in between), got {focal_gamma!r}")
        if float(lambda_region) == 0.0 and float(lambda_voxel) == 0.0 and float(lambda_boundary) == 0.0 \
                and float(lambda_cldice) == 0.0:                   # (the message of the three-lambda rule, kept)
            raise ValueError("lambda_region and lambda_voxel and lambda_boundary must not all be 0")
        cldice_iterations = _check_iterations(cldice_iterations, "cldice_iterations")
        cldice_smooth = _check_smooth(cldice_smooth, "cldice_smooth")
        try:
            boundary_spacing = check_spacing(boundary_spacing)
        except TypeError:
            raise ValueError(f"boundary_spacing must be three positive sizes in mm, got {boundary_spacing!r}") from None
        if any(a > f32_max for a in boundary_spacing):
            raise ValueError(f"boundary_spacing must be finite in fp32, got {boundary_spacing!r}")
        if class_weights is not None:
            if isinstance(class_weights, torch.Tensor):
                class_weights = class_weights.detach().cpu().tolist()
            class_weights = tuple(class_weights)
            if not 2 <= len(class_weights) <= SEG_LOSS_MAX_CLASSES:
                raise ValueError(f"class_weights must hold 2..{SEG_LOSS_MAX_CLASSES} weights, got {len(class_weights)}")
            class_weights = tuple(check_at_least(f"class_weights[{i}]", w, 0.0) for i, w in enumerate(class_weights))
        if ignore_index is not None:
            # the kernel compares the f32 label with float(ignore_index): exact up to 2^24
            if not plain_int(ignore_index) or abs(int(ignore_index)) > 2 ** 24:
                raise ValueError(f"ignore_index must be None or an int with |ignore_index| <= 2^24, got {ignore_index!r}")
            ignore_index = int(ignore_index)
        if top_k is not None:
            top_k = check_finite("top_k", top_k)
            if not 0.0 < top_k <= 1.0:
                raise ValueError(f"top_k must be None or a fraction in (0, 1], got {top_k!r}")
            if float(lambda_voxel) == 0.0:
                raise ValueError("top_k selects the voxels of the cross-entropy term: it needs lambda_voxel > 0")
            if float(lambda_boundary) > 0.0:
                raise ValueError("top_k together with lambda_boundary > 0 is not supported")
            if float(lambda_cldice) > 0.0:
                raise ValueError("top_k together with lambda_cldice > 0 is not supported")
        self._set(alpha=float(alpha), beta=float(beta), batch=check_flag("batch", batch),
                  include_background=check_flag("include_background", include_background), focal_gamma=gamma,
                  class_weights=class_weights, ignore_index=ignore_index, lambda_region=float(lambda_region),
                  lambda_voxel=float(lambda_voxel), top_k=top_k, lambda_boundary=float(lambda_boundary),
                  boundary_spacing=boundary_spacing, lambda_cldice=float(lambda_cldice),
                  cldice_iterations=cldice_iterations, cldice_smooth=cldice_smooth)


def _seg_loss_torch(z: torch.Tensor, y: torch.Tensor, spec: SegLossSpec, w: Optional[torch.Tensor], record=None) -> torch.Tensor:
    """The formulas of ``seg_loss`` in plain torch ops, differentiable by autograd: z [B, vol, C], y [B, vol] labels.
    ``record``: a list that receives (N, k, tau, n_gt, n_eq) of a top-k call."""
    B, _, Cc = z.shape
    y = y.to(z.dtype if z.dtype in (torch.float32, torch.float64) else torch.float32)
    valid = (y >= 0) & (y < Cc) & (y == y.floor())
    if spec.ignore_index is not None:
        valid = valid & (y != spec.ignore_index)
    idx = torch.where(valid, y, torch.zeros_like(y)).long()
    m = valid.to(z.dtype).unsqueeze(-1)
    hot = F.one_hot(idx, Cc).to(z.dtype)
    logp = F.log_softmax(z, dim=-1)
    p = logp.exp()
    t, pm = hot * m, p * m
    dims = (0, 1) if spec.batch else (1,)
    c0 = 0 if spec.include_background else 1
    inter, psum, tsum = (pm * t).sum(dims)[..., c0:], pm.sum(dims)[..., c0:], t.sum(dims)[..., c0:]
    s = SEG_LOSS_SMOOTH
    tversky = (2.0 * inter + s) / (2.0 * inter + 2.0 * spec.alpha * (psum - inter) + 2.0 * spec.beta * (tsum - inter) + s)
    loss = spec.lambda_region * (1.0 - tversky).mean()
    if spec.lambda_voxel > 0.0:
        wt = torch.ones(Cc, dtype=z.dtype, device=z.device) if w is None else w.to(z.dtype)
        wy = wt[idx] * m[..., 0]
        f = -(logp * hot).sum(-1)
        if spec.focal_gamma > 0.0:
            f = f * (p * (1.0 - hot)).sum(-1) ** spec.focal_gamma             # 1 - p_y as the sum of the other classes
        if spec.top_k is not None:
            return loss + spec.lambda_voxel * _top_k_mean((wt[idx] * f)[valid], spec.top_k, record)
        wsum = wy.sum()
        loss = loss + spec.lambda_voxel * ((wy * f).sum() / torch.where(wsum > 0, wsum, torch.ones_like(wsum)))
    return loss


def _top_k_mean(u: torch.Tensor, top_k: float, record=None) -> torch.Tensor:
    """Mean of the k = max(1, floor(top_k N)) largest of the N values u (1-D); values equal to the k-th largest tau share
    the weight the larger ones leave, rho = (k - n_gt) / n_eq each: the value of ``torch.topk(u, k)[0].mean()`` with a
    gradient that does not depend on the order of equal values.  N == 0 gives 0."""
    n = u.numel()
    k = max(1, math.floor(top_k * n))
    if n == 0:
        if record is not None:
            record.append((0, k, u.new_zeros(()), 0, 0))
        return u.sum()
    tau = torch.topk(u.detach(), k, sorted=True).values[-1]
    gt, eq = u.detach() > tau, u.detach() == tau
    n_gt, n_eq = int(gt.sum()), int(eq.sum())
    if record is not None:
        record.append((n, k, tau, n_gt, n_eq))
    return (u[gt].sum() + u[eq].sum() * ((k - n_gt) / n_eq)) / k


class _SegLossFn(torch.autograd.Function):
    """Like ``train._DiceFocalFn``: the value from one streaming pass + a one-workgroup reduction; the gradient from a second
    streaming pass when backward asks for it, already multiplied by the incoming gradient (csrc/segloss.hip)."""

    @staticmethod
    def forward(ctx, logits_cl, target, weights, spec):
        B, H, W, D, Cc = logits_cl.shape
        vol = H * W * D
        ws = torch.empty(L.lib().mivp_seg_loss_ws(B, vol), dtype=torch.float32, device=logits_cl.device)
        loss = torch.empty(1, dtype=torch.float32, device=logits_cl.device)
        ig = spec.ignore_index
        L.call("mivp_seg_loss", L.ptr(logits_cl), L.ptr(target), B, vol, Cc, 1 if spec.include_background else 0,
               1 if spec.batch else 0, spec.alpha, spec.beta, spec.focal_gamma, L.ptr(weights), 0 if ig is None else ig,
               0 if ig is None else 1, spec.lambda_region, spec.lambda_voxel, L.ptr(ws), L.ptr(loss), L.ptr(None), L.stream())
        ctx.save_for_backward(logits_cl, target, ws)
        ctx.weights, ctx.spec = weights, spec
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits_cl, target, ws = ctx.saved_tensors
        spec, ig = ctx.spec, ctx.spec.ignore_index
        B, H, W, D, Cc = logits_cl.shape
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        L.call("mivp_seg_loss_grad", L.ptr(logits_cl), L.ptr(target), B, H * W * D, Cc, 1 if spec.include_background else 0,
               1 if spec.batch else 0, spec.alpha, spec.beta, spec.focal_gamma, L.ptr(ctx.weights), 0 if ig is None else ig,
               0 if ig is None else 1, spec.lambda_region, spec.lambda_voxel, L.ptr(ws), L.ptr(g), L.ptr(dz), L.stream())
        return dz, None, None, None


def _seg_topk_record_offset(B: int, vol: int) -> int:
    """Word offset of the record in a mivp_seg_topk workspace (include/mivp.h)."""
    return (int(L.lib().mivp_seg_loss_ws(B, vol)) + 3) // 4 * 4


class _SegTopkFn(torch.autograd.Function):
    """``_SegLossFn`` with the top-k voxel term (csrc/segtopk.hip).  The caller owns the workspace: it holds the record that
    ``SegLoss.top_k_stats`` reads."""

    @staticmethod
    def forward(ctx, logits_cl, target, weights, spec, ws):
        B, H, W, D, Cc = logits_cl.shape
        loss = torch.empty(1, dtype=torch.float32, device=logits_cl.device)
        ig = spec.ignore_index
        L.call("mivp_seg_topk", L.ptr(logits_cl), L.ptr(target), B, H * W * D, Cc, 1 if spec.include_background else 0,
               1 if spec.batch else 0, spec.alpha, spec.beta, spec.focal_gamma, L.ptr(weights), 0 if ig is None else ig,
               0 if ig is None else 1, spec.lambda_region, spec.lambda_voxel, spec.top_k, L.ptr(ws), L.ptr(loss), L.ptr(None),
               L.stream())
        ctx.save_for_backward(logits_cl, target, ws)
        ctx.weights, ctx.spec = weights, spec
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits_cl, target, ws = ctx.saved_tensors
        spec, ig = ctx.spec, ctx.spec.ignore_index
        B, H, W, D, Cc = logits_cl.shape
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        L.call("mivp_seg_topk_grad", L.ptr(logits_cl), L.ptr(target), B, H * W * D, Cc, 1 if spec.include_background else 0,
               1 if spec.batch else 0, spec.alpha, spec.beta, spec.focal_gamma, L.ptr(ctx.weights), 0 if ig is None else ig,
               0 if ig is None else 1, spec.lambda_region, spec.lambda_voxel, spec.top_k, L.ptr(ws), L.ptr(g), L.ptr(dz),
               L.stream())
        return dz, None, None, None, None


# ---------------------------------------------------------------------------------------------
# Boundary (signed-distance) term: batched distance maps + a fused value / gradient pass (csrc/distmap.hip)
# ---------------------------------------------------------------------------------------------
def _check_ignore(ignore_index):
    if ignore_index is None:
        return None
    if not plain_int(ignore_index) or abs(int(ignore_index)) > 2 ** 24:
        raise ValueError(f"ignore_index must be None or an int with |ignore_index| <= 2^24, got {ignore_index!r}")
    return int(ignore_index)


def _label_batch(target: torch.Tensor):
    """``[B, 1, H, W, D]`` or ``[B, H, W, D]`` labels of any dtype -> (contiguous f32 ``[B, H, W, D]``, (H, W, D))."""
    if target.dim() == 5 and target.shape[1] == 1:
        target = target[:, 0]
    if target.dim() != 4:
        raise ValueError(f"target must be [B, 1, H, W, D] or [B, H, W, D], got {tuple(target.shape)}")
    return target.detach().to(torch.float32).contiguous(), tuple(int(v) for v in target.shape[1:])


def _distmap_launch(tgt: torch.Tensor, dims, num_classes: int, spacing, include_background: bool, ignore_index) -> torch.Tensor:
    """tgt f32 [B, ...] with prod(dims) voxels per sample -> phi f32 [B, K, H, W, D]; the four launches, nothing else."""
    B = tgt.shape[0]
    K = num_classes - (0 if include_background else 1)
    H, W, D = dims
    if H > 65535 or W > 65535 or B * K * H * W * D >= 2 ** 31:
        raise ValueError(f"distance maps of {B} x {K} x {dims}: H and W must be <= 65535 and B K H W D < 2^31")
    phi = torch.empty((B, K, H, W, D), dtype=torch.float32, device=tgt.device)
    ws = torch.empty(max(int(L.lib().mivp_distmap_ws(B, K, i3(dims))), 1), dtype=torch.uint8, device=tgt.device)
    L.call("mivp_distmap_signed", L.ptr(tgt), B, num_classes, 1 if include_background else 0,
           0 if ignore_index is None else ignore_index, 0 if ignore_index is None else 1, i3(dims), (C.c_float * 3)(*spacing),
           L.ptr(phi), L.ptr(ws), L.stream())
    return phi


def signed_distance_maps(target: torch.Tensor, num_classes: int, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                         include_background: bool = False, ignore_index: Optional[int] = None) -> torch.Tensor:
    """Signed Euclidean distance maps of a batch of label maps, on the GPU.  ``target [B, 1, H, W, D]`` (or ``[B, H, W, D]``)
    class indices of any dtype -> float32 ``phi [B, K, H, W, D]`` for the classes c0 .. num_classes - 1 (c0 = 0 with
    ``include_background``, else 1).  Per sample and class, M = {label == c}; a label that is no class for ``seg_loss``
    (non-integer, outside [0, num_classes), or equal to ``ignore_index``) belongs to no M::

        phi = distance to the nearest voxel of M                at voxels outside M     (> 0)
        phi = -(distance to the nearest voxel outside M - 1)    at voxels inside M      (<= 0 at unit spacing)
        phi = 0 everywhere                                      when M is empty or the whole sample

    with distances ``sqrt(sum_a (spacing[a] delta_a)^2)``: ``one_hot2dist`` of the boundary-loss authors,
    ``edt(~M, spacing) * ~M - (edt(M, spacing) - 1) * M`` with scipy's ``distance_transform_edt``.  Exact (the squared
    distances are the exact integers at unit spacing), four launches whatever the batch and class counts are, nothing read
    back: recordable.  H, W <= 65535 and B K H W D < 2^31."""
    sp = check_spacing(spacing)
    ncls = check_classes(num_classes)
    check_gpu("target", target)
    bg = check_flag("include_background", include_background)
    ig = _check_ignore(ignore_index)
    if ncls - (0 if bg else 1) < 1:
        raise ValueError("num_classes=1 has no foreground class: pass include_background=True")
    tgt, dims = _label_batch(target)
    return _distmap_launch(tgt, dims, ncls, sp, bg, ig)


class _BoundaryFn(torch.autograd.Function):
    """The boundary term alone: value from a streaming pass + a one-workgroup reduction, the gradient from a second
    streaming pass when backward asks for it (csrc/distmap.hip).  ``phi`` and ``weight`` are constants."""

    @staticmethod
    def forward(ctx, logits_cl, target, phi, weight, bg, ig, lam):
        B, H, W, D, Cc = logits_cl.shape
        vol = H * W * D
        ws = torch.empty(L.lib().mivp_boundary_loss_ws(B, vol), dtype=torch.float32, device=logits_cl.device)
        loss = torch.empty(1, dtype=torch.float32, device=logits_cl.device)
        L.call("mivp_boundary_loss", L.ptr(logits_cl), L.ptr(target), L.ptr(phi), B, vol, Cc, 1 if bg else 0,
               0 if ig is None else ig, 0 if ig is None else 1, lam, L.ptr(weight), L.ptr(ws), L.ptr(loss), L.ptr(None), 0,
               L.stream())
        ctx.save_for_backward(logits_cl, target, phi, ws)
        ctx.weight, ctx.opts = weight, (bg, ig, lam)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits_cl, target, phi, ws = ctx.saved_tensors
        B, H, W, D, Cc = logits_cl.shape
        bg, ig, lam = ctx.opts
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        L.call("mivp_boundary_loss_grad", L.ptr(logits_cl), L.ptr(target), L.ptr(phi), B, H * W * D, Cc, 1 if bg else 0,
               0 if ig is None else ig, 0 if ig is None else 1, lam, L.ptr(ctx.weight), L.ptr(ws), L.ptr(g), L.ptr(dz), 0,
               L.stream())
        return dz, None, None, None, None, None, None


class _SegBoundaryFn(torch.autograd.Function):
    """``_SegLossFn`` plus the boundary term: mivp_seg_loss, the distance maps of the step's labels, mivp_boundary_loss; the
    backward runs mivp_seg_loss_grad and adds the boundary term's gradient onto the same ``dz`` (accumulate = 1)."""

    @staticmethod
    def forward(ctx, logits_cl, target, weights, spec, bweight):
        B, H, W, D, Cc = logits_cl.shape
        vol = H * W * D
        dev = logits_cl.device
        ws = torch.empty(L.lib().mivp_seg_loss_ws(B, vol), dtype=torch.float32, device=dev)
        bws = torch.empty(L.lib().mivp_boundary_loss_ws(B, vol), dtype=torch.float32, device=dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        ig = spec.ignore_index
        L.call("mivp_seg_loss", L.ptr(logits_cl), L.ptr(target), B, vol, Cc, 1 if spec.include_background else 0,
               1 if spec.batch else 0, spec.alpha, spec.beta, spec.focal_gamma, L.ptr(weights), 0 if ig is None else ig,
               0 if ig is None else 1, spec.lambda_region, spec.lambda_voxel, L.ptr(ws), L.ptr(loss), L.ptr(None), L.stream())
        phi = _distmap_launch(target, (H, W, D), Cc, spec.boundary_spacing, spec.include_background, ig)
        L.call("mivp_boundary_loss", L.ptr(logits_cl), L.ptr(target), L.ptr(phi), B, vol, Cc,
               1 if spec.include_background else 0, 0 if ig is None else ig, 0 if ig is None else 1, spec.lambda_boundary,
               L.ptr(bweight), L.ptr(bws), C.c_void_p(loss.data_ptr() + 4), L.ptr(None), 0, L.stream())
        ctx.save_for_backward(logits_cl, target, ws, phi, bws)
        ctx.weights, ctx.spec, ctx.bweight = weights, spec, bweight
        return loss[0] + loss[1]

    @staticmethod
    def backward(ctx, g):
        logits_cl, target, ws, phi, bws = ctx.saved_tensors
        spec, ig = ctx.spec, ctx.spec.ignore_index
        B, H, W, D, Cc = logits_cl.shape
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        L.call("mivp_seg_loss_grad", L.ptr(logits_cl), L.ptr(target), B, H * W * D, Cc, 1 if spec.include_background else 0,
               1 if spec.batch else 0, spec.alpha, spec.beta, spec.focal_gamma, L.ptr(ctx.weights), 0 if ig is None else ig,
               0 if ig is None else 1, spec.lambda_region, spec.lambda_voxel, L.ptr(ws), L.ptr(g), L.ptr(dz), L.stream())
        L.call("mivp_boundary_loss_grad", L.ptr(logits_cl), L.ptr(target), L.ptr(phi), B, H * W * D, Cc,
               1 if spec.include_background else 0, 0 if ig is None else ig, 0 if ig is None else 1, spec.lambda_boundary,
               L.ptr(ctx.bweight), L.ptr(bws), L.ptr(g), L.ptr(dz), 1, L.stream())
        return dz, None, None, None, None


def _boundary_torch(z: torch.Tensor, y: torch.Tensor, dist: torch.Tensor, bg: bool, ig, weight) -> torch.Tensor:
    """The formulas of ``boundary_loss`` in plain torch ops, differentiable by autograd: z [B, vol, C], y [B, vol] labels,
    dist [B, K, vol]."""
    Cc = z.shape[-1]
    y = y.to(z.dtype if z.dtype in (torch.float32, torch.float64) else torch.float32)
    valid = (y >= 0) & (y < Cc) & (y == y.floor())
    if ig is not None:
        valid = valid & (y != ig)
    c0 = 0 if bg else 1
    p = torch.softmax(z, dim=-1)[..., c0:]
    num = (p * dist.to(z.dtype).transpose(1, 2) * valid.to(z.dtype).unsqueeze(-1)).sum()
    loss = num / ((Cc - c0) * valid.sum().clamp(min=1).to(z.dtype))
    return loss if weight is None else loss * weight.to(z.dtype).reshape(())


def _check_boundary_weight(weight, device):
    if weight is None:
        return None
    if not isinstance(weight, torch.Tensor) or weight.numel() != 1:
        raise ValueError("weight must be None or a tensor holding one number")
    if weight.device != device:
        raise ValueError(f"weight must be on the logits' device {device}, got {weight.device}")
    return weight.detach()


def boundary_loss(logits: torch.Tensor, target: torch.Tensor, *, include_background: bool = False,
                  ignore_index: Optional[int] = None, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                  dist: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The boundary loss of Kervadec et al. (MIDL 2019).  logits [B, C, H, W, D], target [B, 1, H, W, D] (or [B, H, W, D])
    class indices of any dtype.  With p = softmax_c(z), phi = ``signed_distance_maps(target, C, spacing, ...)`` (or ``dist``,
    [B, K, H, W, D], when given), V the valid voxels of the batch (the rule of ``seg_loss``), N = |V|, K = C - c0::

        loss = weight sum_{v in V} sum_{c >= c0} p_c(v) phi_c(v) / (K max(N, 1))

    ``weight``: a one-element tensor on the logits' device (None = 1) that is read on the device, so a recorded step follows
    a schedule of it.  ``phi`` is a constant of the step.  Channels-last f32 CUDA logits with C <= 8 take the kernels: the
    four launches of the maps (unless ``dist`` is given), then two streaming passes; nothing read back, recordable.  Any
    other layout, dtype or device takes the same formulas as plain torch ops and needs ``dist``."""
    if logits.dim() != 5:
        raise ValueError(f"logits must be [B, C, H, W, D], got {tuple(logits.shape)}")
    B, Cc = logits.shape[0], logits.shape[1]
    if Cc < 2:
        raise ValueError(f"logits must have at least 2 classes, got {Cc}")
    if target.numel() != logits.numel() // Cc or target.shape[0] != B:
        raise ValueError(f"target must be [B, 1, H, W, D] for logits {tuple(logits.shape)}, got {tuple(target.shape)}")
    bg = check_flag("include_background", include_background)
    ig = _check_ignore(ignore_index)
    sp = check_spacing(spacing)
    weight = _check_boundary_weight(weight, logits.device)
    K = Cc - (0 if bg else 1)
    dims = tuple(int(v) for v in logits.shape[2:])
    if dist is not None:
        if not isinstance(dist, torch.Tensor) or tuple(dist.shape) != (B, K) + dims or dist.device != logits.device:
            raise ValueError(f"dist must be a [B, K, H, W, D] = {(B, K) + dims} tensor on the logits' device, got "
                             f"{tuple(dist.shape) if isinstance(dist, torch.Tensor) else dist!r}")
        dist = dist.detach()
    base = logits.permute(0, 2, 3, 4, 1)
    if logits.is_cuda and logits.dtype == torch.float32 and base.is_contiguous() and Cc <= SEG_LOSS_MAX_CLASSES:
        tgt = target.detach().to(torch.float32).contiguous()
        phi = _distmap_launch(tgt, dims, Cc, sp, bg, ig) if dist is None else dist.to(torch.float32).contiguous()
        if weight is not None:
            weight = weight.to(torch.float32).contiguous()
        return _BoundaryFn.apply(base, tgt, phi, weight, bg, ig, 1.0)
    if dist is None:
        raise RuntimeError("boundary_loss: only channels-last f32 GPU logits with at most 8 classes build their distance maps "
                           "(on the device); any other layout, dtype or device needs dist=, e.g. signed_distance_maps(target, "
                           "...) of a GPU copy of the labels (the package does not import scipy)")
    return _boundary_torch(base.reshape(B, -1, Cc), target.detach().reshape(B, -1), dist.reshape(B, K, -1), bg, ig, weight)


# ---------------------------------------------------------------------------------------------
# clDice (soft-skeleton) term: brick kernels for the skeleton and its backward (csrc/cldice.hip)
# ---------------------------------------------------------------------------------------------
_CROSS = ((0, 0, 0), (0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0))
_CUBE = tuple((a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))


def _shifted(xp: torch.Tensor, off) -> torch.Tensor:
    """The one-voxel-padded tensor seen from every voxel v at v + off."""
    h, w, d = (n - 2 for n in xp.shape[-3:])
    return xp[..., 1 + off[0]:1 + off[0] + h, 1 + off[1]:1 + off[1] + w, 1 + off[2]:1 + off[2] + d]


class _WindowPoolFn(torch.autograd.Function):
    """min (7-point cross) or max (3x3x3 cube) over the window inside the volume, as plain torch ops.  Backward: the voxels
    of a window that hold the selected value share its gradient equally (``max_pool3d`` gives all to the first)."""

    @staticmethod
    def forward(ctx, x, is_max):
        window = _CUBE if is_max else _CROSS
        xp = F.pad(x, (1,) * 6, value=float("-inf") if is_max else float("inf"))
        out = _shifted(xp, window[0]).clone()
        for off in window[1:]:
            out = torch.maximum(out, _shifted(xp, off)) if is_max else torch.minimum(out, _shifted(xp, off))
        ctx.save_for_backward(x, out)
        ctx.window = window
        return out

    @staticmethod
    def backward(ctx, g):
        x, out = ctx.saved_tensors
        xp = F.pad(x, (1,) * 6, value=float("nan"))
        k = torch.zeros_like(x)
        for off in ctx.window:
            k = k + (_shifted(xp, off) == out).to(x.dtype)
        hp = F.pad(g / k.clamp(min=1.0), (1,) * 6, value=0.0)
        mp = F.pad(out, (1,) * 6, value=float("nan"))
        gx = torch.zeros_like(x)
        for off in ctx.window:
            back = tuple(-o for o in off)
            gx = gx + torch.where(_shifted(mp, back) == x, _shifted(hp, back), torch.zeros_like(x))
        return gx, None


def _relu0(x: torch.Tensor) -> torch.Tensor:
    return torch.where(x > 0, x, torch.zeros_like(x))               # +0 at 0 and below, gradient 0 there


def _soft_skeleton_torch(x: torch.Tensor, n: int) -> torch.Tensor:
    """The definition of ``soft_skeleton`` in plain torch ops on [..., H, W, D]."""
    e = x
    s = None
    for j in range(n + 1):
        e1 = _WindowPoolFn.apply(e, False)
        d = _relu0(e - _WindowPoolFn.apply(e1, True))
        s = d if j == 0 else s + _relu0(d - s * d)
        e = e1
    return s


class _SkeletonFn(torch.autograd.Function):
    """``soft_skeleton`` on the kernels: n + 1 launches forward, n + 3 backward."""

    @staticmethod
    def forward(ctx, x, n):
        B, K, H, W, D = x.shape
        keep = 1 if ctx.needs_input_grad[0] else 0
        ws = torch.empty(max(int(L.lib().mivp_cldice_skeleton_ws(B * K, i3((H, W, D)), n, keep)), 1), dtype=torch.float32,
                         device=x.device)
        out = torch.empty_like(x)
        L.call("mivp_cldice_skeleton", L.ptr(x), B * K, i3((H, W, D)), n, L.ptr(out), L.ptr(ws), keep, L.stream())
        ctx.save_for_backward(x, ws)
        ctx.n, ctx.spent = n, False
        return out

    @staticmethod
    def backward(ctx, g):
        x, ws = ctx.saved_tensors
        if ctx.spent:
            raise RuntimeError("soft_skeleton: the backward overwrites its workspace; a second backward needs a new forward")
        ctx.spent = True
        B, K, H, W, D = x.shape
        g = g.detach().to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        L.call("mivp_cldice_skeleton_grad", L.ptr(x), L.ptr(g), B * K, i3((H, W, D)), ctx.n, L.ptr(ws), L.ptr(dx), L.stream())
        return dx, None


def soft_skeleton(x: torch.Tensor, iterations: int = 3) -> torch.Tensor:
    """The soft skeleton of the clDice authors (``soft_skel``), differentiable.  x [B, K, H, W, D], finite; with::

        erode(x)(v)  = min of x over v and its 6 face neighbours inside the volume
        dilate(x)(v) = max of x over the 3x3x3 cube around v inside the volume
        E_0 = x, E_{j+1} = erode(E_j);  O_j = dilate(E_{j+1});  d_j = relu(E_j - O_j)            j = 0 .. iterations
        S_0 = d_0, S_j = S_{j-1} + relu(d_j - S_{j-1} d_j)

    it returns S_iterations, every operation rounded on its own.  Backward: the voxels of a window that hold the selected
    minimum / maximum share its gradient equally (so it does not depend on memory order), relu'(0) = 0.  Contiguous f32
    CUDA tensors take the kernels (csrc/cldice.hip; one backward per forward); anything else the same definition as plain
    torch ops."""
    if not isinstance(x, torch.Tensor) or x.dim() != 5:
        raise ValueError(f"x must be a [B, K, H, W, D] tensor, got {tuple(x.shape) if isinstance(x, torch.Tensor) else x!r}")
    n = _check_iterations(iterations)
    if x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0:
        return _SkeletonFn.apply(x, n)
    return _soft_skeleton_torch(x, n)


def _cldice_torch(z: torch.Tensor, y: torch.Tensor, dims, n: int, smooth: float, batch: bool, ig, weight) -> torch.Tensor:
    """The formulas of ``cldice_loss`` in plain torch ops: z [B, vol, C], y [B, vol] labels."""
    B, _, Cc = z.shape
    y = y.to(z.dtype if z.dtype in (torch.float32, torch.float64) else torch.float32)
    valid = (y >= 0) & (y < Cc) & (y == y.floor())
    if ig is not None:
        valid = valid & (y != ig)
    idx = torch.where(valid, y, torch.zeros_like(y)).long()
    m = valid.to(z.dtype).unsqueeze(-1)
    p = (torch.softmax(z, dim=-1) * m)[..., 1:].transpose(1, 2).reshape(B, Cc - 1, *dims)
    t = (F.one_hot(idx, Cc).to(z.dtype) * m)[..., 1:].transpose(1, 2).reshape(B, Cc - 1, *dims)
    sp, sl = _soft_skeleton_torch(p, n), _soft_skeleton_torch(t, n)
    ax = (0, 2, 3, 4) if batch else (2, 3, 4)
    tprec = ((sp * t).sum(ax) + smooth) / (sp.sum(ax) + smooth)
    tsens = ((sl * p).sum(ax) + smooth) / (sl.sum(ax) + smooth)
    loss = (1.0 - 2.0 * tprec * tsens / (tprec + tsens)).mean()
    return loss if weight is None else loss * weight.to(z.dtype).reshape(())


def _cldice_args(spec_or_opts):
    n, smooth, batch, ig, lam = spec_or_opts
    return n, smooth, 1 if batch else 0, 0 if ig is None else ig, 0 if ig is None else 1, lam


class _ClDiceFn(torch.autograd.Function):
    """The clDice term alone (csrc/cldice.hip).  ``weight`` is a constant; opts = (iterations, smooth, batch, ignore, lambda)."""

    @staticmethod
    def forward(ctx, logits_cl, target, weight, opts):
        B, H, W, D, Cc = logits_cl.shape
        d3 = i3((H, W, D))
        n, smooth, batch, ign, has, lam = _cldice_args(opts)
        ws = torch.empty(int(L.lib().mivp_cldice_ws(B, Cc, d3, n)), dtype=torch.float32, device=logits_cl.device)
        loss = torch.empty(1, dtype=torch.float32, device=logits_cl.device)
        L.call("mivp_cldice_loss", L.ptr(logits_cl), L.ptr(target), B, Cc, d3, n, smooth, batch, ign, has, lam, L.ptr(weight),
               L.ptr(ws), L.ptr(loss), L.ptr(None), 0, L.stream())
        ctx.save_for_backward(logits_cl, target, ws)
        ctx.weight, ctx.opts, ctx.spent = weight, opts, False
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits_cl, target, ws = ctx.saved_tensors
        if ctx.spent:
            raise RuntimeError("cldice_loss: the backward overwrites its workspace; a second backward needs a new forward")
        ctx.spent = True
        B, H, W, D, Cc = logits_cl.shape
        n, smooth, batch, ign, has, lam = _cldice_args(ctx.opts)
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        L.call("mivp_cldice_loss_grad", L.ptr(logits_cl), L.ptr(target), B, Cc, i3((H, W, D)), n, smooth, batch, ign, has, lam,
               L.ptr(ctx.weight), L.ptr(ws), L.ptr(g), L.ptr(dz), 0, L.stream())
        return dz, None, None, None


class _SegTermsFn(torch.autograd.Function):
    """The region + voxel terms (when either lambda is > 0), the boundary term (when lambda_boundary > 0) and the clDice
    term, in that order; the backward runs their gradient passes in the same order, the first storing ``dz`` and the
    others adding onto it (accumulate = 1)."""

    @staticmethod
    def forward(ctx, logits_cl, target, weights, spec, bweight, cweight):
        B, H, W, D, Cc = logits_cl.shape
        vol, dev, ig = H * W * D, logits_cl.device, spec.ignore_index
        ign, has, bg = 0 if ig is None else ig, 0 if ig is None else 1, 1 if spec.include_background else 0
        d3 = i3((H, W, D))
        loss = torch.zeros(3, dtype=torch.float32, device=dev)
        saved = [logits_cl, target]
        ctx.base = spec.lambda_region > 0.0 or spec.lambda_voxel > 0.0
        ctx.boundary = spec.lambda_boundary > 0.0
        if ctx.base:
            ws = torch.empty(L.lib().mivp_seg_loss_ws(B, vol), dtype=torch.float32, device=dev)
            L.call("mivp_seg_loss", L.ptr(logits_cl), L.ptr(target), B, vol, Cc, bg, 1 if spec.batch else 0, spec.alpha, spec.beta,
                   spec.focal_gamma, L.ptr(weights), ign, has, spec.lambda_region, spec.lambda_voxel, L.ptr(ws), L.ptr(loss),
                   L.ptr(None), L.stream())
            saved.append(ws)
        if ctx.boundary:
            bws = torch.empty(L.lib().mivp_boundary_loss_ws(B, vol), dtype=torch.float32, device=dev)
            phi = _distmap_launch(target, (H, W, D), Cc, spec.boundary_spacing, spec.include_background, ig)
            L.call("mivp_boundary_loss", L.ptr(logits_cl), L.ptr(target), L.ptr(phi), B, vol, Cc, bg, ign, has,
                   spec.lambda_boundary, L.ptr(bweight), L.ptr(bws), C.c_void_p(loss.data_ptr() + 4), L.ptr(None), 0, L.stream())
            saved += [phi, bws]
        cws = torch.empty(int(L.lib().mivp_cldice_ws(B, Cc, d3, spec.cldice_iterations)), dtype=torch.float32, device=dev)
        L.call("mivp_cldice_loss", L.ptr(logits_cl), L.ptr(target), B, Cc, d3, spec.cldice_iterations, spec.cldice_smooth,
               1 if spec.batch else 0, ign, has, spec.lambda_cldice, L.ptr(cweight), L.ptr(cws), C.c_void_p(loss.data_ptr() + 8),
               L.ptr(None), 0, L.stream())
        saved.append(cws)
        ctx.save_for_backward(*saved)
        ctx.weights, ctx.spec, ctx.bweight, ctx.cweight, ctx.spent = weights, spec, bweight, cweight, False
        return (loss[0] + loss[1]) + loss[2]

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        logits_cl, target = saved[0], saved[1]
        rest = saved[2:]
        if ctx.spent:
            raise RuntimeError("seg_loss: the clDice backward overwrites its workspace; a second backward needs a new forward")
        ctx.spent = True
        spec, ig = ctx.spec, ctx.spec.ignore_index
        ign, has, bg = 0 if ig is None else ig, 0 if ig is None else 1, 1 if spec.include_background else 0
        B, H, W, D, Cc = logits_cl.shape
        vol = H * W * D
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        acc = 0
        if ctx.base:
            ws = rest.pop(0)
            L.call("mivp_seg_loss_grad", L.ptr(logits_cl), L.ptr(target), B, vol, Cc, bg, 1 if spec.batch else 0, spec.alpha,
                   spec.beta, spec.focal_gamma, L.ptr(ctx.weights), ign, has, spec.lambda_region, spec.lambda_voxel, L.ptr(ws),
                   L.ptr(g), L.ptr(dz), L.stream())
            acc = 1
        if ctx.boundary:
            phi, bws = rest.pop(0), rest.pop(0)
            L.call("mivp_boundary_loss_grad", L.ptr(logits_cl), L.ptr(target), L.ptr(phi), B, vol, Cc, bg, ign, has,
                   spec.lambda_boundary, L.ptr(ctx.bweight), L.ptr(bws), L.ptr(g), L.ptr(dz), acc, L.stream())
            acc = 1
        cws = rest.pop(0)
        L.call("mivp_cldice_loss_grad", L.ptr(logits_cl), L.ptr(target), B, Cc, i3((H, W, D)), spec.cldice_iterations,
               spec.cldice_smooth, 1 if spec.batch else 0, ign, has, spec.lambda_cldice, L.ptr(ctx.cweight), L.ptr(cws), L.ptr(g),
               L.ptr(dz), acc, L.stream())
        return dz, None, None, None, None, None


def cldice_loss(logits: torch.Tensor, target: torch.Tensor, *, iterations: int = 3, smooth: float = 1.0, batch: bool = False,
                ignore_index: Optional[int] = None, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The clDice loss of Shit et al. (CVPR 2021).  logits [B, C, H, W, D], target [B, 1, H, W, D] (or [B, H, W, D]) class
    indices of any dtype.  p = softmax_c(z) and t = one-hot(label), both taken as 0 at invalid voxels (the rule of
    ``seg_loss``; ``dz`` is exactly 0 there); classes c >= 1 always (the skeleton of the background is not meaningful);
    with SP_c = ``soft_skeleton(p_c, iterations)``, SL_c = ``soft_skeleton(t_c, iterations)`` (a constant), s = ``smooth``
    and sums over the voxels of a sample (of the batch with ``batch``)::

        Tprec = (sum SP_c t_c + s) / (sum SP_c + s)        Tsens = (sum SL_c p_c + s) / (sum SL_c + s)
        loss  = weight mean over (b, c >= 1) [over c >= 1 with batch] of 1 - 2 Tprec Tsens / (Tprec + Tsens)

    ``weight``: a one-element tensor on the logits' device (None = 1), read on the device.  Channels-last f32 CUDA logits
    with C <= 8 take the kernels (2 n + 8 launches for value and gradient, nothing read back, recordable; one backward per
    forward); any other layout, dtype or device takes the same formulas as plain torch ops."""
    if logits.dim() != 5:
        raise ValueError(f"logits must be [B, C, H, W, D], got {tuple(logits.shape)}")
    B, Cc = logits.shape[0], logits.shape[1]
    if Cc < 2:
        raise ValueError(f"logits must have at least 2 classes, got {Cc}")
    if target.numel() != logits.numel() // Cc or target.shape[0] != B:
        raise ValueError(f"target must be [B, 1, H, W, D] for logits {tuple(logits.shape)}, got {tuple(target.shape)}")
    n = _check_iterations(iterations)
    s = _check_smooth(smooth)
    bt = check_flag("batch", batch)
    ig = _check_ignore(ignore_index)
    weight = _check_boundary_weight(weight, logits.device)
    dims = tuple(int(v) for v in logits.shape[2:])
    base = logits.permute(0, 2, 3, 4, 1)
    if logits.is_cuda and logits.dtype == torch.float32 and base.is_contiguous() and Cc <= SEG_LOSS_MAX_CLASSES:
        tgt = target.detach().to(torch.float32).contiguous()
        if weight is not None:
            weight = weight.to(torch.float32).contiguous()
        return _ClDiceFn.apply(base, tgt, weight, (n, s, bt, ig, 1.0))
    return _cldice_torch(base.reshape(B, -1, Cc), target.detach().reshape(B, -1), dims, n, s, bt, ig, weight)


_seg_weight_cache = {}


def _seg_weights(spec: SegLossSpec, class_weights, n_classes: int, device) -> Optional[torch.Tensor]:
    """The weight table on ``device`` (f32 [C]) or None; ``class_weights`` (a tensor) takes precedence over the spec's tuple,
    whose device copy is made once per (weights, device) -- outside a recording."""
    if class_weights is None:
        if spec.class_weights is None:
            return None
        key = (spec.class_weights, str(device))
        if key not in _seg_weight_cache:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("seg_loss: first use of these class_weights inside a recording; run one eager step first "
                                   "or pass the device tensor (losses.SegLoss owns one)")
            _seg_weight_cache[key] = torch.tensor(spec.class_weights, dtype=torch.float32, device=device)
        class_weights = _seg_weight_cache[key]
    if not isinstance(class_weights, torch.Tensor) or class_weights.dim() != 1 or class_weights.shape[0] != n_classes:
        raise ValueError(f"class_weights must hold one weight per class ({n_classes}), got "
                         f"{tuple(class_weights.shape) if isinstance(class_weights, torch.Tensor) else class_weights!r}")
    if class_weights.device != device:
        raise ValueError(f"class_weights must be on the logits' device {device}, got {class_weights.device}")
    return class_weights


def seg_loss(logits: torch.Tensor, target: torch.Tensor, spec: SegLossSpec,
             class_weights: Optional[torch.Tensor] = None, _record=None,
             boundary_weight: Optional[torch.Tensor] = None, cldice_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Tversky region term + weighted (focal) softmax cross-entropy with an ignore label.  logits [B, C, H, W, D], target
    [B, 1, H, W, D] (or [B, H, W, D]) class indices of any dtype; ``class_weights``: a [C] tensor on the logits' device that
    replaces ``spec.class_weights``.

    A voxel is valid when its label is an integer in [0, C) other than ``spec.ignore_index``; an invalid voxel adds to no
    sum and gets an exactly zero gradient.  With p = softmax_c(z), t = one-hot(label), sums over the valid voxels of a sample
    (of the batch when ``spec.batch``) and s = 1e-5::

        TI_c   = (2 I_c + s) / (2 I_c + 2 alpha (P_c - I_c) + 2 beta (T_c - I_c) + s),  I = sum p t, P = sum p, T = sum t
        region = mean over (b, c >= c0) [over c >= c0 when batch] of 1 - TI_c
        voxel  = - sum_v w[y_v] (1 - p_y)^focal_gamma log p_y / sum_v w[y_v]     (valid voxels of the batch; 0 when the sum is 0)
        loss   = lambda_region region + lambda_voxel voxel

    alpha = beta = 0.5 is ``dice_loss``'s Dice, in general MONAI's ``TverskyLoss(smooth_nr = smooth_dr = s / 2)``; focal_gamma
    = 0 is ``F.cross_entropy(weight=, ignore_index=, reduction="mean")``.

    With ``spec.top_k`` the voxel term is the mean over the hardest voxels of the batch only (nnU-Net's
    ``DC_and_topk_loss``).  Over the N valid voxels of the batch, u_v = w[y_v] (1 - p_y)^focal_gamma (-log p_y),
    k = max(1, floor(top_k N)), tau = the k-th largest u, n_gt = #{u > tau}, n_eq = #{u == tau}::

        voxel   = (sum_{u > tau} u + (k - n_gt) tau) / k                   (= torch.topk(u, k)[0].mean(); 0 when N == 0)
        d voxel = (1 / k) sum_v s_v d u_v,  s_v = 1 (u_v > tau), (k - n_gt) / n_eq (u_v == tau), 0 (u_v < tau)

    The normaliser is k, not the weight sum; tied voxels share the remaining weight equally, so the gradient does not
    depend on the order of the voxels; without ties it is autograd's through ``torch.topk``.  Finite logits only.

    With ``spec.lambda_boundary`` > 0 the loss gains ``lambda_boundary boundary_weight boundary`` with ``boundary`` the value
    of ``boundary_loss(logits, target, include_background=, ignore_index=, spacing=spec.boundary_spacing)``: the signed
    distance maps of the step's labels are built on the device inside the call.  ``boundary_weight``: a one-element tensor
    on the logits' device (None = 1), read on the device (``SegLoss`` owns one).

    With ``spec.lambda_cldice`` > 0 the loss gains ``lambda_cldice cldice_weight cldice`` with ``cldice`` the value of
    ``cldice_loss(logits, target, iterations=spec.cldice_iterations, smooth=spec.cldice_smooth, batch=spec.batch,
    ignore_index=)`` (classes c >= 1 whatever ``include_background`` says); ``cldice_weight`` like ``boundary_weight``.  Its
    gradient pass adds onto the same buffer as the other terms'.

    Channels-last f32 CUDA logits (the view the HIP model returns) with C <= 8 take the fused kernels: two streaming passes
    (with ``top_k``: an exact radix select on one stored 32-bit key per voxel between them; with the boundary term: the four
    launches of the maps and two more passes, the gradient added onto the same buffer), nothing read back, recordable.
    Any other layout, dtype or device takes the same formulas as plain torch ops (the boundary term then still needs GPU
    labels for its maps)."""
    if not isinstance(spec, SegLossSpec):
        raise TypeError(f"spec must be a SegLossSpec, got {type(spec).__name__}")
    if logits.dim() != 5:
        raise ValueError(f"logits must be [B, C, H, W, D], got {tuple(logits.shape)}")
    B, Cc = logits.shape[0], logits.shape[1]
    if Cc < 2:
        raise ValueError(f"logits must have at least 2 classes, got {Cc}")
    if target.numel() != logits.numel() // Cc or target.shape[0] != B:
        raise ValueError(f"target must be [B, 1, H, W, D] for logits {tuple(logits.shape)}, got {tuple(target.shape)}")
    w = _seg_weights(spec, class_weights, Cc, logits.device)
    base = logits.permute(0, 2, 3, 4, 1)
    boundary = spec.lambda_boundary > 0.0
    bw = _check_boundary_weight(boundary_weight, logits.device) if boundary else None
    cldice = spec.lambda_cldice > 0.0
    cw = _check_boundary_weight(cldice_weight, logits.device) if cldice else None
    if logits.is_cuda and logits.dtype == torch.float32 and base.is_contiguous() and Cc <= SEG_LOSS_MAX_CLASSES:
        tgt = target.detach().to(torch.float32).contiguous()
        if w is not None and (w.dtype != torch.float32 or not w.is_contiguous()):
            w = w.detach().float().contiguous()
        if cldice:
            bw = None if bw is None else bw.to(torch.float32).contiguous()
            cw = None if cw is None else cw.to(torch.float32).contiguous()
            return _SegTermsFn.apply(base, tgt, None if w is None else w.detach(), spec, bw, cw)
        if boundary:
            if bw is not None:
                bw = bw.to(torch.float32).contiguous()
            if spec.lambda_region == 0.0 and spec.lambda_voxel == 0.0:     # the boundary term alone
                dims = tuple(int(v) for v in logits.shape[2:])
                phi = _distmap_launch(tgt, dims, Cc, spec.boundary_spacing, spec.include_background, spec.ignore_index)
                return _BoundaryFn.apply(base, tgt, phi, bw, spec.include_background, spec.ignore_index, spec.lambda_boundary)
            return _SegBoundaryFn.apply(base, tgt, None if w is None else w.detach(), spec, bw)
        if spec.top_k is None:
            return _SegLossFn.apply(base, tgt, None if w is None else w.detach(), spec)
        vol = tgt.numel() // B
        ws = torch.empty(L.lib().mivp_seg_topk_ws(B, vol), dtype=torch.float32, device=logits.device)
        if _record is not None:
            off = _seg_topk_record_offset(B, vol)
            _record.append(ws[off:off + 5])
        return _SegTopkFn.apply(base, tgt, None if w is None else w.detach(), spec, ws)
    zf, yf = base.reshape(B, -1, Cc), target.detach().reshape(B, -1)
    if cldice:
        dims = tuple(int(v) for v in logits.shape[2:])
        term = spec.lambda_cldice * _cldice_torch(zf, yf, dims, spec.cldice_iterations, spec.cldice_smooth, spec.batch,
                                                  spec.ignore_index, cw)
        if not (boundary or spec.lambda_region > 0.0 or spec.lambda_voxel > 0.0):
            return term
        rest = SegLossSpec(**{**{k: getattr(spec, k) for k in SegLossSpec.__slots__}, "lambda_cldice": 0.0})
        return seg_loss(logits, target, rest, class_weights, _record, boundary_weight) + term
    if not boundary:
        return _seg_loss_torch(zf, yf, spec, None if w is None else w.detach(), _record)
    if not target.is_cuda:
        raise RuntimeError("seg_loss: the distance maps of the boundary term are built on the GPU (no CPU fallback, the "
                           "package does not import scipy); use boundary_loss(dist=...) with maps of your own")
    dist = signed_distance_maps(target, Cc, spec.boundary_spacing, spec.include_background, spec.ignore_index)
    term = spec.lambda_boundary * _boundary_torch(zf, yf, dist.reshape(B, dist.shape[1], -1), spec.include_background,
                                                  spec.ignore_index, bw)
    if spec.lambda_region == 0.0 and spec.lambda_voxel == 0.0:
        return term
    return _seg_loss_torch(zf, yf, spec, None if w is None else w.detach(), _record) + term


class SegLoss(torch.nn.Module):
    """``seg_loss`` as a module that owns the class-weight table as a buffer (it follows ``.to(device)``, so a recorded step
    reads a fixed device tensor).  ``train.step_loss`` uses ``conf.seg_loss`` when the configuration has one."""

    def __init__(self, spec: Optional[SegLossSpec] = None, **options):
        super().__init__()
        if spec is None:
            spec = SegLossSpec(**options)
        elif options or not isinstance(spec, SegLossSpec):
            raise TypeError("SegLoss takes a SegLossSpec or the options of one, not both")
        self.spec = spec
        self.register_buffer("class_weights", None if spec.class_weights is None
                             else torch.tensor(spec.class_weights, dtype=torch.float32))
        # the weight of the boundary term on the device: a recorded step reads it, ``set_boundary_weight`` schedules it
        self.register_buffer("boundary_weight", torch.ones(1, dtype=torch.float32), persistent=False)
        # the same for the clDice term
        self.register_buffer("cldice_weight", torch.ones(1, dtype=torch.float32), persistent=False)
        self._topk_record = None

    def set_cldice_weight(self, value: float) -> None:
        """Set the factor of the clDice term (``lambda_cldice`` times it is the term's weight), like ``set_boundary_weight``."""
        v = check_finite("cldice weight", value)
        if self.cldice_weight.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("SegLoss.set_cldice_weight inside a recording: a recording must not freeze today's weight "
                               "into the graph; call it between replays")
        self.cldice_weight.copy_(torch.tensor([v], dtype=torch.float32))

    def set_boundary_weight(self, value: float) -> None:
        """Set the factor of the boundary term (``lambda_boundary`` times it is the term's weight): a stream-ordered copy into
        the module's buffer, legal between the replays of a recorded step."""
        v = check_finite("boundary weight", value)
        if self.boundary_weight.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("SegLoss.set_boundary_weight inside a recording: a recording must not freeze today's weight "
                               "into the graph; call it between replays")
        self.boundary_weight.copy_(torch.tensor([v], dtype=torch.float32))

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.spec.lambda_cldice > 0.0:
            return seg_loss(logits, target, self.spec, self.class_weights, boundary_weight=self.boundary_weight,
                            cldice_weight=self.cldice_weight)
        if self.spec.lambda_boundary > 0.0:
            return seg_loss(logits, target, self.spec, self.class_weights, boundary_weight=self.boundary_weight)
        if self.spec.top_k is None:
            return seg_loss(logits, target, self.spec, self.class_weights)
        record = []
        loss = seg_loss(logits, target, self.spec, self.class_weights, record)
        self._topk_record = record[0]
        return loss

    def top_k_stats(self):
        """The select of the last call with ``top_k`` set: N valid voxels, k, the threshold tau, the voxels above it and
        the voxels tied at it.  The fused path keeps these words in its workspace on the device; this is the one explicit
        device-to-host copy of them (after a replay of a recorded step: that replay's)."""
        rec = self._topk_record
        if rec is None:
            raise RuntimeError("top_k_stats: no call with top_k set has run yet")
        if isinstance(rec, torch.Tensor):
            raw = rec.detach().cpu().contiguous().view(torch.int32).numpy()
            return dict(N=int(raw[0]), k=int(raw[1]), tau=float(raw[2:3].view(np.float32)[0]), n_gt=int(raw[3]), n_eq=int(raw[4]))
        n, k, tau, n_gt, n_eq = rec
        return dict(N=int(n), k=int(k), tau=float(tau), n_gt=int(n_gt), n_eq=int(n_eq))

    def extra_repr(self) -> str:
        return repr(self.spec)


# ---------------------------------------------------------------------------------------------
# Hausdorff distance-transform term: the fields of the hard prediction and of the labels, a weighted squared error
# (csrc/hausdorff.hip)
# ---------------------------------------------------------------------------------------------
def _check_alpha(alpha) -> float:
    a = check_finite("alpha", alpha)
    if not 0.0 < a <= 4.0:
        raise ValueError(f"alpha must be in (0, 4], got {alpha!r}")
    return a


def _hausdorff_args(logits, target, alpha, include_background, ignore_index, spacing):
    """The checks the three public entries share -> (alpha, bg, ig, spacing, B, C, K, dims)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 5:
        raise ValueError(f"logits must be [B, C, H, W, D], got {tuple(logits.shape) if isinstance(logits, torch.Tensor) else logits!r}")
    B, Cc = int(logits.shape[0]), int(logits.shape[1])
    if not 2 <= Cc <= SEG_LOSS_MAX_CLASSES:
        raise ValueError(f"logits must have 2 .. {SEG_LOSS_MAX_CLASSES} classes, got {Cc}")
    if not isinstance(target, torch.Tensor) or target.numel() != logits.numel() // Cc or target.shape[0] != B:
        raise ValueError(f"target must be [B, 1, H, W, D] for logits {tuple(logits.shape)}, got "
                         f"{tuple(target.shape) if isinstance(target, torch.Tensor) else target!r}")
    if target.device != logits.device:
        raise ValueError(f"target must be on the logits' device {logits.device}, got {target.device}")
    a = _check_alpha(alpha)
    bg = check_flag("include_background", include_background)
    ig = _check_ignore(ignore_index)
    sp = check_spacing(spacing)
    dims = tuple(int(v) for v in logits.shape[2:])
    return a, bg, ig, sp, B, Cc, Cc - (0 if bg else 1), dims


def _edt_sq_np(seeds: np.ndarray, spacing) -> np.ndarray:
    """Exact squared Euclidean distance to the nearest True voxel of ``seeds [H, W, D]`` (inf without one), float64: the
    separable min-plus form, one pass per axis (the CPU restatement of the transform; small volumes)."""
    f = np.where(seeds, 0.0, np.inf)
    for axis, s in enumerate(spacing):
        f = np.moveaxis(f, axis, -1)
        n = f.shape[-1]
        x = np.arange(n, dtype=np.float64)
        out = np.full(f.shape, np.inf)
        for i in range(n):
            np.minimum(out, (float(s) * (x - i)) ** 2 + f[..., i:i + 1], out=out)
        f = np.moveaxis(out, -1, axis)
    return f


def _hausdorff_maps_np(z: np.ndarray, y: np.ndarray, alpha: float, spacing, bg: bool, ig) -> np.ndarray:
    """The weight maps on the CPU: z [B, H, W, D, C], y [B, H, W, D] -> float64 [B, K, H, W, D]."""
    B, Cc = z.shape[0], z.shape[-1]
    c0 = 0 if bg else 1
    yy = y.astype(np.float64)
    ok = (yy >= 0) & (yy < Cc) & (yy == np.floor(yy))
    if ig is not None:
        ok &= yy != float(ig)
    pred = np.argmax(z, axis=-1)                                   # the first maximum
    out = np.zeros((B, Cc - c0) + z.shape[1:4])
    for b in range(B):
        for c in range(c0, Cc):
            for M in (pred[b] == c, ok[b] & (yy[b] == float(c))):
                if M.any() and not M.all():
                    d2 = np.where(M, _edt_sq_np(~M, spacing), _edt_sq_np(M, spacing))
                    out[b, c - c0] += d2 if alpha == 2.0 else d2 ** (0.5 * alpha)
    return out


def _hausdorff_maps_launch(logits_cl: torch.Tensor, tgt: torch.Tensor, dims, alpha, spacing, bg, ig, ws=None) -> torch.Tensor:
    """logits_cl f32 [B, H, W, D, C] contiguous, tgt f32 with B prod(dims) labels -> wmap f32 [B, K, H, W, D]: the four launches."""
    B, Cc = logits_cl.shape[0], logits_cl.shape[-1]
    K = Cc - (0 if bg else 1)
    H, W, D = dims
    if H > 65535 or W > 65535 or 4 * B * K * H * W * D >= 2 ** 31:
        raise ValueError(f"Hausdorff weight maps of {B} x {K} x {dims}: H and W must be <= 65535 and 4 B K H W D < 2^31")
    wmap = torch.empty((B, K, H, W, D), dtype=torch.float32, device=logits_cl.device)
    if ws is None:
        ws = torch.empty(max(int(L.lib().mivp_hausdorff_maps_ws(B, K, i3(dims))), 1), dtype=torch.uint8, device=logits_cl.device)
    L.call("mivp_hausdorff_maps", L.ptr(logits_cl), L.ptr(tgt), B, Cc, 1 if bg else 0, 0 if ig is None else ig,
           0 if ig is None else 1, i3(dims), (C.c_float * 3)(*spacing), alpha, L.ptr(wmap), L.ptr(ws), L.stream())
    return wmap


def _channels_last_f32(logits: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W, D] -> contiguous f32 [B, H, W, D, C]: the view when the storage is that already, else a copy."""
    return logits.detach().permute(0, 2, 3, 4, 1).to(torch.float32).contiguous()


def hausdorff_weight_maps(logits: torch.Tensor, target: torch.Tensor, *, alpha: float = 2.0,
                          spacing: Sequence[float] = (1.0, 1.0, 1.0), include_background: bool = False,
                          ignore_index: Optional[int] = None) -> torch.Tensor:
    """The weight maps of the Hausdorff distance-transform loss.  logits [B, C, H, W, D] (2 <= C <= 8), target
    [B, 1, H, W, D] (or [B, H, W, D]) class indices of any dtype -> float32 ``[B, K, H, W, D]`` for the classes c0 .. C - 1.  Per
    sample and class, P = {argmax_j logits_j == c} (the hard prediction; the lowest index among exact maxima) and
    G = {label == c} (a label that is no class for ``seg_loss`` belongs to no G)::

        field(M)(v) = distance from v to the nearest voxel on the other side of M; 0 everywhere when M is empty or the sample
        maps        = field(P)^alpha + field(G)^alpha

    with distances ``sqrt(sum_a (spacing[a] delta_a)^2)``.  A constant: nothing flows back into the logits.  On the GPU four
    launches whatever the batch and class counts are, nothing read back (csrc/hausdorff.hip); exact integers at ``alpha == 2``
    and unit spacing.  CPU tensors take a numpy restatement of the same definition (small volumes)."""
    a, bg, ig, sp, B, Cc, K, dims = _hausdorff_args(logits, target, alpha, include_background, ignore_index, spacing)
    if logits.is_cuda:
        tgt = target.detach().to(torch.float32).contiguous()
        return _hausdorff_maps_launch(_channels_last_f32(logits), tgt, dims, a, sp, bg, ig)
    z = logits.detach().permute(0, 2, 3, 4, 1).numpy()
    y = target.detach().reshape((B,) + dims).numpy()
    return torch.from_numpy(_hausdorff_maps_np(z, y, a, sp, bg, ig)).to(torch.float32)


class _HausdorffFn(torch.autograd.Function):
    """The term on given weight maps: value from a streaming pass + a one-workgroup reduction, the gradient from a second
    streaming pass when backward asks for it (csrc/hausdorff.hip).  ``wmap`` and ``weight`` are constants."""

    @staticmethod
    def forward(ctx, logits_cl, target, wmap, weight, bg, ig, lam):
        B, H, W, D, Cc = logits_cl.shape
        vol = H * W * D
        ws = torch.empty(L.lib().mivp_hausdorff_loss_ws(B, vol), dtype=torch.float32, device=logits_cl.device)
        loss = torch.empty(1, dtype=torch.float32, device=logits_cl.device)
        L.call("mivp_hausdorff_loss", L.ptr(logits_cl), L.ptr(target), L.ptr(wmap), B, vol, Cc, 1 if bg else 0,
               0 if ig is None else ig, 0 if ig is None else 1, lam, L.ptr(weight), L.ptr(ws), L.ptr(loss), L.ptr(None), 0,
               L.stream())
        ctx.save_for_backward(logits_cl, target, wmap, ws)
        ctx.weight, ctx.opts = weight, (bg, ig, lam)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits_cl, target, wmap, ws = ctx.saved_tensors
        B, H, W, D, Cc = logits_cl.shape
        bg, ig, lam = ctx.opts
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        L.call("mivp_hausdorff_loss_grad", L.ptr(logits_cl), L.ptr(target), L.ptr(wmap), B, H * W * D, Cc, 1 if bg else 0,
               0 if ig is None else ig, 0 if ig is None else 1, lam, L.ptr(ctx.weight), L.ptr(ws), L.ptr(g), L.ptr(dz), 0,
               L.stream())
        return dz, None, None, None, None, None, None


def _hausdorff_torch(z: torch.Tensor, y: torch.Tensor, wmap: torch.Tensor, bg: bool, ig, weight) -> torch.Tensor:
    """The formulas of ``hausdorff_dt_loss`` in plain torch ops, differentiable by autograd: z [B, vol, C], y [B, vol] labels,
    wmap [B, K, vol]."""
    Cc = z.shape[-1]
    y = y.to(z.dtype if z.dtype in (torch.float32, torch.float64) else torch.float32)
    valid = (y >= 0) & (y < Cc) & (y == y.floor())
    if ig is not None:
        valid = valid & (y != ig)
    c0 = 0 if bg else 1
    onehot = (y.unsqueeze(-1) == torch.arange(Cc, dtype=y.dtype, device=y.device)) & valid.unsqueeze(-1)
    err = (torch.softmax(z, dim=-1) - onehot.to(z.dtype))[..., c0:]
    num = (err * err * wmap.to(z.dtype).transpose(1, 2) * valid.to(z.dtype).unsqueeze(-1)).sum()
    loss = num / ((Cc - c0) * valid.sum().clamp(min=1).to(z.dtype))
    return loss if weight is None else loss * weight.to(z.dtype).reshape(())


def _hausdorff_term(logits, target, a, bg, ig, sp, B, Cc, K, dims, weight, maps, lam, maps_ws=None) -> torch.Tensor:
    """``lam weight`` times the term; the kernels for channels-last f32 GPU logits, else the torch composition."""
    if maps is not None:
        if not isinstance(maps, torch.Tensor) or tuple(maps.shape) != (B, K) + dims or maps.device != logits.device:
            raise ValueError(f"maps must be a [B, K, H, W, D] = {(B, K) + dims} tensor on the logits' device, got "
                             f"{tuple(maps.shape) if isinstance(maps, torch.Tensor) else maps!r}")
        maps = maps.detach()
    base = logits.permute(0, 2, 3, 4, 1)
    if logits.is_cuda and logits.dtype == torch.float32 and base.is_contiguous():
        tgt = target.detach().to(torch.float32).contiguous()
        wmap = _hausdorff_maps_launch(base.detach(), tgt, dims, a, sp, bg, ig, maps_ws) if maps is None \
            else maps.to(torch.float32).contiguous()
        if weight is not None:
            weight = weight.to(torch.float32).contiguous()
        return _HausdorffFn.apply(base, tgt, wmap, weight, bg, ig, lam)
    if maps is None:
        maps = hausdorff_weight_maps(logits, target, alpha=a, spacing=sp, include_background=bg, ignore_index=ig)
    term = _hausdorff_torch(base.reshape(B, -1, Cc), target.detach().reshape(B, -1), maps.reshape(B, K, -1), bg, ig, weight)
    return term if lam == 1.0 else lam * term


def hausdorff_dt_loss(logits: torch.Tensor, target: torch.Tensor, *, alpha: float = 2.0, include_background: bool = False,
                      ignore_index: Optional[int] = None, spacing: Sequence[float] = (1.0, 1.0, 1.0),
                      weight: Optional[torch.Tensor] = None, maps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The Hausdorff distance-transform loss of Karimi & Salcudean (IEEE TMI 2019, "HD_DT").  logits [B, C, H, W, D]
    (2 <= C <= 8), target [B, 1, H, W, D] (or [B, H, W, D]) class indices of any dtype.  With p = softmax_c(z), g_c = [y == c],
    Wm = ``hausdorff_weight_maps(logits, target, alpha=, spacing=, ...)`` (or ``maps``, [B, K, H, W, D], when given), V the
    valid voxels of the batch (the rule of ``seg_loss``), N = |V|, K = C - c0::

        loss = weight sum_{v in V} sum_{c >= c0} (p_c(v) - g_c(v))^2 Wm_c(v) / (K max(N, 1))

    The prediction's mask is the hard prediction (the arg-max of the logits), where MONAI's ``HausdorffDTLoss`` thresholds
    the softmax at 0.5: the same set for C = 2 up to exact ties, and independent of how a softmax is rounded.  ``Wm`` is a
    constant of the step; ``weight``: a one-element tensor on the logits' device (None = 1) that is read on the device, so a
    recorded step follows a schedule of it.  Channels-last f32 CUDA logits take the kernels: the four launches of the maps
    (unless ``maps`` is given), then two streaming passes; nothing read back, recordable.  Any other layout, dtype or device
    takes the same formulas as plain torch ops, with the maps from ``hausdorff_weight_maps``."""
    a, bg, ig, sp, B, Cc, K, dims = _hausdorff_args(logits, target, alpha, include_background, ignore_index, spacing)
    weight = _check_boundary_weight(weight, logits.device)
    return _hausdorff_term(logits, target, a, bg, ig, sp, B, Cc, K, dims, weight, maps, 1.0)


class HausdorffDTLoss(torch.nn.Module):
    """``base(logits, target) + lambda_hausdorff weight hausdorff_dt_loss(logits, target, **options)`` (the term alone
    without a ``base``); ``options``: ``alpha``, ``include_background``, ``ignore_index``, ``spacing``.  ``base`` is any
    module of (logits, target), e.g. a ``SegLoss``; ``train.step_loss`` takes the whole as ``conf.seg_loss``.  ``weight`` is a
    device float outside ``state_dict`` that ``set_weight`` schedules between the replays of a recorded step.  The scratch of
    the distance transform (the large part) is allocated once per shape; the maps a backward pass reads are the call's own."""

    def __init__(self, base: Optional[torch.nn.Module] = None, lambda_hausdorff: float = 1.0, *, alpha: float = 2.0,
                 include_background: bool = False, ignore_index: Optional[int] = None,
                 spacing: Sequence[float] = (1.0, 1.0, 1.0)):
        super().__init__()
        if base is not None and not isinstance(base, torch.nn.Module):
            raise TypeError(f"base must be None or a torch.nn.Module of (logits, target), got {base!r}")
        lam = check_at_least("lambda_hausdorff", lambda_hausdorff, 0.0)
        if lam > float(np.finfo(np.float32).max):
            raise ValueError(f"lambda_hausdorff must be finite in fp32, got {lambda_hausdorff!r}")
        self.base = base
        self.lambda_hausdorff = lam
        self.alpha = _check_alpha(alpha)
        self.include_background = check_flag("include_background", include_background)
        self.ignore_index = _check_ignore(ignore_index)
        self.spacing = check_spacing(spacing)
        self.register_buffer("weight", torch.ones(1, dtype=torch.float32), persistent=False)
        self._maps_ws = {}

    def set_weight(self, value: float) -> None:
        """Set the factor of the term (``lambda_hausdorff`` times it is the term's weight): a stream-ordered copy into the
        module's buffer, legal between the replays of a recorded step."""
        v = check_finite("weight", value)
        if self.weight.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("HausdorffDTLoss.set_weight inside a recording: a recording must not freeze today's weight "
                               "into the graph; call it between replays")
        self.weight.copy_(torch.tensor([v], dtype=torch.float32))

    def _scratch(self, device, B: int, K: int, dims):
        key = (str(device), B, K, dims)
        ws = self._maps_ws.get(key)
        if ws is None:
            ws = torch.empty(max(int(L.lib().mivp_hausdorff_maps_ws(B, K, i3(dims))), 1), dtype=torch.uint8, device=device)
            self._maps_ws[key] = ws
        return ws

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        a, bg, ig, sp, B, Cc, K, dims = _hausdorff_args(logits, target, self.alpha, self.include_background,
                                                        self.ignore_index, self.spacing)
        if self.weight.device != logits.device:
            raise ValueError(f"the module is on {self.weight.device}, the logits on {logits.device}: move it with .to()")
        ws = self._scratch(logits.device, B, K, dims) if logits.is_cuda else None
        term = _hausdorff_term(logits, target, a, bg, ig, sp, B, Cc, K, dims, self.weight, None, self.lambda_hausdorff, ws)
        return term if self.base is None else self.base(logits, target) + term

    def extra_repr(self) -> str:
        return (f"lambda_hausdorff={self.lambda_hausdorff}, alpha={self.alpha}, include_background={self.include_background}, "
                f"ignore_index={self.ignore_index}, spacing={self.spacing}")


# ---------------------------------------------------------------------------------------------
# Lovasz-Softmax term: the Lovasz extension of the per-class Jaccard loss on an exact device-wide key sort
# (csrc/lovasz.hip, csrc/sort_common.hpp)
# ---------------------------------------------------------------------------------------------
LOVASZ_CLASSES = ("present", "all")


def _lovasz_args(logits, target, classes, per_image, include_background, ignore_index):
    """The checks the function and the module share -> (all, per_image, bg, ig, B, C, dims)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 5:
        raise ValueError(f"logits must be [B, C, H, W, D], got {tuple(logits.shape) if isinstance(logits, torch.Tensor) else logits!r}")
    B, Cc = int(logits.shape[0]), int(logits.shape[1])
    if not 2 <= Cc <= SEG_LOSS_MAX_CLASSES:
        raise ValueError(f"logits must have 2 .. {SEG_LOSS_MAX_CLASSES} classes, got {Cc}")
    if not isinstance(target, torch.Tensor) or target.numel() != logits.numel() // Cc or target.shape[0] != B:
        raise ValueError(f"target must be [B, 1, H, W, D] for logits {tuple(logits.shape)}, got "
                         f"{tuple(target.shape) if isinstance(target, torch.Tensor) else target!r}")
    if target.device != logits.device:
        raise ValueError(f"target must be on the logits' device {logits.device}, got {target.device}")
    if classes not in LOVASZ_CLASSES:
        raise ValueError(f"classes must be one of {LOVASZ_CLASSES}, got {classes!r}")
    return (classes == "all", check_flag("per_image", per_image), check_flag("include_background", include_background),
            _check_ignore(ignore_index), B, Cc, tuple(int(v) for v in logits.shape[2:]))


def _lovasz_tie_weights(e: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """d loss_seg / d e of one segment by the tie rule: e [n] errors of the valid voxels, g [n] bool foreground.  Inside a group
    of equal e the foreground comes first and gets 1 / (G + K) each (K: background voxels with a larger error); the b tied
    background voxels share J(F, K + b) - J(F, K) = (G - F) / ((G + K)(G + K + b)) equally (1 / b when G + K == 0)."""
    n = e.numel()
    if n == 0:
        return e.new_zeros(0)
    order = torch.argsort(e, descending=True, stable=True)
    es, gs = e[order], g[order].to(e.dtype)
    _, inverse, size = torch.unique_consecutive(es, return_inverse=True, return_counts=True)
    last = torch.cumsum(size, 0) - 1                                  # last sorted position of each group of equal e
    f_end, k_end = torch.cumsum(gs, 0)[last], torch.cumsum(1.0 - gs, 0)[last]
    f_grp = torch.zeros_like(f_end).index_add_(0, inverse, gs)
    b_grp = size.to(e.dtype) - f_grp
    G = gs.sum()
    gk = G + (k_end - b_grp)                                          # G + K, K the background in front of the group
    fg_w = 1.0 / gk.clamp(min=1.0)
    bg_w = torch.where(gk > 0, (G - f_end) / (gk * (gk + b_grp)).clamp(min=1.0), 1.0 / b_grp.clamp(min=1.0))
    ws = torch.where(gs > 0, fg_w[inverse], bg_w[inverse])
    return torch.zeros_like(e).index_put_((order,), ws)


def _lovasz_torch(z: torch.Tensor, y: torch.Tensor, all_classes: bool, per_image: bool, bg: bool, ig, weight) -> torch.Tensor:
    """The formulas of ``lovasz_softmax_loss`` in plain torch ops: z [B, vol, C], y [B, vol] labels.  A segment's value is
    sum_i s_i e_i with s the (constant) tie-rule weights: the Lovasz extension's value, and the tie rule's gradient by autograd."""
    B, _, Cc = z.shape
    y = y.to(z.dtype if z.dtype in (torch.float32, torch.float64) else torch.float32)
    valid = (y >= 0) & (y < Cc) & (y == y.floor())
    if ig is not None:
        valid = valid & (y != ig)
    ex = (z - z.max(-1, keepdim=True).values).exp()
    den = ex.sum(-1, keepdim=True)
    hot = (y.unsqueeze(-1) == torch.arange(Cc, dtype=y.dtype, device=y.device)) & valid.unsqueeze(-1)
    others = (ex * (~hot).to(z.dtype)).sum(-1, keepdim=True)          # 1 - p_y as the sum of the others over the denominator
    err = torch.where(hot, others / den, ex / den)
    total = z.new_zeros(())
    groups = [(err[b], hot[b], valid[b]) for b in range(B)] if per_image else [(err.reshape(-1, Cc), hot.reshape(-1, Cc), valid.reshape(-1))]
    for e_g, h_g, v_g in groups:
        terms = []
        for c in range(0 if bg else 1, Cc):
            e, g = e_g[v_g, c], h_g[v_g, c]
            if all_classes or bool(g.any()):
                terms.append((_lovasz_tie_weights(e.detach(), g) * e).sum())
        if terms:
            total = total + torch.stack(terms).mean()
    loss = total / len(groups)
    return loss if weight is None else loss * weight.to(z.dtype).reshape(())


class _LovaszFn(torch.autograd.Function):
    """The term on the kernels: keys, sort, prefix, statistics and the f64 finalize in forward; the gradient pass on the same
    workspace when backward asks for it (csrc/lovasz.hip).  ``weight`` is a constant."""

    @staticmethod
    def forward(ctx, logits_cl, target, weight, opts, ws):
        B, H, W, D, Cc = logits_cl.shape
        all_classes, per_image, bg, ig, lam = opts
        loss = torch.empty(1, dtype=torch.float32, device=logits_cl.device)
        L.call("mivp_lovasz_loss", L.ptr(logits_cl), L.ptr(target), B, H * W * D, Cc, 1 if bg else 0, 0 if ig is None else ig,
               0 if ig is None else 1, 1 if per_image else 0, 1 if all_classes else 0, lam, L.ptr(weight), L.ptr(ws),
               L.ptr(loss), L.ptr(None), 0, L.stream())
        ctx.save_for_backward(logits_cl, target, ws)
        ctx.weight, ctx.opts = weight, opts
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits_cl, target, ws = ctx.saved_tensors
        B, H, W, D, Cc = logits_cl.shape
        all_classes, per_image, bg, ig, lam = ctx.opts
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        L.call("mivp_lovasz_loss_grad", L.ptr(logits_cl), L.ptr(target), B, H * W * D, Cc, 1 if bg else 0,
               0 if ig is None else ig, 0 if ig is None else 1, 1 if per_image else 0, 1 if all_classes else 0, lam,
               L.ptr(ctx.weight), L.ptr(ws), L.ptr(g), L.ptr(dz), 0, L.stream())
        return dz, None, None, None, None


def _lovasz_workspace(device, B: int, Cc: int, bg: bool, per_image: bool, vol: int) -> torch.Tensor:
    nbytes = int(L.lib().mivp_lovasz_ws(B, Cc, 1 if bg else 0, 1 if per_image else 0, vol))
    if nbytes == 0:
        raise ValueError(f"Lovasz-Softmax of {B} x {Cc} x {vol} voxels: B must be <= 65535 and the keys fewer than 2^31")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _lovasz_term(logits, target, all_classes, per_image, bg, ig, B, Cc, dims, weight, lam, ws=None) -> torch.Tensor:
    """``lam weight`` times the term; the kernels for channels-last f32 GPU logits, else the torch composition."""
    base = logits.permute(0, 2, 3, 4, 1)
    if logits.is_cuda and logits.dtype == torch.float32 and base.is_contiguous():
        tgt = target.detach().to(torch.float32).contiguous()
        if weight is not None:
            weight = weight.to(torch.float32).contiguous()
        if ws is None:
            ws = _lovasz_workspace(logits.device, B, Cc, bg, per_image, math.prod(dims))
        return _LovaszFn.apply(base, tgt, weight, (all_classes, per_image, bg, ig, lam), ws)
    term = _lovasz_torch(base.reshape(B, -1, Cc), target.detach().reshape(B, -1), all_classes, per_image, bg, ig, weight)
    return term if lam == 1.0 else lam * term


def lovasz_softmax_loss(logits: torch.Tensor, target: torch.Tensor, classes: str = "present", per_image: bool = False,
                        include_background: bool = True, ignore_index: Optional[int] = None,
                        weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The Lovasz-Softmax loss of Berman, Triki & Blaschko (CVPR 2018): the convex surrogate of the per-class Jaccard index.
    logits [B, C, H, W, D] (2 <= C <= 8), target [B, 1, H, W, D] (or [B, H, W, D]) class indices of any dtype.  A segment is one
    class c >= c0 of one sample (``per_image``) or of the batch; over its valid voxels (the rule of ``seg_loss``), with
    p = softmax_c(z), g = [y == c], e = g ? 1 - p_c : p_c, G = sum g, J(F, K) = 1 - (G - F) / (G + K), J(0, 0) = 0::

        loss_seg = sum_j e_(j) (J_j - J_(j-1))        errors in descending order; F_j, K_j: foreground, background among the first j

    ``classes="present"`` averages the segments with G > 0 (none: 0, decided on the device), ``"all"`` every segment;
    ``per_image`` averages the samples' means.  Gradient on ties: inside a group of equal e the foreground voxels come first
    and get 1 / (G + K) each, the tied background voxels share their group's difference of J equally -- independent of memory
    order, equal bits from call to call.  ``weight``: a one-element tensor on the logits' device (None = 1), read on the device.
    Channels-last f32 CUDA logits take the kernels (a fixed number of launches, nothing read back, recordable); any other
    layout, dtype or device takes the same formulas and tie rule as plain torch ops."""
    all_classes, per_image, bg, ig, B, Cc, dims = _lovasz_args(logits, target, classes, per_image, include_background, ignore_index)
    weight = _check_boundary_weight(weight, logits.device)
    return _lovasz_term(logits, target, all_classes, per_image, bg, ig, B, Cc, dims, weight, 1.0)


class LovaszSoftmaxLoss(torch.nn.Module):
    """``base(logits, target) + lambda_lovasz weight lovasz_softmax_loss(logits, target, **options)`` (the term alone without
    a ``base``); ``options``: ``classes``, ``per_image``, ``include_background``, ``ignore_index``.  ``base`` is any module of
    (logits, target), e.g. a ``SegLoss``; ``train.step_loss`` takes the whole as ``conf.seg_loss``.  ``weight`` is a device
    float outside ``state_dict`` that ``set_weight`` schedules between the replays of a recorded step.  The workspace (keys,
    the sort's second buffer, the prefix) is allocated once per shape; a backward pass reads it before the next forward."""

    def __init__(self, base: Optional[torch.nn.Module] = None, lambda_lovasz: float = 1.0, *, classes: str = "present",
                 per_image: bool = False, include_background: bool = True, ignore_index: Optional[int] = None):
        super().__init__()
        if base is not None and not isinstance(base, torch.nn.Module):
            raise TypeError(f"base must be None or a torch.nn.Module of (logits, target), got {base!r}")
        lam = check_at_least("lambda_lovasz", lambda_lovasz, 0.0)
        if lam > float(np.finfo(np.float32).max):
            raise ValueError(f"lambda_lovasz must be finite in fp32, got {lambda_lovasz!r}")
        if classes not in LOVASZ_CLASSES:
            raise ValueError(f"classes must be one of {LOVASZ_CLASSES}, got {classes!r}")
        self.base = base
        self.lambda_lovasz = lam
        self.classes = classes
        self.per_image = check_flag("per_image", per_image)
        self.include_background = check_flag("include_background", include_background)
        self.ignore_index = _check_ignore(ignore_index)
        self.register_buffer("weight", torch.ones(1, dtype=torch.float32), persistent=False)
        self._ws = {}

    def set_weight(self, value: float) -> None:
        """Set the factor of the term (``lambda_lovasz`` times it is the term's weight): a stream-ordered copy into the
        module's buffer, legal between the replays of a recorded step."""
        v = check_finite("weight", value)
        if self.weight.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LovaszSoftmaxLoss.set_weight inside a recording: a recording must not freeze today's weight "
                               "into the graph; call it between replays")
        self.weight.copy_(torch.tensor([v], dtype=torch.float32))

    def _scratch(self, device, B: int, Cc: int, vol: int):
        key = (str(device), B, Cc, vol)
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = _lovasz_workspace(device, B, Cc, self.include_background, self.per_image, vol)
        return ws

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        all_classes, per_image, bg, ig, B, Cc, dims = _lovasz_args(logits, target, self.classes, self.per_image,
                                                                   self.include_background, self.ignore_index)
        if self.weight.device != logits.device:
            raise ValueError(f"the module is on {self.weight.device}, the logits on {logits.device}: move it with .to()")
        ws = self._scratch(logits.device, B, Cc, math.prod(dims)) if logits.is_cuda else None
        term = _lovasz_term(logits, target, all_classes, per_image, bg, ig, B, Cc, dims, self.weight, self.lambda_lovasz, ws)
        return term if self.base is None else self.base(logits, target) + term

    def extra_repr(self) -> str:
        return (f"lambda_lovasz={self.lambda_lovasz}, classes={self.classes!r}, per_image={self.per_image}, "
                f"include_background={self.include_background}, ignore_index={self.ignore_index}")
