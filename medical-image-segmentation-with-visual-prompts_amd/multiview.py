"""Phase-1 training: the multi-view self-supervised step of the reference's ``MultiViewTrainer``
(modules/multi_view.py:57-85,115-176) for ``--training-mode self_supervised_learning_encoder``.

Host side: the random draws (``draw_views``: the same numpy calls in the same order as ``random_rotate`` /
``random_mask`` / ``random_permute``, utils.py:267-350, so one seed gives the same views), a fixed device slot they are
loaded into (``ViewSlot``), and the step around the model.  Device side (csrc/multiview.hip): the view builder, the
reconstruction / mutual MSE terms and the rotation CE + NT-Xent heads, values and gradients, with every per-step input
read from device memory so that the whole step records as one graph (``graphed_multiview_step``).

Reference behaviour kept as it is: one keep pattern per view shared by the whole batch; masking in the
rotated frame; the reconstruction target is the visible region and the MSE mean runs over every element, divided by
(1 - ratio); the NT-Xent denominator includes the positive; the mutual term compares perm(rec_k) with rec_i on view i's
visible region, gradient to both, weight 1; one forward per view (the patch-embed BatchNorm uses batch statistics).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L

_MAX_ROWS, _MAX_DIM = 64, 1024


@dataclass
class ViewDraws:
    """What one step draws on the host: rotation counts per sample and view, one keep pattern per view over the patch
    grid (True = visible, the reference's ``~mask``), and the permutation code of the mutual view (None without it)."""
    rot_i: np.ndarray               # int64 [B] in 0..3
    rot_j: np.ndarray
    keep_i: np.ndarray              # bool [gh, gw, gd]
    keep_j: np.ndarray
    perm: Optional[int]
    dims: tuple
    masking_shape: tuple
    ratio: float

    @property
    def batch(self) -> int:
        return int(self.rot_i.shape[0])

    def codes(self) -> np.ndarray:
        return np.concatenate([self.rot_i, self.rot_j]).astype(np.int32)

    def keep_words(self) -> np.ndarray:
        """int32 [2, ceil(n_patches / 32)]: bit p of word p >> 5 = keep of patch p in C order of the grid."""
        return np.stack([pack_keep(self.keep_i), pack_keep(self.keep_j)])

    def keep_voxels(self, which: str = "i") -> torch.Tensor:
        """The reference's ``~mask`` at voxel resolution: bool [H, W, D]."""
        k = self.keep_i if which == "i" else self.keep_j
        m = self.masking_shape
        return torch.from_numpy(np.ascontiguousarray(
            k.repeat(m[0], 0).repeat(m[1], 1).repeat(m[2], 2)))


def pack_keep(keep: np.ndarray) -> np.ndarray:
    flat = np.ascontiguousarray(keep, dtype=bool).reshape(-1)
    nw = (flat.size + 31) // 32
    padded = np.zeros(nw * 32, dtype=np.uint64)
    padded[:flat.size] = flat
    words = (padded.reshape(nw, 32) << np.arange(32, dtype=np.uint64)).sum(1)
    return words.astype(np.uint32).view(np.int32)


def unpack_keep(words: np.ndarray, grid: Sequence[int]) -> np.ndarray:
    n = int(np.prod(grid))
    w = np.asarray(words).view(np.uint32).astype(np.uint64)
    bits = (w[:, None] >> np.arange(32, dtype=np.uint64)) & 1
    return bits.reshape(-1)[:n].astype(bool).reshape(tuple(grid))


def check_shapes(dims: Sequence[int], masking_shape: Sequence[int], mutual: bool) -> tuple:
    dims = tuple(int(v) for v in dims)
    m = tuple(int(v) for v in masking_shape)
    if len(dims) != 3 or len(m) != 3:
        raise ValueError(f"multi-view: 3 spatial dims and a 3-axis masking shape expected, got {dims} / {m}")
    if dims[0] != dims[1]:
        raise ValueError(f"multi-view: the rotation needs H == W, got spatial dims {dims}")
    if any(a % b for a, b in zip(dims, m)):
        raise ValueError(f"Input size {list(dims)} and patch size {list(m)} is not compatible!")
    if mutual and not (dims[0] == dims[1] == dims[2]):
        raise ValueError(f"multi-view: the mutual term permutes axes and needs H == W == D, got {dims}")
    return tuple(a // b for a, b in zip(dims, m))


def draw_views(rs: np.random.RandomState, B: int, dims, masking_shape, ratio: float, mutual: bool) -> ViewDraws:
    """The host draws of one step in the reference's order: rotate i (B x randint(0, 4)), rotate j, mask i
    (choice(n_patches, round(n_patches * (1 - ratio)), replace=False)), mask j, and with the mutual term choice(3)."""
    grid = check_shapes(dims, masking_shape, mutual)
    rot_i = np.array([rs.randint(0, 4) for _ in range(B)], dtype=np.int64)
    rot_j = np.array([rs.randint(0, 4) for _ in range(B)], dtype=np.int64)
    n = int(np.prod(grid).item())
    keeps = []
    for _ in range(2):
        idx = rs.choice(n, round(n * (1 - ratio)), replace=False)
        k = np.zeros(n, dtype=bool)
        k[idx] = True
        keeps.append(k.reshape(grid))
    perm = int(rs.choice(3)) if mutual else None
    return ViewDraws(rot_i, rot_j, keeps[0], keeps[1], perm, tuple(int(v) for v in dims),
                     tuple(int(v) for v in masking_shape), float(ratio))


class ViewSlot:
    """Fixed device buffers of one step's draws -- rotation codes int32 [2B], keep words int32 [2][nw], permutation code
    int32 [1] -- in ONE allocation whose pointer a recorded graph keeps.  ``load`` refreshes the content from a new pinned
    staging buffer without blocking (stream-ordered before the next launch or replay) and does nothing while a graph is
    being recorded (the recording must not freeze one step's draws).  Modelled on ``losses.JitterSlot``."""

    def __init__(self, B: int, dims, masking_shape, ratio: float, mutual: bool, device):
        self.grid = check_shapes(dims, masking_shape, mutual)
        self.B, self.dims, self.mshape = int(B), tuple(int(v) for v in dims), tuple(int(v) for v in masking_shape)
        self.ratio, self.mutual = float(ratio), bool(mutual)
        self.nw = (int(np.prod(self.grid)) + 31) // 32
        self.buf = torch.zeros(2 * self.B + 2 * self.nw + 1, dtype=torch.int32, device=device)
        self.codes = self.buf[:2 * self.B]
        self.keep = self.buf[2 * self.B:2 * self.B + 2 * self.nw]
        self.perm = self.buf[2 * self.B + 2 * self.nw:]
        self._dims = (C.c_int32 * 3)(*self.dims)
        self._mshape = (C.c_int32 * 3)(*self.mshape)
        self.draws = None

    def load(self, draws: ViewDraws):
        if (draws.batch, draws.dims, draws.masking_shape) != (self.B, self.dims, self.mshape) \
                or (draws.perm is not None) != self.mutual or draws.ratio != self.ratio:
            raise ValueError("ViewSlot: the draws do not match the slot's batch / shape / ratio / mutual setting")
        if torch.cuda.is_current_stream_capturing():
            return
        host = np.concatenate([draws.codes(), draws.keep_words().reshape(-1),
                               np.array([draws.perm if draws.perm is not None else 0], dtype=np.int32)])
        self.buf.copy_(torch.from_numpy(host).pin_memory(), non_blocking=True)
        self.draws = draws


def _check_input(x: torch.Tensor, slot: ViewSlot):
    if x.dim() != 5 or tuple(x.shape[2:]) != slot.dims or x.shape[0] != slot.B:
        raise ValueError(f"multi-view: input of shape {tuple(x.shape)} does not match the roi_size {list(slot.dims)} / "
                         f"batch {slot.B} of the draws")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("multi-view: the input volume must be a contiguous fp32 [B, C, H, W, D] tensor")


@torch.no_grad()
def make_views(x: torch.Tensor, slot: ViewSlot):
    """(x_i, x_j, x_k or None) of the draws loaded in ``slot``: mask(rot90(x)) per view, x_k = perm(x_i).  Detached, as the
    reference's views are (``x.detach().clone()``)."""
    _check_input(x, slot)
    xi, xj = torch.empty_like(x), torch.empty_like(x)
    xk = torch.empty_like(x) if slot.mutual else None
    L.call("mivp_mv_views", L.ptr(x), x.shape[0], x.shape[1], slot._dims, slot._mshape, L.ptr(slot.codes), L.ptr(slot.keep),
           L.ptr(slot.perm), L.ptr(xi), L.ptr(xj), L.ptr(xk), L.stream())
    return xi, xj, xk


def _channels_first(t: torch.Tensor) -> torch.Tensor:
    """The model's reconstruction is a channels-first view of channels-last storage: the same bytes at C = 1, a
    channels-first copy otherwise (the kernels' layout)."""
    t = t.float()
    return t if t.is_contiguous() else t.contiguous()


class _MultiViewLossFn(torch.autograd.Function):
    """total = w_rec rec + w_rot rot + w_con con + mut, and the vector [rec, rot, con, mut, total] (not differentiable).
    Forward: the value passes only; backward: the gradient passes, scaled by the incoming gradient read on the device."""

    @staticmethod
    def forward(ctx, rec_i, rec_j, rec_k, rot_i, rot_j, z_i, z_j, x_i, x_j, slot, w, temp):
        dev = slot.buf.device
        vec = torch.zeros(5, dtype=torch.float32, device=dev)
        has_rec = rec_i is not None
        do_rec = has_rec and w["use_rec"]
        if has_rec and (do_rec or rec_k is not None):
            ws = torch.empty(L.lib().mivp_mv_rec_ws(), dtype=torch.float32, device=dev)
            L.call("mivp_mv_rec_loss", L.ptr(rec_i), L.ptr(rec_j if do_rec else None), L.ptr(x_i if do_rec else None),
                   L.ptr(x_j if do_rec else None), L.ptr(rec_k), slot.B, rec_i.shape[1], slot._dims, slot._mshape,
                   L.ptr(slot.keep), L.ptr(slot.perm), int(do_rec), slot.ratio, L.ptr(ws), L.ptr(vec), L.stream())
            has_recmut = 1
        else:
            has_recmut = 0
        dim = z_i.shape[1] if z_i is not None else 0
        hws = torch.empty(max(1, L.lib().mivp_mv_heads_ws(slot.B, max(dim, 1))), dtype=torch.float32,
                          device=dev)
        L.call("mivp_mv_heads", L.ptr(z_i), L.ptr(z_j), slot.B, dim, temp, L.ptr(rot_i), L.ptr(rot_j), L.ptr(slot.codes),
               w["rec"], w["rot"], w["con"], has_recmut, L.ptr(hws), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None),
               L.ptr(None), L.ptr(vec), L.stream())
        ctx.save_for_backward(rec_i, rec_j, rec_k, rot_i, rot_j, z_i, z_j, x_i, x_j, hws)
        ctx.slot, ctx.w, ctx.temp, ctx.do_rec = slot, w, temp, do_rec
        ctx.mark_non_differentiable(vec)
        ctx.set_materialize_grads(False)                      # the vector's (absent) gradient is never filled with zeros
        return vec[4], vec

    @staticmethod
    def backward(ctx, g, _gvec):
        rec_i, rec_j, rec_k, rot_i, rot_j, z_i, z_j, x_i, x_j, hws = ctx.saved_tensors
        slot, w = ctx.slot, ctx.w
        g = g.detach().to(torch.float32).reshape(1).contiguous()
        d = [None] * 7
        if rec_i is not None and (ctx.do_rec or rec_k is not None):
            d[0] = torch.empty_like(rec_i)
            d[1] = torch.empty_like(rec_j) if ctx.do_rec else None
            d[2] = torch.empty_like(rec_k) if rec_k is not None else None
            L.call("mivp_mv_rec_grad", L.ptr(rec_i), L.ptr(rec_j if ctx.do_rec else None), L.ptr(x_i if ctx.do_rec else None),
                   L.ptr(x_j if ctx.do_rec else None), L.ptr(rec_k), slot.B, rec_i.shape[1], slot._dims, slot._mshape,
                   L.ptr(slot.keep), L.ptr(slot.perm), int(ctx.do_rec), slot.ratio, w["rec"], L.ptr(g), L.ptr(d[0]),
                   L.ptr(d[1]), L.ptr(d[2]), L.stream())
        if z_i is not None or rot_i is not None:
            if rot_i is not None:
                d[3], d[4] = torch.empty_like(rot_i), torch.empty_like(rot_j)
            if z_i is not None:
                d[5], d[6] = torch.empty_like(z_i), torch.empty_like(z_j)
            dim = z_i.shape[1] if z_i is not None else 0
            L.call("mivp_mv_heads", L.ptr(z_i), L.ptr(z_j), slot.B, dim, ctx.temp, L.ptr(rot_i), L.ptr(rot_j),
                   L.ptr(slot.codes), w["rec"], w["rot"], w["con"], 0, L.ptr(hws), L.ptr(g), L.ptr(d[5]), L.ptr(d[6]),
                   L.ptr(d[3]), L.ptr(d[4]), L.ptr(None), L.stream())
        return (*d, None, None, None, None, None)


def _check_heads(B: int, dim: int):
    if 2 * B > _MAX_ROWS:
        raise ValueError(f"multi-view heads: 2B = {2 * B} rows exceed the kernel's {_MAX_ROWS}")
    if dim > _MAX_DIM:
        raise ValueError(f"multi-view heads: contrastive dim {dim} exceeds the kernel's {_MAX_DIM}")


def _f32(t):
    return None if t is None else t.float().contiguous()


def multiview_loss(out_i: dict, out_j: dict, out_k: Optional[dict], slot: ViewSlot, conf, x_i, x_j):
    """(total, vector [rec, rot, con, mut, total]) of the configured terms (multi_view.py:128-176)."""
    use_rec, use_rot = bool(conf.use_reconstruction), bool(conf.use_rotation_prediction)
    use_con, use_mut = bool(conf.use_contrastive_learning), bool(conf.use_mutual_learning)
    if not (use_rec or use_rot or use_con or use_mut):
        raise ValueError("No loss defined!")
    if use_mut != slot.mutual:
        raise ValueError("multi-view: use_mutual_learning differs from the draws' mutual setting")
    rec_i = _channels_first(out_i["reconstruction"]) if (use_rec or use_mut) else None
    rec_j = _channels_first(out_j["reconstruction"]) if use_rec else None
    rec_k = _channels_first(out_k["reconstruction"]) if use_mut else None
    rot_i = _f32(out_i["rotation_prediction"]) if use_rot else None
    rot_j = _f32(out_j["rotation_prediction"]) if use_rot else None
    z_i = _f32(out_i["contrastive_coding"]) if use_con else None
    z_j = _f32(out_j["contrastive_coding"]) if use_con else None
    if z_i is not None:
        _check_heads(slot.B, z_i.shape[1])
    else:
        _check_heads(slot.B, 0)
    w = {"rec": float(conf.weight_rec), "rot": float(conf.weight_rot), "con": float(conf.weight_con), "use_rec": use_rec}
    return _MultiViewLossFn.apply(rec_i, rec_j, rec_k, rot_i, rot_j, z_i, z_j, x_i, x_j, slot, w, 0.5)


class ContrastivePairLoss(nn.Module):
    """losses/contrastive_pair_loss.py: NT-Xent of (x_i, x_j) [bs, dim] at temperature ``temp`` on the HIP heads kernel
    (value and gradient).  The buffers keep the reference's names (``temp``, ``neg_mask``) so its state dict loads."""

    def __init__(self, bs: int, temp: float = 0.5):
        super().__init__()
        self.bs = bs
        self.register_buffer("temp", torch.tensor(temp))
        self.register_buffer("neg_mask", (~torch.eye(bs * 2, bs * 2, dtype=torch.bool)).float())
        self._slot = {}

    def forward(self, x_i, x_j):
        B, dim = x_i.shape
        if B != self.bs or tuple(x_j.shape) != (B, dim):
            raise ValueError(f"ContrastivePairLoss(bs={self.bs}): got inputs {tuple(x_i.shape)} / {tuple(x_j.shape)}")
        _check_heads(B, dim)
        return _ContrastiveFn.apply(x_i.float().contiguous(), x_j.float().contiguous(), float(self.temp))


class _ContrastiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_i, z_j, temp):
        B, dim = z_i.shape
        vec = torch.zeros(5, dtype=torch.float32, device=z_i.device)
        ws = torch.empty(L.lib().mivp_mv_heads_ws(B, dim), dtype=torch.float32, device=z_i.device)
        L.call("mivp_mv_heads", L.ptr(z_i), L.ptr(z_j), B, dim, temp, L.ptr(None), L.ptr(None), L.ptr(None), 0.0, 0.0, 1.0, 0,
               L.ptr(ws), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(None), L.ptr(vec), L.stream())
        ctx.save_for_backward(z_i, z_j, ws)
        ctx.temp = temp
        return vec[2]

    @staticmethod
    def backward(ctx, g):
        z_i, z_j, ws = ctx.saved_tensors
        B, dim = z_i.shape
        g = g.detach().to(torch.float32).reshape(1).contiguous()
        dzi, dzj = torch.empty_like(z_i), torch.empty_like(z_j)
        L.call("mivp_mv_heads", L.ptr(z_i), L.ptr(z_j), B, dim, ctx.temp, L.ptr(None), L.ptr(None), L.ptr(None), 0.0, 0.0, 1.0,
               0, L.ptr(ws), L.ptr(g), L.ptr(dzi), L.ptr(dzj), L.ptr(None), L.ptr(None), L.ptr(None), L.stream())
        return dzi, dzj, None


def make_slot(conf, x: torch.Tensor) -> ViewSlot:
    return ViewSlot(x.shape[0], conf.roi_size, conf.masking_shape, float(conf.masking_ratio),
                    bool(conf.use_mutual_learning), x.device)


def multiview_forward_backward(model, opt, conf, x: torch.Tensor, slot: ViewSlot, keep_views: Optional[dict] = None):
    """Views from the draws in ``slot``, one forward per view, the loss terms, ``zero_grad(set_to_none=True)`` and
    backward; returns the loss vector [rec, rot, con, mut, total] (device; no host sync).  ``keep_views``: a dict that
    receives the views (tests)."""
    from .train import unit_grad
    if tuple(int(v) for v in conf.roi_size) != tuple(x.shape[2:]):
        raise ValueError(f"multi-view: roi_size {list(conf.roi_size)} differs from the input's spatial dims {list(x.shape[2:])}")
    x_i, x_j, x_k = make_views(x, slot)
    if keep_views is not None:
        keep_views.update(x_i=x_i, x_j=x_j, x_k=x_k)
    out_i = model(x_i)
    out_j = model(x_j)
    out_k = model(x_k) if slot.mutual else None
    total, vec = multiview_loss(out_i, out_j, out_k, slot, conf, x_i, x_j)
    opt.zero_grad(set_to_none=True)
    total.backward(unit_grad(total))
    return vec


def multiview_step(model, opt, sched, conf, x: torch.Tensor, draws: ViewDraws, slot: Optional[ViewSlot] = None,
                   augment=None):
    """One eager phase-1 step (multi_view.py:115-176): load the draws, forward / backward, ``opt.step()``, ``sched.step()``.
    Returns the loss vector [rec, rot, con, mut, total] on the device.  ``augment``: ``augment.IntensityDraws`` (or an
    ``IntensitySlot`` with draws loaded): the random intensity chain runs on ``x`` before the views are built; or
    ``augment.FilterDraws`` / a ``FilterSlot`` (noise, blur, low resolution); or a list of these, applied in order."""
    check_shapes(tuple(x.shape[2:]), conf.masking_shape, bool(conf.use_mutual_learning))
    slot = slot if slot is not None else make_slot(conf, x)
    slot.load(draws)
    if augment is not None:
        from .augment import apply_slots, as_slots
        x = apply_slots(x, as_slots(augment, x))
    vec = multiview_forward_backward(model, opt, conf, x, slot)
    opt.step()
    if sched is not None:
        sched.step()
    return vec


def graphed_multiview_step(model, opt, sched, conf, x: torch.Tensor, draws, warmup: int = 2, augment=None):
    """``multiview_step`` as a recorded graph (``train.GraphedStep``).  ``x`` is the fixed input tensor (copy new volumes
    into it); ``draws`` is a ViewDraws used for every step or a callable returning the next step's ViewDraws -- the
    step's ``refresh`` loads them into the slot before each warm-up step and replay.  The result's ``loss`` is the loss
    vector [rec, rot, con, mut, total] of the last replay (read it after the replay); ``views`` holds the recorded view
    buffers.  ``augment``: ``augment.IntensityDraws`` used for every step, a callable returning the next step's, or an
    ``IntensitySlot`` the caller reloads; ``refresh`` loads the draws into the slot (``step.augment_slot``) and the two
    intensity launches are recorded in front of the view builder (``x`` itself is left as it is).  The same three forms of
    ``augment.FilterDraws`` / ``FilterSlot``, and a list mixing both kinds (applied in order; ``step.augment_slot`` is then
    the list of slots), are taken as well."""
    from .train import GraphedStep
    check_shapes(tuple(x.shape[2:]), conf.masking_shape, bool(conf.use_mutual_learning))
    slot = make_slot(conf, x)
    views = {}
    aug = None
    if augment is not None:
        from .augment import AugmentChain
        aug = AugmentChain(augment, x)

    def refresh():
        slot.load(draws() if callable(draws) else draws)
        if aug is not None:
            aug.refresh()

    def forward_backward():
        xa = x if aug is None else aug.apply(x)
        return multiview_forward_backward(model, opt, conf, xa, slot, keep_views=views)

    step = GraphedStep(forward_backward, opt, sched, refresh, warmup)
    step.slot, step.views, step.augment_slot = slot, views, None if aug is None else aug.augment_slot
    return step
