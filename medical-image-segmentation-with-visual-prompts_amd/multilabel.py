"""Multi-label targets: overlapping label GROUPS, one sigmoid channel each (csrc/multilabel.hip).

The softmax objectives of ``losses`` and the arg-max finalize of the predictor assume mutually exclusive classes.  The
other common target of 3-D medical segmentation scores sets of labels that overlap -- BraTS: whole tumour, tumour core,
enhancing tumour; KiTS: kidney + masses, masses, tumour; nnU-Net's "region-based training".  A "region" is a connected
lesion in this package (``regions``), so the sets are called groups here.

* ``LabelGroups``        -- the groups, the known labels and the two tables the kernels read (``member``, ``lut``).
* ``MultiLabelSpec`` / ``multilabel_loss`` / ``MultiLabelLoss`` -- Tversky region term + weighted (focal) binary
  cross-entropy over the R sigmoid channels: a statistics pass, a one-workgroup f64 finalize and a gradient pass, nothing
  read back, recordable.  ``conf.seg_loss = MultiLabelLoss(...)`` trains a model with R output channels through
  ``train.step_loss``.
* ``decode_groups``      -- blended logits -> label map (+ the bits map and the sigmoid probabilities), one launch.
* ``group_counts`` / ``group_scores`` -- per-group (intersection, predicted, target) counts on the device, Dice and IoU
  per group on the host.
* ``GroupEvaluation``    -- ``predict_groups`` / ``evaluate_groups`` of ``SlidingWindowPredictor`` (its base class, so that
  the predictor's own body keeps the methods it had); ``evaluate_volume_groups`` is the one-shot wrapper.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from ._host import (LABEL_DTYPES, ImmutableValue, channels_last_or_copy, check_at_least, check_finite, check_flag, check_gpu,
                    plain_int)
from .losses import SEG_LOSS_SMOOTH, _check_ignore, _label_batch

MAX_GROUPS = 8
KNOWN = 256                     # bit 8 of a ``member`` entry: the label is known


def _check_label(name: str, v) -> int:
    if not plain_int(v) or not 0 <= int(v) <= 255:
        raise ValueError(f"{name} must be an integer label in 0..255, got {v!r}")
    return int(v)


def _label_tuple(name: str, seq) -> tuple:
    if isinstance(seq, (str, bytes)) or not hasattr(seq, "__iter__"):
        raise ValueError(f"{name} must be a sequence of integer labels, got {seq!r}")
    out = tuple(_check_label(f"{name}[{i}]", v) for i, v in enumerate(seq))
    if len(set(out)) != len(out):
        raise ValueError(f"{name} has duplicates: {list(out)}")
    return out


class _Value(ImmutableValue):
    """An ``ImmutableValue`` that survives ``copy`` and ``pickle``: a model keeps its configuration, and with it
    ``conf.seg_loss``, so ``copy.deepcopy(model)`` and checkpoints meet these objects."""

    __slots__ = ()

    def __copy__(self):
        return self

    def __deepcopy__(self, memo):
        return self

    def __reduce__(self):
        return type(self), tuple(getattr(self, k) for k in self.__slots__)


class LabelGroups(_Value):
    """R overlapping sets of labels (an immutable value), 1 <= R <= 8, labels in 0..255.

    ``groups``: R non-empty sequences of distinct labels; ``labels``: the known labels (default: 0 and the union of the
    groups; it must hold every label of a group) -- a voxel with any other value is invalid, as in ``seg_loss``;
    ``write``: the label a predicted group writes into the label map.  Two host tables follow from them:

    ``member`` int32 [256]: bits 0..R-1 of entry l = the groups that contain label l, bit 8 set when l is known;
    ``lut`` uint8 [2^R]: the label of each pattern of predicted groups by nnU-Net's rule: start at 0, walk the groups in
    index order, a set bit r overwrites with ``write[r]``.

    The default ``write[r]`` is the label of group r that no later group contains; when that label is not unique
    (groups that are not nested) ``write`` has to be given.  BraTS: ``LabelGroups([(1, 2, 3), (2, 3), (3,)])`` has
    ``write == (1, 2, 3)`` and ``lut == [0, 1, 2, 2, 3, 3, 3, 3]``."""

    __slots__ = ("groups", "labels", "write")

    def __init__(self, groups, labels=None, write=None):
        if isinstance(groups, (str, bytes)) or not hasattr(groups, "__iter__"):
            raise ValueError(f"groups must be 1..{MAX_GROUPS} sequences of labels, got {groups!r}")
        groups = list(groups)
        if not 1 <= len(groups) <= MAX_GROUPS:
            raise ValueError(f"groups must hold 1..{MAX_GROUPS} groups, got {len(groups)}")
        gs = tuple(_label_tuple(f"groups[{r}]", g) for r, g in enumerate(groups))
        for r, g in enumerate(gs):
            if not g:
                raise ValueError(f"groups[{r}] is empty")
        union = sorted(set(v for g in gs for v in g))
        if labels is None:
            known = tuple(sorted(set([0] + union)))
        else:
            known = _label_tuple("labels", labels)
            missing = [v for v in union if v not in known]
            if missing:
                raise ValueError(f"labels must hold every label of a group, {missing} are missing")
        if write is None:
            wr = []
            for r, g in enumerate(gs):
                own = [v for v in g if not any(v in later for later in gs[r + 1:])]
                if len(own) != 1:
                    raise ValueError(f"groups[{r}] = {list(g)} has {len(own)} labels that no later group contains "
                                     f"({own}): pass write=, the label each predicted group writes")
                wr.append(own[0])
            wr = tuple(wr)
        else:
            wr = tuple(_check_label(f"write[{r}]", v) for r, v in enumerate(
                write if hasattr(write, "__iter__") and not isinstance(write, (str, bytes)) else [write]))
            if len(wr) != len(gs):
                raise ValueError(f"write must hold one label per group ({len(gs)}), got {len(wr)}")
        self._set(groups=gs, labels=known, write=wr)

    @property
    def R(self) -> int:
        return len(self.groups)

    @property
    def member(self) -> np.ndarray:
        m = np.zeros(256, dtype=np.int32)
        for v in self.labels:
            m[v] |= KNOWN
        for r, g in enumerate(self.groups):
            for v in g:
                m[v] |= 1 << r
        return m

    @property
    def lut(self) -> np.ndarray:
        out = np.zeros(1 << self.R, dtype=np.uint8)
        for bits in range(1 << self.R):
            lab = 0
            for r in range(self.R):
                if bits >> r & 1:
                    lab = self.write[r]
            out[bits] = lab
        return out

    def tables(self, device):
        """(member int32 [256], lut uint8 [2^R]) on ``device``: uploaded once per device and cached -- outside a recording."""
        device = torch.device(device)
        key = (self, str(device))
        if key not in _table_cache:
            _no_upload_in_recording(device, "LabelGroups tables")
            _table_cache[key] = (torch.from_numpy(self.member).to(device), torch.from_numpy(self.lut).to(device))
        return _table_cache[key]

    def __repr__(self):
        return f"LabelGroups(groups={list(self.groups)}, labels={list(self.labels)}, write={list(self.write)})"


_table_cache: Dict[tuple, tuple] = {}
_vector_cache: Dict[tuple, torch.Tensor] = {}


def _no_upload_in_recording(device, what: str) -> None:
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"multilabel: first use of these {what} inside a recording; run one eager step first")


def _device_vector(values: tuple, device) -> torch.Tensor:
    """A tuple of floats as an f32 tensor on ``device``, uploaded once per (values, device)."""
    key = (values, str(device))
    if key not in _vector_cache:
        _no_upload_in_recording(device, "weights or thresholds")
        _vector_cache[key] = torch.tensor(values, dtype=torch.float32, device=device)
    return _vector_cache[key]


def _check_groups(groups) -> LabelGroups:
    if not isinstance(groups, LabelGroups):
        raise TypeError(f"groups must be a LabelGroups, got {type(groups).__name__}")
    return groups


def _weight_tuple(name: str, w) -> Optional[tuple]:
    if w is None:
        return None
    if isinstance(w, torch.Tensor):
        w = w.detach().cpu().tolist()
    if isinstance(w, (str, bytes)) or not hasattr(w, "__iter__"):
        raise ValueError(f"{name} must hold 1..{MAX_GROUPS} weights or be None, got {w!r}")
    w = tuple(w)
    if not 1 <= len(w) <= MAX_GROUPS:
        raise ValueError(f"{name} must hold 1..{MAX_GROUPS} weights, got {len(w)}")
    f32_max = float(np.finfo(np.float32).max)
    out = tuple(check_at_least(f"{name}[{i}]", v, 0.0) for i, v in enumerate(w))
    if any(v > f32_max for v in out):
        raise ValueError(f"{name} must be finite in fp32, got {w!r}")
    return out


class MultiLabelSpec(_Value):
    """Options of ``multilabel_loss`` (an immutable value; the formulas are in the docstring of ``multilabel_loss``).

    ``alpha``, ``beta`` >= 0: the Tversky weights of false positives / false negatives (0.5, 0.5: Dice); ``batch``: region
    sums over the whole batch instead of per sample; ``focal_gamma``: 0 (plain binary cross-entropy) or >= 1 (an exponent
    in (0, 1) has an unbounded gradient at p -> 1); ``group_weights``: one weight >= 0 per group, or None (all ones);
    ``pos_weight``: one factor >= 0 per group on the positive voxels of that group, or None; ``ignore_index``: the label of
    voxels that take no part, or None; ``lambda_region``, ``lambda_voxel`` >= 0, not both 0."""

    __slots__ = ("alpha", "beta", "batch", "focal_gamma", "group_weights", "pos_weight", "ignore_index", "lambda_region",
                 "lambda_voxel")

    def __init__(self, alpha: float = 0.5, beta: float = 0.5, batch: bool = False, focal_gamma: float = 0.0,
                 group_weights: Optional[Sequence[float]] = None, pos_weight: Optional[Sequence[float]] = None,
                 ignore_index: Optional[int] = None, lambda_region: float = 1.0, lambda_voxel: float = 1.0):
        f32_max = float(np.finfo(np.float32).max)
        for name, v in (("alpha", alpha), ("beta", beta), ("lambda_region", lambda_region), ("lambda_voxel", lambda_voxel)):
            if check_at_least(name, v, 0.0) > f32_max:
                raise ValueError(f"{name} must be finite in fp32, got {v!r}")
        gamma = check_at_least("focal_gamma", focal_gamma, 0.0)
        if 0.0 < gamma < 1.0 or gamma > f32_max:
            raise ValueError(f"focal_gamma must be 0 or >= 1 (its gradient is unbounded at p -> 1 in between), got {focal_gamma!r}")
        if float(lambda_region) == 0.0 and float(lambda_voxel) == 0.0:
            raise ValueError("lambda_region and lambda_voxel must not both be 0")
        self._set(alpha=float(alpha), beta=float(beta), batch=check_flag("batch", batch), focal_gamma=gamma,
                  group_weights=_weight_tuple("group_weights", group_weights), pos_weight=_weight_tuple("pos_weight", pos_weight),
                  ignore_index=_check_ignore(ignore_index), lambda_region=float(lambda_region),
                  lambda_voxel=float(lambda_voxel))


def _group_targets(y: torch.Tensor, member: torch.Tensor, R: int, ignore_index):
    """labels [...] -> (valid bool [...], t bool [..., R]) by the validity rule of the kernels."""
    yf = y.to(torch.float64)
    inr = (yf >= 0) & (yf < 256) & (yf == yf.floor())
    entry = member.to(torch.int64)[torch.where(inr, yf, torch.zeros_like(yf)).long()]
    valid = inr & ((entry & KNOWN) != 0)
    if ignore_index is not None:
        valid = valid & (yf != float(ignore_index))
    t = ((entry.unsqueeze(-1) >> torch.arange(R, device=y.device)) & 1).bool() & valid.unsqueeze(-1)
    return valid, t


def _multilabel_loss_torch(z: torch.Tensor, y: torch.Tensor, member: torch.Tensor, spec: MultiLabelSpec,
                           w: Optional[torch.Tensor], pw: Optional[torch.Tensor]) -> torch.Tensor:
    """The formulas of ``multilabel_loss`` in plain torch ops, differentiable by autograd: z [B, vol, R], y [B, vol]."""
    B, _, R = z.shape
    if z.dtype not in (torch.float32, torch.float64):
        z = z.float()
    valid, tb = _group_targets(y, member, R, spec.ignore_index)
    m, t = valid.to(z.dtype).unsqueeze(-1), tb.to(z.dtype)
    nlp, nlq = -F.logsigmoid(z), -F.logsigmoid(-z)
    p = torch.sigmoid(z)
    pm = p * m
    dims = (0, 1) if spec.batch else (1,)
    inter, psum, tsum = (pm * t).sum(dims), pm.sum(dims), t.sum(dims)
    s = SEG_LOSS_SMOOTH
    tversky = (2.0 * inter + s) / (2.0 * inter + 2.0 * spec.alpha * (psum - inter) + 2.0 * spec.beta * (tsum - inter) + s)
    loss = spec.lambda_region * (1.0 - tversky).mean()
    if spec.lambda_voxel > 0.0:
        wt = torch.ones(R, dtype=z.dtype, device=z.device) if w is None else w.to(z.dtype)
        pos = wt if pw is None else wt * pw.to(z.dtype)
        fp, fn = nlp, nlq
        if spec.focal_gamma > 0.0:
            fp, fn = torch.sigmoid(-z) ** spec.focal_gamma * nlp, p ** spec.focal_gamma * nlq
        f = (t * pos * fp + (m - t) * wt * fn).sum()
        loss = loss + spec.lambda_voxel * f / (R * max(int(valid.sum()), 1))
    return loss


class _MultiLabelFn(torch.autograd.Function):
    """Like ``losses._SegLossFn``: the value from one streaming pass + a one-workgroup reduction; the gradient from a second
    streaming pass when backward asks for it, already multiplied by the incoming gradient (csrc/multilabel.hip)."""

    @staticmethod
    def forward(ctx, logits_cl, target, member, w, pw, spec):
        B, H, W, D, R = logits_cl.shape
        vol = H * W * D
        ws = torch.empty(L.lib().mivp_multilabel_loss_ws(B, vol), dtype=torch.float32, device=logits_cl.device)
        loss = torch.empty(1, dtype=torch.float32, device=logits_cl.device)
        ig = spec.ignore_index
        L.call("mivp_multilabel_loss", L.ptr(logits_cl), L.ptr(target), B, vol, R, L.ptr(member), 1 if spec.batch else 0,
               spec.alpha, spec.beta, spec.focal_gamma, L.ptr(w), L.ptr(pw), 0 if ig is None else ig, 0 if ig is None else 1,
               spec.lambda_region, spec.lambda_voxel, L.ptr(ws), L.ptr(loss), L.ptr(None), L.stream())
        ctx.save_for_backward(logits_cl, target, ws)
        ctx.tables, ctx.spec = (member, w, pw), spec
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        logits_cl, target, ws = ctx.saved_tensors
        (member, w, pw), spec, ig = ctx.tables, ctx.spec, ctx.spec.ignore_index
        B, H, W, D, R = logits_cl.shape
        g = g.detach().to(torch.float32).contiguous()
        dz = torch.empty_like(logits_cl)
        L.call("mivp_multilabel_loss_grad", L.ptr(logits_cl), L.ptr(target), B, H * W * D, R, L.ptr(member),
               1 if spec.batch else 0, spec.alpha, spec.beta, spec.focal_gamma, L.ptr(w), L.ptr(pw), 0 if ig is None else ig,
               0 if ig is None else 1, spec.lambda_region, spec.lambda_voxel, L.ptr(ws), L.ptr(g), L.ptr(dz), L.stream())
        return dz, None, None, None, None, None


def _weights_on(name: str, given, from_spec, R: int, device) -> Optional[torch.Tensor]:
    """The f32 [R] weight table on ``device`` or None; a tensor that is passed takes precedence over the spec's tuple."""
    if given is None:
        if from_spec is None:
            return None
        if len(from_spec) != R:
            raise ValueError(f"{name} must hold one weight per group ({R}), got {len(from_spec)}")
        return _device_vector(from_spec, device)
    if not isinstance(given, torch.Tensor) or given.dim() != 1 or given.shape[0] != R:
        raise ValueError(f"{name} must hold one weight per group ({R}), got "
                         f"{tuple(given.shape) if isinstance(given, torch.Tensor) else given!r}")
    if given.device != device:
        raise ValueError(f"{name} must be on the logits' device {device}, got {given.device}")
    return given.detach().to(torch.float32).contiguous()


def multilabel_loss(logits: torch.Tensor, target: torch.Tensor, groups: LabelGroups, spec: Optional[MultiLabelSpec] = None,
                    group_weights: Optional[torch.Tensor] = None, pos_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Tversky region term + weighted (focal) binary cross-entropy over R overlapping label groups.  logits
    [B, R, H, W, D] (R = ``groups.R``), target [B, 1, H, W, D] (or [B, H, W, D]) labels of any dtype; ``group_weights`` /
    ``pos_weight``: [R] tensors on the logits' device that replace the spec's tuples (``MultiLabelLoss`` owns them).

    V: the valid voxels -- the label is an integer in 0..255, is known to ``groups`` and is not ``spec.ignore_index``;
    N = |V| over the batch.  With t_r = [label in group r], p_r = sigmoid(z_r), s = 1e-5, sums over V of a sample (of the
    batch when ``spec.batch``), w = group_weights, pi = pos_weight, gamma = focal_gamma::

        I_r = sum p_r t_r,  P_r = sum p_r,  T_r = sum t_r
        TI_r   = (2 I + s) / (2 I + 2 alpha (P - I) + 2 beta (T - I) + s)
        region = mean over (b, r) of 1 - TI_r                          (over r alone when batch)
        f_r    = w_r [ t_r pi_r (1 - p_r)^gamma (-log p_r) + (1 - t_r) p_r^gamma (-log(1 - p_r)) ]
        voxel  = sum_{v in V} sum_r f_r / (R max(N, 1))
        loss   = lambda_region region + lambda_voxel voxel

    An invalid voxel adds to no sum and gets an exactly zero gradient in all R channels.  log p and log(1 - p) come from
    e = exp(-|z|), log1p(e) and one reciprocal: they stay finite and keep their digits at |z| = 30.  gamma = 0 with
    pos_weight = None is ``F.binary_cross_entropy_with_logits`` on the R group planes.

    CUDA logits take the kernels (three launches, nothing read back, recordable; any dtype or layout is first brought to
    channels-last f32, which is a view of what the HIP model returns); CPU tensors take the same formulas as torch ops."""
    groups = _check_groups(groups)
    if spec is None:
        spec = MultiLabelSpec()
    elif not isinstance(spec, MultiLabelSpec):
        raise TypeError(f"spec must be a MultiLabelSpec, got {type(spec).__name__}")
    if logits.dim() != 5:
        raise ValueError(f"logits must be [B, R, H, W, D], got {tuple(logits.shape)}")
    B, R = logits.shape[0], logits.shape[1]
    if R != groups.R:
        raise ValueError(f"logits have {R} channels, groups has {groups.R} groups")
    if target.numel() != logits.numel() // R or target.shape[0] != B:
        raise ValueError(f"target must be [B, 1, H, W, D] for logits {tuple(logits.shape)}, got {tuple(target.shape)}")
    dev = logits.device
    w = _weights_on("group_weights", group_weights, spec.group_weights, R, dev)
    pw = _weights_on("pos_weight", pos_weight, spec.pos_weight, R, dev)
    tgt, dims = _label_batch(target)
    if tuple(logits.shape[2:]) != dims:
        raise ValueError(f"target must be [B, 1, H, W, D] for logits {tuple(logits.shape)}, got {tuple(target.shape)}")
    if tgt.device != dev:
        raise ValueError(f"target must be on the logits' device {dev}, got {tgt.device}")
    member = groups.tables(dev)[0]
    base = logits.permute(0, 2, 3, 4, 1)
    if logits.is_cuda:
        return _MultiLabelFn.apply(base.to(torch.float32).contiguous(), tgt, member, w, pw, spec)
    return _multilabel_loss_torch(base.reshape(B, -1, R), tgt.reshape(B, -1), member, spec, w, pw)


class MultiLabelLoss(torch.nn.Module):
    """``multilabel_loss`` as a module, callable as ``(logits, y)``: it owns the member table and the two weight tables as
    buffers (they follow ``.to(device)``, so a recorded step reads fixed device tensors).  ``train.step_loss`` uses
    ``conf.seg_loss`` when the configuration has one: ``conf.seg_loss = MultiLabelLoss(groups, spec)`` trains a model with
    ``output_channels_downstream = groups.R``."""

    def __init__(self, groups: LabelGroups, spec: Optional[MultiLabelSpec] = None, **options):
        super().__init__()
        self.groups = _check_groups(groups)
        if spec is None:
            spec = MultiLabelSpec(**options)
        elif options or not isinstance(spec, MultiLabelSpec):
            raise TypeError("MultiLabelLoss takes a MultiLabelSpec or the options of one, not both")
        for name in ("group_weights", "pos_weight"):
            v = getattr(spec, name)
            if v is not None and len(v) != groups.R:
                raise ValueError(f"{name} must hold one weight per group ({groups.R}), got {len(v)}")
            self.register_buffer(name, None if v is None else torch.tensor(v, dtype=torch.float32))
        self.spec = spec

    def forward(self, logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return multilabel_loss(logits, target, self.groups, self.spec, self.group_weights, self.pos_weight)

    def extra_repr(self) -> str:
        return f"{self.groups!r}, {self.spec!r}"


# ---------------------------------------------------------------------------------------------
# decode and counts
# ---------------------------------------------------------------------------------------------
def logit_thresholds(thresholds, R: int) -> tuple:
    """A probability threshold q in (0, 1), or R of them, as R logit-space thresholds: log(q / (1 - q)) in float64, rounded
    once to f32 (q = 0.5 gives exactly 0)."""
    if isinstance(thresholds, torch.Tensor):
        thresholds = thresholds.detach().cpu().tolist()
    qs = list(thresholds) if hasattr(thresholds, "__iter__") and not isinstance(thresholds, (str, bytes)) else [thresholds] * R
    if len(qs) != R:
        raise ValueError(f"thresholds must be one probability or one per group ({R}), got {len(qs)}")
    out = []
    for i, q in enumerate(qs):
        q = check_finite(f"thresholds[{i}]", q)
        if not 0.0 < q < 1.0:
            raise ValueError(f"thresholds[{i}] must be a probability in (0, 1), got {q!r}")
        out.append(float(np.float32(math.log(q / (1.0 - q)))))
    return tuple(out)


def decode_groups(logits: torch.Tensor, groups: LabelGroups, thresholds: Union[float, Sequence[float]] = 0.5,
                  return_bits: bool = False, return_probs: bool = False) -> Dict[str, torch.Tensor]:
    """Logits ``[B, R, H, W, D]`` of R group channels (the planes ``predict(return_logits=True)`` returns, or the model's
    channels-last view) -> ``{"labels": uint8 [B, 1, H, W, D]}``: group r is predicted where ``sigmoid(z_r) > thresholds[r]``
    (compared in logit space: a logit equal to its threshold is not predicted) and the label is ``groups.lut`` of the
    pattern.  ``return_bits``: also ``"bits"`` uint8 ``[B, 1, H, W, D]``, bit r = group r (what ``group_counts`` takes);
    ``return_probs``: also ``"probs"`` fp32 ``[B, R, H, W, D]``.  One launch, no host read."""
    groups = _check_groups(groups)
    check_gpu("logits", logits)
    if logits.dim() != 5 or logits.shape[1] != groups.R:
        raise ValueError(f"logits must be [B, {groups.R}, H, W, D] for {groups.R} groups, got {tuple(logits.shape)}")
    check_flag("return_bits", return_bits)
    check_flag("return_probs", return_probs)
    R, B, dims = groups.R, int(logits.shape[0]), tuple(int(v) for v in logits.shape[2:])
    tau = _device_vector(logit_thresholds(thresholds, R), logits.device)
    lut = groups.tables(logits.device)[1]
    src, clast = channels_last_or_copy(logits)
    out = {"labels": torch.empty((B, 1) + dims, dtype=torch.uint8, device=logits.device)}
    if return_bits:
        out["bits"] = torch.empty((B, 1) + dims, dtype=torch.uint8, device=logits.device)
    if return_probs:
        out["probs"] = torch.empty((B, R) + dims, dtype=torch.float32, device=logits.device)
    L.call("mivp_multilabel_decode", L.ptr(src), B, dims[0] * dims[1] * dims[2], R, clast, L.ptr(tau), L.ptr(lut),
           L.ptr(out["labels"]), L.ptr(out.get("bits")), L.ptr(out.get("probs")), L.stream())
    return out


def _label_map(name: str, t: torch.Tensor) -> torch.Tensor:
    check_gpu(name, t)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype not in (torch.uint8, torch.float32):
        t = t.float()
    return t.contiguous()


def group_counts(pred: torch.Tensor, target: torch.Tensor, groups: LabelGroups, ignore_index: Optional[int] = None,
                 out: Optional[torch.Tensor] = None, *, pred_bits: bool = False) -> torch.Tensor:
    """int64 ``[R, 3]`` device table of (|pred_r and t_r|, |pred_r|, |t_r|) over the valid voxels of ``target`` (labels; the
    validity rule of ``multilabel_loss``).  ``pred``: a label map of the same number of voxels, mapped through the groups
    like the target -- the arg-max labels of a softmax model can be scored by groups -- or, with ``pred_bits=True``, the
    uint8 bits map of ``decode_groups``.  ``out``: an earlier table to add onto, so that a data set can be pooled.  One
    launch, integer atomics only, no host read."""
    groups = _check_groups(groups)
    check_flag("pred_bits", pred_bits)
    ig = _check_ignore(ignore_index)
    p, t = _label_map("pred", pred), _label_map("target", target)
    if pred_bits and p.dtype != torch.uint8:
        raise ValueError(f"a bits map is uint8, got {pred.dtype}")
    if p.numel() != t.numel() or p.numel() == 0 or p.numel() >= 2 ** 31:
        raise ValueError(f"pred and target must hold the same number of voxels (1 .. 2^31 - 1), got {tuple(pred.shape)} and "
                         f"{tuple(target.shape)}")
    if p.device != t.device:
        raise ValueError(f"pred is on {p.device}, target on {t.device}")
    if out is None:
        out = torch.zeros((groups.R, 3), dtype=torch.int64, device=p.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (groups.R, 3) \
            or out.device != p.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 [{groups.R}, 3] table on {p.device}")
    L.call("mivp_group_counts", L.ptr(p), LABEL_DTYPES[p.dtype], 0 if pred_bits else 1, L.ptr(t), LABEL_DTYPES[t.dtype],
           p.numel(), groups.R, L.ptr(groups.tables(p.device)[0]), 0 if ig is None else ig, 0 if ig is None else 1,
           L.ptr(out), L.stream())
    return out


def group_scores(counts) -> Dict[str, np.ndarray]:
    """``{"dice": float64 [R], "iou": float64 [R]}`` on the host from an ``[R, 3]`` table of (intersection, predicted, target)
    counts: Dice = 2 I / (P + T), IoU = I / (P + T - I), NaN where both sets are empty -- such a group says nothing about
    the prediction, and the per-group means of BraTS / KiTS leave it out (``numpy.nanmean``).  ``SegMetrics.compute``
    (``_host.iou_dice``) instead adds 1e-6 to its denominators, which turns that case into a 0 inside its mean over the
    classes; elsewhere the two differ by less than 1e-6 relative.  A device table costs the one host read."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"counts must be an [R, 3] table, got {c.shape}")
    c = c.astype(np.float64)
    inter, both = c[:, 0], c[:, 1] + c[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        dice = np.where(both > 0, 2.0 * inter / both, np.nan)
        iou = np.where(both > 0, inter / (both - inter), np.nan)
    return {"dice": dice, "iou": iou}


# ---------------------------------------------------------------------------------------------
# the predictor
# ---------------------------------------------------------------------------------------------
class GroupEvaluation:
    """The multi-label methods of ``SlidingWindowPredictor`` (its base class, so that the predictor's own body keeps the
    methods it had).  Both are built on the public ``predict(x, return_logits=True)`` of a predictor whose ``num_classes``
    is the number of groups; the arg-max labels of that call are dropped."""

    def _group_logits(self, x, groups, thresholds):
        groups = _check_groups(groups)
        if self.ncls != groups.R:
            raise ValueError(f"the predictor was built for num_classes={self.ncls}, groups has {groups.R} groups")
        logit_thresholds(thresholds, groups.R)                     # refused before the prediction runs
        return self.predict(x, return_logits=True)["logits"]

    def predict_groups(self, x: torch.Tensor, groups: LabelGroups, thresholds: Union[float, Sequence[float]] = 0.5,
                       return_bits: bool = False, return_probs: bool = False) -> Dict[str, torch.Tensor]:
        """``decode_groups(predict(x, return_logits=True)["logits"], groups, thresholds, return_bits, return_probs)``: the
        whole-volume prediction of a model with one sigmoid channel per group as a label map."""
        return decode_groups(self._group_logits(x, groups, thresholds), groups, thresholds, return_bits, return_probs)

    def evaluate_groups(self, x: torch.Tensor, seg: torch.Tensor, groups: LabelGroups,
                        thresholds: Union[float, Sequence[float]] = 0.5, ignore_index: Optional[int] = None,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``group_counts`` of the bits map of ``predict_groups(x, groups, thresholds)`` against ``seg [1, 1, H, W, D]``
        (labels): the int64 ``[R, 3]`` device table, added onto ``out`` when given; ``group_scores`` turns it into Dice and
        IoU per group.  No host read."""
        self._check_input(seg, "seg", channels=1)
        _check_ignore(ignore_index)
        bits = decode_groups(self._group_logits(x, groups, thresholds), groups, thresholds, return_bits=True)["bits"]
        return group_counts(bits, seg, groups, ignore_index, out, pred_bits=True)


def evaluate_volume_groups(model, x: torch.Tensor, seg: torch.Tensor, roi: Sequence[int], groups: LabelGroups,
                           thresholds: Union[float, Sequence[float]] = 0.5, ignore_index: Optional[int] = None, out=None,
                           overlap: float = 0.5, mode: str = "gaussian", sigma_scale: float = 0.125, sub_batch: int = 10,
                           graph: bool = False, mirror_axes: Sequence[int] = (), skip=None, *, fit=None) -> torch.Tensor:
    """One-shot ``SlidingWindowPredictor(..., num_classes=groups.R, ...).evaluate_groups(x, seg, groups, thresholds,
    ignore_index, out)``: the per-group count table of the whole-volume prediction.  Keyword-only ``fit``: the predictor's
    ``fit=``."""
    from . import inference
    return inference._one_shot(model, x, None, _check_groups(groups).R, roi, overlap, mode, sigma_scale, sub_batch, graph,
                               mirror_axes, skip, fit).evaluate_groups(x, seg, groups, thresholds, ignore_index, out)
