"""Float64 reference of the Tversky + weighted (focal) cross-entropy loss with an ignore label (test helper, not a test
module).  Written from the definition in DESIGN 4.33 / include/mivp.h; nothing here shares code with the package.

Layouts (the kernels' own): logits [B, vol, C] (channels last), target [B, vol] (labels stored as f32), gradient like the
logits.  Options are a plain dict (``opts(...)``).

  valid voxel: label an integer in [0, C) and not ``ignore_index``; everything else adds to no sum and has gradient 0
  I = sum p t, P = sum p, T = sum t over the valid voxels of a sample (of the batch when ``batch``), p = softmax_c(z), s = 1e-5
  TI_c   = (2 I + s) / (2 I + 2 alpha (P - I) + 2 beta (T - I) + s)
  region = mean over (row, c >= c0) of 1 - TI_c                     (rows: the samples, or the one batch-wide row)
  voxel  = - sum_v w[y_v] (1 - p_y)^gamma log p_y / sum_v w[y_v]    (valid voxels of the whole batch; 0 when the sum is 0)
  loss   = lambda_region region + lambda_voxel voxel
1 - p_y is the sum of the other classes' probabilities and log p_y comes from log_softmax, so the float64 run keeps its
digits where the logits saturate (in float64 ``1 - p`` is 0 from a 37-logit gap on).

The bars are those of the sibling kernel (tests/loss_optim_ref.py): value 2e-5 max(1, |want|), gradient rel-L2 < 1e-4 and per
element LOSS_MARGIN x E32 x max |g64| with E32 from the float32 run of THIS file's formulas on the same case."""
import itertools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_optim_ref import (LOSS_L2_BAR, LOSS_MARGIN, LOSS_VALUE_BAR, U32, assert_within_located, gen,  # noqa: E402,F401
                            loss_grad_bar, loss_yardstick, rel_l2)

F64, F32 = torch.float64, torch.float32
SMOOTH = 1e-5
WEIGHTS8 = (0.5, 2.0, 1.0, 3.0, 0.25, 1.5, 0.75, 4.0)


def opts(alpha=0.5, beta=0.5, batch=False, include_background=True, focal_gamma=0.0, class_weights=None, ignore_index=None,
         lambda_region=1.0, lambda_voxel=1.0):
    return dict(alpha=alpha, beta=beta, batch=batch, include_background=include_background, focal_gamma=focal_gamma,
                class_weights=None if class_weights is None else tuple(float(w) for w in class_weights),
                ignore_index=ignore_index, lambda_region=lambda_region, lambda_voxel=lambda_voxel)


def opts_name(o):
    w = "none" if o["class_weights"] is None else "given"
    return (f"a{o['alpha']:g} b{o['beta']:g} batch{int(o['batch'])} bg{int(o['include_background'])} g{o['focal_gamma']:g} "
            f"w-{w} ig{o['ignore_index']} lr{o['lambda_region']:g} lv{o['lambda_voxel']:g}")


# ---------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------
def is_class(target, C):
    """bool [B, vol]: the label is an integer in [0, C)."""
    y = target.to(F64)
    return (y >= 0) & (y < C) & (y == y.floor())


def valid_mask(target, C, ignore_index):
    v = is_class(target, C)
    return v if ignore_index is None else v & (target.to(F64) != float(ignore_index))


def class_index(target, C):
    """int64 [B, vol]: the label where it is a class, 0 elsewhere (such voxels are masked by the caller)."""
    return torch.where(is_class(target, C), target.to(F64), torch.zeros((), dtype=F64)).long()


def _weights(o, C, dtype):
    return torch.ones(C, dtype=dtype) if o["class_weights"] is None else torch.tensor(o["class_weights"], dtype=F64).to(dtype)


def _tversky(I, P, T, o):
    return (2.0 * I + SMOOTH) / (2.0 * I + 2.0 * o["alpha"] * (P - I) + 2.0 * o["beta"] * (T - I) + SMOOTH)


def seg_loss_ref64(logits, target, o, dtype=F64):
    """(loss, d loss / d logits) by autograd in ``dtype`` (float64: the reference; float32: the same formulas at the kernels'
    precision, the yardstick E32)."""
    B, vol, C = logits.shape
    z = logits.detach().to(dtype).clone().requires_grad_(True)
    m = valid_mask(target, C, o["ignore_index"]).to(dtype)
    idx = class_index(target, C)
    hot = F.one_hot(idx, C).to(dtype)
    t = hot * m.unsqueeze(-1)
    logp = F.log_softmax(z, -1)
    p = logp.exp()
    pm = p * m.unsqueeze(-1)
    c0 = 0 if o["include_background"] else 1
    dims = (0, 1) if o["batch"] else (1,)
    I, P, T = (pm * t).sum(dims)[..., c0:], pm.sum(dims)[..., c0:], t.sum(dims)[..., c0:]
    loss = o["lambda_region"] * (1.0 - _tversky(I, P, T, o)).mean()
    wy = _weights(o, C, dtype)[idx] * m
    f = -(logp * hot).sum(-1)
    if o["focal_gamma"] != 0:
        f = f * (p * (1.0 - hot)).sum(-1) ** o["focal_gamma"]
    W = wy.sum()
    if float(W) > 0:
        loss = loss + o["lambda_voxel"] * (wy * f).sum() / W
    else:
        loss = loss + 0.0 * z.sum()                                # keeps the graph when only the voxel term was asked for
    loss.backward()
    return loss.detach().to(F64), z.grad.detach()


def seg_stats(logits, target, o, p_valid=None):
    """(I, P, T), each [rows, C] float64: rows = B, or 1 with ``batch``.  ``p_valid``: the mask P is summed under (default:
    the valid voxels)."""
    z = logits.to(F64)
    C = z.shape[-1]
    m = valid_mask(target, C, o["ignore_index"]).to(F64).unsqueeze(-1)
    mp = m if p_valid is None else p_valid.to(F64).unsqueeze(-1)
    p = z.softmax(-1)
    t = F.one_hot(class_index(target, C), C).to(F64) * m
    I, P, T = (p * t).sum(1), (p * mp).sum(1), t.sum(1)
    if o["batch"]:
        I, P, T = I.sum(0, keepdim=True), P.sum(0, keepdim=True), T.sum(0, keepdim=True)
    return I, P, T


def seg_grad_closed(logits, target, o, stats=None, sample_of=None, voxel_valid=None, voxel_weights=None, wsum=None):
    """The gradient again, in closed form (float64), with the hooks the corruption tests need:
      d region / d p_c = qa_c - t_c qb_c at a valid voxel, qa = wd 2 alpha N / D^2, qb = wd (2 / D - 2 (1 - alpha - beta) N / D^2),
      N = 2 I + s, D = the Tversky denominator, wd = lambda_region / (rows (C - c0)); dz_c = p_c (q_c - sum_k p_k q_k)
      d voxel / d z_c = lambda_voxel w_y / W f'(p_y) p_y (delta_cy - p_c),  f'(p) p = gamma p (1 - p)^(gamma - 1) log p - (1 - p)^gamma
    ``stats``: (I, P, T) rows to use instead of the case's own (any number of rows; wd keeps the case's row count);
    ``sample_of`` [B, vol] int64: the statistics row each voxel uses (default: its sample, or row 0 with ``batch``);
    ``voxel_valid`` [B, vol] bool: the voxels that get a voxel-term gradient (default: the valid ones; a label that is no
    class counts as class 0 there); ``voxel_weights``: the table the per-voxel weight is read from (W keeps the true one);
    ``wsum``: the normaliser to use instead of W."""
    z = logits.to(F64)
    B, vol, C = z.shape
    c0 = 0 if o["include_background"] else 1
    rows = 1 if o["batch"] else B
    wd = o["lambda_region"] / (rows * (C - c0))
    I, P, T = seg_stats(z, target, o) if stats is None else stats
    a, b = o["alpha"], o["beta"]
    N, D = 2.0 * I + SMOOTH, 2.0 * I + 2.0 * a * (P - I) + 2.0 * b * (T - I) + SMOOTH
    qa, qb = wd * 2.0 * a * N / (D * D), wd * (2.0 / D - 2.0 * (1.0 - a - b) * N / (D * D))
    qa[:, :c0], qb[:, :c0] = 0.0, 0.0
    if sample_of is None:
        sample_of = torch.zeros((B, vol), dtype=torch.int64) if o["batch"] else torch.arange(B).unsqueeze(1).expand(B, vol)
    valid = valid_mask(target, C, o["ignore_index"])
    m = valid.to(F64).unsqueeze(-1)
    idx = class_index(target, C)
    hot = F.one_hot(idx, C).to(F64)
    p = z.softmax(-1)
    q = qa[sample_of] - hot * m * qb[sample_of]
    g = p * (q - (p * q).sum(-1, keepdim=True)) * m
    w = _weights(o, C, F64)
    W = float((w[idx] * valid.to(F64)).sum()) if wsum is None else float(wsum)
    if o["lambda_voxel"] != 0 and W > 0:
        vv = (valid if voxel_valid is None else voxel_valid).to(F64)
        wy = (w if voxel_weights is None else torch.as_tensor(voxel_weights, dtype=F64))[idx] * vv
        py, om = (p * hot).sum(-1), (p * (1.0 - hot)).sum(-1)
        logp = (F.log_softmax(z, -1) * hot).sum(-1)
        gam = float(o["focal_gamma"])
        fp = -torch.ones_like(py) if gam == 0 else gam * py * om ** (gam - 1.0) * logp - om ** gam
        g = g + (o["lambda_voxel"] * wy / W * fp).unsqueeze(-1) * (hot - p)
    return g


class SegRef:
    """Reference value and gradient of a case with its yardstick; ``zero``: the reference gradient is zero everywhere (the
    kernel then owes bit-exact zeros, and E32 has no scale to refer to)."""

    def __init__(self, z, y, o):
        self.l64, self.g64 = seg_loss_ref64(z, y, o)
        self.l32, self.g32 = seg_loss_ref64(z, y, o, dtype=F32)
        self.zero = not bool(self.g64.abs().max() > 0)
        if not self.zero:
            self.e32, self.scale = loss_yardstick(self.g32, self.g64)
            self.bar_abs, self.bar_norm = loss_grad_bar(self.g32, self.g64)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def seg_inputs(B, vol, C, seed, kind="plain", ignore_index=None):
    """(logits [B, vol, C] f32, target [B, vol] f32).  Logits 2 randn, labels uniform in 0..C-1, then
    ignored:        20 % of the voxels carry ``ignore_index`` (with any kind, when an ignore label is given, unless noted)
    sample_ignored: sample 1 is the ignore label everywhere
    all_ignored:    the whole batch is
    absent:         class C - 2 occurs nowhere
    low_classes:    only classes 0 and 1 occur
    bad_labels:     a third of the voxels hold half-integers, -2, -1, C, C + 3 or 1e9
    saturated:      logits uniform in [-30, 30], a quarter of them exactly -30 or +30
    quad_tail:      the ignore label fills voxels 4..7 of sample 1 and the last vol % 4 (or 4) voxels of every sample, and
                    nothing else"""
    g = gen(seed)
    z = 2.0 * torch.randn((B, vol, C), generator=g, dtype=F32)
    y = torch.randint(0, C, (B, vol), generator=g).to(F32)
    spread = torch.rand((B, vol), generator=g) < 0.2
    ig = None if ignore_index is None else float(ignore_index)
    if kind == "absent":
        y[y == float(C - 2)] = float(C - 1)
    elif kind == "low_classes":
        y = torch.randint(0, 2, (B, vol), generator=g).to(F32)
    elif kind == "bad_labels":
        bad = torch.tensor([0.5, 1.5, -2.0, -1.0, float(C), float(C + 3), 1e9, C - 0.5], dtype=F32)
        pick = torch.randint(0, len(bad), (B, vol), generator=g)
        hit = torch.rand((B, vol), generator=g) < 1.0 / 3.0
        y = torch.where(hit, bad[pick], y)
    elif kind == "saturated":
        z = 60.0 * torch.rand((B, vol, C), generator=g, dtype=F32) - 30.0
        pin = torch.rand((B, vol, C), generator=g) < 0.25
        z[pin] = torch.sign(z[pin]) * 30.0
    else:
        assert kind in ("plain", "ignored", "sample_ignored", "all_ignored", "quad_tail"), kind
    if kind == "quad_tail":
        assert ig is not None and vol >= 8
        y[1, 4:8] = ig
        y[:, vol - (vol % 4 or 4):] = ig
    elif ig is not None:
        y[spread] = ig
        if kind == "sample_ignored":
            y[1] = ig
        if kind == "all_ignored":
            y[:] = ig
    else:
        assert kind not in ("ignored", "sample_ignored", "all_ignored"), kind
    return z, y


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_hip_segloss.py (tests/test_segloss_host.py checks the bars on the same draws)
# ---------------------------------------------------------------------------------------------
SCALAR_VOLS = ((3, 3, 7), (5, 7, 9), (13, 79, 1))       # 63, 315, 1027 voxels: vol % 4 != 0; one and two partial rows
VEC_VOLS = ((1, 1, 4), (2, 2, 2), (6, 7, 8))            # 4, 8, 336 voxels: 16-byte loads of four voxels
CLASSES = (2, 3, 4, 5, 6, 7, 8)
AB = ((0.5, 0.5), (0.3, 0.7))
GAMMAS = (0.0, 1.0, 2.0)
IGNORES = (None, 255, -1)
LAMBDAS = ((1.0, 0.0), (0.0, 1.0))                      # each term alone


def batch_of(vol):
    return 5 if vol == 4 else 3


def ladder_options(C):
    """Six option sets that between them hold every option value: run at every C on both paths."""
    w = WEIGHTS8[:C]
    return (opts(),
            opts(0.3, 0.7, True, False, 2.0, w, 255),
            opts(0.3, 0.7, True, True, 1.0, w, -1, 0.5, 2.0),
            opts(0.5, 0.5, False, False, 1.0, None, 255, 1.0, 0.0),
            opts(0.3, 0.7, False, True, 2.0, w, -1, 0.0, 1.0),
            opts(0.3, 0.7, False, False, 0.0, w, None))


def ladder_case(dims, C, o):
    vol = dims[0] * dims[1] * dims[2]
    ig = o["ignore_index"]
    return seg_inputs(batch_of(vol), vol, C, 1000 * C + vol, "plain" if ig is None else "ignored", ig)


PRODUCT_CLASSES = (2, 5)
PRODUCT_DIMS = ((3, 3, 7), (6, 7, 8))                   # one scalar, one vectorised; B = 3: 189 and 1008 voxels in all


def product_options(C, ignore_index):
    """The full product of the option values at one ignore label: 2 x 2 x 2 x 3 x 2 x 2 = 96 sets."""
    out = []
    for bg, batch, (a, b), gam, wts, (lr, lv) in itertools.product((True, False), (False, True), AB, GAMMAS, (False, True),
                                                                   LAMBDAS):
        out.append(opts(a, b, batch, bg, gam, WEIGHTS8[:C] if wts else None, ignore_index, lr, lv))
    return out


PARTIAL_ROW_VOLS = ((2052, 3), (2053, 3))               # (voxels, partial rows per sample)
CAP_VOL = 66 * 64 * 64                                  # 270 336 voxels: the 256-row cap, the statistics loop strides
GRID_CAP_DIMS = (101, 101, 103)                         # scalar gradient pass beyond its 8192 workgroups at B = 2


def big_options(C=2):
    return opts(0.3, 0.7, True, False, 2.0, WEIGHTS8[:C], 255)


def special_cases():
    """(name, C, kind, options) of the special operands; each runs at B = 3 on 315 (scalar) and 336 (vectorised) voxels."""
    w3, w4 = (1.0, 0.0, 2.0), (0.0, 0.0, 3.0, 1.0)
    return (
        ("sample ignored", 3, "sample_ignored", opts(0.3, 0.7, False, True, 1.0, w3, 255)),
        ("sample ignored, batch", 3, "sample_ignored", opts(0.5, 0.5, True, False, 0.0, None, -1)),
        ("batch ignored", 3, "all_ignored", opts(0.3, 0.7, False, True, 2.0, w3, 255)),
        ("batch ignored, voxel alone", 2, "all_ignored", opts(focal_gamma=0.0, ignore_index=-1, lambda_region=0.0)),
        ("zero-weight class", 3, "plain", opts(0.5, 0.5, False, True, 0.0, w3, None)),
        ("zero-weight class, ignore", 3, "ignored", opts(0.3, 0.7, True, True, 2.0, w3, 255)),
        ("absent class", 5, "absent", opts(0.3, 0.7, False, False, 1.0, WEIGHTS8[:5], None)),
        ("absent class, batch", 5, "absent", opts(0.5, 0.5, True, True, 0.0, None, 255)),
        ("only zero-weight classes", 4, "low_classes", opts(0.3, 0.7, False, True, 1.0, w4, None)),
        ("only zero-weight classes, voxel alone", 4, "low_classes", opts(0.5, 0.5, False, True, 2.0, w4, 255, 0.0, 1.0)),
        ("bad labels", 4, "bad_labels", opts(0.3, 0.7, False, True, 1.0, WEIGHTS8[:4], None)),
        ("bad labels, ignore", 4, "bad_labels", opts(0.5, 0.5, True, False, 2.0, WEIGHTS8[:4], 255)),
        ("bad labels, ignore a class", 4, "bad_labels", opts(0.5, 0.5, False, True, 0.0, None, 2)),
        ("saturated g0", 3, "saturated", opts(0.5, 0.5, False, True, 0.0, w3, None)),
        ("saturated g1", 3, "saturated", opts(0.3, 0.7, False, False, 1.0, None, 255)),
        ("saturated g2", 2, "saturated", opts(0.3, 0.7, True, True, 2.0, (0.5, 2.0), -1)),
        ("saturated g2, voxel alone", 8, "saturated", opts(0.5, 0.5, False, True, 2.0, WEIGHTS8, None, 0.0, 1.0)),
        ("quad and tail ignored", 3, "quad_tail", opts(0.3, 0.7, False, True, 1.0, w3, 255)),
        ("quad and tail ignored, batch", 5, "quad_tail", opts(0.5, 0.5, True, False, 2.0, WEIGHTS8[:5], -1)),
    )


SPECIAL_VOLS = (315, 336)


def special_inputs(i, vol):
    name, C, kind, o = special_cases()[i]
    return seg_inputs(3, vol, C, 77 + vol + i, kind, o["ignore_index"])


FORMS_VOLS = (315, 336)


def forms_case(vol):
    o = opts(0.3, 0.7, False, False, 2.0, (0.5, 2.0, 1.0), 255)
    z, y = seg_inputs(3, vol, 3, 55 + vol, "ignored", 255)
    return z, y, o


WRAPPER_DIMS = ((5, 7, 9), (6, 7, 8))


def wrapper_case(dims):
    vol = dims[0] * dims[1] * dims[2]
    o = opts(0.3, 0.7, False, True, 1.0, WEIGHTS8[:4], 255, 1.0, 0.5)
    z, y = seg_inputs(3, vol, 4, 66 + vol, "ignored", 255)
    return z, y, o
