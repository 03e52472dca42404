"""Float64 reference of the multi-label (overlapping label groups) loss, and numpy restatements of the two tables, the decode
and the group counts (test helper, not a test module).  Written from the definitions in DESIGN 4.45 / include/mivp.h;
nothing here shares code with the package.

Layouts (the kernels' own): logits [B, vol, R] (channels last), target [B, vol] (labels stored as f32), gradient like the
logits.  Groups are a list of tuples of labels, options a plain dict (``opts(...)``).

  valid voxel: the label is an integer in 0..255, known (0 and the union of the groups unless ``labels`` says otherwise) and
  not ``ignore_index``; V = the valid voxels, N = |V| over the batch
  t_r = [label in group r], p_r = sigmoid(z_r), s = 1e-5, sums over V of a sample (of the batch when ``batch``)
  I = sum p t, P = sum p, T = sum t;  TI_r = (2 I + s) / (2 I + 2 alpha (P - I) + 2 beta (T - I) + s)
  region = mean over (row, r) of 1 - TI_r
  f_r    = w_r [ t_r pi_r (1 - p_r)^gamma (-log p_r) + (1 - t_r) p_r^gamma (-log(1 - p_r)) ]
  voxel  = sum_V sum_r f_r / (R max(N, 1));   loss = lambda_region region + lambda_voxel voxel
-log p and -log(1 - p) are ``-logsigmoid(+-z)`` and 1 - p is ``sigmoid(-z)``, so the float64 run keeps its digits where the
logits saturate.

The bars are the siblings' (tests/segloss_ref.py, tests/loss_optim_ref.py): value 2e-5 max(1, |want|), gradient rel-L2 < 1e-4
and per element LOSS_MARGIN x E32 x max |g64| with E32 from the float32 run of THIS file's formulas on the same case."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_optim_ref import (LOSS_L2_BAR, LOSS_MARGIN, LOSS_VALUE_BAR, assert_within_located, gen,  # noqa: E402,F401
                            loss_grad_bar, loss_yardstick, rel_l2)

F64, F32 = torch.float64, torch.float32
SMOOTH = 1e-5
KNOWN = 256
BRATS = [(1, 2, 3), (2, 3), (3,)]
GROUPS = {1: [(1,)], 3: BRATS, 8: [(1, 2, 3, 4, 5, 6, 7, 8), (2, 3, 4, 5, 6, 7, 8), (3, 4, 5, 6, 7, 8), (4, 5, 6, 7, 8),
                                    (5, 6, 7, 8), (6, 7, 8), (7, 8), (8,)]}
WEIGHTS8 = (0.5, 2.0, 1.0, 3.0, 0.25, 1.5, 0.75, 4.0)
POS8 = (2.0, 0.5, 3.0, 1.0, 1.5, 0.25, 4.0, 0.75)


def opts(alpha=0.5, beta=0.5, batch=False, focal_gamma=0.0, group_weights=None, pos_weight=None, ignore_index=None,
         lambda_region=1.0, lambda_voxel=1.0):
    return dict(alpha=alpha, beta=beta, batch=batch, focal_gamma=focal_gamma,
                group_weights=None if group_weights is None else tuple(float(w) for w in group_weights),
                pos_weight=None if pos_weight is None else tuple(float(w) for w in pos_weight),
                ignore_index=ignore_index, lambda_region=lambda_region, lambda_voxel=lambda_voxel)


# ---------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------
def member_np(groups, labels=None):
    """int32 [256]: bits 0..R-1 = the groups that contain the label, bit 8 = the label is known."""
    known = set([0] + [v for g in groups for v in g]) if labels is None else set(labels)
    m = np.zeros(256, dtype=np.int32)
    for v in known:
        m[v] |= KNOWN
    for r, g in enumerate(groups):
        for v in g:
            m[v] |= 1 << r
    return m


def lut_np(groups, write):
    """uint8 [2^R]: start at 0, walk the groups in index order, a set bit r overwrites with write[r]."""
    R = len(groups)
    out = np.zeros(1 << R, dtype=np.uint8)
    for bits in range(1 << R):
        for r in range(R):
            if bits & (1 << r):
                out[bits] = write[r]
    return out


def default_write(groups):
    return [[v for v in g if all(v not in h for h in groups[r + 1:])][0] for r, g in enumerate(groups)]


def valid_and_targets(target, groups, ignore_index, labels=None):
    """(valid bool [...], t bool [..., R]) of labels stored in any dtype."""
    y = torch.as_tensor(target).to(F64)
    mem = torch.from_numpy(member_np(groups, labels)).long()
    inr = (y >= 0) & (y < 256) & (y == y.floor())
    e = mem[torch.where(inr, y, torch.zeros((), dtype=F64)).long()]
    valid = inr & ((e & KNOWN) != 0)
    if ignore_index is not None:
        valid = valid & (y != float(ignore_index))
    t = torch.stack([((e >> r) & 1).bool() & valid for r in range(len(groups))], dim=-1)
    return valid, t


# ---------------------------------------------------------------------------------------------
# the loss
# ---------------------------------------------------------------------------------------------
def multilabel_ref64(logits, target, groups, o, dtype=F64):
    """(loss, d loss / d logits) by autograd in ``dtype`` (float64: the reference; float32: the same formulas at the kernels'
    precision, the yardstick E32)."""
    B, vol, R = logits.shape
    z = logits.detach().to(dtype).clone().requires_grad_(True)
    valid, tb = valid_and_targets(target, groups, o["ignore_index"])
    m, t = valid.to(dtype).unsqueeze(-1), tb.to(dtype)
    p, q = torch.sigmoid(z), torch.sigmoid(-z)
    nlp, nlq = -F.logsigmoid(z), -F.logsigmoid(-z)
    dims = (0, 1) if o["batch"] else (1,)
    I, P, T = (p * t).sum(dims), (p * m).sum(dims), t.sum(dims)
    ti = (2.0 * I + SMOOTH) / (2.0 * I + 2.0 * o["alpha"] * (P - I) + 2.0 * o["beta"] * (T - I) + SMOOTH)
    loss = o["lambda_region"] * (1.0 - ti).mean()
    w = torch.ones(R, dtype=dtype) if o["group_weights"] is None else torch.tensor(o["group_weights"], dtype=F64).to(dtype)
    pi = torch.ones(R, dtype=dtype) if o["pos_weight"] is None else torch.tensor(o["pos_weight"], dtype=F64).to(dtype)
    gam = o["focal_gamma"]
    fpos, fneg = (nlp, nlq) if gam == 0 else (q ** gam * nlp, p ** gam * nlq)
    f = (w * (t * pi * fpos + (m - t) * fneg)).sum()
    loss = loss + o["lambda_voxel"] * f / (R * max(int(valid.sum()), 1)) + 0.0 * z.sum()
    loss.backward()
    return loss.detach().to(F64), z.grad.detach()


class MlRef:
    """Reference value and gradient of a case with its yardstick (the structure of segloss_ref.SegRef); ``zero``: the
    reference gradient is zero everywhere (the kernel then owes bit-exact zeros, and E32 has no scale to refer to)."""

    def __init__(self, z, y, groups, o):
        self.l64, self.g64 = multilabel_ref64(z, y, groups, o)
        self.l32, self.g32 = multilabel_ref64(z, y, groups, o, dtype=F32)
        self.zero = not bool(self.g64.abs().max() > 0)
        self.valid = valid_and_targets(y, groups, o["ignore_index"])[0]
        if not self.zero:
            self.e32, self.scale = loss_yardstick(self.g32, self.g64)
            self.bar_abs, self.bar_norm = loss_grad_bar(self.g32, self.g64)


def inputs(B, vol, groups, seed, kind="plain", ignore_index=None):
    """(logits [B, vol, R] f32, target [B, vol] f32).  Logits 2 randn, labels uniform over the known labels, then
    ignored:        about 20 % of the voxels carry ``ignore_index`` and a tenth hold half-integers or unknown labels
    sample_invalid: sample 1 holds an unknown label everywhere
    absent:         the labels of the last group occur nowhere (they become 0)
    saturated:      logits uniform in [-30, 30], a quarter of them exactly -30 or +30"""
    g = gen(seed)
    R = len(groups)
    known = torch.tensor(sorted(set([0] + [v for gr in groups for v in gr])), dtype=F32)
    z = 2.0 * torch.randn((B, vol, R), generator=g, dtype=F32)
    y = known[torch.randint(0, len(known), (B, vol), generator=g)]
    if kind == "ignored":
        assert ignore_index is not None
        y[torch.rand((B, vol), generator=g) < 0.2] = float(ignore_index)
        bad = torch.tensor([0.5, 1.5, -1.0, 200.0, 256.0, 1e9, float("nan"), 77.0], dtype=F32)
        hit = torch.rand((B, vol), generator=g) < 0.1
        y = torch.where(hit, bad[torch.randint(0, len(bad), (B, vol), generator=g)], y)
    elif kind == "sample_invalid":
        y[1] = 99.0
    elif kind == "absent":
        for v in groups[-1]:
            y[y == float(v)] = 0.0
    elif kind == "saturated":
        z = 60.0 * torch.rand((B, vol, R), generator=g, dtype=F32) - 30.0
        pin = torch.rand((B, vol, R), generator=g) < 0.25
        z[pin] = torch.sign(z[pin]) * 30.0
    else:
        assert kind == "plain", kind
    return z, y


def loss_cases(R):
    """(name, kind, options) of the loss cases at R groups."""
    w = list(WEIGHTS8[:R])
    w[R // 2] = 0.0                                                # one group weight is 0
    return (
        ("defaults", "plain", opts()),
        ("batch", "plain", opts(batch=True)),
        ("alpha != beta", "plain", opts(0.3, 0.7)),
        ("gamma 2, weights", "plain", opts(0.3, 0.7, False, 2.0, w, POS8[:R])),
        ("ignore + bad labels", "ignored", opts(0.5, 0.5, False, 1.0, None, POS8[:R], 255)),
        ("sample invalid", "sample_invalid", opts(0.3, 0.7, False, 0.0, WEIGHTS8[:R], None)),
        ("sample invalid, batch", "sample_invalid", opts(batch=True, focal_gamma=2.0)),
        ("absent group", "absent", opts(0.3, 0.7, False, 1.0)),
        ("absent group, batch", "absent", opts(batch=True)),
        ("saturated g0", "saturated", opts()),
        ("saturated g2", "saturated", opts(0.3, 0.7, True, 2.0, WEIGHTS8[:R], POS8[:R])),
        ("region alone", "plain", opts(0.3, 0.7, lambda_voxel=0.0)),
        ("voxel alone", "plain", opts(focal_gamma=2.0, pos_weight=POS8[:R], lambda_region=0.0)),
    )


# ---------------------------------------------------------------------------------------------
# decode and counts
# ---------------------------------------------------------------------------------------------
def logit_thresholds_np(qs, R):
    qs = [qs] * R if np.isscalar(qs) else list(qs)
    return np.array([np.float32(np.log(np.float64(q) / (1.0 - np.float64(q)))) for q in qs], dtype=np.float32)


def decode_np(z_planes, groups, write, qs):
    """z_planes f32 [R, ...] -> (labels uint8 [...], bits uint8 [...])."""
    R = len(groups)
    tau = logit_thresholds_np(qs, R)
    bits = np.zeros(z_planes.shape[1:], dtype=np.uint8)
    for r in range(R):
        bits |= (z_planes[r] > tau[r]).astype(np.uint8) << r
    return lut_np(groups, write)[bits], bits


def counts_np(pred, target, groups, ignore_index=None, pred_bits=False):
    """int64 [R, 3]: (|pred_r and t_r|, |pred_r|, |t_r|) over the valid voxels of target."""
    valid, t = valid_and_targets(np.asarray(target, dtype=np.float64), groups, ignore_index)
    if pred_bits:
        pb = torch.as_tensor(np.asarray(pred).astype(np.int64))
        p = torch.stack([((pb >> r) & 1).bool() for r in range(len(groups))], dim=-1)
    else:
        mem = torch.from_numpy(member_np(groups)).long()
        y = torch.as_tensor(np.asarray(pred, dtype=np.float64))
        inr = (y >= 0) & (y < 256) & (y == y.floor())
        e = torch.where(inr, mem[torch.where(inr, y, torch.zeros((), dtype=F64)).long()], torch.zeros((), dtype=torch.int64))
        p = torch.stack([((e >> r) & 1).bool() for r in range(len(groups))], dim=-1)
    p = p & valid.unsqueeze(-1)
    R = len(groups)
    return np.array([[int((p[..., r] & t[..., r]).sum()), int(p[..., r].sum()), int(t[..., r].sum())] for r in range(R)],
                    dtype=np.int64)
