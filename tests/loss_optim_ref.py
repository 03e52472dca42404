"""Float64 references of the loss, optimizer and metric-count kernels (test helper, not a test module).

Everything is float64 torch / numpy on the CPU, written from the formulas in the header comment of csrc/loss.hip, in
oracle/loss_ref.py, in the comment of ``k_adamw_multi`` / ``k_ema_multi`` (csrc/proto.hip) and in csrc/metrics.hip; nothing
here shares code with the package.

Layouts (the kernels' own): logits [B, vol, C] (channels last), target [B, vol] (class indices stored as f32), gradient like
the logits.  ``seg_counts_ref`` takes the logical [B, C, vol] logits, whatever the memory layout under test.

Kinds of bar:
  loss value     2e-5 max(1, |want|) against float64 (the project's bar)
  loss gradient  rel-L2 < 1e-4 (the project's bar) AND, per element, |got - g64| <= LOSS_MARGIN * E32 * max |g64| where
                 E32 = max |g32 - g64| / max |g64| (floored at 2^-24) is what THIS file's formulas lose when run in f32 on the
                 same case.  LOSS_MARGIN is the next power of two above twice the worst kernel / E32 ratio measured on an
                 MI355X over every case of tests/test_hip_loss_optim.py (DESIGN 5.3 lists them).
  AdamW, EMA     per element within a propagated rounding bound: unit roundoff 2^-24 per f32 operation, sqrt and divide
                 correctly rounded, FMA contraction only removes roundings, bounds carried from step to step
  counts         integer-exact"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from exact_ref import assert_equal_located, gen  # noqa: E402,F401

F64, F32 = torch.float64, torch.float32
U32 = 2.0 ** -24                 # unit roundoff of f32
TINY = 2.0 ** -126               # smallest normal f32: covers underflow (gradual or flushed) of one operation
LOSS_MARGIN = 8.0                # measured: see the module docstring and DESIGN 5.3
LOSS_VALUE_BAR = 2e-5
LOSS_L2_BAR = 1e-4


def f32_of(x):
    """The f32 value a C float parameter receives, as a Python float."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------
# located comparison within a bound
# ---------------------------------------------------------------------------------------------
def assert_within_located(got, ref64, bound, layout, what=""):
    """|got - ref64| <= bound at every element (a NaN in ``got`` fails).  ``bound`` is a tensor of the reference's shape or
    a number; ``layout`` names the axes (one letter each), as in exact_ref.assert_equal_located.  A failure lists the first
    ten offending indices with got / want / bound."""
    g = got.detach().to(F64).cpu()
    r = ref64.detach().to(F64).cpu()
    b = bound.detach().to(F64).cpu().expand_as(r) if isinstance(bound, torch.Tensor) else torch.full_like(r, float(bound))
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} != reference {tuple(r.shape)}"
    assert len(layout) == g.dim(), (layout, tuple(g.shape))
    assert bool(torch.isfinite(r).all()) and bool((b >= 0).all()), f"{what}: the reference or its bound is not finite"
    bad = ~((g - r).abs() <= b)
    if not bool(bad.any()):
        return
    idx = [tuple(int(i) for i in row) for row in torch.nonzero(bad)[:10]]
    lines = [f"{what}: {int(bad.sum())} of {g.numel()} elements leave the bound of the float64 reference"
             f" (axes {layout}, shape {tuple(g.shape)})"]
    for i in idx:
        lines.append(f"  {i}: got {float(g[i])!r} want {float(r[i])!r} bound {float(b[i]):.3e}"
                     f" (off by {abs(float(g[i]) - float(r[i])):.3e})")
    msg = "\n".join(lines)
    print(msg)
    raise AssertionError(msg)


def rel_l2(a, b):
    a, b = a.detach().to(F64).cpu().reshape(-1), b.detach().to(F64).cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------
# Dice + sigmoid focal loss
# ---------------------------------------------------------------------------------------------
def _onehot(target, C, dtype):
    return (target.to(F64).unsqueeze(-1) == torch.arange(C, dtype=F64)).to(dtype)


def dice_focal_ref64(logits, target, include_background, gamma, dtype=F64):
    """(loss, d loss / d logits) by autograd in ``dtype`` (float64: the reference; float32: the same formulas at the kernels'
    precision, the yardstick E32).  logits [B, vol, C], target [B, vol]; gamma < 0: the Dice term alone.
      dice_bc = 1 - (2 I + 1e-5) / (P + T + 1e-5),  I = sum p t, P = sum p, T = sum t over the voxels, p = softmax_c(z)
      focal   = mean over (b, voxel, c) of exp(gamma logsigmoid(-z (2t - 1))) (z - z t - logsigmoid(z))
      loss    = mean_bc dice_bc + focal, class 0 dropped from both when include_background is false"""
    C = logits.shape[-1]
    z = logits.detach().to(dtype).clone().requires_grad_(True)
    t = _onehot(target, C, dtype)
    p = z.softmax(-1)
    c0 = 0 if include_background else 1
    pz, tz, zz = p[..., c0:], t[..., c0:], z[..., c0:]
    inter, den = (pz * tz).sum(1), pz.sum(1) + tz.sum(1)
    loss = (1.0 - (2.0 * inter + 1e-5) / (den + 1e-5)).mean()
    if gamma >= 0:
        bce = zz - zz * tz - F.logsigmoid(zz)
        loss = loss + ((F.logsigmoid(-zz * (2.0 * tz - 1.0)) * gamma).exp() * bce).mean()
    loss.backward()
    return loss.detach().to(F64), z.grad.detach()


def dice_stats(logits, target):
    """(I, P, T), each [B, C] float64."""
    z = logits.to(F64)
    p, t = z.softmax(-1), _onehot(target, z.shape[-1], F64)
    return (p * t).sum(1), p.sum(1), t.sum(1)


def dice_focal_grad_closed(logits, target, include_background, gamma, stats=None, sample_of=None, focal_classes=None):
    """The gradient again, in closed form (float64), with the hooks the corruption tests need:
      d dice mean / d p_c = wd (Nn / Dn^2 - 2 t / Dn) =: q_c (0 for a dropped class), dz_c = p_c (q_c - sum_k p_k q_k)
      d focal / d z_c = wf w ((sigmoid(z) - t) - bce gamma s sigmoid(z s)),  s = 2t - 1, w = exp(gamma logsigmoid(-z s))
    ``stats``: (I, P, T) to use instead of the case's own; ``sample_of`` [B, vol] int64: the sample whose Dice sums each
    voxel uses (default: its own); ``focal_classes``: the classes that get a focal term (default: every kept class)."""
    z = logits.to(F64)
    B, vol, C = z.shape
    c0 = 0 if include_background else 1
    ncls = C - c0
    wd, wf = 1.0 / (B * ncls), 1.0 / (B * ncls * vol)
    I, P, T = dice_stats(z, target) if stats is None else stats
    Dn, Nn = P + T + 1e-5, 2.0 * I + 1e-5
    qa, qb = wd * Nn / (Dn * Dn), wd * 2.0 / Dn
    qa[:, :c0], qb[:, :c0] = 0.0, 0.0
    if sample_of is None:
        sample_of = torch.arange(B).unsqueeze(1).expand(B, vol)
    t = _onehot(target, C, F64)
    p = z.softmax(-1)
    q = qa[sample_of] - t * qb[sample_of]
    g = p * (q - (p * q).sum(-1, keepdim=True))
    if gamma >= 0:
        s = 2.0 * t - 1.0
        w = (gamma * F.logsigmoid(-z * s)).exp()
        bce = z - z * t - F.logsigmoid(z)
        gf = wf * (w * (torch.sigmoid(z) - t) - bce * gamma * w * s * torch.sigmoid(z * s))
        keep = torch.zeros(C, dtype=F64)
        keep[list(range(c0, C)) if focal_classes is None else list(focal_classes)] = 1.0
        g = g + gf * keep
    return g


def loss_yardstick(g32, g64):
    """(E32, max |g64|): what the f32 run of the reference formulas loses on this case, floored at one unit roundoff."""
    scale = float(g64.abs().max())
    assert scale > 0
    return max(float((g32.to(F64) - g64).abs().max()) / scale, U32), scale


def loss_grad_bar(g32, g64, margin=LOSS_MARGIN):
    """The per-element bar of a case: margin E32 max |g64| (absolute), and the same in the normalised max norm."""
    e32, scale = loss_yardstick(g32, g64)
    return margin * e32 * scale, margin * e32


# ---------------------------------------------------------------------------------------------
# rounding-bound arithmetic: (value, bound) pairs, float64 tensors
# ---------------------------------------------------------------------------------------------
def _rnd(val, err):
    """One f32 rounding of a result whose un-rounded form is within ``err`` of ``val``."""
    return err + U32 * (val.abs() + err) + TINY


def _add(a, ea, b, eb):
    v = a + b
    return v, _rnd(v, ea + eb)


def _mul(a, ea, b, eb):
    v = a * b
    return v, _rnd(v, a.abs() * eb + b.abs() * ea + ea * eb)


def _div(a, ea, b, eb):
    v = a / b
    lo = b.abs() - eb
    assert bool((lo > 0).all()), "a divisor's bound reaches zero"
    return v, _rnd(v, (ea + v.abs() * eb) / lo)


def _sqrt(a, ea):
    v = a.sqrt()
    return v, _rnd(v, (a + ea).sqrt() - (a - ea).clamp_min(0.0).sqrt())


def _c(x, like):
    return torch.full_like(like, float(x))


# ---------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------
def adam_hyper_row(lr, betas, eps, weight_decay, step):
    """[8] f32 as FusedAdamW._hyper builds it: lr, beta1, beta2, eps, weight_decay, 1 - beta1^t, sqrt(1 - beta2^t), 0."""
    b1, b2 = betas
    return np.asarray([lr, b1, b2, eps, weight_decay, 1.0 - b1 ** float(step), math.sqrt(1.0 - b2 ** float(step)), 0.0],
                      np.float32)


class AdamState:
    """p, m, v of one tensor as float64 references with their bounds (zero for a state that is exactly the f32 start)."""

    def __init__(self, p, m=None, v=None):
        self.p = p.detach().to(F64).cpu().clone()
        self.m = torch.zeros_like(self.p) if m is None else m.detach().to(F64).cpu().clone()
        self.v = torch.zeros_like(self.p) if v is None else v.detach().to(F64).cpu().clone()
        self.ep, self.em, self.ev = (torch.zeros_like(self.p) for _ in range(3))


def adamw_ref64(st, g, hyper):
    """One step of torch.optim.AdamW's single-tensor formulas as k_adamw_multi quotes them, on the f32 row ``hyper``:
        p *= 1 - lr wd ; m = m + (g - m) (1 - b1) ; v = v b2 + (g g) (1 - b2)
        denom = sqrt(v) / bc2_sqrt + eps ; p -= (lr / bc1) (m / denom)
    Returns a new AdamState: float64 values of that step from ``st``'s values, and bounds on |f32 result - value| for any f32
    evaluation of these operations that starts within ``st``'s bounds (every operation rounds once, or not at all where
    a multiply-add is contracted).  The row's 1 - beta1^t is itself a rounding of the double value that torch divides by:
    it carries half an ulp of its own, so that both ways of forming lr / bc1 are inside."""
    h = [float(x) for x in np.asarray(hyper, np.float32)]
    lr, b1, b2, eps, wd, bc1, bc2s = h[:7]
    g = g.detach().to(F64).cpu()
    z = torch.zeros_like(g)
    k = lambda x: _c(x, g)                                        # noqa: E731
    out = AdamState(st.p)
    # p1 = p (1 - lr wd)
    t, et = _mul(k(lr), z, k(wd), z)
    a, ea = _add(k(1.0), z, -t, et)
    p1, ep1 = _mul(st.p, st.ep, a, ea)
    # m' = m + (g - m) (1 - b1)
    c1, ec1 = _add(k(1.0), z, k(-b1), z)
    d, ed = _add(g, z, -st.m, st.em)
    dc, edc = _mul(d, ed, c1, ec1)
    out.m, out.em = _add(st.m, st.em, dc, edc)
    # v' = v b2 + (g g) (1 - b2)
    c2, ec2 = _add(k(1.0), z, k(-b2), z)
    vb, evb = _mul(st.v, st.ev, k(b2), z)
    gg, egg = _mul(g, z, g, z)
    ggc, eggc = _mul(gg, egg, c2, ec2)
    out.v, out.ev = _add(vb, evb, ggc, eggc)
    # denom = sqrt(v') / bc2_sqrt + eps
    s, es = _sqrt(out.v, out.ev)
    r, er = _div(s, es, k(bc2s), z)
    den, eden = _add(r, er, k(eps), z)
    # p' = p1 - (lr / bc1) (m' / denom)
    step, estep = _div(k(lr), z, k(bc1), k(U32 * bc1))
    q, eq = _div(out.m, out.em, den, eden)
    sq, esq = _mul(step, estep, q, eq)
    out.p, out.ep = _add(p1, ep1, -sq, esq)
    return out


# ---------------------------------------------------------------------------------------------
# EMA
# ---------------------------------------------------------------------------------------------
def ema_om(tau):
    """1 - tau as k_ema_multi forms it: f32(1 - f32(tau))."""
    return float(np.float32(1.0) - np.float32(tau))


def ema_ref64(teacher, student, tau):
    """(tau t + om s, bound) with tau = f32(tau) and om = f32(1 - f32(tau)): two product roundings and one of the sum (one
    product rounding less under contraction)."""
    t, s = teacher.detach().to(F64).cpu(), student.detach().to(F64).cpu()
    z = torch.zeros_like(t)
    a, ea = _mul(_c(f32_of(tau), t), z, t, z)
    b, eb = _mul(_c(ema_om(tau), t), z, s, z)
    return _add(a, ea, b, eb)


# ---------------------------------------------------------------------------------------------
# per-class counts of arg-max(logits) against a label volume
# ---------------------------------------------------------------------------------------------
def seg_counts_ref(logits, target, C):
    """int64 [C, 3]: |pred == c & target == c|, |pred == c|, |target == c| with pred = torch.argmax over the class axis of
    logits [B, C, vol] (the FIRST maximum); a label outside 0..C-1 or not an integer matches no class.  NaN logits are out of
    contract."""
    assert logits.shape[1] == C and not bool(torch.isnan(logits).any())
    pred = torch.argmax(logits.to(F64), dim=1).reshape(-1)
    tgt = target.to(F64).reshape(-1)
    out = torch.zeros((C, 3), dtype=torch.int64)
    for c in range(C):
        pc, tc = pred == c, tgt == float(c)
        out[c] = torch.tensor([int((pc & tc).sum()), int(pc.sum()), int(tc.sum())])
    return out


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_hip_loss_optim.py (tests/test_loss_optim_host.py checks the bars on the same draws)
# ---------------------------------------------------------------------------------------------
SCALAR_VOLS = ((3, 3, 7), (5, 7, 9), (13, 79, 1))       # 63, 315, 1027 voxels: vol % 4 != 0
VEC_VOLS = ((1, 1, 4), (2, 2, 2), (6, 7, 8))            # 4, 8, 336 voxels: 16-byte loads of four voxels
LOSS_CLASSES = (2, 3, 4, 5, 6, 7, 8)
LOSS_MODES = ((1, 4.0), (0, 4.0), (1, -1.0), (0, -1.0))  # (include_background, gamma); gamma < 0: Dice alone


def loss_inputs(B, vol, C, seed, kind="plain"):
    """(logits [B, vol, C] f32, target [B, vol] f32).  plain: 2 randn logits, labels uniform in 0..C-1.
    sample_bg: sample 1 is class 0 everywhere.  absent: class C - 2 occurs nowhere.  saturated: logits uniform in
    [-30, 30], a quarter of them exactly -30 or +30."""
    g = gen(seed)
    z = 2.0 * torch.randn((B, vol, C), generator=g, dtype=F32)
    y = torch.randint(0, C, (B, vol), generator=g).to(F32)
    if kind == "sample_bg":
        y[1] = 0.0
    elif kind == "absent":
        y[y == float(C - 2)] = float(C - 1)
    elif kind == "saturated":
        z = 60.0 * torch.rand((B, vol, C), generator=g, dtype=F32) - 30.0
        pin = torch.rand((B, vol, C), generator=g) < 0.25
        z[pin] = torch.sign(z[pin]) * 30.0
    else:
        assert kind == "plain", kind
    return z, y


LADDER = (1, 7, 255, 256, 257, 1023, 1024, 1025, 2048, 3 * 1024 + 1)
LADDER_SHAPES = tuple((n,) for n in LADDER) + ((3, 5, 7), (2, 1024), (4, 3, 3, 3, 3))
# f32 numbers throughout, so that torch (which works on the Python doubles) and the kernel (which gets the f32 row) start
# from the same values; beta1 > 0.5 keeps torch's lerp on the formula the kernel quotes
ADAM_GROUPS = tuple(dict(lr=f32_of(lr), betas=(f32_of(b1), f32_of(b2)), eps=f32_of(eps), weight_decay=f32_of(wd))
                    for lr, b1, b2, eps, wd in ((1e-3, 0.9, 0.999, 1e-8, 0.01), (5e-3, 0.8, 0.99, 1e-6, 0.1),
                                                (2e-2, 0.95, 0.9995, 1e-8, 0.0), (3e-4, 0.85, 0.98, 1e-7, 0.3),
                                                (1e-2, 0.9, 0.95, 1e-5, 0.05), (7e-3, 0.75, 0.999, 1e-8, 1.0),
                                                (1e-1, 0.99, 0.9999, 1e-3, 0.02), (4e-3, 0.6, 0.9, 1e-8, 0.5)))
ADAM_STEPS = 3
ADAM_NO_GRAD, ADAM_ZERO_GRAD = 3, 8                     # ladder indices: a tensor that never steps, an all-zero gradient


def adam_case(shapes=LADDER_SHAPES, seed=11, steps=ADAM_STEPS, no_grad=ADAM_NO_GRAD, zero_grad=ADAM_ZERO_GRAD, group_of=None):
    """Start values and per-step gradients (f32 CPU tensors): tensor i belongs to group i % 8 unless ``group_of`` says
    otherwise; gradients grow with the step and differ in scale per tensor."""
    g = gen(seed)
    n = len(shapes)
    group_of = [i % len(ADAM_GROUPS) for i in range(n)] if group_of is None else list(group_of)
    p0 = [torch.randn(s, generator=g, dtype=F32) for s in shapes]
    grads = []
    for step in range(steps):
        row = []
        for i, s in enumerate(shapes):
            gr = torch.randn(s, generator=g, dtype=F32) * (1.0 + step) * (10.0 ** ((i % 5) - 2))
            row.append(None if i == no_grad else torch.zeros(s, dtype=F32) if i == zero_grad else gr)
        grads.append(row)
    return dict(shapes=list(shapes), group_of=group_of, p0=p0, grads=grads, no_grad=no_grad)


def adam_reference(case, steps=None):
    """[step][tensor] AdamState after each step (None for the tensor without gradient)."""
    states = [None if i == case["no_grad"] else AdamState(p) for i, p in enumerate(case["p0"])]
    out = []
    for step, row in enumerate(case["grads"][:steps]):
        hyper = [adam_hyper_row(step=step + 1, **grp) for grp in ADAM_GROUPS]
        states = [None if st is None else adamw_ref64(st, gr, hyper[gi]) for st, gr, gi in zip(states, row, case["group_of"])]
        out.append(states)
    return out


MANY_SIZES = tuple({383: 1025, 384: 3 * 1024 + 1, 399: 257}.get(i, i % 5 + 1) for i in range(400))


def adam_many_case():
    """400 tensors (more than the 384 gradient pointers of one launch): groups are contiguous runs of 50, so that a
    torch-style optimizer lists the tensors in this order."""
    return adam_case(tuple((n,) for n in MANY_SIZES), seed=12, steps=2, no_grad=-1, zero_grad=-1,
                     group_of=[i // 50 for i in range(400)])


EMA_TAUS = (0.0, 0.5, 0.996, 1.0)


def ema_case(seed=13):
    g = gen(seed)
    teachers = [torch.randn(s, generator=g, dtype=F32) for s in LADDER_SHAPES]
    students = [torch.randn(s, generator=g, dtype=F32) * 3.0 for s in LADDER_SHAPES]
    return teachers, students


SEG_VALUES = (-1.0, 0.0, 0.5, 1.0, 2.0)


def seg_case(B, vol, C, seed):
    """(logits [B, C, vol] f32 drawn from five values with every 7th voxel constant over the channels, target [B, vol] f32:
    labels in -1..C+1 with every 11th voxel holding a non-integer)."""
    g = gen(seed)
    vals = torch.tensor(SEG_VALUES, dtype=F32)
    z = vals[torch.randint(0, len(vals), (B, C, vol), generator=g)]
    flat = torch.arange(B * vol).reshape(B, vol)
    same = (flat % 7 == 3).unsqueeze(1).expand(B, C, vol)
    z = torch.where(same, z[:, :1].expand(B, C, vol), z)
    y = torch.randint(-1, C + 2, (B, vol), generator=g).to(F32)
    y[flat % 11 == 5] += 0.5
    return z.contiguous(), y
