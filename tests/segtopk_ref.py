"""Float64 reference of the top-k (hard-voxel) cross-entropy of the fused segmentation loss (test helper, not a test
module).  Written from the definition in DESIGN 4.34 / include/mivp.h; nothing here shares code with the package (the region
term and the bars come from tests/segloss_ref.py and tests/loss_optim_ref.py, test helpers as well).

Over the VALID voxels of the whole batch (label an integer in [0, C) and not the ignore label):
  u_v   = w[y_v] (1 - p_y)^gamma (-log p_y)             N = their number, k = max(1, floor(top_k N)) in float64
  tau   = the k-th largest u, n_gt = #{u > tau}, n_eq = #{u == tau}, rho = (k - n_gt) / n_eq
  s_v   = 1 (u_v > tau) | rho (u_v == tau) | 0 (u_v < tau, or invalid)                      sum s_v = k
  voxel = (sum_{u > tau} u + (k - n_gt) tau) / k,   d voxel = (1 / k) sum_v s_v d u_v       (N == 0: 0 and 0)
  loss  = lambda_region region + lambda_voxel voxel

A kernel computes u in f32, so which voxels it selects can only be compared with the float64 selection on inputs where no
u lies closer to tau than the kernel's error: ``assert_case_is_decidable`` is that condition on the INPUTS, with
band = LOSS_MARGIN x E_u and E_u = max |u32 - u64| of the float32 run of these formulas (floored at 2^-24 max u).  A kernel
whose keys are within band / 2 of u64 then provably selects what the reference selects (ties by construction included:
bit-equal operands give bit-equal keys)."""
import itertools
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segloss_ref as R  # noqa: E402
from loss_optim_ref import (LOSS_L2_BAR, LOSS_MARGIN, LOSS_VALUE_BAR, U32, assert_within_located, gen,  # noqa: E402,F401
                            loss_grad_bar, loss_yardstick, rel_l2)

F64, F32 = torch.float64, torch.float32
KEY_MARGIN = LOSS_MARGIN          # band = KEY_MARGIN x E_u; the measured kernel / E_u ratios are in DESIGN 5.6


def opts(top_k, **kw):
    return dict(R.opts(**kw), top_k=top_k)


def opts_name(o):
    return R.opts_name(o) + f" top_k {o['top_k']:.6g}"


def base_opts(o):
    return {k: v for k, v in o.items() if k != "top_k"}


# ---------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------
def u_of(logits, target, o, dtype=F64, requires_grad=False):
    """(z, u [B, vol] in ``dtype`` (0 at an invalid voxel), valid [B, vol] bool)."""
    C = logits.shape[-1]
    z = logits.detach().to(dtype).clone().requires_grad_(requires_grad)
    valid = R.valid_mask(target, C, o["ignore_index"])
    idx = R.class_index(target, C)
    hot = F.one_hot(idx, C).to(dtype)
    logp = F.log_softmax(z, -1)
    f = -(logp * hot).sum(-1)
    if o["focal_gamma"] != 0:
        f = f * (logp.exp() * (1.0 - hot)).sum(-1) ** o["focal_gamma"]
    w = torch.ones(C, dtype=dtype) if o["class_weights"] is None else torch.tensor(o["class_weights"], dtype=F64).to(dtype)
    return z, w[idx] * f * valid.to(dtype), valid


def k_of(top_k, N):
    return max(1, math.floor(top_k * N))


class Select:
    """N, k, tau, n_gt, n_eq, rho and the weights s [B, vol] of a u map.  The keyword arguments plant the errors the host
    test must see: ``k_shift`` (k off by one), ``ties_all`` (every tied voxel selected: >= instead of the shared weight),
    ``per_sample`` (tau of each sample on its own), ``count_invalid`` (N = every voxel)."""

    def __init__(self, u, valid, top_k, k_shift=0, ties_all=False, per_sample=False, count_invalid=False):
        if per_sample:
            rows = [Select(u[b:b + 1], valid[b:b + 1], top_k) for b in range(u.shape[0])]
            self.N, self.k = sum(r.N for r in rows), sum(r.k for r in rows if r.N)
            self.s = torch.cat([r.s for r in rows])
            self.tau = None
            return
        uv = u.detach()[valid]
        self.N = int(valid.numel() if count_invalid else uv.numel())
        self.k = min(max(1, k_of(top_k, self.N) + k_shift), max(1, uv.numel()))
        self.s = torch.zeros_like(u.detach())
        if uv.numel() == 0:
            self.tau, self.n_gt, self.n_eq, self.rho = 0.0, 0, 0, 0.0
            return
        self.tau = torch.sort(uv, descending=True).values[self.k - 1]
        gt, eq = (u.detach() > self.tau) & valid, (u.detach() == self.tau) & valid
        self.n_gt, self.n_eq = int(gt.sum()), int(eq.sum())
        self.rho = 1.0 if ties_all else (self.k - self.n_gt) / self.n_eq
        self.s[gt] = 1.0
        self.s[eq] = self.rho


def voxel_value(u, sel):
    """(sum_{u > tau} u + (k - n_gt) tau) / k as sum s u / k (the same number: s = rho on the tie group)."""
    return (sel.s.to(u.dtype) * u).sum() / sel.k if sel.N else 0.0 * u.sum()


def topk_loss(logits, target, o, dtype=F64, sel=None, norm=None):
    """(loss, d loss / d logits, Select) by autograd in ``dtype``.  ``sel``: the selection to use (the float32 yardstick run
    takes the float64 one: on a decidable case it is its own); ``norm``: the normaliser instead of k."""
    bo = base_opts(o)
    l_r, g_r = R.seg_loss_ref64(logits, target, dict(bo, lambda_voxel=0.0), dtype)
    z, u, valid = u_of(logits, target, o, dtype, requires_grad=True)
    if sel is None:
        sel = Select(u, valid, o["top_k"])
    vox = voxel_value(u, sel)
    if norm is not None:
        vox = vox * sel.k / norm
    vox.backward()
    return l_r + o["lambda_voxel"] * vox.detach().to(F64), g_r + o["lambda_voxel"] * z.grad.detach(), sel


def topk_grad_closed(logits, target, o, sel=None, norm=None):
    """The gradient in closed form (float64): the region part of segloss_ref.seg_grad_closed plus
    lambda_voxel s_v w_y / k f'(p_y) p_y (delta_cy - p_c),  f'(p) p = gamma p (1 - p)^(gamma - 1) log p - (1 - p)^gamma."""
    bo = base_opts(o)
    z = logits.to(F64)
    C = z.shape[-1]
    g = R.seg_grad_closed(z, target, dict(bo, lambda_voxel=0.0))
    _, u, valid = u_of(logits, target, o)
    if sel is None:
        sel = Select(u, valid, o["top_k"])
    if sel.N == 0:
        return g
    idx = R.class_index(target, C)
    hot = F.one_hot(idx, C).to(F64)
    p = z.softmax(-1)
    w = torch.ones(C, dtype=F64) if o["class_weights"] is None else torch.tensor(o["class_weights"], dtype=F64)
    py, om = (p * hot).sum(-1), (p * (1.0 - hot)).sum(-1)
    logp = (F.log_softmax(z, -1) * hot).sum(-1)
    gam = float(o["focal_gamma"])
    fp = -torch.ones_like(py) if gam == 0 else gam * py * om ** (gam - 1.0) * logp - om ** gam
    coef = o["lambda_voxel"] * sel.s * w[idx] * valid.to(F64) / (sel.k if norm is None else norm) * fp
    return g + coef.unsqueeze(-1) * (hot - p)


def e_u(logits, target, o):
    """(E_u, u64, valid): what the float32 run of the formulas loses on u, floored at one unit roundoff of max u."""
    _, u64, valid = u_of(logits, target, o)
    _, u32, _ = u_of(logits, target, o, F32)
    if not bool(valid.any()):
        return 0.0, u64, valid
    return max(float((u32.to(F64) - u64)[valid].abs().max()), U32 * float(u64[valid].max())), u64, valid


def band(logits, target, o):
    return KEY_MARGIN * e_u(logits, target, o)[0]


def assert_case_is_decidable(logits, target, o, what=""):
    """No float64 u of a valid voxel lies within ``band`` of tau unless it EQUALS tau (a tie by construction)."""
    e, u64, valid = e_u(logits, target, o)
    sel = Select(u64, valid, o["top_k"])
    if sel.N == 0:
        return sel
    d = (u64[valid] - sel.tau).abs()
    near = (d <= KEY_MARGIN * e) & (d > 0)
    assert not bool(near.any()), (f"{what}: {int(near.sum())} voxels lie within {KEY_MARGIN * e:.3e} of tau {float(sel.tau)!r} "
                                  f"(nearest {float(d[d > 0].min()):.3e}): pick another seed or fraction")
    return sel


class TopkRef:
    """Value, gradient, selection and bars of a case (``zero``: the reference gradient is zero everywhere)."""

    def __init__(self, z, y, o):
        self.l64, self.g64, self.sel = topk_loss(z, y, o)
        self.l32, self.g32, _ = topk_loss(z, y, o, F32, sel=self.sel)
        self.zero = not bool(self.g64.abs().max() > 0)
        if not self.zero:
            self.e32, self.scale = loss_yardstick(self.g32, self.g64)
            self.bar_abs, self.bar_norm = loss_grad_bar(self.g32, self.g64)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
FIVE = ((0.5, -1.25, 2.0, 0.0, -0.75, 1.5, -2.5, 0.25), (-1.0, 0.75, 0.5, 2.25, -0.5, 0.0, 1.0, -1.75),
        (2.5, 2.0, -1.5, 0.25, 1.25, -0.25, 0.75, 0.5), (0.0, 0.125, -0.375, 1.0, 3.0, -2.0, 0.5, -1.0),
        (-2.0, 1.0, 0.25, -0.5, 0.0, 2.75, -1.25, 1.5))


def topk_inputs(B, vol, C, seed, kind, ignore_index=None):
    """(logits [B, vol, C] f32, target [B, vol] f32).  Kinds of segloss_ref.seg_inputs (plain, ignored, all_ignored,
    bad_labels, low_classes), and
    zeros:  every logit 0 (every u equal under unit weights)
    five:   every voxel's logits are one of 5 fixed vectors: at most 5 C distinct u, bit-exact ties
    wide:   a quarter of the voxels have one logit at +30 or -30, the rest 2 randn: u from ~1e-13 to 60"""
    if kind in ("zeros", "five", "wide"):
        z, y = R.seg_inputs(B, vol, C, seed, "plain" if ignore_index is None else "ignored", ignore_index)
        g = gen(seed + 7)
        if kind == "zeros":
            z = torch.zeros_like(z)
        elif kind == "five":
            z = torch.tensor(FIVE, dtype=F32)[:, :C][torch.randint(0, 5, (B, vol), generator=g)]
        else:
            hit = torch.rand((B, vol), generator=g) < 0.25
            col = torch.randint(0, C, (B, vol), generator=g)
            sign = torch.where(torch.rand((B, vol), generator=g) < 0.5, -30.0, 30.0)
            z = torch.where(hit.unsqueeze(-1) & (torch.arange(C) == col.unsqueeze(-1)), sign.unsqueeze(-1), z)
        return z.contiguous(), y
    return R.seg_inputs(B, vol, C, seed, kind, ignore_index)


def frac_for(k, N):
    """A fraction with max(1, floor(frac N)) == k."""
    f = 1.0 if k >= N else (k + 0.5) / N
    assert k_of(f, N) == k, (k, N, f)
    return f


def tie_fracs(z, y, o):
    """Fractions that put k at 1, at N, and on the first, an inner and the last element of the largest tie group of u64
    that has at least three members (on a case without one: 1, N and three values between)."""
    _, u64, valid = u_of(z, y, dict(o, top_k=1.0))
    uv = torch.sort(u64[valid], descending=True).values
    N = uv.numel()
    if N == 0:
        return [0.5]
    ks = {1, N}
    vals, counts = torch.unique_consecutive(uv, return_counts=True)
    if int(counts.max()) >= 3:
        i = int(counts.argmax())
        first = int(counts[:i].sum()) + 1
        ks |= {first, first + int(counts[i]) // 2, first + int(counts[i]) - 1}
    else:
        ks |= {max(1, N // 10), max(1, N // 2), max(1, (9 * N) // 10)}
    return [frac_for(k, N) for k in sorted(ks)]


W8 = R.WEIGHTS8

# (name, B, vol, C, kind, seed, options without top_k, fractions: a tuple, or "ties" for tie_fracs)
_SELECT = [
    ("one voxel", 1, 1, 2, "plain", 1, dict(), (1.0, 0.3)),
    ("one voxel of two", 2, 1, 2, "ignored", 24, dict(ignore_index=255), (0.5, 1.0)),
    ("one voxel per sample", 3, 1, 3, "plain", 2, dict(class_weights=W8[:3]), "ties"),
    ("scalar B1", 1, 63, 4, "plain", 33, dict(focal_gamma=2.0), "ties"),
    ("scalar B2 ignore", 2, 63, 5, "ignored", 4, dict(class_weights=W8[:5], ignore_index=255), "ties"),
    ("scalar B3 batch", 3, 63, 6, "ignored", 5, dict(batch=True, ignore_index=-1, include_background=False), "ties"),
    ("vec B1", 1, 64, 7, "plain", 6, dict(class_weights=W8[:7], focal_gamma=1.0), "ties"),
    ("vec B2", 2, 64, 8, "ignored", 7, dict(ignore_index=255, alpha=0.3, beta=0.7), "ties"),
    ("vec B3", 3, 64, 2, "plain", 8, dict(class_weights=W8[:2]), "ties"),
    ("rows B1", 1, 2053, 2, "ignored", 9, dict(class_weights=W8[:2], ignore_index=255), (0.1,)),
    ("rows B2", 2, 2053, 3, "plain", 10, dict(focal_gamma=2.0), (0.1, 0.5)),
    ("rows B3", 3, 2053, 2, "ignored", 11, dict(ignore_index=255, batch=True), "ties"),
    ("flush 2x20^3", 2, 8000, 2, "ignored", 12, dict(class_weights=W8[:2], ignore_index=255), (0.1, 0.01)),
    ("all zero logits", 2, 64, 3, "zeros", 13, dict(), (0.01, 0.3, 0.5, 1.0)),
    ("all zero logits, scalar", 3, 63, 2, "zeros", 14, dict(ignore_index=255), (0.3, 1.0)),
    ("five vectors", 2, 336, 3, "five", 15, dict(), "ties"),
    ("five vectors, weights, scalar", 3, 315, 4, "five", 16, dict(class_weights=W8[:4], ignore_index=255, focal_gamma=2.0), "ties"),
    ("wide exponents", 2, 2053, 3, "wide", 17, dict(), (0.02, 0.2, 0.6)),
    ("wide exponents, focal", 2, 336, 4, "wide", 18, dict(focal_gamma=2.0, class_weights=W8[:4]), (0.05, 0.3)),
    ("zero-weight class", 3, 315, 3, "plain", 19, dict(class_weights=(1.0, 0.0, 2.0)), (0.1, 0.5, 1.0)),
    ("all ignored", 3, 64, 3, "all_ignored", 20, dict(ignore_index=255, class_weights=(1.0, 0.0, 2.0)), (0.1,)),
    ("all ignored, voxel alone", 2, 63, 2, "all_ignored", 21, dict(ignore_index=-1, lambda_region=0.0), (0.5,)),
    ("bad labels", 3, 315, 4, "bad_labels", 22, dict(class_weights=W8[:4]), (0.1, 0.5)),
    ("bad labels, ignore", 2, 64, 4, "bad_labels", 23, dict(ignore_index=2, focal_gamma=2.0), "ties"),
]


def select_cases():
    """[(name, z, y, options with top_k)] of tests/test_hip_segtopk.py's exact-select test, one entry per fraction."""
    out = []
    for name, B, vol, C, kind, seed, kw, fracs in _SELECT:
        z, y = topk_inputs(B, vol, C, seed, kind, kw.get("ignore_index"))
        o0 = opts(1.0, **kw)
        for f in (tie_fracs(z, y, o0) if fracs == "ties" else fracs):
            out.append((f"{name} (B {B} vol {vol} C {C})", z, y, dict(o0, top_k=f)))
    return out


PRODUCT_SHAPE = (3, 63, 3)
PRODUCT_TOP_K = 0.3


def product_cases():
    """{per-sample, batch} x {weights, none} x {focal 0, 2} x {ignore, none} at one small shape."""
    B, vol, C = PRODUCT_SHAPE
    out = []
    for batch, wts, gam, ig in itertools.product((False, True), (True, False), (0.0, 2.0), (255, None)):
        z, y = topk_inputs(B, vol, C, 31, "plain" if ig is None else "ignored", ig)
        o = opts(PRODUCT_TOP_K, alpha=0.3, beta=0.7, batch=batch, focal_gamma=gam, class_weights=W8[:C] if wts else None,
                 ignore_index=ig)
        out.append((opts_name(o), z, y, o))
    return out


def forms_case(vol):
    o = opts(0.25, alpha=0.3, beta=0.7, focal_gamma=2.0, class_weights=(0.5, 2.0, 1.0), ignore_index=255)
    z, y = topk_inputs(3, vol, 3, 41 + vol, "ignored", 255)
    return z, y, o


FORMS_VOLS = (315, 336)
GRAPH_DIMS = (6, 7, 8)


def graph_cases():
    """Two batch contents of one shape for the recorded call: different N, k and tau."""
    o = opts(0.2, class_weights=(0.5, 2.0, 1.0), ignore_index=255, focal_gamma=2.0)
    return o, [topk_inputs(2, 336, 3, 51, "ignored", 255), topk_inputs(2, 336, 3, 52, "wide", None)]


def all_gpu_cases():
    """Every (name, z, y, o) whose selection the GPU file compares with the reference."""
    out = select_cases() + product_cases()
    out += [(f"forms {v}",) + forms_case(v) for v in FORMS_VOLS]
    o, batches = graph_cases()
    out += [(f"graph {i}", z, y, o) for i, (z, y) in enumerate(batches)]
    return out
