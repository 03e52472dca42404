"""Float64 references of the prompt-path and row-reduction kernels (test helper, not a test module).

Every function is plain float64 torch on the CPU, written from the formulas of include/mivp.h and the reference lines it
cites (relative_positional_encoding.py:99-142, swin_block.py:187-225); nothing here shares code with the kernels.  bf16 is
emulated only at the rounding points the kernels document: the LayerNorm output that feeds the to_k / to_v GEMM, and the
stored ``kp`` / ``vp`` / ``qa`` / ``ka`` / ``wg_a`` / ``wg_n``.

Scaling conventions (taken from the callers, swin_ops.swin_block_forward / swin_block_backward):

* ``kp`` and ``ka`` are stored multiplied by log2(e) (the attention kernels keep logits in log2 units); the factor is the f32
  constant ``LOG2E`` below, as the kernels multiply in f32.  ``vp`` carries no factor.
* ``dkp`` handed to mivp_prompt_kv_bwd is the window-summed ``dkp_part`` of the attention backward: the gradient with respect
  to the UN-scaled prompt keys K = LN(prompt) Wk^T, not to the stored ``kp``.  ``wg_a`` is its head-merged bf16 relayout, with
  no factor either.
* ``dka`` handed to mivp_relbias_grad is the window-summed ``dka_part``: dS^T qa with dS taken with respect to the natural-log
  logit, i.e. the gradient with respect to ``ka / log2(e)``.  The table gradients are therefore the plain adjoint of the
  selection ``tables -> ka / log2(e)``.

Reused: tests/exact_ref.py (draws, located comparison) and attn_ref.PAD_BIAS."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_ref import PAD_BIAS  # noqa: E402,F401  (bf16 value of -30000 log2 e)
from exact_ref import assert_equal_located, draw, gen, ulp_distance  # noqa: E402,F401

F64 = torch.float64
LOG2E = float(np.float32(math.log2(math.e)))          # the f32 constant the kernels multiply with
U32 = 2.0 ** -24                                      # unit roundoff of f32


def round_up(v, m):
    return (v + m - 1) // m * m


def f32_of(x):
    """The f32 value a C float parameter receives."""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------
# bf16 rounding and the interval rule
# ---------------------------------------------------------------------------------------------
def bf16_rne(x):
    """Round-to-nearest-even of float64 values to bf16 (8 significant bits), done in float64 in ONE rounding (going through
    f32 first would round twice).  Normal range only, which is all the tests use."""
    x = x.to(F64)
    _, e = torch.frexp(x)                              # x = m 2^e, 0.5 <= |m| < 1
    q = torch.ldexp(torch.ones_like(x), e - 8)         # spacing of bf16 numbers in x's binade
    return torch.round(x / q) * q                      # torch.round: half to even


def assert_rounds_from_interval(got, ref, b, what=""):
    """Every stored bf16 element is the rounding of SOME value in [ref - b, ref + b]: rounding is monotone, so that is
    bf16(ref - b) <= got <= bf16(ref + b).  Bit-equal to bf16(ref) wherever the interval holds no rounding boundary, one
    neighbour where it does."""
    g = got.detach().to(F64).cpu()
    assert g.shape == ref.shape == b.shape, (what, tuple(g.shape), tuple(ref.shape), tuple(b.shape))
    assert bool(torch.isfinite(ref).all()) and bool((b >= 0).all()), what
    lo, hi = bf16_rne(ref - b), bf16_rne(ref + b)
    bad = ~((g >= lo) & (g <= hi))                     # NaN in got fails both compares
    if bool(bad.any()):
        idx = [tuple(int(i) for i in row) for row in torch.nonzero(bad)[:10]]
        lines = [f"{what}: {int(bad.sum())} of {g.numel()} stored values are not the bf16 rounding of a value within the "
                 f"derived bound of the float64 reference (shape {tuple(g.shape)})"]
        lines += [f"  {i}: got {float(g[i])!r}, reference {float(ref[i])!r} +- {float(b[i]):.3e}" for i in idx]
        msg = "\n".join(lines)
        print(msg)
        raise AssertionError(msg)


# ---------------------------------------------------------------------------------------------
# row reductions
# ---------------------------------------------------------------------------------------------
def reduce_rows_int(x):
    """int64 column sums of an integer-valued [n, rows] float64 matrix and the sums of absolute values (every partial sum
    of any summation order is bounded by the latter)."""
    xi = x.to(torch.int64)
    assert bool((xi.to(F64) == x).all())
    return xi.sum(0), xi.abs().sum(0)


def reduce_rows_bound(x):
    """(float64 column sums, bound): any f32 summation tree of n terms errs by at most (n - 1) u sum |x|."""
    n = x.shape[0]
    return x.to(F64).sum(0), max(n - 1, 0) * U32 * x.to(F64).abs().sum(0)


# ---------------------------------------------------------------------------------------------
# token scores (relative_positional_encoding.py:128-138)
# ---------------------------------------------------------------------------------------------
def token_scores(W, E, scale):
    """ts[h][t] = scale * sum_k W[h][k] E[t][k]   (W [heads, e], E [np, e])."""
    return scale * (W @ E.t())


def token_scores_grads(dts, W, E, scale):
    """Hand-written adjoints of ``token_scores``: dW = scale dts E, dE = scale dts^T W."""
    return scale * (dts @ E), scale * (dts.t() @ W)


def token_scores_bounds(dts, W, E, scale):
    """Per-element bounds of the f32 kernels against float64: (terms) u scale sum |a||b| with e terms in the forward sum,
    np terms in dW and heads terms in dE."""
    heads, e = W.shape
    n_p = E.shape[0]
    s = abs(scale)
    b_ts = e * U32 * s * (W.abs() @ E.abs().t())
    if dts is None:
        return b_ts, None, None
    return b_ts, n_p * U32 * s * (dts.abs() @ E.abs()), heads * U32 * s * (dts.abs().t() @ W.abs())


# ---------------------------------------------------------------------------------------------
# relative-position bias (relative_positional_encoding.py:99-142)
# ---------------------------------------------------------------------------------------------
def slot_coords(window):
    """[Nq, 3] int64: (i0, i1, i2) of window slot n = (i0 w1 + i1) w2 + i2."""
    w0, w1, w2 = window
    n = torch.arange(w0 * w1 * w2)
    return torch.stack([n // (w1 * w2), (n // w2) % w1, n % w2], 1)


def relbias_full(t_h, t_w, t_d, ts, window):
    """bias [heads, Nq, Nq + Np]: T_h[k0 - i0 + w0 - 1] + T_w[k1 - i1 + w1 - 1] + T_d[k2 - i2 + w2 - 1] for window keys (the
    tables carry scale / 3 already), ts[h][t] for prompt key t in every query row."""
    w0, w1, w2 = window
    c = slot_coords(window)
    i, k = c[:, None, :], c[None, :, :]
    content = t_h[:, k[..., 0] - i[..., 0] + w0 - 1] + t_w[:, k[..., 1] - i[..., 1] + w1 - 1] \
        + t_d[:, k[..., 2] - i[..., 2] + w2 - 1]
    if ts is None or ts.shape[1] == 0:
        return content
    Nq = c.shape[0]
    return torch.cat([content, ts[:, None, :].expand(-1, Nq, -1)], 2)


def aug_dims(window, n_prompt):
    w0, w1, w2 = window
    Nq = w0 * w1 * w2
    Nqp = round_up(Nq, 16)
    Npp = round_up(n_prompt, 16)
    aug = w0 + w1 + w2 - 1
    return dict(Nq=Nq, Nqp=Nqp, Np=n_prompt, Npp=Npp, Nkp=round_up(Nqp + Npp, 32), aug=aug, augp=round_up(aug, 4))


def relbias_qa(window, n_prompt=0):
    """qa [Nqp, augp]: onehot(i0) | onehot(i1) | onehot(i2) without its last entry; rows >= Nq and columns >= aug zero."""
    w0, w1, w2 = window
    d = aug_dims(window, n_prompt)
    c = slot_coords(window)
    qa = torch.zeros((d["Nqp"], d["augp"]), dtype=F64)
    n = torch.arange(d["Nq"])
    qa[n, c[:, 0]] = 1.0
    qa[n, w0 + c[:, 1]] = 1.0
    keep = c[:, 2] < w2 - 1
    qa[n[keep], w0 + w1 + c[keep, 2]] = 1.0
    return qa


def relbias_ka_terms(t_h, t_w, t_d, window):
    """The window rows of ka in natural units, [heads, Nq, aug], and the sum of the absolute values of the table operands
    of each entry (for the rounding bound).  The one-hot of i2 lacks its last entry, so the i2 = w2 - 1 term T_d[k2] is folded
    into the i0 columns (whose one-hot always holds a one) and subtracted from the i2 columns:
      a <  w0        : T_h[k0 - a + w0 - 1] + T_d[k2]
      a <  w0 + w1   : T_w[k1 - (a - w0) + w1 - 1]
      a <  aug       : T_d[k2 - (a - w0 - w1) + w2 - 1] - T_d[k2]"""
    w0, w1, w2 = window
    c = slot_coords(window)
    k0, k1, k2 = c[:, 0], c[:, 1], c[:, 2]
    fold = t_d[:, k2]                                                     # [heads, Nq]: query i2 = w2 - 1 -> index k2
    a0, a1, a2 = torch.arange(w0), torch.arange(w1), torch.arange(w2 - 1)
    th = t_h[:, k0[:, None] - a0[None] + w0 - 1]                          # [heads, Nq, w0]
    tw = t_w[:, k1[:, None] - a1[None] + w1 - 1]
    td = t_d[:, k2[:, None] - a2[None] + w2 - 1]
    val = torch.cat([th + fold[..., None], tw, td - fold[..., None]], 2)
    mag = torch.cat([th.abs() + fold.abs()[..., None], tw.abs(), td.abs() + fold.abs()[..., None]], 2)
    return val, mag


def relbias_ka(t_h, t_w, t_d, ts, window, n_prompt):
    """Un-rounded float64 ka [heads, Nkp, augp] in stored (log2) units, and its rounding bound b (same shape): window rows
    2^-22 (|T| + |T'|) of the table operands (two f32 additions / one addition and the multiplication by log2 e, each within
    2^-24 relative, and log2 e < 2); prompt rows ts log2 e in the w0 columns (one multiplication: 2^-24 |value|); rows
    Nq..Nqp-1 and Nqp+Np..Nkp-1 PAD_BIAS in the w0 columns (exact); everything else zero."""
    w0 = window[0]
    d = aug_dims(window, n_prompt)
    heads = t_h.shape[0]
    ka = torch.zeros((heads, d["Nkp"], d["augp"]), dtype=F64)
    b = torch.zeros_like(ka)
    val, mag = relbias_ka_terms(t_h, t_w, t_d, window)
    ka[:, :d["Nq"], :d["aug"]] = val * LOG2E
    b[:, :d["Nq"], :d["aug"]] = 2.0 ** -22 * mag
    ka[:, d["Nq"]:d["Nqp"], :w0] = PAD_BIAS
    ka[:, d["Nqp"] + n_prompt:, :w0] = PAD_BIAS
    if n_prompt:
        ka[:, d["Nqp"]:d["Nqp"] + n_prompt, :w0] = (ts * LOG2E)[:, :, None]
        b[:, d["Nqp"]:d["Nqp"] + n_prompt, :w0] = U32 * (ts * LOG2E).abs()[:, :, None]
    return ka, b


def bias_from_aug(qa, ka, window, n_prompt):
    """bias [heads, Nq, Nq + Np] in natural units rebuilt from augmentation images: <qa[n], ka[h][m]> / log2 e."""
    d = aug_dims(window, n_prompt)
    rows = torch.cat([torch.arange(d["Nq"]), d["Nqp"] + torch.arange(n_prompt)])
    return torch.einsum("na,hma->hnm", qa[:d["Nq"]].to(F64), ka[:, rows].to(F64)) / LOG2E


def relbias_grad(dka, window):
    """Hand-written adjoint of ``tables -> ka / log2 e`` (see the module docstring): dka [heads, Nkp, 32] -> d_th, d_tw, d_td
    [heads, 2 w - 1].  Only rows < Nq and columns < aug take part.  Works in the dtype of ``dka`` (int64 for the exact test)."""
    w0, w1, w2 = window
    c = slot_coords(window)
    heads = dka.shape[0]
    out = [torch.zeros((heads, 2 * w - 1), dtype=dka.dtype) for w in window]
    for m in range(c.shape[0]):
        k0, k1, k2 = (int(v) for v in c[m])
        g = dka[:, m]
        for a in range(w0):
            out[0][:, k0 - a + w0 - 1] += g[:, a]
            out[2][:, k2] += g[:, a]                                      # the folded T_d[k2] of the i0 columns
        for a in range(w1):
            out[1][:, k1 - a + w1 - 1] += g[:, w0 + a]
        for a in range(w2 - 1):
            out[2][:, k2 - a + w2 - 1] += g[:, w0 + w1 + a]
            out[2][:, k2] -= g[:, w0 + w1 + a]
    return out


# ---------------------------------------------------------------------------------------------
# prompt tokens -> LayerNorm -> to_k / to_v (swin_block.py:205-214 applied to the prompt rows)
# ---------------------------------------------------------------------------------------------
def layernorm(x, g, b, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b


def head_split(rows, heads, Npp):
    """[Np, C] head-merged rows (channel = head hd + j) -> [heads, Npp, hd], rows >= Np zero."""
    n_p, Cc = rows.shape
    out = torch.zeros((heads, Npp, Cc // heads), dtype=rows.dtype)
    out[:, :n_p] = rows.reshape(n_p, heads, Cc // heads).permute(1, 0, 2)
    return out


def head_merge(x, n_p):
    """[heads, Npp, hd] -> [Np, C]."""
    heads, _, hd = x.shape
    return x[:, :n_p].permute(1, 0, 2).reshape(n_p, heads * hd)


def prompt_kv(prompt, ln_w, ln_b, wqkv, heads, Npp, eps, y_gemm=None):
    """yln = LayerNorm(prompt) [Np, C]; K = bf16(yln) Wk^T, V = bf16(yln) Wv^T with Wk / Wv = rows C..2C-1 / 2C..3C-1 of wqkv
    (bf16 numbers); returns (yln, kp, vp, bk, bv): kp = K log2 e and vp = V as [heads, Npp, hd] float64 BEFORE the bf16 store,
    and the bounds b = C 2^-24 sum_c |y_c w_c| of an f32 accumulation of C terms (times log2 e for kp).  ``y_gemm``: take the GEMM
    input from these rows (the GPU's own yln) instead of the float64 LayerNorm."""
    Cc = prompt.shape[1]
    yln = layernorm(prompt, ln_w, ln_b, eps)
    y16 = bf16_rne(yln if y_gemm is None else y_gemm.to(F64))
    wk, wv = wqkv[Cc:2 * Cc], wqkv[2 * Cc:3 * Cc]
    kp = head_split(y16 @ wk.t(), heads, Npp) * LOG2E
    vp = head_split(y16 @ wv.t(), heads, Npp)
    bk = head_split(Cc * U32 * (y16.abs() @ wk.abs().t()), heads, Npp) * LOG2E
    bv = head_split(Cc * U32 * (y16.abs() @ wv.abs().t()), heads, Npp)
    return yln, kp, vp, bk, bv


def prompt_kv_smooth(prompt, ln_w, ln_b, wqkv, heads, eps):
    """The differentiable map without rounding points: (K, V) [heads, Np, hd], un-scaled (the backward kernel differentiates
    this: the bf16 rounding of the GEMM input is a straight-through)."""
    n_p, Cc = prompt.shape
    y = layernorm(prompt, ln_w, ln_b, eps)
    wk, wv = wqkv[Cc:2 * Cc], wqkv[2 * Cc:3 * Cc]
    split = lambda r: r.reshape(n_p, heads, Cc // heads).permute(1, 0, 2)
    return split(y @ wk.t()), split(y @ wv.t())


def prompt_kv_bwd(dkp, dvp, prompt, ln_w, ln_b, wqkv, heads, eps, dtype=F64):
    """Autograd of sum(dkp K) + sum(dvp V) through ``prompt_kv_smooth`` in ``dtype`` (float64 = the reference, float32 = the
    same formulas at the kernel's precision, for the run-time error bar).  dkp / dvp [heads, Npp, hd] w.r.t. the un-scaled
    K / V; rows >= Np are ignored.  Returns (dprompt [Np, C], wg_ln [2, Np, C]): per-row dbeta terms (the gradient w.r.t. the
    LayerNorm output), then per-row dgamma terms (that gradient times the normalised row)."""
    n_p, Cc = prompt.shape
    p = prompt.to(dtype).clone().requires_grad_(True)
    g_rows = ln_w.to(dtype).expand(n_p, Cc).clone().requires_grad_(True)      # one copy of gamma / beta per row:
    b_rows = ln_b.to(dtype).expand(n_p, Cc).clone().requires_grad_(True)      # autograd then yields the per-row terms
    K, V = prompt_kv_smooth(p, g_rows, b_rows, wqkv.to(dtype), heads, eps)
    ((dkp[:, :n_p].to(dtype) * K).sum() + (dvp[:, :n_p].to(dtype) * V).sum()).backward()
    return p.grad.detach(), torch.stack([b_rows.grad.detach(), g_rows.grad.detach()])


def rel_max_err(got, ref):
    """max |got - ref| / max |ref| against a float64 reference."""
    r = ref.detach().to(F64).cpu()
    return float((got.detach().to(F64).cpu() - r).abs().max() / r.abs().max())
