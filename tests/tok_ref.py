"""Float64 restatement of the four Swin token kernels and of the weight fragment images (test helper, not a test module).

Written from include/mivp.h (the entries mivp_swin_qkv_fwd, mivp_swin_proj_mlp_fwd, mivp_swin_proj_mlp_bwd, mivp_swin_qkv_bwd,
mivp_pack_weight_frags, mivp_pack_block_weights and the comment "Weight fragment images") and from the block's reference
semantics (oracle/swin_ref.py::swin_block is the statement to compare against).  Plain torch on the CPU; nothing here shares
code with the kernels or walks their tiles.

Every operator takes ``dt`` (the arithmetic type) and ``rnd`` (what a bf16 storage point does):

    dt = float64, rnd = identity    the block's contract in exact arithmetic (the autograd checks, the oracle comparison)
    dt = float64, rnd = bf16_rne    the reference of the GPU tests: float64 sums over the operands the kernels really multiply
    dt = float32, rnd = bf16_f32    an f32 / bf16 emulation from the same formulas (the sensitivity tests; ``err32``)

Storage points (mivp.h, and ``emulate_bf16`` of oracle/swin_ref.py::swin_block): both LayerNorm outputs enter their GEMM as
bf16; t1 lives as bf16 (the second LayerNorm reads the stored values); q, k, v, t1, y, dO, dt1, dn_out, dyw, d_pj, dx are
stored bf16; in mivp_swin_qkv_bwd the q part enters the GEMM as the bf16 value of dq * q_scale ("multiplied by q_scale inside").

Tables: ``tok_src`` / ``tok_dst`` are [P][Nqp] voxel indices shared by the batch.  Source -1 is a zero-padding voxel: it still
goes through attn_norm (so it becomes ln_b) and its residual row is ZERO -- oracle/swin_ref.py:291-296, 307 gathers the
residual ``tok`` from a zero frame; -2 marks slots >= Nq, whose q / k / v rows are zero.  Destination -1 writes nothing.

Bounds (u = 2^-24, the unit roundoff of f32; every bound is per element and none is measured):

  dot     an f32 sum of n products in any order, against float64:  n u sum |a||b|           (Higham, Accuracy and Stability 3.5)
  ln      LayerNorm of a row of C exact values in f32.  With A = mean |x|, r = (var + eps)^-1/2, h = (x - mean) r:
              mean:  |dm| <= C u A =: e_m          (C - 1 additions and a division)
              x - m: |dd| <= e_m + u |d|
              var + eps: relative error <= (C + 4) u + 2 e_m r     (squares, C - 1 additions, division, + eps; sum |d| <= C sigma,
                                                                    sigma r <= 1)
              r:     relative error <= half of that + 4 u           (rsqrtf: 2 ulp allowed)
              y = h w + b:  |dy| <= |w| r e_m + |h w| ((C + 4) u / 2 + e_m r + 7 u) + u |y|      =: width
          The bf16 operand of the following GEMM is the rounding of some value in [y - width, y + width]: bit-equal to bf16(y)
          unless the interval holds a rounding boundary, then it may be the neighbour, a change of at most
          D = bf16(y + width) - bf16(y - width) in that operand, which moves output n by at most sum_c D_c |W[n][c]|.
  out     a stored bf16 output is the rounding of some value within the bound of its float64 reference (``check_interval``).
  err32   LayerNorm backward cancels: no useful a-priori bound.  The same formulas in plain f32 torch give
          err32 = max |f32 - f64| / max |f64|; the kernel's f32 value must stay within (8 err32 + 2^-22) max |f64| of the
          float64 one (8: another summation tree, as in test_hip_prompt_path.py), and the stored bf16 value is the rounding of
          such a value (rule ``out``).  A flat allowance of 2^-9 |f64| for that rounding would be too small: round-to-nearest
          to 8 significant bits errs by up to half an ulp, which is 2^-8 |v| just above a power of two and 2^-9 |v| only just
          below the next; tests/test_tok_ref_host.py shows the plain f32 / bf16 emulation leaving a 2^-9 |f64| allowance."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prompt_ref import LOG2E, U32, bf16_rne, f32_of  # noqa: E402,F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SLACK = 1.0 + 2.0 ** -10                               # second-order terms of the first-order bounds above


def ident(t):
    return t


def bf16_f32(t):
    """The bf16 storage point of the f32 emulation."""
    return t.to(BF16).to(t.dtype)


def desc(B, P, Nq, C, heads, vol, eps=1e-6):
    """The descriptor fields the token kernels read, with the f32 values of the two float fields."""
    return SimpleNamespace(B=B, P=P, Nq=Nq, Nqp=(Nq + 15) // 16 * 16, C=C, heads=heads, vol_in=vol, vol_out=vol,
                           q_scale=f32_of((C // heads) ** -0.5), ln_eps=f32_of(eps))


class Located(AssertionError):
    """A failed check that carries the failing element indices (``where``: list of tuples)."""

    def __init__(self, msg, where):
        super().__init__(msg)
        self.where = where


# ---------------------------------------------------------------------------------------------
# pieces
# ---------------------------------------------------------------------------------------------
def gather_rows(x, table, B):
    """x [B, vol, C], table [P, Nqp] -> rows [B*P, Nqp, C]; negative entries give zero rows."""
    P, Nqp = table.shape
    idx = table.reshape(-1).clamp(min=0)
    rows = x[:, idx]
    rows = torch.where((table.reshape(-1) >= 0)[None, :, None], rows, torch.zeros_like(rows))      # +0 rows, whatever x holds
    return rows.reshape(B * P, Nqp, x.shape[-1])


def scatter_rows(rows, table, B, vol):
    """rows [B*P, Nqp, C] -> [B, vol, C] through an injective table; voxels no entry names are NaN, -1 entries write nothing."""
    P, Nqp = table.shape
    C = rows.shape[-1]
    out = torch.full((B, vol, C), float("nan"), dtype=rows.dtype)
    flat = table.reshape(-1)
    keep = flat >= 0
    out[:, flat[keep]] = rows.reshape(B, P * Nqp, C)[:, keep]
    return out


def layer_norm(x, w, b, eps):
    """LayerNorm over the last axis in x's type -> (y, mean, rstd, xhat)."""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = ((d * d).mean(-1, keepdim=True) + eps) ** -0.5
    h = d * rstd
    return h * w + b, mean, rstd, h


def ln_width(x, w, y, rstd, h):
    """The f32 error interval of a LayerNorm output (module docstring, ``ln``); float64 operands."""
    C = x.shape[-1]
    e_m = C * U32 * x.abs().mean(-1, keepdim=True)
    return SLACK * (w.abs() * rstd * e_m + (h * w).abs() * ((C + 4) * U32 / 2 + e_m * rstd + 7 * U32) + U32 * y.abs())


def ln_operand(y, width):
    """bf16 GEMM operand of a float64 LayerNorm output and the largest change D a neighbour rounding can make to it."""
    return bf16_rne(y), (bf16_rne(y + width) - bf16_rne(y - width)).abs()


def ln_backward(g, w, rstd, h):
    """Gradient of LayerNorm with respect to its input, g = gradient with respect to its output."""
    gw = g * w
    return rstd * (gw - gw.mean(-1, keepdim=True) - h * (gw * h).mean(-1, keepdim=True))


def to_heads(t, heads):
    """[B*P, Nqp, C] -> [B*P, heads, Nqp, hd]"""
    BP, Nqp, C = t.shape
    return t.reshape(BP, Nqp, heads, C // heads).permute(0, 2, 1, 3).contiguous()


def from_heads(t):
    BP, heads, Nqp, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(BP, Nqp, heads * hd)


def _lin(a, W, n_extra, rounded, D=None, extra_mag=None):
    """a W^T with its ``dot`` bound over (K + n_extra) f32 operations; ``D`` as in ``ln``; extra_mag: |addends| after the sum."""
    acc = a @ W.t()
    if not rounded:
        return acc, None
    mag = a.abs() @ W.abs().t()
    if extra_mag is not None:
        mag = mag + extra_mag
    bound = (a.shape[-1] + n_extra) * U32 * mag
    if D is not None:
        bound = bound + D @ W.abs().t()
    return acc, SLACK * bound


# ---------------------------------------------------------------------------------------------
# mivp_swin_qkv_fwd
# ---------------------------------------------------------------------------------------------
def qkv_fwd(d, x, tok_src, ln_w, ln_b, Wq, Wk, Wv, dt=F64, rnd=bf16_rne):
    """q, k, v [B*P][heads][Nqp][hd] (q times q_scale, k times log2 e; values BEFORE the output rounding) and, with rounding
    in float64, their per-element bounds bq / bk / bv, the float64 LayerNorm output ``ln`` and its interval ``ln_width``."""
    c = lambda t: t.to(dt)
    rounded = rnd is not ident
    rows = gather_rows(c(x), tok_src, d.B)
    y, _, rstd, h = layer_norm(rows, c(ln_w), c(ln_b), d.ln_eps)
    pad = (tok_src == -2).repeat(d.B, 1)[..., None]                      # slots >= Nq: zero rows, not ln_b
    y = torch.where(pad, torch.zeros_like(y), y)
    D = width = None
    if rounded and dt == F64:
        width = torch.where(pad, torch.zeros_like(y), ln_width(rows, c(ln_w), y, rstd, h))
        a, D = ln_operand(y, width)
    else:
        a = rnd(y)
    out = SimpleNamespace(ln=y, ln_width=width)
    for name, W, sc in (("q", Wq, d.q_scale), ("k", Wk, LOG2E), ("v", Wv, 1.0)):
        acc, b = _lin(a, c(W), 0, rounded and dt == F64, D)
        setattr(out, name, to_heads(acc * sc, d.heads))
        if b is not None:                                               # the closing multiplication rounds once more
            b = b * abs(sc) + (U32 * (acc * sc).abs() if sc != 1.0 else 0.0)
            setattr(out, "b" + name, to_heads(b, d.heads))
    return out


# ---------------------------------------------------------------------------------------------
# mivp_swin_proj_mlp_fwd
# ---------------------------------------------------------------------------------------------
def proj_mlp_fwd(d, o, x, tok_src, tok_dst, Wp, bp, ln_w, ln_b, Wm, bm, keep=None, scale=1.0, t1_stored=None, dt=F64,
                 rnd=bf16_rne):
    """t1 [B*P][Nqp][C] = (o Wp^T + bp) * keep * scale + shortcut and y [B][vol][C] (NaN where no destination names a voxel),
    both BEFORE their output rounding, with bounds b_t1 / b_y (y-shaped) in float64.  The residual of a -1 source is zero
    (oracle/swin_ref.py:291-296, 307: ``tok`` is gathered from a zero-padded frame).  ``keep`` [B*P][Nqp][C] in {0, 1} and
    ``scale`` = the f32 dropout scale.  ``t1_stored``: the bf16 values the second LayerNorm reads when they are known (the
    GPU's own t1 output), else rnd(t1)."""
    c = lambda t: t.to(dt)
    rounded = rnd is not ident and dt == F64
    short = gather_rows(c(x), tok_src, d.B)
    km = None if keep is None else c(keep) * scale
    pj_mag = None
    acc, _ = _lin(c(o), c(Wp), 0, False)
    pj = acc + c(bp)
    if km is not None:
        pj = pj * km
    t1 = pj + short
    out = SimpleNamespace(t1=t1)
    if rounded:
        pj_mag = c(o).abs() @ c(Wp).abs().t() + c(bp).abs()
        if km is not None:
            pj_mag = pj_mag * km
        out.b_t1 = SLACK * (d.C + 3) * U32 * (pj_mag + short.abs())
    t1s = rnd(t1) if t1_stored is None else c(t1_stored)
    n, _, rstd, h = layer_norm(t1s, c(ln_w), c(ln_b), d.ln_eps)
    D = None
    if rounded:
        a, D = ln_operand(n, ln_width(t1s, c(ln_w), n, rstd, h))
    else:
        a = rnd(n)
    acc2, b2 = _lin(a, c(Wm), 2, rounded, D, extra_mag=(t1s.abs() + c(bm).abs()) if rounded else None)
    t2 = acc2 + t1s + c(bm)
    out.t2 = t2
    out.y = scatter_rows(t2, tok_dst, d.B, d.vol_out)
    if rounded:
        out.b_y = scatter_rows(b2, tok_dst, d.B, d.vol_out)
    return out


# ---------------------------------------------------------------------------------------------
# mivp_swin_proj_mlp_bwd
# ---------------------------------------------------------------------------------------------
def proj_mlp_bwd(d, dy, tok_dst, t1, ln_w, Wm, Wp, keep=None, scale=1.0, operand_stored=None, dt=F64, rnd=bf16_rne):
    """dyw (dy in window order, zero rows where cropped), dn_out = dyw Wm (gradient w.r.t. the mlp_norm output),
    dt1 = dyw + LNbwd(dn_out; t1), d_pj = dt1 * keep * scale, dO = rnd(d_pj) Wp; all [B*P][Nqp][C], before their output
    rounding.  ``operand_stored``: the bf16 values the dO GEMM multiplies when they are known (the GPU's own dt1 / d_pj)."""
    c = lambda t: t.to(dt)
    rounded = rnd is not ident and dt == F64
    dyw = gather_rows(c(dy), tok_dst, d.B)
    dn, b_dn = _lin(dyw, c(Wm).t(), 0, rounded)
    _, _, rstd, h = layer_norm(c(t1), c(ln_w), torch.zeros_like(c(ln_w)), d.ln_eps)
    dt1 = dyw + ln_backward(dn, c(ln_w), rstd, h)
    d_pj = dt1 if keep is None else dt1 * (c(keep) * scale)
    a = rnd(d_pj) if operand_stored is None else c(operand_stored)
    dO, b_dO = _lin(a, c(Wp).t(), 0, rounded)
    return SimpleNamespace(dyw=dyw, dn_out=dn, b_dn=b_dn, dt1=dt1, d_pj=d_pj, dO=dO, b_dO=b_dO)


# ---------------------------------------------------------------------------------------------
# mivp_swin_qkv_bwd
# ---------------------------------------------------------------------------------------------
def qkv_bwd(d, dq, dk, dv, x, tok_src, ln_w, Wq, Wk, Wv, dt1, dt=F64, rnd=bf16_rne):
    """dn_out [B*P][Nqp][C] = rnd(dq q_scale) Wq + dk Wk + dv Wv (dq w.r.t. the stored, pre-scaled q; dk w.r.t. the un-scaled k),
    dx_rows = dt1 + LNbwd(dn_out; gathered x) and dx [B][vol][C] = dx_rows scattered through tok_src: rows with a negative
    source write nothing and voxels no source names stay untouched (NaN here), as the kernel headers say ("zero-pad /
    padding-slot tokens have no voxel to write"); the scatter is a plain store, so it is only defined for distinct sources."""
    c = lambda t: t.to(dt)
    rounded = rnd is not ident and dt == F64
    if rnd is ident:
        gq = from_heads(c(dq)) * d.q_scale
    else:                                                                 # one f32 product, then bf16: as the kernels form it
        gq = (from_heads(dq.to(F32)) * d.q_scale).to(BF16).to(dt)
    g = torch.cat([gq, from_heads(c(dk)), from_heads(c(dv))], -1)
    W = torch.cat([c(Wq), c(Wk), c(Wv)], 0)                               # [3C][C]
    dn, b_dn = _lin(g, W.t(), 0, rounded)
    rows = gather_rows(c(x), tok_src, d.B)
    _, _, rstd, h = layer_norm(rows, c(ln_w), torch.zeros_like(c(ln_w)), d.ln_eps)
    dx_rows = c(dt1) + ln_backward(dn, c(ln_w), rstd, h)
    return SimpleNamespace(dn_out=dn, b_dn=b_dn, dx_rows=dx_rows, dx=scatter_rows(dx_rows, tok_src, d.B, d.vol_in))


# ---------------------------------------------------------------------------------------------
# weight fragment images
# ---------------------------------------------------------------------------------------------
def frag_image(W, k_steps, paired):
    """[ceil(rows / 16)][k_steps][64][8] image of a row-major [rows][cols] matrix, zero padded (mivp.h): lane 16 g + r of (nt, s)
    holds W[16 nt + r][32 s + 8 g + e], or, paired, W[..][32 s + 4 g + e] (e < 4) | W[..][32 s + 16 + 4 g + e - 4].  A GATHER:
    every image element looks its source up."""
    rows, cols = W.shape
    nt = torch.arange((rows + 15) // 16).view(-1, 1, 1, 1)
    s = torch.arange(k_steps).view(1, -1, 1, 1)
    lane = torch.arange(64).view(1, 1, -1, 1)
    e = torch.arange(8).view(1, 1, 1, -1)
    r, g = lane % 16, lane // 16
    row = (16 * nt + r).expand(-1, k_steps, -1, 8)
    col = (32 * s + (16 * (e // 4) + 4 * g + e % 4 if paired else 8 * g + e)).expand(nt.shape[0], -1, -1, -1)
    ok = (row < rows) & (col < cols)
    img = W[row.clamp(max=rows - 1), col.clamp(max=cols - 1)]
    return torch.where(ok, img, torch.zeros_like(img))


def _scatter_image(W, k_steps, paired):
    """The same image as a SCATTER: every matrix element computes where it goes (independent of ``frag_image``)."""
    rows, cols = W.shape
    img = torch.zeros(((rows + 15) // 16) * k_steps * 512, dtype=W.dtype)
    row = torch.arange(rows).view(-1, 1).expand(rows, cols)
    col = torch.arange(cols).view(1, -1).expand(rows, cols)
    nt, r, s, k = row // 16, row % 16, col // 32, col % 32
    if paired:
        g, e = (k % 16) // 4, 4 * (k // 16) + k % 4
    else:
        g, e = k // 8, k % 8
    img[((nt * k_steps + s) * 64 + 16 * g + r) * 8 + e] = W
    return img


def block_images(C, wq, wk, wv, wproj, wmlp, with_natural):
    """Every image mivp_pack_block_weights builds from the f32 masters, as flat bf16 tensors keyed by its output names."""
    ks, ct = (C + 31) // 32, (C + 15) // 16
    b = lambda t: t.to(F32).to(BF16)
    wqkv = torch.cat([b(wq), b(wk), b(wv)], 0)
    both = lambda W: torch.cat([_scatter_image(W, ks, True)] + ([_scatter_image(W, ks, False)] if with_natural else []))
    return dict(wqkv_rm=wqkv.reshape(-1), wqkv_f=_scatter_image(wqkv, ks, False), wproj_f=_scatter_image(b(wproj), ks, False),
                wmlp_f=both(b(wmlp)), wqkv_t=_scatter_image(wqkv.t().contiguous(), (3 * 16 * ct + 31) // 32, False),
                wmlp_t=_scatter_image(b(wmlp).t().contiguous(), ks, False), wproj_t=both(b(wproj).t().contiguous()))


# ---------------------------------------------------------------------------------------------
# assertion helpers shared by the CPU sensitivity tests and the GPU tests
# ---------------------------------------------------------------------------------------------
def _fail(what, bad, g, ref, bound, kind):
    where = [tuple(int(i) for i in row) for row in torch.nonzero(bad)]
    lines = [f"{what}: {len(where)} of {g.numel()} elements {kind} (shape {tuple(g.shape)})"]
    lines += [f"  {i}: got {float(g[i])!r}, float64 {float(ref[i])!r}, bound {float(bound[i]):.3e}" for i in where[:8]]
    raise Located("\n".join(lines), where)


def check_interval(got, ref, bound, what):
    """Stored bf16 ``got`` is the rounding of some value in [ref - bound, ref + bound], element by element (elements whose
    reference is NaN are not compared: the caller checks those exactly).  Returns an observation, the worst distance of the
    reference from the stored value's rounding cell in units of the bound (0 = every element is the rounding of the reference)."""
    g = got.detach().to(F64).cpu()
    assert g.shape == ref.shape == bound.shape, (what, tuple(g.shape), tuple(ref.shape), tuple(bound.shape))
    use = ~torch.isnan(ref)
    r, b = torch.where(use, ref, torch.zeros_like(ref)), torch.where(use, bound, torch.zeros_like(bound))
    lo, hi = bf16_rne(r - b), bf16_rne(r + b)
    bad = use & ~((g >= lo) & (g <= hi))
    if bool(bad.any()):
        _fail(what, bad, g, ref, bound, "are not the bf16 rounding of a value within the derived bound of the float64 reference")
    # observation for the [margin] lines: how far the reference lies outside the rounding cell of the stored value, in bounds
    _, e = torch.frexp(g)
    half_ulp = torch.ldexp(torch.ones_like(g), e - 9)
    ratio = torch.where(use & (b > 0), ((g - r).abs() - half_ulp).clamp(min=0) / b.clamp(min=1e-300), torch.zeros_like(r))
    return float(ratio.max()) if ratio.numel() else 0.0


def check_err32(got, ref64, ref32, what):
    """The ``err32`` bar of the module docstring, per element; NaN references are not compared.  Returns (worst ratio, err32)."""
    assert ref64.shape == ref32.shape, what
    use = ~torch.isnan(ref64)
    r = torch.where(use, ref64, torch.zeros_like(ref64))
    top = float(r.abs().max())
    err32 = float(torch.where(use, (ref32.to(F64) - r).abs(), torch.zeros_like(r)).max()) / top
    bar = torch.full_like(r, (8 * err32 + 2.0 ** -22) * top)
    return check_interval(got, ref64, bar, what + f" (err32 {err32:.2e})"), err32


def check_bits_equal(a, b, what):
    """Bit equality of two bf16 tensors, located."""
    ia, ib = a.detach().cpu().contiguous().view(torch.int16), b.detach().cpu().contiguous().view(torch.int16)
    assert ia.shape == ib.shape, what
    bad = ia != ib
    if bool(bad.any()):
        where = [tuple(int(i) for i in row) for row in torch.nonzero(bad)]
        raise Located(f"{what}: {len(where)} of {ia.numel()} elements differ in their bits; first at {where[0]}: "
                      f"{float(a.cpu()[where[0]])!r} != {float(b.cpu()[where[0]])!r}", where)


def check_qkv_structure(d, tok_src, q, k, v, what):
    """The exact properties of mivp_swin_qkv_fwd's outputs [B*P][heads][Nqp][hd] (bf16): slots >= Nq (-2) are +0 bits, and all
    rows with source -1 carry identical bits (each is ln_b through the same weights)."""
    src = tok_src.repeat(d.B, 1)                                          # [B*P][Nqp]
    for name, t in (("q", q), ("k", k), ("v", v)):
        rows = t.detach().cpu().contiguous().view(torch.int16).permute(0, 2, 1, 3).reshape(-1, d.C)      # [T][C] bit rows
        pad = (src.reshape(-1) == -2)
        bad = pad[:, None] & (rows != 0)
        if bool(bad.any()):
            where = [tuple(int(i) for i in row) for row in torch.nonzero(bad)]
            raise Located(f"{what} {name}: padding slot rows must be +0 bits; first wrong (token row, channel) {where[0]}", where)
        zp = torch.nonzero(src.reshape(-1) == -1).reshape(-1)
        if zp.numel() > 1:
            bad = rows[zp] != rows[zp[0]][None]
            if bool(bad.any()):
                where = [(int(zp[i]), int(j)) for i, j in torch.nonzero(bad)]
                raise Located(f"{what} {name}: rows with source -1 must carry identical bits; first (token row, channel) "
                              f"{where[0]} differs from token row {int(zp[0])}", where)


def stored(t):
    """The bf16 values a kernel (or the emulation) stores, from f32 / f64 values."""
    return t.to(F32).to(BF16)


# ---------------------------------------------------------------------------------------------
# synthetic tables and operands (shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------------------------
def make_tables(P, Nq, vol, seed, dup=True):
    """tok_src / tok_dst [P][Nqp] int64 over ``vol`` >= P Nq + 8 voxels: distinct random sources and destinations, so some voxels
    are read by nobody and some written by nobody; slots >= Nq are (-2, -1); a few content slots are zero padding (-1, -1) in
    the first, a middle and the last position; a few more are cropped (source kept, destination -1); with ``dup`` the slot
    before the last of the last window gathers the voxel of slot 1 of window 0 (needs P >= 2; destinations stay injective)."""
    Nqp = (Nq + 15) // 16 * 16
    assert Nq < Nqp and vol >= P * Nq + 8 and Nq >= 8
    g = torch.Generator().manual_seed(seed)
    src = torch.full((P, Nqp), -2, dtype=torch.int64)
    dst = torch.full((P, Nqp), -1, dtype=torch.int64)
    src[:, :Nq] = torch.randperm(vol, generator=g)[:P * Nq].view(P, Nq)
    dst[:, :Nq] = torch.randperm(vol, generator=g)[:P * Nq].view(P, Nq)
    for pw, s in ((0, 0), (P // 2, Nq // 2), (P - 1, Nq - 1), (0, Nq - 1)):
        src[pw, s], dst[pw, s] = -1, -1
    for pw, s in ((0, 3), (P - 1, 2)):
        dst[pw, s] = -1
    if dup:
        assert P >= 2
        src[P - 1, Nq - 2] = src[0, 1]
    return src, dst


def randn_bf16(g, *shape, scale=1.0, shift=0.0):
    """bf16-representable float64 values (what a bf16 device tensor holds)."""
    return (torch.randn(shape, generator=g, dtype=F32) * scale + shift).to(BF16).to(F64)


def block_operands(d, seed):
    """Random operands of one block at descriptor ``d``: weights bf16-representable, LayerNorm parameters and biases f32."""
    g = torch.Generator().manual_seed(seed)
    C = d.C
    f = lambda *s, scale=1.0, shift=0.0: (torch.randn(s, generator=g, dtype=F32) * scale + shift).to(F64)
    T = d.B * d.P
    o = SimpleNamespace(
        x=randn_bf16(g, d.B, d.vol_in, C, scale=0.8, shift=0.1), ln1_w=f(C, scale=0.2, shift=1.0), ln1_b=f(C, scale=0.1),
        ln2_w=f(C, scale=0.2, shift=1.0), ln2_b=f(C, scale=0.1), bp=f(C, scale=0.1), bm=f(C, scale=0.1),
        Wq=randn_bf16(g, C, C, scale=C ** -0.5), Wk=randn_bf16(g, C, C, scale=C ** -0.5), Wv=randn_bf16(g, C, C, scale=C ** -0.5),
        Wp=randn_bf16(g, C, C, scale=C ** -0.5), Wm=randn_bf16(g, C, C, scale=C ** -0.5),
        o=randn_bf16(g, T, d.Nqp, C, scale=0.7), t1=randn_bf16(g, T, d.Nqp, C, scale=0.9, shift=0.05),
        dy=randn_bf16(g, d.B, d.vol_out, C, scale=0.5), dt1=randn_bf16(g, T, d.Nqp, C, scale=0.5),
        dq=randn_bf16(g, T, d.heads, d.Nqp, C // d.heads, scale=0.5), dk=randn_bf16(g, T, d.heads, d.Nqp, C // d.heads, scale=0.5),
        dv=randn_bf16(g, T, d.heads, d.Nqp, C // d.heads, scale=0.5))
    return o
