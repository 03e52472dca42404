"""Float64 restatement of the encoder's down-sampling path (test helper, not a test module).

Written from include/mivp.h (mivp_patch_embed, mivp_patch_im2col, mivp_patch_merge_fwd, mivp_patch_merge_bwd, mivp_ln_wgrad) and
the kernel headers of csrc/norm_embed.hip, csrc/merge_up.hip and csrc/wgrad.hip; oracle/swin_ref.py::patch_merge,
torch.nn.functional.conv3d and F.layer_norm are the statements to compare against (tests/test_merge_ref_host.py).  Plain torch
on the CPU.  The gather is index arithmetic per (token, part), not the strided slices of the oracle, and nothing here walks a
kernel's tiles.

``dt`` / ``rnd`` as in tests/tok_ref.py:

    dt = float64, rnd = identity    the contract in exact arithmetic (the autograd and oracle comparisons)
    dt = float64, rnd = bf16_rne    the reference of the GPU tests: float64 sums over the operands the kernels really multiply
    dt = float32, rnd = bf16_f32    an f32 / bf16 emulation from the same formulas (``err32``)

Layouts.  x [B, H, W, D, C]; tokens t = ((b oh + h) ow + w) od + d over the output grid; rows [T, kC] with k = 8 (merge_last) or
4 parts of C channels in the order of c_off8 / c_off4: (h, w, d) = 000 100 010 001 110 101 011 111, or (h, w) = 00 10 01 11.  An
odd axis gets ONE zero plane at the front, also D when D is not merged, so part p of token (h, w, d) reads voxel
(2h + p_h - H%2, 2w + p_w - W%2, 2d + p_d - D%2) (d - D%2 when D is not merged) and is +0 where a coordinate is -1.  Every voxel
is the source of exactly one (token, part): the backward scatter is a bijection onto x (``merge_gather`` asserts it).

Storage points.  The LayerNorm output enters the reduction GEMM as bf16; y, dx, wg_dn, wg_x and n_out are stored bf16.
mivp_patch_merge_bwd takes the row sums of the LayerNorm backward from the handed-in forward output:

    dYn = dy W                                 (gradient w.r.t. the LayerNorm output; = wg_dn)
    m1  = sum_n dy_n wgam_n / kC               wgam = W gamma
    m2  = sum_n dy_n (yfwd_n - wbet_n) / kC    wbet = W beta;  yfwd is the STORED bf16 forward output, so m2 carries its rounding
    dx  = rstd (dYn gamma - m1 - xhat m2)      scattered;  with the exact y = W (gamma xhat + beta) this is LayerNorm backward

In the f32 emulation the row statistics of the backward are the documented one-pass form: mean = sum / kC,
var = max(sumsq / kC - mean^2, 0).

Bounds (u = 2^-24; per element; none measured; ``dot``, ``ln``, ``out`` and ``err32`` are the rules of tests/tok_ref.py):

  y        kC u sum |a||W| + sum D |W|: a = the bf16 LayerNorm output, D the change a neighbour rounding of that operand can make
  wg_dn    Cout u sum |dy||W| (a linear bf16 GEMM: bit-equal to float64 for integer operands under conditions (a) and (b))
  wg_x     exact: the gathered rows
  dx       err32
  conv     exact for integer operands; otherwise Cin*8 + 1 terms
  n_out    ``ln`` interval (``ln_width``); a -1 source is a zero row: xhat = 0 and n = beta exactly; a -2 source gives +0
  dbeta    sum_t dn: exact for integer dn while sum |dn| < 2^24
  dgamma   sum_t dn_t xhat_t.  The kernel forms xhat in f32: by ``ln`` with w = 1, b = 0 its error is
               dxh = r e_m + |xhat| ((C + 4) u / 2 + e_m r + 7 u) + u |xhat|
           and the T products and their sum are a ``dot`` of T terms:  T u sum |dn||xhat| + sum |dn| dxh."""
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as Fnn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tok_ref import (BF16, F32, F64, SLACK, U32, Located, _lin, bf16_f32, check_bits_equal, check_err32,  # noqa: E402,F401
                     check_interval, gather_rows, ident, layer_norm, ln_backward, ln_operand, ln_width, make_tables,
                     randn_bf16, stored)
from prompt_ref import bf16_rne, f32_of  # noqa: E402,F401
from exact_ref import assert_equal_located, assert_exact_inputs, draw, first_exact, gen  # noqa: E402,F401

LN_EPS = f32_of(1e-6)                                                    # MivpMergeDesc.ln_eps as ops.merge_desc fills it
ORDER8 = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
ORDER4 = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0))


# ---------------------------------------------------------------------------------------------
# geometry and dispatch, restated from the launchers
# ---------------------------------------------------------------------------------------------
def merge_odims(dims, merge_last):
    return tuple((n + (n & 1)) // 2 if (a < 2 or merge_last) else n + (n & 1) for a, n in enumerate(dims))


def merge_tokens(B, dims, merge_last):
    o = merge_odims(dims, merge_last)
    return B * o[0] * o[1] * o[2]


def merge_fwd_arm(B, dims, C, Cout, merge_last):
    """(KS, ny, per_y) of mivp_patch_merge_fwd; KS None where the entry refuses."""
    kC = (8 if merge_last else 4) * C
    KS = (kC + 31) // 32
    gx = (merge_tokens(B, dims, merge_last) + 63) // 64
    n_tiles = (Cout + 15) // 16
    lds = 64 * (64 * KS + 16) + 2048 * KS + 64 * 12 + 256 * KS
    resident = 256 * min(8, 160 * 1024 // lds)
    ny = max(1, min(n_tiles, resident // gx))
    while n_tiles % ny:
        ny -= 1
    return (KS if KS in (1, 2, 4, 6, 8, 12, 24) else None), ny, n_tiles // ny


def merge_bwd_arm(B, dims, C, Cout, merge_last):
    """(NS, ny, per_y) of mivp_patch_merge_bwd; NS None where the entry refuses."""
    kC = (8 if merge_last else 4) * C
    NS = (Cout + 31) // 32
    gx = (merge_tokens(B, dims, merge_last) + 63) // 64
    n_ct = (kC + 15) // 16
    ny = max(1, min((1024 + gx - 1) // gx, n_ct // 3))
    return (NS if NS in (1, 2, 3, 4, 6, 12) else None), ny, (n_ct + ny - 1) // ny


def embed_arm(Cin, mode):
    return f"{'cin1' if Cin == 1 else 'cinN'}_mode{mode}"


def smallest_nblk(C):
    """The smallest nblk with (nblk * 256) % (C / 8) == 0."""
    G = C // 8
    n = 1
    while (n * 256) % G:
        n += 1
    return n


# ---------------------------------------------------------------------------------------------
# gather / scatter
# ---------------------------------------------------------------------------------------------
def merge_index(B, dims, merge_last, tokens=None):
    """inv [T', k] int64: the flat voxel index ((b H + h) W + w) D + d that (token, part) reads, -1 in the front pad.  ``tokens``
    (int64 indices) restricts the rows; None = all T tokens, and then the map is asserted to name every voxel exactly once."""
    H, W, D = dims
    oh, ow, od = merge_odims(dims, merge_last)
    T = B * oh * ow * od
    t = torch.arange(T) if tokens is None else tokens.to(torch.int64)
    b, rem = t // (oh * ow * od), t % (oh * ow * od)
    o = (rem // (ow * od), (rem // od) % ow, rem % od)
    cols = []
    for off in (ORDER8 if merge_last else ORDER4):
        xc = []
        for a in range(3):
            merged = a < 2 or merge_last
            xc.append((2 * o[a] + off[a] if merged else o[a]) - (dims[a] & 1))
        ok = (xc[0] >= 0) & (xc[1] >= 0) & (xc[2] >= 0)
        assert bool((xc[0] < H).all() and (xc[1] < W).all() and (xc[2] < D).all())
        vox = ((b * H + xc[0]) * W + xc[1]) * D + xc[2]
        cols.append(torch.where(ok, vox, torch.full_like(vox, -1)))
    inv = torch.stack(cols, 1)
    if tokens is None:
        named = inv[inv >= 0]
        assert named.numel() == B * H * W * D and torch.equal(named.sort().values, torch.arange(B * H * W * D))
    return inv


def merge_gather(x, merge_last, tokens=None):
    """x [B, H, W, D, C] -> (rows [T', kC] with +0 pad parts, inv [T', k])."""
    B, H, W, D, C = x.shape
    inv = merge_index(B, (H, W, D), merge_last, tokens)
    flat = x.reshape(-1, C)
    rows = flat[inv.clamp(min=0)]                                        # [T', k, C]
    rows = torch.where((inv >= 0)[..., None], rows, torch.zeros_like(rows))
    return rows.reshape(inv.shape[0], -1), inv


def merge_scatter(rows, inv, shape):
    """rows [T, kC] -> [B, H, W, D, C] through ``inv``; pad parts write nothing, voxels nobody names stay NaN."""
    C = shape[-1]
    out = torch.full((int(torch.tensor(shape[:-1]).prod()), C), float("nan"), dtype=rows.dtype)
    parts = rows.reshape(inv.shape[0], inv.shape[1], C)
    keep = inv >= 0
    out[inv[keep]] = parts[keep]
    return out.reshape(shape)


# ---------------------------------------------------------------------------------------------
# mivp_patch_merge_fwd
# ---------------------------------------------------------------------------------------------
def merge_fwd(x, ln_w, ln_b, W, merge_last, eps=LN_EPS, dt=F64, rnd=bf16_rne, tokens=None):
    """y [T', Cout] BEFORE its output rounding, ``bound`` (float64 with rounding only), the gathered rows, the LayerNorm output
    ``ln`` and the row statistics."""
    c = lambda t: t.to(dt)
    rounded = rnd is not ident and dt == F64
    rows, inv = merge_gather(c(x), merge_last, tokens)
    n, mean, rstd, h = layer_norm(rows, c(ln_w), c(ln_b), eps)
    D = None
    if rounded:
        a, D = ln_operand(n, ln_width(rows, c(ln_w), n, rstd, h))
    else:
        a = rnd(n)
    y, bound = _lin(a, c(W), 0, rounded, D)
    return SimpleNamespace(y=y, bound=bound, rows=rows, inv=inv, ln=n, mean=mean, rstd=rstd, xhat=h)


# ---------------------------------------------------------------------------------------------
# mivp_patch_merge_bwd
# ---------------------------------------------------------------------------------------------
def merge_bwd(dy, x, yfwd, ln_w, wgam, wbet, W, merge_last, eps=LN_EPS, dt=F64, rnd=bf16_rne):
    """dy, yfwd [T, Cout]; wgam, wbet [Cout]; W [Cout, kC] -> dx [B, H, W, D, C], wg_dn (= dYn) with its ``dot`` bound b_dn and
    wg_x (the gathered rows), all before their output rounding."""
    c = lambda t: t.to(dt)
    rounded = rnd is not ident and dt == F64
    rows, inv = merge_gather(c(x), merge_last)
    kC = rows.shape[-1]
    dYn, b_dn = _lin(c(dy), c(W).t(), 0, rounded)
    m1 = (c(dy) * c(wgam)).sum(-1, keepdim=True) / kC
    m2 = (c(dy) * (c(yfwd) - c(wbet))).sum(-1, keepdim=True) / kC
    if dt == F64:
        mean = rows.mean(-1, keepdim=True)
        var = ((rows - mean) ** 2).mean(-1, keepdim=True)
    else:                                                                 # the kernel's one-pass statistics
        mean = rows.sum(-1, keepdim=True) / kC
        var = ((rows * rows).sum(-1, keepdim=True) / kC - mean * mean).clamp(min=0)
    rstd = (var + eps) ** -0.5
    dx_rows = rstd * (dYn * c(ln_w) - m1 - (rows - mean) * rstd * m2)
    return SimpleNamespace(dx=merge_scatter(dx_rows, inv, tuple(x.shape)), dx_rows=dx_rows, wg_dn=dYn, b_dn=b_dn, wg_x=rows,
                           inv=inv, m1=m1, m2=m2, rstd=rstd)


def merge_wvec(W, ln_w, ln_b):
    """wgam, wbet as f32-valued float64 (the two weight-only vectors the backward is handed), formed in float64."""
    return (W @ ln_w).to(F32).to(F64), (W @ ln_b).to(F32).to(F64)


# ---------------------------------------------------------------------------------------------
# mivp_patch_embed, mivp_patch_im2col
# ---------------------------------------------------------------------------------------------
def embed_conv(x, w, bias):
    """x [B, Cin, H, W, D], w [C, Cin, 2, 2, 2], bias [C] (float64) -> (conv + bias, its absolute-value bound), channels last
    [B, H/2, W/2, D/2, C]."""
    ref = Fnn.conv3d(x, w, bias, stride=2)
    bound = Fnn.conv3d(x.abs(), w.abs(), bias.abs(), stride=2)
    return ref.permute(0, 2, 3, 4, 1).contiguous(), bound.permute(0, 2, 3, 4, 1).contiguous()


def embed_stats(conv, bound):
    """Per-channel (sum | sum of squares) [2C] of a channels-last conv output, and the same over the absolute-value bound."""
    C = conv.shape[-1]
    v, b = conv.reshape(-1, C), bound.reshape(-1, C)
    return torch.cat([v.sum(0), (v * v).sum(0)]), torch.cat([b.sum(0), (b * b).sum(0)])


def im2col(x):
    """x [B, Cin, H, W, D] -> [B (H/2)(W/2)(D/2), Cin*8], column ci*8 + a*4 + b*2 + c = x[b, ci, 2h + a, 2w + b, 2d + c]."""
    B, Cin, H, W, D = x.shape
    p = x.reshape(B, Cin, H // 2, 2, W // 2, 2, D // 2, 2).permute(0, 2, 4, 6, 1, 3, 5, 7)
    return p.reshape(B * (H // 2) * (W // 2) * (D // 2), Cin * 8)


# ---------------------------------------------------------------------------------------------
# mivp_ln_wgrad
# ---------------------------------------------------------------------------------------------
def ln_wgrad(x, tok_src, dn, gamma, beta, eps, B=1, dt=F64, rnd=bf16_rne):
    """x [T, C] (tok_src None) or [B, vol, C] gathered through tok_src [P, Nqp]; dn [T, C] -> n [T, C] before its output rounding,
    its ``ln`` interval ``width``, dbeta, dgamma and the bound b_dgamma (module docstring).  Source -1: a zero row (n = beta, the
    row contributes to both sums); source -2: n = +0 and no contribution (dn of such a row is never read)."""
    c = lambda t: t.to(dt)
    C = x.shape[-1]
    if tok_src is None:
        rows = c(x).reshape(-1, C)
        pad = torch.zeros(rows.shape[0], dtype=torch.bool)
    else:
        rows = gather_rows(c(x), tok_src, B).reshape(-1, C)
        pad = (tok_src == -2).repeat(B, 1).reshape(-1)
    T = rows.shape[0]
    n, _, rstd, h = layer_norm(rows, c(gamma), c(beta), eps)
    live = (~pad)[:, None]
    n = torch.where(live, n, torch.zeros_like(n))
    g = torch.where(live, torch.nan_to_num(c(dn)), torch.zeros_like(n))
    out = SimpleNamespace(n=n, dbeta=g.sum(0), dgamma=(g * h).sum(0), pad=pad, xhat=h)
    if dt == F64:
        out.width = torch.where(live, ln_width(rows, c(gamma), n, rstd, h), torch.zeros_like(n))
        dxh = ln_width(rows, torch.ones_like(c(gamma)), h, rstd, h)
        out.b_dgamma = SLACK * (T * U32 * (g.abs() * h.abs()).sum(0) + (g.abs() * dxh).sum(0))
        out.b_dbeta = g.abs().sum(0)
    return out


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------
def merge_operands(B, dims, C, Cout, merge_last, seed, offset=0.0, zero_token=None):
    """x (bf16 values), LayerNorm parameters (f32 values), W [Cout, kC] (bf16 values), dy [T, Cout] (bf16 values).  ``offset``:
    a per-channel shift of about ``offset`` standard deviations (rows whose mean is far from zero); ``zero_token``: that token's
    whole neighbourhood is +0 (var = 0, rstd = eps^-1/2)."""
    g = torch.Generator().manual_seed(seed)
    kC = (8 if merge_last else 4) * C
    T = merge_tokens(B, dims, merge_last)
    x = torch.randn((B, *dims, C), generator=g, dtype=F32) * 0.8
    if offset:
        x = x + 0.8 * offset * (1.0 + 0.1 * torch.randn((C,), generator=g, dtype=F32))
    x = x.to(BF16).to(F64)
    f = lambda *s, scale=1.0, shift=0.0: (torch.randn(s, generator=g, dtype=F32) * scale + shift).to(F64)
    o = SimpleNamespace(x=x, ln_w=f(kC, scale=0.2, shift=1.0), ln_b=f(kC, scale=0.1), W=randn_bf16(g, Cout, kC, scale=kC ** -0.5),
                        dy=randn_bf16(g, T, Cout, scale=0.5))
    if zero_token is not None:
        inv = merge_index(B, dims, merge_last, torch.tensor([zero_token]))[0]
        o.x.reshape(-1, C)[inv[inv >= 0]] = 0.0
    return o


def plant_twins(x, merge_last, tokens):
    """Copies the gathered row of tokens[0] into the neighbourhoods of the other tokens (in place) so that all of them gather the
    same row; tokens[0] must sit in every front pad the others sit in (token 0 of the grid does).  Returns nothing; the caller
    asserts the rows' equality on the reference."""
    B, H, W, D, C = x.shape
    rows, inv = merge_gather(x, merge_last, torch.tensor(tokens))
    base = rows[0].reshape(-1, C)
    flat = x.reshape(-1, C)
    for i in range(1, len(tokens)):
        for p in range(inv.shape[1]):
            if int(inv[i, p]) >= 0:
                flat[int(inv[i, p])] = base[p]
            else:
                assert not bool(base[p].any()), "the twin sits in a front pad the base token does not"


# ---------------------------------------------------------------------------------------------
# the cases whose assertions are exact (shared with tests/test_merge_ref_host.py, which proves conditions (a) and (b) on them)
# ---------------------------------------------------------------------------------------------
# mivp_patch_embed: (B, Cin, dims, C); B ovol = 1, 105 (no multiple of 256), 2160
EMBED_CASES = [(B, Cin, dims, C) for Cin in (1, 4) for C in (8, 48) for B, dims in ((1, (2, 2, 2)), (1, (6, 10, 14)), (2, (20, 24, 18)))]

# mivp_patch_merge_bwd: (B, dims, C, Cout, merge_last, offset, zero_token)
BWD_CASES = ([(1, (5, 6, 4), 48, co, True, 0.0, None) for co in (16, 64, 96, 128, 192, 384)]              # the NS ladder
             + [(1, (6 + (p >> 2 & 1), 4 + (p >> 1 & 1), 4 + (p & 1)), 48, 96, True, 0.0, None) for p in range(8)]   # parities
             + [(1, (7, 5, 5), 96, 192, False, 0.0, None),                # D odd and not merged: a whole zero plane
                (2, (40, 40, 32), 48, 96, True, 0.0, None),               # 12800 tokens: ny below its cap
                (2, (9, 6, 3), 8, 16, False, 0.0, None),                  # kC = 32: two channel tiles, ny = 1
                (1, (10, 25, 2), 16, 32, True, 0.0, None),                # T = 65: a dead tail of 63 rows
                (1, (6, 5, 4), 48, 96, True, 2.0, None),                  # rows about 2 sigma off zero
                (1, (6, 5, 4), 48, 96, True, 0.0, 7)])                    # one all-zero neighbourhood


def embed_exact(B, Cin, dims, C, seed=0):
    """Integer operands of one mivp_patch_embed case at the densest draw that meets conditions (a) and (b): x, w in -2 .. 2, bias
    and shift in -3 .. 3, scale a power of two.  -> namespace(x, w, bias, scale, shift, conv, sums, y and their bounds)."""
    def make(dens):
        g = gen(1000 * seed + 97 * C + 13 * Cin + B * dims[0] * dims[1] * dims[2])
        x = draw(g, (B, Cin, *dims), range(-2, 3), dens)
        w = draw(g, (C, Cin, 2, 2, 2), range(-2, 3))
        bias, shift = draw(g, (C,), range(-3, 4)), draw(g, (C,), range(-3, 4))
        scale = 2.0 ** draw(g, (C,), (-1, 0, 1))
        conv, bound = embed_conv(x, w, bias)
        sums, b_sums = embed_stats(conv, bound)
        y, b_y = conv * scale + shift, bound * scale + shift.abs()
        p = SimpleNamespace(x=x, w=w, bias=bias, scale=scale, shift=shift, conv=conv, sums=sums, b_sums=b_sums, y=y, b_y=b_y,
                            density=dens)
        return (sums, y), (b_sums, b_y), (False, True), p
    return first_exact(make)


def bwd_exact(B, dims, C, Cout, merge_last, seed=0):
    """Integer dy [T, Cout] and W [Cout, kC] (-2 .. 2) at the densest draw of dy for which wg_dn = dy W meets (a) and (b)."""
    kC = (8 if merge_last else 4) * C
    T = merge_tokens(B, dims, merge_last)

    def make(dens):
        g = gen(1000 * seed + 7 * Cout + kC + T)
        dy = draw(g, (T, Cout), range(-2, 3), dens)
        W = draw(g, (Cout, kC), range(-2, 3))
        p = SimpleNamespace(dy=dy, W=W, wg_dn=dy @ W, b_dn=dy.abs() @ W.abs(), density=dens)
        return p.wg_dn, p.b_dn, True, p
    return first_exact(make)
