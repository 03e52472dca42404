"""Float64 references, launch geometry and f32 restatements of the BatchNorm pieces (csrc/norm_embed.hip: mivp_bn_stats,
mivp_bn_finalize, mivp_affine_act, mivp_bn_bwd_stats, mivp_bn_bwd_apply) and of the point sampling (csrc/proto.hip:
mivp_sample_points_fwd / _bwd) -- test helper, not a test module.

Plain torch on the CPU, written from include/mivp.h and the kernel headers; nothing here imports the package.  The BatchNorm
reference is the formula of training-mode batch normalisation (and float64 autograd through F.batch_norm + F.leaky_relu for
the backward); the sampling reference is F.grid_sample over F.affine_grid of the identity on the cropped float64 volume, the
call the reference project makes, never an interpolation matrix.

Bounds.  u = 2^-24, the unit roundoff of f32.  Every bound counts the f32 roundings of the kernel's own operation sequence,
each relative to the magnitude it rounds (first order; SLACK = 1 + 2^-10 covers the second-order terms); a contracted
multiply-add only removes a rounding.  Where a kernel stores bf16 the bound adds half a bf16 spacing at |ref| + bound
(``with_bf16``).  None is measured.

  bn_stats      part rows summed in float64 by the test against sum x, sum x^2.  x is bf16, so f * f is exact in f32 (16
                significant bits): the only roundings are the additions.  A thread adds ``trips`` terms, then one thread per
                channel adds the ceil(256 / G) owners of its group: the longest chain has k = trips + ceil(256 / G) terms
                (``chain_len``), so |err| <= k u sum |term| per channel.
  bn_finalize   the kernel sums the rows in double: D = (nblk + 4) 2^-53 is its whole relative error on s1 / n, s2 / n and
                mean^2 (``e_mean``, ``e_var``; they enter rstd as e_var / (2 (var + eps))).  On top, the final f32 roundings:
                  rstd   = (float)(1 / sqrt(var + eps))       1:  u |rstd|
                  scale  = w * rstd                            2:  2 u |scale|           (1 u when w is NULL: 1.f * rstd)
                  mean   = (float)mean                         1:  u |mean|
                  shift  = b - (float)mean * scale             (float)mean 1 + scale 2 + product 1 on |mean scale|, the
                                                               subtraction 1 on |b| + |mean scale|:  5 u |mean scale| + u |b|
                  running = (1.f - m) * r + m * (float)v       with A = (1 - m) r, B = m v:  1.f - m, its product and the sum
                                                               on A; (float)v, its product and the sum on B:  3 u (|A| + |B|)
  affine_act    z = x * scale + shift:  e32 = 2 u (|x scale| + |shift|)  (product, sum).  z <= 0 with LeakyReLU stores 0.01f z:
                0.01 e32 + 2 u |0.01 z| (the constant 0.01f is 0.375 u off 0.01, the product) <= 0.03 e32, so e32 covers it.
  gate          the backward kernels recompute z in f32 from scale / shift that are themselves f32 roundings of the
                reference's: the sign of z is decided wherever |z64| > 4 u (|x scale| + |shift|) (``gate_margin``) or
                z64 == 0 exactly with dyadic operands (planted).  Cases assert that no element lies in between.
  bwd sums      S1 = sum gz, gz = dy or fl(0.01f dy) (2 u |gz|):                     (k + 2) u sum |gz|
                S2 = sum gz (x - mu) rs with mu, rs the f32 roundings of the reference's mean, rstd:
                     per term gz 2, x - mu 1, product 1, rs 1, product 1 = 6 u |term|, and u |mu| |gz rs| for mu:
                                                                                     (k + 6) u sum |term| + u sum |mu gz rs|
  bwd dx        sums, scale, mean, rstd reach the kernel as f32 roundings of the reference's (1 u each), inv_n = 1.f / (float)n 1:
                  k2 = S2 inv_n rs          S2 1 + inv_n 1 + product 1 + rs 1 + product 1              5 u |k2|
                  cb = -scale k2            scale 1 + 5 + product 1                                    7 u |cb|
                  cc = scale (mu k2 - S1 inv_n)   mu k2: 1 + 5 + 1 = 7;  S1 inv_n: 1 + 1 + 1 = 3;  the difference 1 on both;
                                            scale 1 + product 1 on both          u |scale| (10 |mu k2| + 6 |S1 / n|)
                  dx = ca gz + cb x + cc    ca gz: scale 1 + gz 2 + product 1 = 4;  cb x: 7 + 1 = 8;  two additions: 2 on all
                  |err| <= u (6 |scale gz| + 10 |cb x| + |scale| (12 |mu k2| + 8 |S1 / n|))
  sampling fwd  out = sum over 8 taps of wt val, wt = a product of three per-axis weights: (3 weight roundings + 2 product
                roundings + 8 accumulations) u sum |wt val| = 13 u grid_sample(|vol|).  The weight roundings are counted
                relative to each weight; tests/test_norm_sample_host.py shows the tabulated weights within one f32 rounding
                of the float64 position over the whole domain.
  sampling bwd  the same chain over the (at most 8) samples that touch a voxel: 13 u (autograd of the same call on |gout|),
                then bf16."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as Fnn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_optim_ref import assert_within_located, f32_of, rel_l2  # noqa: E402,F401
from exact_ref import assert_equal_located  # noqa: E402,F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
SLOPE = 0.01
EPS = f32_of(1e-5)
MOMENTUM = f32_of(0.1)


def bf16_half_spacing(v):
    """Half the spacing of bf16 at |v| (float64 tensor): 2^(e - 8) for 2^e <= |v| < 2^(e + 1), the subnormal spacing below 2^-126."""
    _, e = torch.frexp(v.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 9)


def with_bf16(ref, bound):
    """Bound of a stored bf16 value: the f32 bound plus half a bf16 spacing at |ref| + bound."""
    b = bound * SLACK
    return b + bf16_half_spacing(ref.abs() + b)


def used(got, ref, bound):
    """Largest used fraction of a bound: max |got - ref| / bound over the elements with a positive bound."""
    g, r = got.detach().to(F64).cpu(), ref.to(F64)
    b = bound if isinstance(bound, torch.Tensor) else torch.full_like(r, float(bound))
    ok = b > 0
    return float(((g - r).abs()[ok] / b[ok]).max()) if bool(ok.any()) else 0.0


# ---------------------------------------------------------------------------------------------
# launch geometry, restated from ops._nblk / fixed_group_grid and the kernels' loops
# ---------------------------------------------------------------------------------------------
def group_step(G):
    return G // math.gcd(G, 256)


def group_grid(items, G, cap):
    """Blocks of a fixed-channel-group launch: min(cap, ceil(items / 256)) rounded DOWN to a multiple of G / gcd(G, 256), at least one."""
    step = group_step(G)
    want = max(1, min(cap, (items + 255) // 256))
    return max(step, want // step * step)


def stats_nblk(n_vox, C):
    return group_grid(n_vox * (C // 8), C // 8, 1024)


def apply_grid(n_vox, C):
    return group_grid(n_vox * (C // 8), C // 8, 4096)


def trips(items, nblk):
    return (items + nblk * 256 - 1) // (nblk * 256)


def chain_len(items, nblk, G):
    """Terms of the longest f32 addition chain of a statistics kernel: one thread's trips plus the owners one reducing thread adds."""
    return trips(items, nblk) + (256 + G - 1) // G


def live_blocks(items):
    """Blocks that own at least one item on the first trip; the rows of all others must be exactly 0."""
    return (items + 255) // 256


def path(n_vox, C, nblk, cap):
    """The paths a case reaches, for the test ids and the table of DESIGN 5.14."""
    G, items = C // 8, n_vox * (C // 8)
    tags = [f"G{G}"]
    if 256 % G:
        tags.append("rotating")
    if 2 * C > 256:
        tags.append("multi_o")
    if live_blocks(items) < nblk:
        tags.append("empty_blocks")
    if nblk == cap // group_step(G) * group_step(G):
        tags.append("cap")
    if trips(items, nblk) > 1:
        tags.append(f"trips{trips(items, nblk)}" + ("_tail" if items % (nblk * 256) else ""))
    if items % 256:
        tags.append("ragged")
    return "-".join(tags)


# ---------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def bn_operands(n_vox, C, seed, lrelu=True):
    """x, dy [n_vox, C] (bf16-valued float64), weight / bias [C] (f32-valued), with per-channel offsets and spreads so that mean and
    variance differ from channel to channel (a neighbouring group's constants are wrong constants).  Elements whose LeakyReLU
    gate would be undecided (module docstring, ``gate``) are redrawn; the caller still asserts the condition."""
    g = gen(seed)
    off = torch.randn(C, generator=g, dtype=F32) * 0.7
    spread = 0.5 + torch.rand(C, generator=g, dtype=F32)
    w = (1.0 + 0.3 * torch.randn(C, generator=g, dtype=F32)).to(F64)
    b = (0.3 * torch.randn(C, generator=g, dtype=F32)).to(F64)
    x = (torch.randn((n_vox, C), generator=g, dtype=F32) * spread + off).to(BF16).to(F64)
    dy = torch.randn((n_vox, C), generator=g, dtype=F32).to(BF16).to(F64)
    for fill in (0.75, -1.25, 0.4375, 2.0):
        st = bn_forward(x, w, b)
        bad = gate_undecided(x, st.scale32, st.shift32)
        if not bool(bad.any()):
            break
        x[bad] = fill
    return SimpleNamespace(x=x, dy=dy, w=w, b=b)


def plant_zeros(x, scale, shift, rows=(0, 3)):
    """Dyadic constants that make z exactly zero in every precision: channel 0 gets scale 1, shift 0 and x = 0 in ``rows``;
    channel 1 gets scale 2, shift -2 and x = 1 in ``rows`` (all in place).  Returns the planted (row, channel) pairs."""
    scale[0], shift[0], scale[1], shift[1] = 1.0, 0.0, 2.0, -2.0
    where = []
    for r in rows:
        x[r, 0], x[r, 1] = 0.0, 1.0
        where += [(r, 0), (r, 1)]
    return where


def plant_symmetric_zero_channel(o, rows=(0, 3)):
    """Channel 0 gets mean exactly 0 (second half = minus the first, sums of bf16 values are exact in float64) and bias 0, so
    x = 0 gives z = 0 exactly in every precision.  In place; returns the planted rows."""
    n = o.x.shape[0]
    h = n // 2
    o.x[h:2 * h, 0] = -o.x[:h, 0]
    if n & 1:
        o.x[-1, 0] = 0.0
    o.b[0] = 0.0
    where = []
    for r in rows:
        o.x[r, 0] = o.x[r + h, 0] = 0.0
        where += [r, r + h]
    return where


# ---------------------------------------------------------------------------------------------
# references (float64)
# ---------------------------------------------------------------------------------------------
def bn_sums(x):
    """(sum x | sum x^2) [2C] and the sums of the absolute terms."""
    return torch.cat([x.sum(0), (x * x).sum(0)]), torch.cat([x.abs().sum(0), (x * x).sum(0)])


def r32(t):
    """The f32 rounding of a float64 tensor, as float64."""
    return t.to(F32).to(F64)


def bn_forward(x, w, b, eps=EPS):
    """Training-mode statistics and the per-channel affine in float64, with the f32 roundings the backward kernels are fed."""
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = (var + eps) ** -0.5
    scale = w * rstd
    shift = b - mean * scale
    return SimpleNamespace(n=n, mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, scale32=r32(scale), shift32=r32(shift),
                           mean32=r32(mean), rstd32=r32(rstd))


def gate_margin(x, scale, shift):
    return 4.0 * U32 * ((x * scale).abs() + shift.abs())


def gate_undecided(x, scale, shift):
    """Elements with 0 < |z64| <= the margin: an f32 evaluation of z may land on the other side of the gate."""
    z = x * scale + shift
    return (z != 0) & (z.abs() <= gate_margin(x, scale, shift))


def finalize_ref(part, count, w, b, eps, momentum, rmean, rvar):
    """part [nblk, 2C] (f32-valued float64); w, b, rmean, rvar [C] float64 or None -> the values and bounds of every output."""
    nblk, C = part.shape[0], part.shape[1] // 2
    s1, s2 = part[:, :C].sum(0), part[:, C:].sum(0)
    a1, a2 = part[:, :C].abs().sum(0), part[:, C:].abs().sum(0)
    D = (nblk + 4) * 2.0 ** -53
    mean = s1 / count
    raw = s2 / count - mean * mean
    var = raw.clamp(min=0.0)
    e_mean = D * a1 / count
    e_var = D * (a2 / count + 3 * mean * mean)
    rstd = (var + eps) ** -0.5
    rel = e_var / (2 * (var + eps))
    wv = torch.ones(C, dtype=F64) if w is None else w
    bv = torch.zeros(C, dtype=F64) if b is None else b
    scale = wv * rstd
    shift = bv - mean * scale
    o = SimpleNamespace(mean=mean, raw_var=raw, var=var, rstd=rstd, scale=scale, shift=shift)
    o.b_mean = SLACK * (U32 * mean.abs() + e_mean)
    o.b_rstd = SLACK * rstd * (U32 + rel)
    o.b_scale = SLACK * scale.abs() * ((1 if w is None else 2) * U32 + rel)
    o.b_shift = SLACK * ((5 * U32 + rel) * (mean * scale).abs() + U32 * bv.abs() + e_mean * scale.abs())
    if rmean is not None:
        unbiased = var * count / (count - 1.0) if count > 1.0 else var
        keep = 1.0 - momentum
        o.rmean = keep * rmean + momentum * mean
        o.rvar = keep * rvar + momentum * unbiased
        o.b_rmean = SLACK * (3 * U32 * ((keep * rmean).abs() + (momentum * mean).abs()) + momentum * e_mean)
        o.b_rvar = SLACK * (3 * U32 * ((keep * rvar).abs() + (momentum * unbiased).abs())
                            + momentum * e_var * (count / (count - 1.0) if count > 1.0 else 1.0))
    return o


def affine_ref(x, scale, shift, lrelu):
    """z = x scale + shift (LeakyReLU 0.01) in float64 and its f32 bound e32."""
    z = x * scale + shift
    y = torch.where(z > 0, z, SLOPE * z) if lrelu else z
    return y, 2.0 * U32 * ((x * scale).abs() + shift.abs())


def bn_backward_autograd(x, dy, w, b, lrelu, eps=EPS):
    """dx, dgamma, dbeta by float64 autograd through F.batch_norm(training=True) (+ F.leaky_relu)."""
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = Fnn.batch_norm(xr, None, None, wr, br, True, 0.0, eps)
    if lrelu:
        y = Fnn.leaky_relu(y, SLOPE)
    y.backward(dy)
    return xr.grad, wr.grad, br.grad


def bn_backward_closed(x, dy, w, b, lrelu, eps=EPS, train=True):
    """The header formulas of csrc/norm_embed.hip in float64: dz = dy act'(z) (slope 0.01 where z <= 0), S1 = sum dz,
    S2 = sum dz xhat, dx = scale (dz - S1 / n - xhat S2 / n); the eval form drops both sums from dx.  Also the absolute-value
    quantities of the bounds."""
    st = bn_forward(x, w, b, eps)
    z = x * st.scale + st.shift
    gz = torch.where(z <= 0, SLOPE * dy, dy) if lrelu else dy
    xhat = (x - st.mean) * st.rstd
    S1, S2 = gz.sum(0), (gz * xhat).sum(0)
    n = st.n
    dx = st.scale * (gz - S1 / n - xhat * S2 / n) if train else st.scale * gz
    return SimpleNamespace(st=st, z=z, gz=gz, xhat=xhat, S1=S1, S2=S2, dx=dx)


def bwd_sums_bounds(c, k):
    """Bounds of (S1 | S2) for a chain of k terms (module docstring, ``bwd sums``)."""
    b1 = (k + 2) * U32 * c.gz.abs().sum(0)
    b2 = (k + 6) * U32 * (c.gz * c.xhat).abs().sum(0) + U32 * (c.st.mean.abs() * (c.gz * c.st.rstd).abs()).sum(0)
    return SLACK * torch.cat([b1, b2])


def bwd_dx_bound(c, x, train=True):
    """The f32 bound of dx before its bf16 rounding (module docstring, ``bwd dx``)."""
    sc, n = c.st.scale.abs(), c.st.n
    if not train:
        return 6 * U32 * (sc * c.gz.abs())
    k2 = (c.S2 / n * c.st.rstd).abs()
    return U32 * (6 * sc * c.gz.abs() + 10 * sc * k2 * x.abs() + sc * (12 * c.st.mean.abs() * k2 + 8 * (c.S1 / n).abs()))


# ---------------------------------------------------------------------------------------------
# f32 restatements of the kernels' operation order (tests/test_norm_sample_host.py); ``bug`` injects a plausible mistake
# ---------------------------------------------------------------------------------------------
def _thread_walk(n_vox, C, nblk):
    """it [trips, nblk * 256] item index of every thread per trip (-1 past the end) and the thread's channel group."""
    G, items, T = C // 8, n_vox * (C // 8), nblk * 256
    it = torch.arange(T)[None, :] + T * torch.arange(trips(items, nblk))[:, None]
    return torch.where(it < items, it, torch.full_like(it, -1)), torch.arange(T) % G


def emul_stats(terms1, terms2, n_vox, C, nblk):
    """The statistics kernels in f32: terms [n_vox, C] (f32) are added per thread trip by trip, then per block by the owners of each
    channel group in thread order -> part [nblk, 2C] f32."""
    G = C // 8
    it, grp = _thread_walk(n_vox, C, nblk)
    t1, t2 = terms1.reshape(-1, 8), terms2.reshape(-1, 8)
    zero = torch.zeros((1, 8), dtype=F32)
    t1, t2 = torch.cat([t1, zero]), torch.cat([t2, zero])                  # index -1: the +0 an idle thread keeps
    s1 = torch.zeros((nblk * 256, 8), dtype=F32)
    s2 = torch.zeros_like(s1)
    for row in it:
        s1 = s1 + t1[row]
        s2 = s2 + t2[row]
    s1, s2, grp = s1.view(nblk, 256, 8), s2.view(nblk, 256, 8), grp.view(nblk, 256)
    a1 = torch.zeros((nblk, G, 8), dtype=F32)
    a2 = torch.zeros_like(a1)
    blk = torch.arange(nblk)
    for t in range(256):
        a1[blk, grp[:, t]] += s1[:, t]
        a2[blk, grp[:, t]] += s2[:, t]
    return torch.cat([a1.reshape(nblk, C), a2.reshape(nblk, C)], 1)


def emul_bn_stats(x, nblk):
    f = x.to(F32)
    return emul_stats(f, f * f, x.shape[0], x.shape[1], nblk)


def _const_rows(v, n_vox, C, grid, bug=None):
    """Per-element view [n_vox, C] of a per-channel constant as the fixed-group threads hold it.  bug 'neighbour_group': the 256
    threads of block 1 hold the constants of the next channel group (for one block's worth of items per trip)."""
    out = v.to(F32)[None, :].expand(n_vox, C).clone()
    if bug == "neighbour_group":
        G = C // 8
        it, _ = _thread_walk(n_vox, C, grid)
        mine = it[:, 256:512].reshape(-1)
        mine = mine[mine >= 0]
        vox, cg = mine // G, mine % G
        wrong = v.to(F32).view(G, 8)[(cg + 1) % G]
        out.view(n_vox, G, 8)[vox, cg] = wrong
    return out


def emul_affine(x, scale, shift, lrelu, grid=None, bug=None):
    """k_affine_act in f32 -> the stored bf16 values (as f32); unwritten elements are NaN.  bugs: 'neighbour_group', 'tail'
    (the last items % 256 items are never written)."""
    n_vox, C = x.shape
    sc, sh = _const_rows(scale, n_vox, C, grid, bug), _const_rows(shift, n_vox, C, grid, bug)
    f = x.to(F32) * sc + sh
    if lrelu:
        f = torch.where(f > 0, f, f32_const(SLOPE) * f)
    y = f.to(BF16).to(F32)
    if bug == "tail":
        items = n_vox * (C // 8)
        y.view(-1, 8)[items - items % 256:] = float("nan")
    return y


def f32_const(v):
    return torch.tensor(v, dtype=F32)


def _gz32(x, dy, sc, sh, lrelu, bug=None):
    gz = dy.to(F32)
    if lrelu:
        z = x.to(F32) * sc + sh
        gate = (z < 0) if bug == "strict_gate" else (z <= 0)
        gz = torch.where(gate, gz * f32_const(SLOPE), gz)
    return gz


def emul_bwd_stats(x, dy, scale, shift, mean, rstd, lrelu, nblk, bug=None):
    n_vox, C = x.shape
    gz = _gz32(x, dy, scale.to(F32), shift.to(F32), lrelu, bug)
    t2 = gz * (x.to(F32) - mean.to(F32)) * rstd.to(F32)
    return emul_stats(gz, t2, n_vox, C, nblk)


def emul_bwd_apply(x, dy, scale, shift, mean, rstd, sums, lrelu, grid=None, bug=None, n_for_inv=None):
    """k_bn_bwd_apply in f32 -> stored bf16 dx (as f32).  bugs: 'strict_gate', 'neighbour_group', 'per_batch_n' (n_for_inv)."""
    n_vox, C = x.shape
    inv_n = f32_const(1.0) / f32_const(float(n_for_inv if bug == "per_batch_n" else n_vox))
    sc, mu, rs = scale.to(F32), mean.to(F32), rstd.to(F32)
    s = sums.to(F32)
    k2 = s[C:] * inv_n * rs
    ca, cb, cc = sc, -sc * k2, sc * (mu * k2 - s[:C] * inv_n)
    gz = _gz32(x, dy, sc, shift.to(F32), lrelu, bug)
    nb = bug if bug == "neighbour_group" else None
    A, Bc, Cc_ = (_const_rows(v, n_vox, C, grid, nb) for v in (ca, cb, cc))
    return (A * gz + Bc * x.to(F32) + Cc_).to(BF16).to(F32)


def emul_finalize(part, count, w, b, eps, momentum, rmean, rvar, bug=None):
    """k_bn_finalize: double sums, f32 tail.  bug 'unbiased_scale': the unbiased variance enters rstd."""
    C = part.shape[1] // 2
    s1, s2 = part[:, :C].to(F64).sum(0), part[:, C:].to(F64).sum(0)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp(min=0.0)
    if bug == "unbiased_scale" and count > 1:
        var = var * count / (count - 1.0)
    rstd = ((var + float(eps)) ** -0.5).to(F32)
    sc = (w.to(F32) if w is not None else torch.ones(C, dtype=F32)) * rstd
    mf = mean.to(F32)
    sh = (b.to(F32) if b is not None else torch.zeros(C, dtype=F32)) - mf * sc
    o = SimpleNamespace(scale=sc, shift=sh, mean=mf, rstd=rstd)
    if rmean is not None:
        unb = var * count / (count - 1.0) if (count > 1.0 and bug != "unbiased_scale") else var
        keep, m = f32_const(1.0) - f32_const(momentum), f32_const(momentum)
        o.rmean = keep * rmean.to(F32) + m * mf
        o.rvar = keep * rvar.to(F32) + m * unb.to(F32)
    return o


# ---------------------------------------------------------------------------------------------
# mivp_bn_finalize cases
# ---------------------------------------------------------------------------------------------
FINALIZE_NBLK = (1, 3, 255, 256, 257, 768, 769, 1024, 1025, 2048)
FINALIZE_C = (1, 8, 48)


def finalize_part(nblk, C, seed):
    """A synthetic part array (f32-valued float64): per row the sums of m = 1 .. 64 draws per channel, sum x^2 consistent with sum x."""
    g = gen(seed)
    m = torch.randint(1, 65, (nblk, 1), generator=g).to(F64)
    mu = torch.randn(C, generator=g, dtype=F64) * 0.8
    sd = 0.5 + torch.rand(C, generator=g, dtype=F64)
    s1 = m * mu + m.sqrt() * sd * torch.randn((nblk, C), generator=g, dtype=F64)
    s2 = m * sd * sd * (0.7 + 0.6 * torch.rand((nblk, C), generator=g, dtype=F64)) + s1 * s1 / m
    return r32(torch.cat([s1, s2], 1)), float(m.sum())


def clamp_part(nblk=5, m=1000):
    """One constant channel x = v whose f32 partial sums make sum x^2 / n - mean^2 negative in double, contracted or not: row i
    holds (fl(m v), the f32 below fl(m v^2)).  -> (part [nblk, 2], count, v); the caller asserts the sign of both forms."""
    from fractions import Fraction
    for v in (1.296875, 0.8203125, 2.640625, 1.7109375):
        p1 = float(np.float32(m * v))
        p2 = float(np.nextafter(np.float32(m * v * v), np.float32(0)))
        count = float(nblk * m)
        s1, s2 = nblk * p1, nblk * p2                                       # exact in double: small multiples of f32 values
        mean = s1 / count
        plain = s2 / count - mean * mean
        fused = float(Fraction(s2 / count) - Fraction(mean) ** 2)
        if plain < -2.0 ** -30 and fused < -2.0 ** -30:
            part = torch.tensor([[p1, p2]] * nblk, dtype=F64)
            return part, count, v, plain, fused
    raise AssertionError("no constant channel with a negative variance found")


# ---------------------------------------------------------------------------------------------
# point sampling
# ---------------------------------------------------------------------------------------------
def crop_of(dims, jitter):
    j = [0] * 6 if jitter is None else [int(v) for v in jitter]
    return [(j[2 * a], dims[a] - j[2 * a] - j[2 * a + 1]) for a in range(3)]


def grid_sample_ref(vol, out_dims, jitter, gout=None):
    """vol [B, C, H, W, D] float64 -> sampled [B, N, C] through the reference project's call on the cropped volume; with
    ``gout`` [B, N, C] also the gradient w.r.t. the whole volume [B, C, H, W, D] (zero outside the crop)."""
    B = vol.shape[0]
    v = vol.detach().clone().requires_grad_(gout is not None)
    (a0, n0), (a1, n1), (a2, n2) = crop_of(vol.shape[2:], jitter)
    crop = v[:, :, a0:a0 + n0, a1:a1 + n1, a2:a2 + n2]
    theta = torch.eye(3, 4, dtype=F64)[None].expand(B, 3, 4)
    grid = Fnn.affine_grid(theta, [B, 1, *[int(o) for o in out_dims]], align_corners=False)
    s = Fnn.grid_sample(crop, grid, mode="bilinear", padding_mode="reflection", align_corners=False)
    out = s.flatten(2).transpose(1, 2)
    if gout is None:
        return out.detach()
    out.backward(gout)
    return out.detach(), v.grad


SAMPLE_ROUNDINGS = 3 + 2 + 8


def sample_fwd_ref(vol, out_dims, jitter):
    """(reference, bound) of the forward: the bound is the same call on |vol| (module docstring, ``sampling fwd``)."""
    return grid_sample_ref(vol, out_dims, jitter), SLACK * SAMPLE_ROUNDINGS * U32 * grid_sample_ref(vol.abs(), out_dims, jitter)


def sample_bwd_ref(vol_shape, out_dims, jitter, gout):
    """(gradient [B, H, W, D, C], f32 bound, touched mask) of the backward by float64 autograd through the same call."""
    zero = torch.zeros(vol_shape, dtype=F64)
    _, g = grid_sample_ref(zero, out_dims, jitter, gout)
    _, ga = grid_sample_ref(zero, out_dims, jitter, gout.abs())
    _, touched = grid_sample_ref(zero, out_dims, jitter, torch.ones_like(gout))
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
    return cl(g), SAMPLE_ROUNDINGS * U32 * cl(ga), cl(touched) > 0


def axis_positions(n_crop, n_out):
    """Sample positions of one axis of the cropped volume, from grid_sample itself: a ramp 0 .. n_crop - 1 sampled in float64."""
    ramp = torch.arange(n_crop, dtype=F64).view(1, 1, n_crop, 1, 1)
    return grid_sample_ref(ramp, (n_out, 1, 1), None).reshape(n_out)


def emul_sample_fwd(vol, tabs, out_dims, bug=None):
    """k_sample_points_fwd in f32 from host tables (lo, hi, w per axis): vol [B, C, H, W, D] -> [B, N, C].  bug 'batch_stride':
    sample b starts H W D elements after sample b - 1 instead of C H W D (the same buffer at B = 1)."""
    B, C, H, W, D = vol.shape
    v = vol.to(F32)
    if bug == "batch_stride":
        flat, n = v.reshape(-1), H * W * D
        idx = (torch.arange(B)[:, None, None] * n + torch.arange(C)[None, :, None] * n + torch.arange(n)[None, None, :])
        v = flat[idx].view(B, C, H, W, D)
    acc = torch.zeros((B, C, *out_dims), dtype=F32)
    wts = []
    for (lo, hi, w) in tabs:
        w = torch.from_numpy(np.asarray(w)).to(F32)
        wts.append(((torch.from_numpy(np.asarray(lo)).long(), f32_const(1.0) - w), (torch.from_numpy(np.asarray(hi)).long(), w)))
    for ih, wh in wts[0]:
        for iw, ww in wts[1]:
            for idd, wd in wts[2]:
                wt = (wh[:, None, None] * ww[None, :, None]) * wd[None, None, :]
                acc = acc + wt * v[:, :, ih][:, :, :, iw][:, :, :, :, idd]
    return acc.flatten(2).transpose(1, 2)


def emul_sample_bwd(gout, tabs_bwd, dims, out_dims):
    """k_sample_points_bwd in f32 from host tables (i1, w1, i2, w2 per axis): gout [B, N, C] -> stored bf16 [B, H, W, D, C] (as f32)."""
    B, N, C = gout.shape
    g = gout.to(F32).view(B, *out_dims, C)
    taps = []
    for (i1, w1, i2, w2) in tabs_bwd:
        pair = []
        for idx, w in ((i1, w1), (i2, w2)):
            idx = torch.from_numpy(np.asarray(idx)).long()
            w = torch.from_numpy(np.asarray(w)).to(F32)
            pair.append((idx.clamp(min=0), torch.where(idx >= 0, w, torch.zeros_like(w)), idx >= 0))
        taps.append(pair)
    acc = torch.zeros((B, *dims, C), dtype=F32)
    for ih, fh, vh in taps[0]:
        for iw, fw, vw in taps[1]:
            for idd, fd, vd in taps[2]:
                wt = (fh[:, None, None] * fw[None, :, None]) * fd[None, None, :]
                live = vh[:, None, None] & vw[None, :, None] & vd[None, None, :]
                term = wt[None, ..., None] * g[:, ih][:, :, iw][:, :, :, idd]
                acc = torch.where(live[None, ..., None], acc + term, acc)
    return acc.to(BF16).to(F32)


# ---------------------------------------------------------------------------------------------
# cases (shared by tests/test_norm_sample_host.py and tests/test_hip_norm_sample.py)
# ---------------------------------------------------------------------------------------------
SMALL_DIMS = (3, 5, 7)
SMALL_N = 2 * 3 * 5 * 7
# (n_vox, C): every channel-group count at 210 voxels, then one full block plus two threads
BN_SMALL = [(SMALL_N, C) for C in (8, 16, 24, 40, 48, 144, 768)] + [(43, 48)]
# the 1024-block cap of the statistics kernels (1023 at step 3) and the second trip with a tail
BN_STATS_CAP = [(1024 * 256 + 7, 8), (1023 * 256 // 6 + 5, 48)]
# the 4096-block cap of affine_act / bn_bwd_apply (4095 at step 3) and their second trip
BN_APPLY_CAP = [(4096 * 256 + 5, 8), (-(-4095 * 256 // 6) + 11, 48)]


def bn_id(case):
    return f"n{case[0]}_C{case[1]}"


# (layout, dtype) x C at the issue's geometry; C = 3 is forward only
SAMPLE_MAIN = dict(B=2, dims=(20, 16, 24), out=(5, 4, 6), jitter=(1, 2, 0, 3, 2, 1))
# (dims, out, jitter): an output axis of length 1; crop == out (zero-weight upper taps) with a one-voxel crop on two axes
SAMPLE_EDGES = [((8, 8, 8), (1, 1, 1), None), ((16, 9, 8), (2, 1, 1), (7, 7, 4, 4, 3, 4))]


def reduced(dims, rf):
    return tuple(max(int(n // rf), 1) for n in dims)


def sample_extremes():
    """rf = 8 and 16 on 32^3 and 24^3 with every jitter component at 0 and at ceil(rf) - 1, one axis pair at a time."""
    out = []
    for n in (32, 24):
        for rf in (8, 16):
            top = int(math.ceil(rf)) - 1
            for j in ((0, 0, 0, 0, 0, 0), (top,) * 6, (top, 0, 0, top, top, top), (0, top, top, 0, 0, 0)):
                if min(n - j[0] - j[1], n - j[2] - j[3], n - j[4] - j[5]) >= 1:
                    out.append(((n, n, n), reduced((n, n, n), rf), j))
    return out


def sample_volume(B, C, dims, seed, jitter=None, nan_outside=False):
    """vol [B, C, H, W, D] bf16-valued float64; with ``nan_outside`` a copy whose voxels outside the crop are NaN (no kernel may
    read them) is returned as well."""
    g = gen(seed)
    vol = (torch.randn((B, C, *dims), generator=g, dtype=F32) + 0.25).to(BF16).to(F64)
    if not nan_outside:
        return vol
    fed = torch.full_like(vol, float("nan"))
    (a0, n0), (a1, n1), (a2, n2) = crop_of(dims, jitter)
    fed[:, :, a0:a0 + n0, a1:a1 + n1, a2:a2 + n2] = vol[:, :, a0:a0 + n0, a1:a1 + n1, a2:a2 + n2]
    return vol, fed
