"""Numpy restatement of the soft skeleton and the clDice term (test helper, not a test module).  Written from the definitions
in include/mivp.h / DESIGN 4.36; no torch pooling, nothing shared with the package.

Fields are arrays [..., H, W, D]; every function works in the dtype it is given (numpy rounds each float32 operation on its
own, so the float32 run is the kernels' arithmetic):

  erode(x)(v)  = min of x over v and its 6 face neighbours inside the volume
  dilate(x)(v) = max of x over the 3x3x3 cube around v inside the volume
  E_0 = x, E_{j+1} = erode(E_j);  O_j = dilate(E_{j+1});  d_j = relu(E_j - O_j)       j = 0 .. n
  S_0 = d_0, S_j = S_{j-1} + relu(d_j - S_{j-1} d_j);  soft_skeleton(x, n) = S_n       relu(x) = x > 0 ? x : +0

Backward: a pooled voxel o hands its gradient to the k voxels of its window that hold the selected value, g(o) / k each;
relu'(0) = 0.

The term, on planar p, t [B, K, H, W, D] (classes c >= 1, zeros at invalid voxels), s = smooth:
  SP = S_n(p), SL = S_n(t);  Tprec = (sum SP t + s) / (sum SP + s), Tsens = (sum SL p + s) / (sum SL + s)
  cl = 1 - 2 Tprec Tsens / (Tprec + Tsens), value = mean over (row, class); rows = samples, or the batch.

``Bugs`` plants the kernel bugs that tests/test_cldice_host.py shows the bars to catch."""
import itertools
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_optim_ref import LOSS_L2_BAR, LOSS_MARGIN, LOSS_VALUE_BAR, U32  # noqa: E402,F401

CROSS = ((0, 0, 0), (0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0))
CUBE = tuple(itertools.product((-1, 0, 1), repeat=3))
IGNORE = 255


class Bugs:
    """Deviations from the definition (all off: the definition)."""

    def __init__(self, erode_cube=False, halo_zero=False, first_index=False, one_iteration_less=False, relu_grad_at_zero=False):
        self.erode_cube, self.halo_zero, self.first_index = erode_cube, halo_zero, first_index
        self.one_iteration_less, self.relu_grad_at_zero = one_iteration_less, relu_grad_at_zero


NONE = Bugs()


def _pad(a, fill):
    return np.pad(a, [(0, 0)] * (a.ndim - 3) + [(1, 1)] * 3, constant_values=fill)


def _shift(ap, off):
    """The padded array seen from every voxel v at v + off."""
    h, w, d = (n - 2 for n in ap.shape[-3:])
    return ap[..., 1 + off[0]:1 + off[0] + h, 1 + off[1]:1 + off[1] + w, 1 + off[2]:1 + off[2] + d]


def _pool(x, window, sign, bugs=NONE):
    """min (sign -1) or max (sign +1) of x over the window inside the volume."""
    fill = 0.0 if bugs.halo_zero else (-np.inf if sign > 0 else np.inf)
    xp = _pad(x, x.dtype.type(fill))
    out = _shift(xp, window[0]).copy()
    for off in window[1:]:
        out = np.maximum(out, _shift(xp, off)) if sign > 0 else np.minimum(out, _shift(xp, off))
    return out


def _pool_bwd(x, pooled, g, window, bugs=NONE):
    """d loss / d x from g = d loss / d pooled: tied voxels share equally (first_index: the first of the window takes all)."""
    xp = _pad(x, x.dtype.type(np.nan))
    eq = [_shift(xp, off) == pooled for off in window]
    out = np.zeros_like(x)
    if bugs.first_index:
        taken = np.zeros(x.shape, bool)
        for off, e in zip(window, eq):
            c = np.where(e & ~taken, g, x.dtype.type(0))
            taken |= e
            out += _shift(_pad(c, x.dtype.type(0)), tuple(-o for o in off))
        return out
    k = np.zeros(x.shape, x.dtype)
    for e in eq:
        k += e
    h = g / np.maximum(k, 1)
    hp, mp = _pad(h, x.dtype.type(0)), _pad(pooled, x.dtype.type(np.nan))
    for off in window:
        back = tuple(-o for o in off)
        out += np.where(_shift(mp, back) == x, _shift(hp, back), x.dtype.type(0))
    return out


def relu(x):
    return np.where(x > 0, x, x.dtype.type(0))


def erode(x, bugs=NONE):
    return _pool(x, CUBE if bugs.erode_cube else CROSS, -1, bugs)


def dilate(x, bugs=NONE):
    return _pool(x, CUBE, +1, bugs)


def _tape(x, n, bugs=NONE):
    if bugs.one_iteration_less:
        n = n - 1
    E = [x]
    for _ in range(n + 1):
        E.append(erode(E[-1], bugs))
    O = [dilate(E[j + 1], bugs) for j in range(n + 1)]
    d = [relu(E[j] - O[j]) for j in range(n + 1)]
    S = [d[0]]
    for j in range(1, n + 1):
        S.append(S[-1] + relu(d[j] - S[-1] * d[j]))
    return n, E, O, d, S


def soft_skeleton(x, n, bugs=NONE):
    return _tape(x, n, bugs)[4][-1]


def soft_skeleton_bwd(x, n, g, bugs=NONE):
    """d loss / d x from g = d loss / d S_n, in x's dtype."""
    n, E, O, d, S = _tape(x, n, bugs)
    one, zero = x.dtype.type(1), x.dtype.type(0)

    def on(v):
        return (v >= 0) if bugs.relu_grad_at_zero else (v > 0)

    gs = g.astype(x.dtype)
    A = [None] * (n + 1)
    for j in range(n, 0, -1):
        gr = np.where(on(d[j] - S[j - 1] * d[j]), gs, zero)
        A[j] = np.where(on(E[j] - O[j]), gr * (one - S[j - 1]), zero)
        gs = gs - gr * d[j]
    A[0] = np.where(on(E[0] - O[0]), gs, zero)
    window = CUBE if bugs.erode_cube else CROSS
    G = _pool_bwd(E[n + 1], O[n], -A[n], CUBE, bugs)
    for j in range(n, -1, -1):
        G = A[j] + _pool_bwd(E[j], E[j + 1], G, window, bugs)
        if j >= 1:
            G = G + _pool_bwd(E[j], O[j - 1], -A[j - 1], CUBE, bugs)
    return G


def cldice(p, t, n, smooth, batch, bugs=NONE):
    """(value, d value / d p) in p's dtype; p, t [B, K, H, W, D]."""
    dt = p.dtype.type
    t = t.astype(p.dtype)
    SP, SL = soft_skeleton(p, n, bugs), soft_skeleton(t, n, bugs)
    ax = (0, 2, 3, 4) if batch else (2, 3, 4)
    a1, a2 = (SP * t).sum(ax, keepdims=True), SP.sum(ax, keepdims=True)
    a3, a4 = (SL * p).sum(ax, keepdims=True), SL.sum(ax, keepdims=True)
    s = dt(smooth)
    P, S = (a1 + s) / (a2 + s), (a3 + s) / (a4 + s)
    cl = dt(1) - dt(2) * P * S / (P + S)
    m = dt(1.0 / cl.size)
    dP, dS = -dt(2) * S * S / ((P + S) * (P + S)), -dt(2) * P * P / ((P + S) * (P + S))
    gSP = m * dP * (t / (a2 + s) - (a1 + s) / ((a2 + s) * (a2 + s)))
    gp = soft_skeleton_bwd(p, n, np.broadcast_to(gSP, p.shape).astype(p.dtype), bugs) + m * dS * SL / (a4 + s)
    return cl.sum() * m, gp


# ---------------------------------------------------------------------------------------------
# the term on logits [B, vol, C] (channels last) and labels [B, vol] (f32)
# ---------------------------------------------------------------------------------------------
def valid_mask(y, C, ignore):
    y = y.astype(np.float64)
    v = (y >= 0) & (y < C) & (y == np.floor(y))
    return v if ignore is None else v & (y != float(ignore))


def softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def planar(a, dims):
    """[B, vol, C] -> classes c >= 1 as [B, K, H, W, D]."""
    B, vol, C = a.shape
    return np.ascontiguousarray(np.moveaxis(a[..., 1:], -1, 1)).reshape(B, C - 1, *dims)


def one_hot_planar(y, C, ignore, dims, dtype):
    valid = valid_mask(y, C, ignore)
    hot = (y[..., None] == np.arange(C, dtype=np.float64)) & valid[..., None]
    return planar(hot.astype(dtype), dims)


def term(z, y, dims, n, smooth, batch, ignore, dtype=np.float64, p_planar=None, bugs=NONE):
    """(value, d value / d z [B, vol, C], planar p) in ``dtype``.  ``p_planar``: the p the skeleton side works on (the
    kernel's own, as the GPU test passes it); the softmax Jacobian is always this function's softmax of z."""
    B, vol, C = z.shape
    valid = valid_mask(y, C, ignore)
    pz = softmax(z.astype(dtype))
    p = planar(pz * valid[..., None], dims) if p_planar is None else p_planar.astype(dtype)
    t = one_hot_planar(y, C, ignore, dims, dtype)
    value, gp = cldice(p, t, n, smooth, batch, bugs)
    g = np.zeros((B, vol, C), dtype)
    g[..., 1:] = np.moveaxis(gp.reshape(B, C - 1, vol), 1, -1)
    dz = pz * (g - (pz * g).sum(-1, keepdims=True)) * valid[..., None]
    return value, dz, p


def yardstick(g32, g64):
    """(E32, max |g64|) as tests/loss_optim_ref.py defines it."""
    scale = float(np.abs(g64).max())
    assert scale > 0
    return max(float(np.abs(g32.astype(np.float64) - g64).max()) / scale, U32), scale


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
SMALL = ((1, 1, 4), (2, 2, 2))
SHAPES = SMALL + ((3, 3, 7), (5, 7, 9), (6, 7, 8), (11, 10, 21))     # the last: 1.3 bricks of 8 x 8 x 16 along every axis
KINDS = ("noise", "tube", "grid16", "binary", "zeros", "ones")


def rng(*seed):
    return np.random.default_rng([zlib.crc32(s.encode()) if isinstance(s, str) else int(s) for s in seed])


def _seed_of(kind):
    return KINDS.index(kind) if kind in KINDS else 17


def tube(dims, r):
    """A soft tube along the volume's diagonal, in [0, 1]."""
    H, W, D = dims
    h, w, d = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij")
    tt = d / max(D - 1, 1)
    dist2 = (h - tt * (H - 1)) ** 2 + (w - (W - 1) / 2 - 0.3 * (W - 1) * np.sin(3.0 * tt)) ** 2
    return np.exp(-dist2 / (2.0 * r * r))


def fields(kind, nf, dims, seed=0):
    """f32 [nf, H, W, D]."""
    g = rng(seed, _seed_of(kind), nf, *dims)
    shape = (nf,) + tuple(dims)
    if kind == "noise":
        x = g.random(shape)
    elif kind == "tube":
        x = 0.8 * np.stack([tube(dims, 1.0 + 0.5 * (i % 3)) for i in range(nf)]) + 0.2 * g.random(shape)
    elif kind == "grid16":
        x = g.integers(0, 17, shape) / 16.0
    elif kind == "binary":
        x = (g.random(shape) < 0.6).astype(np.float64)
    elif kind == "zeros":
        x = np.zeros(shape)
    else:
        assert kind == "ones", kind
        x = np.ones(shape)
    return x.astype(np.float32)


def term_case(kind, B, C, dims, ignore, seed=0):
    """(logits f32 [B, vol, C], labels f32 [B, vol]).  Labels: a tube of class 1 (+ class 2 blobs ...) in background, 10 %
    of the voxels the ignore label (when given) and a few half-integers.  kind: noise (2 randn), tube (logits follow a tube),
    pm30 (every logit -30 or +30), grid16 logits (multiples of 1 / 16: ties after the softmax)."""
    g = rng(seed, kind, B, C, *dims)
    vol = dims[0] * dims[1] * dims[2]
    tb = np.stack([tube(dims, 1.2) for _ in range(B)]).reshape(B, vol)
    y = np.where(tb > 0.4, 1.0, 0.0)
    extra = g.integers(0, C, (B, vol)).astype(np.float64)
    y = np.where(g.random((B, vol)) < 0.25, extra, y)
    if kind == "noise":
        z = 2.0 * g.standard_normal((B, vol, C))
    elif kind == "tube":
        z = g.standard_normal((B, vol, C))
        z[..., 1] += 5.0 * (tb - 0.5)
    elif kind == "pm30":
        z = np.where(g.random((B, vol, C)) < 0.5, -30.0, 30.0)
    else:
        assert kind == "grid16", kind
        z = g.integers(-32, 33, (B, vol, C)) / 16.0
    if ignore is not None:
        y = np.where(g.random((B, vol)) < 0.1, float(ignore), y)
    y = np.where(g.random((B, vol)) < 0.05, y + 0.5, y)
    return z.astype(np.float32), y.astype(np.float32)
