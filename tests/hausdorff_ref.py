"""Float64 references of the Hausdorff distance-transform loss term and its weight maps (test helper, not a test module).
Written from the definition in DESIGN 4.39 / include/mivp.h; nothing here shares code with the package.  Label cases, the
validity rule, the shapes and the bars' constants are those of tests/distmap_ref.py.

Layouts (the kernels' own): logits [B, vol, C] (channels last), labels [B, H, W, D] stored as f32, maps [B, K, H, W, D] for the
classes c0 .. C - 1, gradient like the logits.

  P_c = {argmax_j z_j == c}, the lowest index among exact maxima, at every voxel;  G_c = {y == c}, valid labels only
  field(M)(v) = scipy's distance_transform_edt(M) inside M, distance_transform_edt(~M) outside; 0 where M is empty or the sample
  Wm_c = field(P_c)^alpha + field(G_c)^alpha
  loss = w sum_valid sum_{c >= c0} (p_c - g_c)^2 Wm_c / (K max(N, 1))
  d loss / d z_j = w p_j (q_j - sum_c p_c q_c) / (K max(N, 1)),  q_c = 2 (p_c - g_c) Wm_c for c >= c0, else 0

Bars.  Maps at unit spacing and alpha == 2 are sums of two exact integers: equal bits.  Any other spacing or alpha:
LOSS_MARGIN x E32 x max |Wm64| per element, E32 the error of ``weight_maps(..., dtype=float32)`` (the same formula in f32 numpy:
the f32 root squared or raised to alpha) against float64, floored at one unit roundoff.  The spacing the reference sees is the
f32 value the kernel receives (ANISO32).  Value: VALUE_BAR max(1, A), A = the float64 loss without w (every term is >= 0).
Gradient: rel-L2 < LOSS_L2_BAR and LOSS_MARGIN x E32 x max |g64| per element, E32 from the f32 run of THIS file's formulas."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distmap_ref as D  # noqa: E402
from distmap_ref import (ANISO, IGNORE, LABEL_CASES, SHAPES, VALUE_BAR, assert_within_located, gen, ids_shape,  # noqa: E402,F401
                         is_class, labels, ndi, rel_l2)
from loss_optim_ref import LOSS_L2_BAR, LOSS_MARGIN, U32, loss_grad_bar, loss_yardstick  # noqa: E402,F401

F64, F32 = torch.float64, torch.float32
UNIT = (1.0, 1.0, 1.0)
ANISO32 = tuple(float(np.float32(s)) for s in ANISO)
LOGIT_KINDS = ("randn", "pm30", "ties")


def logits(kind, B, vol, C, seed=3):
    """f32 [B, vol, C].  randn: 2 randn; pm30: their signs times 30 (most voxels tie between several classes); ties: small
    integers, plus planted voxels where all classes, the last two, and the first and last class hold the exact maximum."""
    g = gen(seed + vol + 31 * C)
    z = 2.0 * torch.randn((B, vol, C), generator=g, dtype=F32)
    if kind == "pm30":
        return torch.sign(z) * 30.0
    if kind == "ties":
        z = torch.randint(-2, 3, (B, vol, C), generator=g).to(F32)
        z[:, 0::7] = 1.5                                           # all classes tie: class 0
        z[:, 1::7, C - 2:] = 4.0                                   # the last two tie above the rest: class C - 2
        z[:, 2::7, 0] = 5.0
        z[:, 2::7, C - 1] = 5.0                                    # the first and the last tie: class 0
        return z
    assert kind == "randn", kind
    return z


def pred_classes(z):
    """int64 [B, vol]: the lowest index among the exact maxima of each voxel's logits, by comparisons alone."""
    zn = z.numpy()
    return torch.from_numpy((zn == zn.max(-1, keepdims=True)).argmax(-1))


def field_sq(M, spacing, edt=None):
    """Squared field of one mask [H, W, D] in float64; zeros when M is empty or everything."""
    if not M.any() or M.all():
        return np.zeros(M.shape)
    edt = edt or (lambda m: ndi().distance_transform_edt(m, sampling=spacing))
    d2 = np.where(M, edt(M), edt(~M)) ** 2                         # edt(m): to the nearest voxel where m is False
    if tuple(spacing) == UNIT:                                     # integers: the root's rounding is taken out again
        assert float(np.abs(d2 - np.rint(d2)).max()) < 1e-9
        d2 = np.rint(d2)
    return d2


class MapRef:
    """P, G bool [B, K, H, W, D]; fp2, fg2 the squared fields (float64); ``wm(alpha)`` the weight maps."""

    def __init__(self, z, y, spacing=UNIT, include_background=False, ignore_index=None, edt=None):
        B, dims, C = y.shape[0], tuple(y.shape[1:]), z.shape[-1]
        c0 = 0 if include_background else 1
        ok = is_class(y, C, ignore_index).numpy()
        yn = y.numpy()
        pred = pred_classes(z).numpy().reshape((B,) + dims)
        shape = (B, C - c0) + dims
        self.P, self.G = np.zeros(shape, bool), np.zeros(shape, bool)
        self.fp2, self.fg2 = np.zeros(shape), np.zeros(shape)
        for b in range(B):
            for k in range(C - c0):
                self.P[b, k] = pred[b] == c0 + k
                self.G[b, k] = ok[b] & (yn[b] == float(c0 + k))
                self.fp2[b, k] = field_sq(self.P[b, k], spacing, edt)
                self.fg2[b, k] = field_sq(self.G[b, k], spacing, edt)

    def wm(self, alpha, dtype=np.float64):
        return weight_maps(self.fp2, self.fg2, alpha, dtype)


def weight_maps(fp2, fg2, alpha, dtype=np.float64):
    """field(P)^alpha + field(G)^alpha from the float64 squared fields.  float32: every operation in f32 from the f32 root."""
    if dtype == np.float64:
        return fp2 + fg2 if alpha == 2.0 else fp2 ** (0.5 * alpha) + fg2 ** (0.5 * alpha)
    rp, rg = np.sqrt(fp2).astype(np.float32), np.sqrt(fg2).astype(np.float32)
    out = rp * rp + rg * rg if alpha == 2.0 else rp ** np.float32(alpha) + rg ** np.float32(alpha)
    assert out.dtype == np.float32
    return out


def map_bar(wm64, wm32):
    """(absolute per-element bar, E32) of a map case; E32 relative to max |Wm64|, floored at one unit roundoff."""
    scale = float(np.abs(wm64).max())
    if scale == 0.0:
        return 0.0, U32
    e32 = max(float(np.abs(wm32.astype(np.float64) - wm64).max()) / scale, U32)
    return LOSS_MARGIN * e32 * scale, e32


# ---------------------------------------------------------------------------------------------
# the loss term
# ---------------------------------------------------------------------------------------------
def hausdorff_ref(z, y, wmap, include_background, ignore_index, weight=None, dtype=F64, all_voxels=False, shift=0, no_target=False):
    """(loss, d loss / d logits, A), written out by hand in ``dtype``.  z [B, vol, C], y [B, vol], wmap [B, K, vol].
    Corruptions: ``all_voxels`` (the mean over all voxels), ``shift`` (wmap[c - c0 + shift]), ``no_target`` (p^2, not (p - g)^2)."""
    C = z.shape[-1]
    c0 = 0 if include_background else 1
    zz = z.to(dtype)
    e = (zz - zz.max(-1, keepdim=True).values).exp()
    p = e / e.sum(-1, keepdim=True)
    ok = is_class(y, C, ignore_index)
    valid = ok.to(dtype)
    g = ((y.to(F64).unsqueeze(-1) == torch.arange(C, dtype=F64)) & ok.unsqueeze(-1)).to(dtype)
    if no_target:
        g = torch.zeros_like(g)
    n = float(y.numel()) if all_voxels else max(float(valid.sum()), 1.0)
    w = torch.tensor(1.0 if weight is None else float(np.float32(weight)), dtype=dtype)
    norm = torch.tensor(float((C - c0) * n), dtype=dtype)
    wm = D.phit_of(wmap.to(dtype), C, c0, shift)                   # [B, vol, C], zeros below c0
    d = p - g
    q = 2.0 * d * wm
    s = (p * q).sum(-1, keepdim=True)
    A = ((d * d * wm).sum(-1) * valid).sum() / norm
    grad = w * p * (q - s) * valid.unsqueeze(-1) / norm
    return (w * A).to(F64), grad, float(A)


class HdRef:
    def __init__(self, z, y, wmap, include_background, ignore_index, weight=None):
        self.l64, self.g64, self.A = hausdorff_ref(z, y, wmap, include_background, ignore_index, weight)
        self.l32, self.g32, _ = hausdorff_ref(z, y, wmap, include_background, ignore_index, weight, dtype=F32)
        self.zero = not bool(self.g64.abs().max() > 0)
        if not self.zero:
            self.e32, self.scale = loss_yardstick(self.g32, self.g64)
            self.bar_abs, self.bar_norm = loss_grad_bar(self.g32, self.g64)


def loss_case(shape, include_background, saturated=False, all_ignored=False, seed=3):
    """(z [B, vol, C] f32, y [B, vol] f32, wmap [B, K, vol] f32, ignore label) on the ``bad`` labels of a shape: invalid voxels
    of all three kinds; wmap = the float64 reference's maps at unit spacing and alpha = 2 (integers, exact in f32)."""
    B, C, dims = shape
    yv = labels("bad", B, C, dims, seed)
    if all_ignored:
        yv[:] = float(IGNORE)
    vol = dims[0] * dims[1] * dims[2]
    z = logits("pm30" if saturated else "randn", B, vol, C, seed)
    wm = MapRef(z, yv, UNIT, include_background, IGNORE).wm(2.0)
    assert float(wm.max()) < 2 ** 24 and np.array_equal(wm, np.rint(wm))
    return z, yv.reshape(B, vol), torch.from_numpy(wm).to(F32).reshape(B, -1, vol), IGNORE
