"""Float64 restatement of the Lovasz-Softmax loss term (test helper, not a test module).  Written from the definition in
DESIGN 4.40 / include/mivp.h; nothing here shares code with the package.  The validity rule, the label generator and the bars'
constants are those of tests/distmap_ref.py and tests/loss_optim_ref.py.

Layouts (the kernels' own): logits [B, vol, C] (channels last), labels [B, vol] stored as f32, gradient like the logits;
per-segment arrays [S][N]: segment b K + k (class c0 + k of sample b, N = vol) with per_image, else segment k (N = B vol, the
batch in memory order).

  e = g ? 1 - p_c : p_c over the valid voxels (1 - p_y as the sum of the other exponentials over the denominator), G = sum g
  J(F, K) = 1 - (G - F) / (G + K), J(0, 0) = 0
  loss_seg = sum_j e_(j) (J_j - J_(j-1)), errors descending              (``extension``: this line, literally)
  tie rule: in a group of equal e the foreground first, 1 / (G + K) each; the b tied background voxels share
            J(F, K + b) - J(F, K) = (G - F) / ((G + K) (G + K + b)) equally, 1 / b when G + K == 0     (``tie_weights``)
  loss_seg = sum_i s_i e_i with s the tie-rule weights (tests/test_lovasz_host.py: equal to the line above for every order)
  group (sample with per_image, else the batch) = mean of its segments with G > 0 ("present"; none: 0) or of all of them;
  loss = w mean of the groups;   dz_k = w p_k (q_k - sum_c p_c q_c),  q_c = factor_c s_c sgn_c,  sgn = -1 on the foreground

``keys``: the order is taken from a given u32 key array [S][N] (the kernel's own: ascending keys are descending errors, bit 0
of KEY_TOP - key the foreground flag, KEY_INVALID an invalid voxel) instead of from the float64 errors, so a float32 near-tie
cannot reorder the reference.

Bars.  Keys: |e(key) - e64| <= KEY_BAND x E_u, E_u = max |e32 - e64| of the float32 run of these formulas, floored at one unit
roundoff of max e (the band / 2 of tests/segtopk_ref.py); flags and G exact.  Value: VALUE_BAR max(1, A), A the float64 value
without its weight.  Gradient: per element LOSS_MARGIN x E32 x max |g64|, E32 from the float32 run of THIS file's formulas in
the same order."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from distmap_ref import IGNORE, VALUE_BAR, is_class, labels  # noqa: E402,F401
from loss_optim_ref import (LOSS_L2_BAR, LOSS_MARGIN, U32, assert_within_located, gen, loss_grad_bar,  # noqa: E402,F401
                            loss_yardstick, rel_l2)

F64, F32 = torch.float64, torch.float32
KEY_TOP, KEY_INVALID = 0x7F000001, 0xFFFFFFFF
KEY_BAND = LOSS_MARGIN / 2                                   # 4 x E_u
SHAPES = ((2, 3, (5, 6, 7)), (2, 3, (17, 19, 23)))           # one workgroup; several, with a ragged tail
CONTENTS = ("randn", "pm30", "equal")


def ids_shape(s):
    return f"B{s[0]}C{s[1]}_{'x'.join(str(d) for d in s[2])}"


def logits(kind, B, vol, C, seed=3):
    """f32 [B, vol, C].  randn: 2 randn; pm30: their signs times 30 (massive ties at 0 and 1); equal: every logit 0.25."""
    z = 2.0 * torch.randn((B, vol, C), generator=gen(seed + vol + 31 * C), dtype=F32)
    if kind == "pm30":
        return torch.sign(z) * 30.0
    if kind == "equal":
        return torch.full_like(z, 0.25)
    assert kind == "randn", kind
    return z


def label_case(case, B, C, dims, seed=0):
    """f32 [B, vol].  blobs; absent: class 1 nowhere in sample 0; ignored: about 20 % of blobs set to IGNORE; none: all IGNORE."""
    y = labels("absent" if case == "absent" else "blobs", B, C, dims, seed).reshape(B, -1).clone()
    if case == "ignored":
        y[torch.rand(y.shape, generator=gen(seed + 77)) < 0.2] = float(IGNORE)
    elif case == "none":
        y[:] = float(IGNORE)
    return y


def to_segments(a, c0, per_image):
    """[B, vol, C] -> [S, N]."""
    B, vol, C = a.shape
    a = np.moveaxis(a[..., c0:], -1, 1)                      # [B, K, vol]
    return a.reshape(B * (C - c0), vol) if per_image else np.moveaxis(a, 1, 0).reshape(C - c0, B * vol)


def from_segments(s, B, vol, C, c0, per_image):
    """[S, N] -> [B, vol, C], zeros below c0."""
    K = C - c0
    a = s.reshape(B, K, vol) if per_image else np.moveaxis(s.reshape(K, B, vol), 0, 1)
    out = np.zeros((B, vol, C), s.dtype)
    out[..., c0:] = np.moveaxis(a, 1, -1)
    return out


def softmax_errors(z, y, ignore_index, dtype=np.float64):
    """(p, e, hot, valid): z [B, vol, C] -> p, e [B, vol, C] in ``dtype``; hot [B, vol, C] and valid [B, vol] bool."""
    C = z.shape[-1]
    zz = z.numpy().astype(dtype)
    ex = np.exp(zz - zz.max(-1, keepdims=True))
    den = ex.sum(-1, keepdims=True)
    valid = is_class(y, C, ignore_index).numpy()
    hot = (y.numpy().astype(np.float64)[..., None] == np.arange(C)) & valid[..., None]
    others = np.where(hot, 0, ex).sum(-1, keepdims=True)
    e = np.where(hot, others / den, ex / den)
    assert e.dtype == dtype
    return ex / den, e, hot, valid


def jaccard(F, K, G):
    return 0.0 if F == 0 and K == 0 else 1.0 - (G - F) / (G + K)


def extension(e_sorted, g_sorted):
    """sum_j e_(j) (J_j - J_(j-1)) and the differences, literally, for errors given in their (descending) order."""
    G = int(np.sum(g_sorted))
    F = K = 0
    prev, diffs = 0.0, []
    for g in g_sorted:
        F, K = F + int(g), K + int(not g)
        J = jaccard(F, K, G)
        diffs.append(J - prev)
        prev = J
    diffs = np.array(diffs, np.float64)
    return float(np.dot(np.asarray(e_sorted, np.float64), diffs)), diffs


def order_keys(e, g):
    """Integer keys of one segment's valid voxels from exact comparisons of e: ascending = e descending, foreground first."""
    _, rank = np.unique(e, return_inverse=True)
    return 2 * (rank.max(initial=0) - rank.reshape(-1)) + (~g).astype(np.int64)


def tie_weights(okey, g, dtype=np.float64):
    """d loss_seg / d e_i by the tie rule.  okey: any integer keys whose ascending order is the segment's order and whose
    equality is the tie (foreground and background of one error hold different keys, the foreground's the smaller); g bool."""
    n = okey.shape[0]
    if n == 0:
        return np.zeros(0, dtype)
    uniq, inv, cnt = np.unique(okey, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    fg_u = np.zeros(len(uniq), bool)
    fg_u[inv] = g
    assert np.array_equal(fg_u[inv], g), "a tie group mixes foreground and background"
    f_before = np.cumsum(cnt * fg_u) - cnt * fg_u
    k_before = np.cumsum(cnt * ~fg_u) - cnt * ~fg_u
    G = dtype(g.sum())
    gk = G + k_before.astype(dtype)
    b = cnt.astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        w_fg = dtype(1) / gk
        w_bg = np.where(gk > 0, (G - f_before.astype(dtype)) / (gk * (gk + b)), dtype(1) / b)
    s = np.where(fg_u, w_fg, w_bg)[inv]
    assert s.dtype == dtype
    return s


def lovasz_ref(z, y, classes="present", per_image=False, include_background=True, ignore_index=None, weight=None, keys=None,
               dtype=np.float64):
    """(loss, d loss / d logits [B, vol, C], A, counts [S, 2]) in ``dtype``; A = the value without its weight.  ``keys`` u32
    [S][N] (numpy): the order and the ties are the keys'; None: those of this run's float64 errors."""
    B, vol, C = z.shape
    c0 = 0 if include_background else 1
    K = C - c0
    p, e, hot, valid = softmax_errors(z, y, ignore_index, dtype)
    E, Gm = to_segments(e, c0, per_image), to_segments(hot, c0, per_image)
    V = to_segments(np.repeat(valid[..., None], C, -1), c0, per_image)
    if keys is None:
        e64 = to_segments(softmax_errors(z, y, ignore_index)[1], c0, per_image)
    S = E.shape[0]
    seg_loss, counts = np.zeros(S, dtype), np.zeros((S, 2), np.int64)
    Sw = np.zeros(E.shape, dtype)
    for s in range(S):
        v = V[s]
        g = Gm[s][v]
        if keys is None:
            ok = order_keys(e64[s][v], g)
        else:
            assert np.array_equal(keys[s] != KEY_INVALID, v), "the keys' valid voxels are not the reference's"
            ok = keys[s][v].astype(np.int64)
            assert np.array_equal((KEY_TOP - ok) & 1, g.astype(np.int64)), "the keys' foreground flags are not the reference's"
        w = tie_weights(ok, g, dtype)
        Sw[s][v] = w
        seg_loss[s] = (w * E[s][v]).sum(dtype=dtype)
        counts[s] = (g.sum(), v.sum())
    groups = B if per_image else 1
    factor = np.zeros(S, dtype)
    total = dtype(0)
    for gi in range(groups):
        segs = [gi * K + k for k in range(K)]
        use = [s for s in segs if classes == "all" or counts[s, 0] > 0]
        for s in use:
            factor[s] = dtype(1) / dtype(len(use) * groups)
            total += seg_loss[s] * factor[s]
    wv = dtype(1.0 if weight is None else np.float32(weight))
    sgn = np.where(Gm, dtype(-1), dtype(1))
    q = from_segments(Sw * sgn * factor[:, None], B, vol, C, c0, per_image)
    grad = wv * p * (q - (p * q).sum(-1, keepdims=True)) * valid[..., None]
    assert grad.dtype == dtype
    return float(wv * total), torch.from_numpy(grad.astype(np.float64)), float(total), counts


class LvRef:
    """Float64 and float32 runs of a case in one order (the keys' when given), and the gradient's bars."""

    def __init__(self, z, y, keys=None, weight=None, **opts):
        self.l64, self.g64, self.A, self.counts = lovasz_ref(z, y, weight=weight, keys=keys, **opts)
        _, self.g32, _, _ = lovasz_ref(z, y, weight=weight, keys=keys, dtype=np.float32, **opts)
        self.zero = not bool(self.g64.abs().max() > 0)
        if not self.zero:
            self.e32, self.scale = loss_yardstick(self.g32, self.g64)
            self.bar_abs, self.bar_norm = loss_grad_bar(self.g32, self.g64)


def key_errors(keys):
    """(e f32 as float64, foreground flag, valid) of a u32 key array."""
    valid = keys != KEY_INVALID
    k = np.where(valid, KEY_TOP - keys.astype(np.int64), 0)
    return (k >> 1).astype(np.uint32).view(np.float32).astype(np.float64), (k & 1).astype(bool) & valid, valid


def e_u(z, y, ignore_index):
    """(E_u, e64 [B, vol, C], valid): what the float32 run loses on e, floored at one unit roundoff of max e."""
    _, e64, _, valid = softmax_errors(z, y, ignore_index)
    _, e32, _, _ = softmax_errors(z, y, ignore_index, np.float32)
    if not valid.any():
        return 0.0, e64, valid
    return max(float(np.abs(e32.astype(np.float64) - e64)[valid].max()), U32 * float(e64[valid].max())), e64, valid
