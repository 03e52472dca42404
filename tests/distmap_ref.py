"""Float64 references of the batched signed distance maps and of the boundary loss term (test helper, not a test module).
Written from the definitions in DESIGN 4.35 / include/mivp.h; nothing here shares code with the package.

Layouts (the kernels' own): labels [B, H, W, D] stored as f32, phi [B, K, H, W, D] for the classes c0 .. C - 1 (c0 = 0 with
``include_background``, else 1), logits [B, vol, C] (channels last), gradient like the logits.

  M = {label == c}; a label that is no class (non-integer, outside [0, C), the ignore label) is in no M
  phi = edt(~M, spacing) ~M - (edt(M, spacing) - 1) M with scipy's distance_transform_edt; 0 where M is empty or the sample
  valid voxel: the rule of tests/segloss_ref.py; N = their number in the batch, K = C - c0
  loss = w sum_valid sum_{c >= c0} p_c phi_c / (K max(N, 1)),  d loss / d z_j = w p_j (phit_j - sum_c p_c phit_c) / (K max(N, 1))

Bars: the maps at unit spacing are integer-exact under the root and within 2^-22 max(1, |phi64|) (one f32 root at <= 1 ulp
plus one rounded subtraction); the value within 2e-5 max(1, A), A = sum |p_c phi_c| / (K N) (the sum is signed and cancels);
the gradient rel-L2 < LOSS_L2_BAR and per element LOSS_MARGIN x E32 x max |g64|, E32 from the f32 run of THIS file's
formulas on the same case (tests/loss_optim_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_optim_ref import (LOSS_L2_BAR, LOSS_MARGIN, U32, assert_within_located, gen, loss_grad_bar,  # noqa: E402,F401
                            loss_yardstick, rel_l2)

F64, F32 = torch.float64, torch.float32
VALUE_BAR = 2e-5
MAP_BAR = 2.0 ** -22
ANISO = (0.8, 0.8, 2.5)                                 # the spacing of tests/test_hip_surface.py
IGNORE = 255

# (B, C, (H, W, D)): D crossing one and two 64-lane steps, vol not a multiple of 4 and above 1024 (several partial rows),
# batch and class strides that differ
SHAPES = ((2, 3, (5, 6, 70)), (1, 2, (3, 4, 130)), (3, 2, (9, 7, 5)), (1, 2, (1, 1, 67)), (2, 4, (17, 3, 64)))
LABEL_CASES = ("blobs", "absent", "full", "corner", "faces", "checker", "bad")
ids_shape = lambda s: f"B{s[0]}C{s[1]}_" + "x".join(str(v) for v in s[2])  # noqa: E731


def ndi():
    return pytest.importorskip("scipy.ndimage")


# ---------------------------------------------------------------------------------------------
# labels
# ---------------------------------------------------------------------------------------------
def _blobs(g, B, C, dims):
    """Background with a few boxes and balls of every foreground class."""
    H, W, D = dims
    y = torch.zeros((B,) + dims, dtype=F32)
    hh, ww, dd = torch.meshgrid(torch.arange(H), torch.arange(W), torch.arange(D), indexing="ij")
    for b in range(B):
        for c in range(1, C):
            for _ in range(2):
                ctr = [int(torch.randint(0, n, (1,), generator=g)) for n in dims]
                r = [1 + int(torch.randint(0, max(n // 3, 1) + 1, (1,), generator=g)) for n in dims]
                if int(torch.randint(0, 2, (1,), generator=g)):
                    m = ((hh - ctr[0]).abs() <= r[0]) & ((ww - ctr[1]).abs() <= r[1]) & ((dd - ctr[2]).abs() <= r[2])
                else:
                    m = ((hh - ctr[0]) / r[0]) ** 2 + ((ww - ctr[1]) / r[1]) ** 2 + ((dd - ctr[2]) / r[2]) ** 2 <= 1.0
                y[b][m] = float(c)
    return y


def labels(case, B, C, dims, seed=0):
    """f32 [B, H, W, D].  blobs: random boxes and balls; absent: class 1 nowhere in sample 0 (present in the next); full:
    class 1 fills sample 0; corner: class C - 1 in the far corner voxel of sample 0 alone; faces: class 1 everywhere but the
    centre voxel; checker: a 3-D checkerboard of classes 0 and 1; bad: blobs with 255, 1.5 and -1 scattered through them."""
    g = gen(1000 * seed + 7 * B + C + sum(dims))
    y = _blobs(g, B, C, dims)
    H, W, D = dims
    if case == "absent":
        y[0][y[0] == 1.0] = 0.0
        if B > 1:
            y[1, H // 2, W // 2, D // 3:D // 2 + 1] = 1.0
    elif case == "full":
        y[0] = 1.0
    elif case == "corner":
        y[0] = 0.0
        y[0, H - 1, W - 1, D - 1] = float(C - 1)
    elif case == "faces":
        y[:] = 1.0
        y[:, H // 2, W // 2, D // 2] = 0.0
    elif case == "checker":
        hh, ww, dd = torch.meshgrid(torch.arange(H), torch.arange(W), torch.arange(D), indexing="ij")
        y[:] = ((hh + ww + dd) % 2).to(F32)
    elif case == "bad":
        y[:, :, :, D // 4:D // 2] = 1.0                            # a slab of class 1 for the bad labels to sit in
        bad = torch.tensor([float(IGNORE), 1.5, -1.0], dtype=F32)
        hit = torch.rand(y.shape, generator=g) < 0.15
        y = torch.where(hit, bad[torch.randint(0, 3, y.shape, generator=g)], y)
    else:
        assert case == "blobs", case
    return y


def is_class(y, C, ignore_index):
    yy = y.to(F64)
    ok = (yy >= 0) & (yy < C) & (yy == yy.floor())
    return ok if ignore_index is None else ok & (yy != float(ignore_index))


# ---------------------------------------------------------------------------------------------
# the maps
# ---------------------------------------------------------------------------------------------
class MapRef:
    """phi float64 [B, K, H, W, D]; inside (bool) = M; d2 = the squared distance under the root at every voxel (to M
    outside, to the complement inside; 0 in a degenerate (b, c)); zero [B, K] = M empty or the whole sample."""

    def __init__(self, y, C, spacing=(1.0, 1.0, 1.0), include_background=False, ignore_index=None, edt=None):
        edt = edt or (lambda m: ndi().distance_transform_edt(m, sampling=spacing))
        c0 = 0 if include_background else 1
        B, K = y.shape[0], C - c0
        ok = is_class(y, C, ignore_index).numpy()
        yn = y.numpy()
        self.phi = np.zeros((B, K) + tuple(y.shape[1:]))
        self.inside = np.zeros(self.phi.shape, bool)
        self.d2 = np.zeros(self.phi.shape)
        self.zero = np.zeros((B, K), bool)
        for b in range(B):
            for k in range(K):
                M = ok[b] & (yn[b] == float(c0 + k))
                self.inside[b, k] = M
                if not M.any() or M.all():
                    self.zero[b, k] = True
                    continue
                d_out, d_in = edt(~M), edt(M)                      # to the nearest voxel of M / of the complement
                self.phi[b, k] = d_out * ~M - (d_in - 1.0) * M
                self.d2[b, k] = np.where(M, d_in, d_out) ** 2


def edt_brute(spacing):
    """distance_transform_edt by all-pairs distances (volumes of a few hundred voxels): for every non-zero voxel of the
    mask the distance to the nearest zero voxel, 0 at the zero voxels."""
    def run(mask):
        idx = np.stack(np.meshgrid(*[np.arange(n) for n in mask.shape], indexing="ij"), -1).reshape(-1, 3) * np.asarray(spacing)
        zero = idx[~mask.reshape(-1)]
        d = np.sqrt(((idx[:, None, :] - zero[None, :, :]) ** 2).sum(-1)).min(1)
        return np.where(mask.reshape(-1), d, 0.0).reshape(mask.shape)
    return run


# ---------------------------------------------------------------------------------------------
# the loss term
# ---------------------------------------------------------------------------------------------
def phit_of(phi, C, c0, shift=0):
    """phi [B, K, vol] -> [B, vol, C] with zeros below c0; ``shift``: read phi[c - c0 + shift] (mod K): a corruption."""
    B, K, vol = phi.shape
    out = torch.zeros((B, vol, C), dtype=phi.dtype)
    for c in range(c0, C):
        out[..., c] = phi[:, (c - c0 + shift) % K]
    return out


def boundary_ref(z, y, phi, include_background, ignore_index, weight=None, dtype=F64, all_voxels=False, shift=0):
    """(loss, d loss / d logits, A), written out by hand in ``dtype``.  z [B, vol, C], y [B, vol], phi [B, K, vol].
    ``all_voxels`` (a corruption): the mean over all voxels instead of the valid ones."""
    C = z.shape[-1]
    c0 = 0 if include_background else 1
    zz = z.to(dtype)
    e = (zz - zz.max(-1, keepdim=True).values).exp()
    p = e / e.sum(-1, keepdim=True)
    valid = is_class(y, C, ignore_index).to(dtype)
    n = float(y.numel()) if all_voxels else max(float(valid.sum()), 1.0)
    w = torch.tensor(1.0 if weight is None else float(np.float32(weight)), dtype=dtype)
    norm = torch.tensor(float((C - c0) * n), dtype=dtype)
    ph = phit_of(phi.to(dtype), C, c0, shift)
    s = (p * ph).sum(-1)
    loss = w * (s * valid).sum() / norm
    grad = w * p * (ph - s.unsqueeze(-1)) * valid.unsqueeze(-1) / norm
    A = float(((p * ph).abs().sum(-1) * valid).sum() / norm)
    return loss.to(F64), grad, A


class BoundaryRef:
    def __init__(self, z, y, phi, include_background, ignore_index, weight=None):
        self.l64, self.g64, self.A = boundary_ref(z, y, phi, include_background, ignore_index, weight)
        self.l32, self.g32, _ = boundary_ref(z, y, phi, include_background, ignore_index, weight, dtype=F32)
        self.zero = not bool(self.g64.abs().max() > 0)
        if not self.zero:
            self.e32, self.scale = loss_yardstick(self.g32, self.g64)
            self.bar_abs, self.bar_norm = loss_grad_bar(self.g32, self.g64)


def loss_case(shape, include_background, saturated=False, all_ignored=False, seed=3):
    """(z [B, vol, C] f32, y [B, vol] f32, phi [B, K, vol] f32, ignore label) on the ``bad`` labels of a shape: invalid
    voxels of all three kinds; phi = the float64 reference's maps rounded to f32."""
    B, C, dims = shape
    yv = labels("bad", B, C, dims, seed)
    if all_ignored:
        yv[:] = float(IGNORE)
    ref = MapRef(yv, C, (1.0, 1.0, 1.0), include_background, IGNORE)
    vol = dims[0] * dims[1] * dims[2]
    g = gen(seed + vol)
    z = 2.0 * torch.randn((B, vol, C), generator=g, dtype=F32)
    if saturated:
        z = torch.sign(z) * 30.0
    phi = torch.from_numpy(ref.phi).to(F32).reshape(B, -1, vol)
    return z, yv.reshape(B, vol), phi, IGNORE
