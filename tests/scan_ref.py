"""CPU restatement of mivp_amd.scan in numpy / torch (test helper, not a test module).

Orientation is ``permute`` + ``flip`` of the whole array, the intensity map is evaluated in float64 and rounded once,
and the resize is stated twice: by ``torch.nn.functional.interpolate`` on the CPU and by a float64 evaluation of the same
formula written out here (separable, one axis at a time).  Nothing here reads the per-axis tables of ``ScanGeometry``."""
import numpy as np
import torch
import torch.nn.functional as F


def orient(x, perm, flip):
    """Native [..., H, W, D] -> oriented: oriented axis a is native axis perm[a], reversed where flip[a]."""
    lead = x.dim() - 3
    y = x.permute(*range(lead), *[lead + p for p in perm])
    dims = [lead + a for a in range(3) if flip[a]]
    return (y.flip(dims) if dims else y).contiguous()


def unorient(y, perm, flip):
    """The inverse of ``orient``."""
    lead = y.dim() - 3
    dims = [lead + a for a in range(3) if flip[a]]
    x = y.flip(dims) if dims else y
    inv = [list(perm).index(j) for j in range(3)]
    return x.permute(*range(lead), *[lead + p for p in inv]).contiguous()


def intensity(x, a_min=-1000.0, a_max=1000.0, b_min=0.0, b_max=1.0, clip=True):
    """fp32 result of one fused multiply-add and clamp: the fp32 value x, times fp32 s plus fp32 t evaluated in float64
    (exact for the integer inputs of the tests) and rounded once, then clamped to [b_min, b_max]."""
    s64 = (b_max - b_min) / (a_max - a_min)
    s, t = float(np.float32(s64)), float(np.float32(b_min - a_min * s64))
    y = (x.to(torch.float32).double() * s + t).to(torch.float32)
    if clip:
        y = y.clamp(float(np.float32(b_min)), float(np.float32(b_max)))
    return y


def trilinear_torch(x, size):
    """``F.interpolate(mode='trilinear', align_corners=False)`` of [C, H, W, D] (or [H, W, D]) in x's dtype on the CPU."""
    v = x if x.dim() == 4 else x[None]
    out = F.interpolate(v[None], size=tuple(size), mode="trilinear", align_corners=False)[0]
    return out if x.dim() == 4 else out[0]


def trilinear_f64(x, size):
    """The same formula in float64, one axis at a time: src = max((dst + 0.5) * n_in / n_out - 0.5, 0), the two
    neighbours floor(src) and min(floor(src) + 1, n_in - 1), weight src - floor(src) on the upper one."""
    y = x.double()
    lead = y.dim() - 3
    for a in range(3):
        n_in, n_out = y.shape[lead + a], int(size[a])
        src = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp(min=0.0)
        lo = src.floor().long().clamp(max=n_in - 1)
        hi = (lo + 1).clamp(max=n_in - 1)
        w = (src - lo.double()).reshape([-1 if i == lead + a else 1 for i in range(y.dim())])
        y = y.index_select(lead + a, lo) * (1.0 - w) + y.index_select(lead + a, hi) * w
    return y


def nearest_torch(x, size):
    """``F.interpolate(mode='nearest')`` of an [H, W, D] map on the CPU, in x's dtype."""
    if x.dtype in (torch.uint8, torch.float32, torch.float64):
        return F.interpolate(x[None, None], size=tuple(size), mode="nearest")[0, 0]
    return F.interpolate(x[None, None].double(), size=tuple(size), mode="nearest")[0, 0].to(x.dtype)


def prepare_scan(raw, geom, **kw):
    """[C, H, W, D] -> (fp32 torch result, float64 result) [C, H', W', D'] of map -> orient -> resize."""
    v = orient(intensity(raw, **kw), geom.perm, geom.flip)
    if not geom.resized:
        return v, v.double()
    return trilinear_torch(v, geom.size), trilinear_f64(v, geom.size)


def prepare_labels(seg, geom):
    v = orient(seg, geom.perm, geom.flip)
    return (nearest_torch(v, geom.size) if geom.resized else v).to(torch.uint8)


def restore_labels(labels, geom):
    v = nearest_torch(labels, geom.oriented_shape) if geom.resized else labels
    return unorient(v, geom.perm, geom.flip)


def affine_for(perm, flip, zooms=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """A 4 x 4 affine whose RAS orientation is (perm, flip): native axis perm[a] points along world axis a (against it
    where flip[a]) with voxel size zooms[perm[a]]."""
    a = np.eye(4)
    a[:3, :3] = 0.0
    for w in range(3):
        a[w, perm[w]] = (-1.0 if flip[w] else 1.0) * zooms[perm[w]]
    a[:3, 3] = origin
    return a
