"""Exact-integer parity helpers (test helper, not a test module).

The convolution and GEMM kernels are linear with bf16 operands and fp32 accumulation.  Fed small integers (or dyadic
values where a kernel has 1/4 and 3/4 weights) every product and every partial sum is an exactly representable fp32
number in ANY summation order, so the kernel's result has to equal a float64 reference bit for bit at every element:
no tolerance, and a failure names the voxel and the channel.  Two conditions make "exact" true and both are asserted on
the float64 reference of every case (``assert_exact_inputs``):

  (a)  sum |a| * |b| over the reduction axis < 2**24 for every output element (the same float64 op applied to the
       absolute values): every partial sum, in any order and any grouping, is then an integer (or dyadic) below 2**24;
  (b)  where the kernel stores bf16, the reference is a bf16 number everywhere: the store's rounding mode never enters.

Everything here is float64 torch on the CPU (torch.nn.functional and autograd); nothing shares code with the kernels.
Tensors are channels-first [B, C, H, W, D] unless a name says otherwise."""
import itertools

import torch
import torch.nn.functional as F

EXACT_LIMIT = float(2 ** 24)
DENSITIES = (0.5, 0.25, 0.12, 0.06, 0.03, 0.015, 0.008)


# ---------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def draw(g, shape, values, density=1.0):
    """float64 tensor of ``shape``: each element one of ``values`` (uniform), kept with probability ``density``, else 0."""
    vals = torch.tensor([float(v) for v in values], dtype=torch.float64)
    shape = tuple(int(s) for s in shape)
    pick = vals[torch.randint(0, len(vals), shape, generator=g)]
    if density >= 1.0:
        return pick
    return pick * (torch.rand(shape, generator=g) < density)


def is_bf16(t):
    """Elementwise: the float64 value survives fp32 -> bf16 -> float64 unchanged."""
    return t.float().bfloat16().double() == t


def first_exact(make, densities=DENSITIES):
    """``make(density) -> (ref, bound, stored_bf16, payload)``: the payload of the densest draw whose float64 reference
    meets conditions (a) and (b).  The choice looks at the reference only, never at a kernel's output; the caller still
    asserts the conditions on what it gets back."""
    for dens in densities:
        ref, bound, stored_bf16, payload = make(dens)
        if exact_ok(ref, bound, stored_bf16):
            return payload
    raise AssertionError("no density in %r gives an exact case" % (densities,))


# ---------------------------------------------------------------------------------------------
# conditions (a) and (b)
# ---------------------------------------------------------------------------------------------
def _pairs(ref, bound, stored_bf16):
    if isinstance(ref, torch.Tensor):
        return [(ref, bound, stored_bf16)]
    flags = stored_bf16 if isinstance(stored_bf16, (tuple, list)) else [stored_bf16] * len(ref)
    return list(zip(ref, bound, flags))


def exact_ok(ref, bound, stored_bf16):
    return all(bool((b < EXACT_LIMIT).all()) and bool((r.abs() <= b).all()) and (not s or bool(is_bf16(r).all()))
               for r, b, s in _pairs(ref, bound, stored_bf16))


def assert_exact_inputs(ref, bound, stored_bf16, what=""):
    """Conditions (a) and (b) on 100 % of the reference's elements.  ``bound`` is the reference op applied to the absolute
    values of its operands; ``stored_bf16`` says whether the kernel stores this tensor as bf16.  Tuples check several
    outputs of one case."""
    for k, (r, b, s) in enumerate(_pairs(ref, bound, stored_bf16)):
        assert r.dtype == torch.float64 and b.dtype == torch.float64 and r.shape == b.shape, (what, k)
        assert bool(torch.isfinite(b).all()), (what, k)
        worst = float(b.max()) if b.numel() else 0.0
        assert worst < EXACT_LIMIT, f"{what}[{k}]: condition (a) violated: sum |a||b| reaches {worst:.0f} >= 2**24"
        assert bool((r.abs() <= b).all()), f"{what}[{k}]: the bound is not the absolute-value form of the reference op"
        if s:
            bad = ~is_bf16(r)
            assert not bool(bad.any()), (f"{what}[{k}]: condition (b) violated: {int(bad.sum())} of {r.numel()} reference "
                                         f"values are not bf16 numbers (first: {float(r[bad][0])})")


def assert_bf16_operands(*tensors):
    """The operands handed to a kernel as bf16 must already be bf16 numbers (the cast on the way to the device is exact)."""
    for k, t in enumerate(tensors):
        if t is not None:
            assert bool(is_bf16(t).all()), f"operand {k} is not bf16-representable"


# ---------------------------------------------------------------------------------------------
# located comparison
# ---------------------------------------------------------------------------------------------
def _border_report(idx, dims):
    """How many mismatching voxels lie on a face / an edge / a corner of the (H, W, D) volume, and in its interior."""
    names = ("interior", "face", "edge", "corner")
    count = dict.fromkeys(names, 0)
    seen = set()
    for b, h, w, d, _ in idx:
        if (b, h, w, d) in seen:
            continue
        seen.add((b, h, w, d))
        on = sum(1 for v, n in zip((h, w, d), dims) if v == 0 or v == n - 1)
        count[names[on]] += 1
    return count


def assert_equal_located(got, ref, layout, what=""):
    """torch.equal(got, ref) on float64 copies, every element, no tolerance.  ``layout`` names the axes of both tensors:
    a permutation of "bhwdc" for volumes (mismatches are reported as (b, h, w, d, c) and counted per face, edge and
    corner), any other string of distinct letters otherwise (mismatches are reported as plain indices)."""
    g = got.detach().double().cpu()
    r = ref.detach().double().cpu()
    assert g.shape == r.shape, f"{what}: shape {tuple(g.shape)} != reference {tuple(r.shape)}"
    assert len(layout) == g.dim(), (layout, tuple(g.shape))
    if torch.equal(g, r):
        return
    volume = sorted(layout) == sorted("bhwdc")
    if volume:
        perm = [layout.index(a) for a in "bhwdc"]
        g, r = g.permute(perm), r.permute(perm)
    bad = torch.nonzero(~((g == r) | (torch.isnan(g) & torch.isnan(r))))
    idx = [tuple(int(i) for i in row) for row in bad]
    lines = [f"{what}: {len(idx)} of {g.numel()} elements differ from the float64 reference"
             f" (axes {'bhwdc' if volume else layout}, shape {tuple(g.shape)})"]
    for i in idx[:10]:
        lines.append(f"  {i}: got {float(g[i])!r} want {float(r[i])!r}")
    if volume:
        lines.append(f"  voxels by position: {_border_report(idx, tuple(g.shape[1:4]))}")
    msg = "\n".join(lines)
    print(msg)
    raise AssertionError(msg)


def ulp_distance(got, ref64):
    """|got - fp32(ref64)| in units of the fp32 spacing at fp32(ref64), elementwise (float64)."""
    r32 = ref64.double().float()
    g32 = got.detach().float().cpu()
    spacing = (torch.nextafter(r32.abs(), torch.full_like(r32, float("inf"))) - r32.abs()).double()
    return (g32.double() - r32.double()).abs() / spacing


# ---------------------------------------------------------------------------------------------
# float64 references (each returns the reference and its absolute-value bound)
# ---------------------------------------------------------------------------------------------
def _per_channel(v, like):
    return v.view(1, -1, *([1] * (like.dim() - 2)))


def affine_input(x, scale=None, shift=None):
    """x * scale + shift per channel: the conv's input after a BatchNorm-affine prologue without activation."""
    if scale is None:
        return x
    return x * _per_channel(scale, x) + _per_channel(shift, x)


def conv3d_ref(x, w, bias=None, scale=None, shift=None, residual=None):
    """3x3x3 'same' convolution of affine_input(x) (+ bias, + residual).  The padding is zero AFTER the affine."""
    xin = affine_input(x, scale, shift)
    ref = F.conv3d(xin, w, bias, padding=1)
    bound = F.conv3d(xin.abs(), w.abs(), None if bias is None else bias.abs(), padding=1)
    if residual is not None:
        ref, bound = ref + residual, bound + residual.abs()
    return ref, bound


def conv3d_grads_ref(xin, w, dy):
    """Autograd of F.conv3d(xin, w, padding=1) under the upstream gradient dy: ((dx, dw, db), their bounds)."""
    def grads(a, b, c):
        a = a.clone().requires_grad_(True)
        b = b.clone().requires_grad_(True)
        bias = torch.zeros(b.shape[0], dtype=torch.float64, requires_grad=True)
        F.conv3d(a, b, bias, padding=1).backward(c)
        return a.grad, b.grad, bias.grad
    return grads(xin, w, dy), grads(xin.abs(), w.abs(), dy.abs())


def conv_transpose_ref(x, w, stride, dy):
    """F.conv_transpose3d with kernel == stride, no bias: ((y, dx, dw), their bounds)."""
    def run(a, b, c):
        a = a.clone().requires_grad_(True)
        b = b.clone().requires_grad_(True)
        y = F.conv_transpose3d(a, b, None, stride=stride)
        y.backward(c)
        return y.detach(), a.grad, b.grad
    return run(x, w, dy), run(x.abs(), w.abs(), dy.abs())


def upcat_ref(x, skip, scale, sdims, dy):
    """cat(crop(trilinear-upsample(x, align_corners=False)), skip) and its gradients: ((y, dx, dskip), their bounds)."""
    def run(a, s, c):
        a = a.clone().requires_grad_(True)
        up = F.interpolate(a, scale_factor=tuple(float(v) for v in scale), mode="trilinear", align_corners=False)
        up = up[..., :sdims[0], :sdims[1], :sdims[2]]
        if s is not None:
            s = s.clone().requires_grad_(True)
            y = torch.cat([up, s], 1)
        else:
            y = up
        y.backward(c)
        return y.detach(), a.grad, (None if s is None else s.grad)
    return run(x, skip, dy), run(x.abs(), None if skip is None else skip.abs(), dy.abs())


def matmul_tn_ref(a, b):
    """A^T B over the leading (token) axis: (ref, bound)."""
    return a.t() @ b, a.abs().t() @ b.abs()


def conv_window(xpad, b, h, w, d):
    """The 3x3x3 input window [C, 3, 3, 3] of output voxel (b, h, w, d) in a volume padded by one voxel per side."""
    return xpad[b, :, h:h + 3, w:w + 3, d:d + 3]


def taps():
    return list(itertools.product(range(3), repeat=3))
