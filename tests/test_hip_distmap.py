"""Direct parity tests of the batched signed distance maps and the boundary loss term (csrc/distmap.hip) against
tests/distmap_ref.py (float64, CPU), and of the wrappers above them.

The entry points are called through ``_lib.call`` on their own operands: every output and the workspace of exactly ``*_ws``
size sit between guard words that must come back untouched, and the outputs start as the guard pattern (a NaN), so an
element that was never written is seen as well.

Bars (tests/test_distmap_host.py shows on the CPU that f32 torch meets the loss bars on these very cases and that plausible
kernel bugs do not):
  maps, unit spacing   sign pattern equal; rint(phi^2) outside and rint((1 - phi)^2) inside are scipy's exact integers;
                       |phi - phi64| <= 2^-22 max(1, |phi64|); the two zero cases owe +0.0 in every bit
  maps, anisotropic    the squared distance recovered from phi within relative 1e-5 of scipy's, zeros in the same places
  value                2e-5 max(1, A), A = sum |p_c phi_c| / (K N) in float64
  gradient             rel-L2 < 1e-4, per element LOSS_MARGIN x E32 x max |g64|; exact zeros at invalid voxels"""
import math
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distmap_ref as R  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import losses, surface
from mivp_amd._host import i3

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
GUARD = 64                                                        # floats: 256 bytes, keeps the payload 16-byte aligned
PATTERN = 0x7FC0BEEF                                              # a quiet NaN with a payload no arithmetic produces
BOOLS = (False, True)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not torch.equal(bits(a), bits(b)):
        bad = torch.nonzero(bits(a) != bits(b))
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} elements differ in their bits; first at {first}: "
                             f"{float(a.cpu()[first])!r} != {float(b.cpu()[first])!r}")


class Guarded:
    """One f32 tensor between two guards, all filled with PATTERN; ``init`` None leaves it so (an output to be written)."""

    def __init__(self, shape, init=None):
        self.n = int(math.prod(shape))
        self.flat = torch.empty(self.n + 2 * GUARD, dtype=F32, device=DEV)
        self.flat.view(torch.int32).fill_(PATTERN)
        self.t = self.flat[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def done(self, what, written=True):
        raw = self.flat.cpu().view(torch.int32)
        guards = torch.cat([raw[:GUARD], raw[GUARD + self.n:]])
        bad = torch.nonzero(guards != PATTERN)
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} guard words were overwritten, first at guard offset {int(bad[0])}"
        if written:
            left = torch.nonzero(raw[GUARD:GUARD + self.n] == PATTERN)
            assert left.numel() == 0, f"{what}: {left.shape[0]} elements were never written, first at offset {int(left[0])}"
        return self.t.cpu().clone()


# =============================================================================================
# the maps
# =============================================================================================
def map_call(y, C, spacing, bg, ignore):
    """phi [B, K, H, W, D] on the CPU from labels y [B, H, W, D] (CPU f32), through guarded operands."""
    B, dims = y.shape[0], tuple(y.shape[1:])
    K = C - (0 if bg else 1)
    vol = math.prod(dims)
    nbytes = int(L.lib().mivp_distmap_ws(B, K, i3(dims)))
    assert nbytes == (2 * B * K * vol * 4 + 255) // 256 * 256 + 2 * B * K * vol * 8 and nbytes % 4 == 0
    ws, phi = Guarded((nbytes // 4,)), Guarded((B, K) + dims)
    yd = Guarded(tuple(y.shape), y)
    L.call("mivp_distmap_signed", L.ptr(yd.t), B, C, int(bg), 0 if ignore is None else ignore, 0 if ignore is None else 1, i3(dims),
           (L.C.c_float * 3)(*spacing), L.ptr(phi.t), L.ptr(ws.t), L.stream())
    torch.cuda.synchronize()
    ws.done("workspace", written=False)
    assert_same_bits(yd.done("labels"), y, "the labels are read only")
    return phi.done("phi")


@lru_cache(maxsize=None)
def map_case(shape, case, bg, aniso):
    R.ndi()
    B, C, dims = shape
    y = R.labels(case, B, C, dims)
    sp = R.ANISO if aniso else (1.0, 1.0, 1.0)
    return y, R.MapRef(y, C, sp, bg, R.IGNORE), map_call(y, C, sp, bg, R.IGNORE)


@pytest.mark.parametrize("bg", BOOLS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids_shape)
def test_maps_at_unit_spacing_are_integer_exact(shape, bg):
    fails = []
    for case in R.LABEL_CASES:
        y, ref, got = map_case(shape, case, bg, False)
        g = got.double().numpy()
        what = f"{R.ids_shape(shape)} {case} bg {bg}"
        assert float(ref.d2.max()) < 2 ** 15
        if not (np.array_equal(g > 0, ref.phi > 0) and np.array_equal(g < 0, ref.phi < 0)):
            fails.append(f"{what}: the sign pattern differs at {int(((g > 0) != (ref.phi > 0)).sum() + ((g < 0) != (ref.phi < 0)).sum())} voxels")
            continue
        sq = np.where(ref.inside, (1.0 - g) ** 2, g ** 2)
        live = np.broadcast_to(~ref.zero[:, :, None, None, None], g.shape)
        if not np.array_equal(np.rint(sq)[live], np.rint(ref.d2)[live]):
            fails.append(f"{what}: {int((np.rint(sq) != np.rint(ref.d2))[live].sum())} squared distances are not scipy's integers")
        err = np.abs(g - ref.phi) / np.maximum(1.0, np.abs(ref.phi))
        ulps = float((np.abs(g - ref.phi) / np.spacing(np.maximum(np.abs(ref.phi), 1e-30).astype(np.float32)).astype(np.float64)).max())
        print(f"[distmap] {what}: max error {float(err.max()):.3e} relative, {ulps:.3f} ulp")
        if not float(err.max()) <= R.MAP_BAR:
            fails.append(f"{what}: max error {float(err.max()):.3e} > 2^-22")
        zero = got[torch.from_numpy(np.broadcast_to(ref.zero[:, :, None, None, None], g.shape).copy())]
        if ref.zero.any() and not torch.equal(bits(zero), torch.zeros_like(bits(zero))):
            fails.append(f"{what}: a degenerate class's map is not +0.0 in every bit")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("bg", BOOLS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids_shape)
def test_maps_at_anisotropic_spacing(shape, bg):
    fails = []
    for case in R.LABEL_CASES:
        y, ref, got = map_case(shape, case, bg, True)
        g = got.double().numpy()
        what = f"{R.ids_shape(shape)} {case} bg {bg}"
        sq = np.where(ref.inside, (1.0 - g) ** 2, g ** 2)
        live = np.broadcast_to(~ref.zero[:, :, None, None, None], g.shape)
        err = (np.abs(sq - ref.d2) / np.maximum(ref.d2, 1e-30))[live]
        print(f"[distmap aniso] {what}: max relative error of the squared distance {float(err.max()) if err.size else 0.0:.3e}")
        if err.size and not float(err.max()) <= 1e-5:
            fails.append(f"{what}: squared distance off by {float(err.max()):.3e} relative")
        if not np.array_equal(g == 0, ref.phi == 0):
            fails.append(f"{what}: zeros in other places")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("aniso", BOOLS, ids=["unit", "aniso"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids_shape)
def test_batched_fields_are_the_single_volume_transform(shape, aniso):
    """Field (b, c) against the map assembled from two ``surface.distance_transform_sq`` calls on that sample: equal bits."""
    B, C, dims = shape
    sp = R.ANISO if aniso else (1.0, 1.0, 1.0)
    for case in ("blobs", "bad", "full"):
        y, ref, got = map_case(shape, case, True, aniso)
        for b in range(B):
            for k in range(C):
                M = torch.from_numpy(ref.inside[b, k]).to(DEV)
                d_out = surface.distance_transform_sq(M.to(torch.uint8), sp).cpu()
                d_in = surface.distance_transform_sq((~M).to(torch.uint8), sp).cpu()
                inside = ref.inside[b, k]
                d2 = np.where(inside, d_in.numpy(), d_out.numpy())
                root = np.sqrt(d2)                                 # f32, correctly rounded (a vectorised torch.sqrt need not be)
                want = np.where(np.isinf(d2), np.float32(0.0), np.where(inside, np.float32(1.0) - root, root))
                assert want.dtype == np.float32
                assert_same_bits(got[b, k], torch.from_numpy(want), f"{R.ids_shape(shape)} {case} field ({b}, {k}) {'aniso' if aniso else 'unit'}")


def test_maps_are_reproducible_and_samples_independent():
    B, C, dims = R.SHAPES[0]
    y = R.labels("bad", B, C, dims)
    a = map_call(y, C, R.ANISO, False, R.IGNORE)
    b = map_call(y, C, R.ANISO, False, R.IGNORE)
    assert_same_bits(a, b, "a second identical call")
    y2 = y.clone()
    y2[1] = R.labels("checker", B, C, dims)[1]
    c = map_call(y2, C, R.ANISO, False, R.IGNORE)
    assert_same_bits(c[0], a[0], "sample 0 after sample 1's labels changed")
    assert not torch.equal(c[1], a[1])
    y3 = torch.stack([y[1], y[0]])
    d = map_call(y3, C, R.ANISO, False, R.IGNORE)
    assert_same_bits(d[0], a[1], "sample 1 moved to slot 0")
    assert_same_bits(d[1], a[0], "sample 0 moved to slot 1")


# =============================================================================================
# the loss term
# =============================================================================================
def loss_call(z, y, phi, bg, ig, lam=1.0, weight=None, form="fused", gscale=None, onto=None):
    """(loss, dz) on the CPU.  fused: mivp_boundary_loss with dlogits; split: the value call without dlogits, then
    mivp_boundary_loss_grad on the same workspace with ``gscale`` (None: NULL).  ``onto``: dz's content, accumulate = 1."""
    B, vol, Cc = z.shape
    n_ws = int(L.lib().mivp_boundary_loss_ws(B, vol))
    assert n_ws == 2 * B * max(1, min(256, (vol + 1023) // 1024)) + 4
    ws, loss, dz = Guarded((n_ws,)), Guarded((1,)), Guarded((B, vol, Cc), onto)
    zd, yd, pd = Guarded(tuple(z.shape), z), Guarded(tuple(y.shape), y), Guarded(tuple(phi.shape), phi)
    wd = None if weight is None else torch.tensor([weight], dtype=F32, device=DEV)
    gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    acc = 0 if onto is None else 1
    ibg, ign, has = int(bg), 0 if ig is None else ig, 0 if ig is None else 1
    if form == "fused":
        assert gscale is None
        L.call("mivp_boundary_loss", L.ptr(zd.t), L.ptr(yd.t), L.ptr(pd.t), B, vol, Cc, ibg, ign, has, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(loss.t), L.ptr(dz.t), acc, L.stream())
    else:
        L.call("mivp_boundary_loss", L.ptr(zd.t), L.ptr(yd.t), L.ptr(pd.t), B, vol, Cc, ibg, ign, has, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(loss.t), None, 0, L.stream())
        L.call("mivp_boundary_loss_grad", L.ptr(zd.t), L.ptr(yd.t), L.ptr(pd.t), B, vol, Cc, ibg, ign, has, lam, L.ptr(wd),
               L.ptr(ws.t), L.ptr(gs), L.ptr(dz.t), acc, L.stream())
    torch.cuda.synchronize()
    ws.done("workspace", written=False)
    for gd, src, name in ((zd, z, "logits"), (yd, y, "labels"), (pd, phi, "phi")):
        assert_same_bits(gd.done(name), src, f"{name} are read only")
    return loss.done("loss value")[0], dz.done("dlogits")


def failures(got_loss, got_dz, ref, what, k=1.0):
    """Print the case's figures, then return the list of bars it misses (k: the incoming gradient)."""
    out = []
    want = float(ref.l64)
    if not abs(float(got_loss) - want) <= R.VALUE_BAR * max(1.0, ref.A):
        out.append(f"{what}: loss {float(got_loss)!r}, float64 {want!r} (A {ref.A:.3e})")
    if ref.zero or k == 0.0:
        if not bool(got_dz.double().abs().max() == 0):
            out.append(f"{what}: a zero gradient is owed, max |dz| {float(got_dz.abs().max()):.3e}")
        return out
    g64 = k * ref.g64
    err = float((got_dz.double() - g64).abs().max()) / (abs(k) * ref.scale)
    print(f"[boundary-ratio] {what}: E32 {ref.e32:.3e} kernel {err:.3e} ratio {err / ref.e32:.3f} bar {ref.bar_norm:.3e}")
    l2 = R.rel_l2(got_dz, g64)
    if not l2 < R.LOSS_L2_BAR:
        out.append(f"{what}: gradient rel-L2 {l2:.3e}")
    try:
        R.assert_within_located(got_dz, g64, abs(k) * ref.bar_abs, "bvc", what)
    except AssertionError as e:
        out.append(str(e))
    return out


@pytest.mark.parametrize("sat", BOOLS, ids=["randn", "pm30"])
@pytest.mark.parametrize("bg", BOOLS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids_shape)
def test_value_and_gradient(shape, bg, sat):
    """Both kernels of every shape (vol % 4 == 0: 16-byte loads; else scalar) with weight 0, 0.37 and NULL."""
    z, y, phi, ig = R.loss_case(shape, bg, sat)
    invalid = ~R.is_class(y, z.shape[-1], ig)
    assert bool(invalid.any())
    fails = []
    for w in (None, 0.37, 0.0):
        what = f"{R.ids_shape(shape)} bg {bg} {'+-30' if sat else 'randn'} weight {w}"
        ref = R.BoundaryRef(z, y, phi, bg, ig, w)
        loss, dz = loss_call(z, y, phi, bg, ig, 1.0, w)
        fails += failures(loss, dz, ref, what)
        if w != 0.0 and not torch.equal(bits(dz[invalid]), torch.zeros_like(bits(dz[invalid]))):
            fails.append(f"{what}: an invalid voxel's gradient is not +0 in every bit")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=R.ids_shape)
def test_structure(shape):
    """Everything ignored; accumulate onto a known dz; the split form with a gscale against the fused form; lambda."""
    z, y, phi, ig = R.loss_case(shape, False)
    what = R.ids_shape(shape)
    ref = R.BoundaryRef(z, y, phi, False, ig, 0.37)
    l_f, g_f = loss_call(z, y, phi, False, ig, 1.0, 0.37)
    # every voxel ignored: value 0 and a zero gradient
    l_0, g_0 = loss_call(z, torch.full_like(y, float(ig)), phi, False, ig, 1.0, None)
    assert float(l_0) == 0.0 and torch.equal(bits(g_0), torch.zeros_like(bits(g_0))), what
    # accumulate = 1: dz + g in the bits
    onto = torch.randn(z.shape, generator=R.gen(5), dtype=F32) * float(g_f.abs().max())
    l_a, g_a = loss_call(z, y, phi, False, ig, 1.0, 0.37, onto=onto)
    assert_same_bits(g_a, onto + g_f, what + ": accumulate onto a known dz, fused")
    l_s, g_s = loss_call(z, y, phi, False, ig, 1.0, 0.37, form="split", gscale=None, onto=onto)
    assert_same_bits(g_s, onto + g_f, what + ": accumulate onto a known dz, split")
    assert_same_bits(l_a.reshape(1), l_f.reshape(1), what + ": value")
    # split against fused
    for gs in (1.0, None):
        l_k, g_k = loss_call(z, y, phi, False, ig, 1.0, 0.37, form="split", gscale=gs)
        assert_same_bits(g_k, g_f, what + f": split with gscale {gs} against fused")
        assert_same_bits(l_k.reshape(1), l_f.reshape(1), what + ": value")
    fails = []
    for gs in (-2.5, 0.0):
        l_k, g_k = loss_call(z, y, phi, False, ig, 1.0, 0.37, form="split", gscale=gs)
        assert_same_bits(l_k.reshape(1), l_f.reshape(1), what + f": value, gscale {gs}")
        fails += failures(l_k, g_k, ref, what + f" gscale {gs}", gs)
    # lambda_boundary multiplies like the weight: 0.5 x 0.74 = 0.37 exactly in f32's product
    l_l, g_l = loss_call(z, y, phi, False, ig, 0.5, 0.74)
    fails += failures(l_l, g_l, R.BoundaryRef(z, y, phi, False, ig, float(np.float32(0.5) * np.float32(0.74))), what + " lambda 0.5")
    assert not fails, "\n".join(fails)


# =============================================================================================
# the wrappers
# =============================================================================================
def wrapper_case(shape, bg):
    B, C, dims = shape
    z, y, phi, ig = R.loss_case(shape, bg)
    return z, y, phi, ig, B, C, dims


@pytest.mark.parametrize("bg", BOOLS)
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=R.ids_shape)
def test_public_functions(shape, bg):
    """``signed_distance_maps`` on integer labels; ``boundary_loss`` on the kernels (maps built inside, and ``dist=``) and on the
    plain-torch path with ``dist=``, with an incoming gradient."""
    z, y, phi, ig, B, C, dims = wrapper_case(shape, bg)
    K = phi.shape[1]
    yd = y.view(B, 1, *dims).to(DEV)
    maps = losses.signed_distance_maps(yd, C, include_background=bg, ignore_index=ig)
    assert tuple(maps.shape) == (B, K) + dims and maps.dtype == F32
    assert_same_bits(maps.cpu(), map_call(y.view(B, *dims), C, (1.0, 1.0, 1.0), bg, ig), "signed_distance_maps against the entry")
    assert float(((maps.cpu().view(B, K, -1).double() - phi.double()).abs() / phi.double().abs().clamp(min=1.0)).max()) <= R.MAP_BAR
    ref = R.BoundaryRef(z, y, maps.cpu().view(B, K, -1), bg, ig, 0.37)          # the term on the maps it was given
    yi = torch.where(R.is_class(y, C, None), y, torch.full_like(y, float(ig))).view(B, *dims).long().to(DEV)
    maps_i = losses.signed_distance_maps(yi, C, include_background=bg, ignore_index=ig)        # int64 [B, H, W, D]
    assert_same_bits(maps_i, maps, "integer labels")
    w = torch.tensor([0.37], device=DEV)
    fails = []
    for dist, name in ((None, "maps inside"), (maps, "dist=")):
        base = z.view(B, *dims, C).to(DEV).requires_grad_(True)
        got = losses.boundary_loss(base.permute(0, 4, 1, 2, 3), yd, include_background=bg, ignore_index=ig, dist=dist, weight=w)
        assert "BoundaryFn" in type(got.grad_fn).__name__
        (got * 2.5).backward()
        fails += failures(got.detach().cpu(), base.grad.cpu().view(B, -1, C), ref, f"boundary_loss {name} {dims}", 2.5)
    plain = z.view(B, *dims, C).permute(0, 4, 1, 2, 3).contiguous().to(DEV).requires_grad_(True)
    got = losses.boundary_loss(plain, yd, include_background=bg, ignore_index=ig, dist=maps, weight=w)
    assert "BoundaryFn" not in type(got.grad_fn).__name__                                     # the composition, not the kernels
    (got * 0.7).backward()
    grad = plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(B, -1, C)
    fails += failures(got.detach().cpu(), grad, ref, f"boundary_loss channels-first {dims}", 0.7)
    with pytest.raises(RuntimeError, match="needs dist="):
        losses.boundary_loss(plain, yd, include_background=bg, ignore_index=ig)
    assert not fails, "\n".join(fails)


def seg_run(spec, z, y, B, C, dims, module=None, up=1.0):
    base = z.view(B, *dims, C).to(DEV).requires_grad_(True)
    yd = y.view(B, 1, *dims).to(DEV)
    got = module(base.permute(0, 4, 1, 2, 3), yd) if module is not None else losses.seg_loss(base.permute(0, 4, 1, 2, 3), yd, spec)
    (got * up).backward()
    torch.cuda.synchronize()
    return got.detach().cpu(), base.grad.cpu().view(B, -1, C)


@pytest.mark.parametrize("bg", BOOLS)
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=R.ids_shape)
def test_seg_loss_with_the_boundary_term(shape, bg):
    """seg_loss(lambda_boundary) = seg_loss without it + lambda_boundary boundary_loss in value and gradient, within the
    bars of the boundary term; the term alone; SegLoss with lambda_boundary = 0 has the bits of the path without the field."""
    z, y, phi, ig, B, C, dims = wrapper_case(shape, bg)
    opts = dict(alpha=0.3, beta=0.7, include_background=bg, focal_gamma=2.0, ignore_index=ig, class_weights=(0.5, 2.0, 1.0, 3.0)[:C])
    lam = 1.5
    l_base, g_base = seg_run(losses.SegLossSpec(**opts), z, y, B, C, dims, up=2.5)
    phi = losses.signed_distance_maps(y.view(B, 1, *dims).to(DEV), C, include_background=bg, ignore_index=ig).cpu().view(phi.shape)
    ref = R.BoundaryRef(z, y, phi, bg, ig, lam)                    # the term on the maps the call builds (tested above)
    fails = []
    for sp in (losses.SegLossSpec(lambda_boundary=lam, **opts), ):
        l_all, g_all = seg_run(sp, z, y, B, C, dims, up=2.5)
        fails += failures(l_all - l_base, g_all - g_base, ref, f"seg_loss with the term minus without {dims}", 2.5)
        mod = losses.SegLoss(sp).to(DEV)
        assert mod.boundary_weight.is_cuda
        l_mod, g_mod = seg_run(sp, z, y, B, C, dims, module=mod, up=2.5)
        assert_same_bits(l_mod.reshape(1), l_all.reshape(1), "SegLoss value")
        assert_same_bits(g_mod, g_all, "SegLoss gradient")
        mod.set_boundary_weight(2.0)
        l_two, g_two = seg_run(sp, z, y, B, C, dims, module=mod, up=2.5)
        fails += failures(l_two - l_base, g_two - g_base, R.BoundaryRef(z, y, phi, bg, ig, lam * 2.0), "boundary weight 2", 2.5)
    # (the differences carry one rounding of the sum per element on top of the boundary term's own error; the bars stay the
    # boundary term's)
    only = losses.SegLossSpec(lambda_region=0.0, lambda_voxel=0.0, lambda_boundary=lam, include_background=bg, ignore_index=ig)
    l_only, g_only = seg_run(only, z, y, B, C, dims)
    fails += failures(l_only, g_only, ref, f"the boundary term alone {dims}")
    # contiguous channels-first logits: the plain-torch composition with maps from the device
    plain = z.view(B, *dims, C).permute(0, 4, 1, 2, 3).contiguous().to(DEV).requires_grad_(True)
    got = losses.seg_loss(plain, y.view(B, 1, *dims).to(DEV), only)
    got.backward()
    fails += failures(got.detach().cpu(), plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(B, -1, C), ref, "torch path alone")
    # lambda_boundary = 0: the bits of the parent's path (the autograd function of the two-pass kernels alone)
    zero = losses.SegLossSpec(lambda_boundary=0.0, **opts)
    base = z.view(B, *dims, C).to(DEV).requires_grad_(True)
    out = losses.SegLoss(zero).to(DEV)(base.permute(0, 4, 1, 2, 3), y.view(B, 1, *dims).to(DEV))
    assert type(out.grad_fn).__name__.startswith("_SegLossFn")
    (out * 2.5).backward()
    assert_same_bits(out.detach().cpu().reshape(1), l_base.reshape(1), "lambda_boundary = 0: value")
    assert_same_bits(base.grad.cpu().view(B, -1, C), g_base, "lambda_boundary = 0: gradient")
    assert not fails, "\n".join(fails)


def test_recorded_step_follows_new_labels_and_a_new_weight():
    """A SegLoss with the boundary term, value + backward, in one graph on one stream; replays with new logits, new labels
    (class 2 disappears from sample 0) and a new boundary weight have the bits of the eager call on the same content."""
    shape = R.SHAPES[0]
    B, C, dims = shape
    z, y, phi, ig = R.loss_case(shape, False)
    spec = losses.SegLossSpec(alpha=0.3, beta=0.7, include_background=False, ignore_index=ig, lambda_boundary=0.5,
                              boundary_spacing=R.ANISO)
    mod = losses.SegLoss(spec).to(DEV)
    zs = z.view(B, *dims, C).to(DEV).requires_grad_(True)
    ys = y.view(B, 1, *dims).to(DEV).clone()

    def step():
        zs.grad = None
        loss = mod(zs.permute(0, 4, 1, 2, 3), ys)
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g = step()
        with pytest.raises(RuntimeError, match="inside a recording"):
            mod.set_boundary_weight(0.1)
    grad_g = zs.grad
    z2 = 2.0 * torch.randn(z.shape, generator=R.gen(11), dtype=F32)
    y2 = R.labels("blobs", B, C, dims, seed=9)
    y2[0][y2[0] == 2.0] = 0.0
    y2[1, 0, 0, :3] = 255.0
    assert not bool((y2[0] == 2.0).any()) and bool((y2[1] == 2.0).any())
    for zn, yn, wn in ((z, y.view(B, *dims), 1.0), (z2, y2, 0.37), (z, y2, 0.0), (z2, y.view(B, *dims), 2.0)):
        with torch.no_grad():
            zs.copy_(zn.view(B, *dims, C))
        ys.copy_(yn.view(B, 1, *dims))
        mod.set_boundary_weight(wn)
        graph.replay()
        torch.cuda.synchronize()
        got_l, got_g = loss_g.detach().cpu().clone(), grad_g.detach().cpu().clone()
        ze = zn.view(B, *dims, C).to(DEV).requires_grad_(True)
        want = mod(ze.permute(0, 4, 1, 2, 3), yn.view(B, 1, *dims).to(DEV))
        want.backward()
        assert_same_bits(got_l.reshape(1), want.detach().cpu().reshape(1), f"replayed value, weight {wn}")
        assert_same_bits(got_g, ze.grad.cpu(), f"replayed gradient, weight {wn}")
