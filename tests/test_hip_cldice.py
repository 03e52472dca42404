"""Direct parity tests of the soft-skeleton kernels and the clDice term (csrc/cldice.hip) against tests/cldice_ref.py
(numpy, CPU), and of the wrappers above them.

The entry points are called through ``_lib.call`` on their own operands: every output and the workspace of exactly ``*_ws``
size sit between guard words that must come back untouched, and they start as the guard pattern (a NaN), so an element
that was never written is seen as well.

Bars (tests/test_cldice_host.py shows on the CPU that the definition meets them and that plausible kernel bugs do not):
  skeleton forward    the bits of the float32 restatement; on the 1/16 grid with n <= 3 also those of float64
  skeleton backward   against the float64 restatement on the same f32 input: per element LOSS_MARGIN x E32 x max |g64| and
                      rel-L2 < LOSS_L2_BAR, E32 from the float32 restatement on the same case; exact zeros where they are owed
  planar p            LOSS_MARGIN x max(E32, 2^-24) against the float64 softmax, E32 from the float32 softmax; +0 at invalid voxels
  term value          LOSS_VALUE_BAR max(1, |want|), the reference taken on the kernel's own p
  term gradient       the bars of the skeleton backward; +0 in every bit at invalid voxels"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cldice_ref as R  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import losses
from mivp_amd._host import i3

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
GUARD = 64
PATTERN = 0x7FC0BEEF
NF_OF = ((1, 2), (3, 3), (3, 8))                                   # (B, C): 1, 6 and 21 fields


def ids_shape(d):
    return "x".join(str(v) for v in d)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_same_bits(a, b, what):
    ba, bb = bits(a), bits(b)
    assert ba.shape == bb.shape, what
    if not np.array_equal(ba, bb):
        bad = np.argwhere(ba != bb)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ba.size} elements differ in their bits; first at {first}: "
                             f"{float(np.asarray(ba.view(np.float32))[first])!r} != {float(np.asarray(bb.view(np.float32))[first])!r}")


class Guarded:
    """One f32 tensor between two guards, all filled with PATTERN; ``init`` None leaves it so (an output to be written)."""

    def __init__(self, shape, init=None):
        self.n = int(math.prod(shape))
        self.flat = torch.empty(self.n + 2 * GUARD, dtype=F32, device=DEV)
        self.flat.view(torch.int32).fill_(PATTERN)
        self.t = self.flat[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.t.copy_(torch.from_numpy(np.array(init, dtype=np.float32, order="C", copy=True).reshape(shape)))

    def done(self, what, written=True):
        raw = self.flat.cpu().view(torch.int32)
        guards = torch.cat([raw[:GUARD], raw[GUARD + self.n:]])
        bad = torch.nonzero(guards != PATTERN)
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} guard words were overwritten, first at guard offset {int(bad[0])}"
        if written:
            left = torch.nonzero(raw[GUARD:GUARD + self.n] == PATTERN)
            assert left.numel() == 0, f"{what}: {left.shape[0]} elements were never written, first at offset {int(left[0])}"
        return self.t.cpu().clone().numpy()


def within(got, g64, g32, what):
    """The list of gradient bars the case misses, after printing its figures."""
    got = np.asarray(got, np.float64)
    if not np.abs(g64).max() > 0:
        return [] if not np.abs(got).max() > 0 else [f"{what}: a zero gradient is owed, max |g| {np.abs(got).max():.3e}"]
    e32, scale = R.yardstick(g32, g64)
    err = np.abs(got - g64)
    worst = float(err.max()) / scale
    print(f"[cldice-ratio] {what}: E32 {e32:.3e} kernel {worst:.3e} ratio {worst / e32:.3f}")
    out = []
    if not worst <= R.LOSS_MARGIN * e32:
        at = tuple(int(i) for i in np.unravel_index(int(err.argmax()), err.shape))
        out.append(f"{what}: element {at} got {got[at]!r} want {g64[at]!r}: {worst / e32:.2f} x E32 > {R.LOSS_MARGIN}")
    l2 = R.rel_l2(got, g64)
    if not l2 < R.LOSS_L2_BAR:
        out.append(f"{what}: rel-L2 {l2:.3e}")
    return out


# =============================================================================================
# the skeleton
# =============================================================================================
def skel_call(x, n, g=None):
    """S_n (and dx when ``g`` is given) from fields x [nf, H, W, D] (numpy f32), through guarded operands."""
    nf, dims = x.shape[0], tuple(x.shape[1:])
    F = x.size
    keep = 0 if g is None else 1
    nws = int(L.lib().mivp_cldice_skeleton_ws(nf, i3(dims), n, keep))
    assert nws == (2 * n + 4 if keep else 2) * F
    xd, out, ws = Guarded(x.shape, x), Guarded(x.shape), Guarded((nws,))
    L.call("mivp_cldice_skeleton", L.ptr(xd.t), nf, i3(dims), n, L.ptr(out.t), L.ptr(ws.t), keep, L.stream())
    dx = None
    if g is not None:
        gd, dxd = Guarded(x.shape, g), Guarded(x.shape)
        L.call("mivp_cldice_skeleton_grad", L.ptr(xd.t), L.ptr(gd.t), nf, i3(dims), n, L.ptr(ws.t), L.ptr(dxd.t), L.stream())
        torch.cuda.synchronize()
        assert_same_bits(gd.done("g"), g, "the incoming gradient is read only")
        dx = dxd.done("dx")
    torch.cuda.synchronize()
    ws.done("workspace", written=False)
    assert_same_bits(xd.done("x"), x, "the input is read only")
    return out.done("skeleton"), dx


def iterations_of(dims):
    return (1, 3, 16) if dims in R.SMALL else (1, 3)


@pytest.mark.parametrize("dims", R.SHAPES, ids=ids_shape)
def test_skeleton_forward_has_the_bits_of_the_restatement(dims):
    for n in iterations_of(dims):
        for B, C in NF_OF:
            nf = B * (C - 1)
            for kind in (R.KINDS if nf <= 6 else ("noise", "grid16")):
                x = R.fields(kind, nf, dims)
                got, _ = skel_call(x, n)
                what = f"{ids_shape(dims)} nf {nf} n {n} {kind}"
                assert_same_bits(got, R.soft_skeleton(x, n), what)
                if kind == "grid16" and n <= 3:
                    assert np.array_equal(got.astype(np.float64), R.soft_skeleton(x.astype(np.float64), n)), what
                for axis in (1, 2, 3):
                    flipped, _ = skel_call(np.ascontiguousarray(np.flip(x, axis)), n)
                    assert_same_bits(np.ascontiguousarray(np.flip(flipped, axis)), got, what + f" flipped along axis {axis}")
                    if nf > 1 or kind not in ("noise", "grid16"):
                        break


@pytest.mark.parametrize("dims", R.SHAPES, ids=ids_shape)
def test_skeleton_backward(dims):
    fails = []
    for n in iterations_of(dims):
        for B, C in NF_OF[:2] if n != 3 else NF_OF:
            nf = B * (C - 1)
            for kind in R.KINDS:
                x = R.fields(kind, nf, dims)
                g = R.rng(7, nf, *dims).uniform(-1, 1, x.shape).astype(np.float32)
                s, dx = skel_call(x, n, g)
                what = f"{ids_shape(dims)} nf {nf} n {n} {kind}"
                assert_same_bits(s, R.soft_skeleton(x, n), what + ": forward with keep")
                g64 = R.soft_skeleton_bwd(x.astype(np.float64), n, g.astype(np.float64))
                if kind in ("zeros", "ones"):
                    assert not np.abs(g64).max() > 0
                    assert_same_bits(dx, np.zeros_like(x), what + ": zero gradients are owed")
                    continue
                fails += within(dx, g64, R.soft_skeleton_bwd(x, n, g), what)
    assert not fails, "\n".join(fails)


# =============================================================================================
# the term
# =============================================================================================
def term_call(z, y, dims, n, smooth, batch, ig, lam=1.0, weight=None, form="fused", gscale=None, onto=None):
    """(loss, dz [B, vol, C], planar p [B, K, H, W, D]) as numpy."""
    B, vol, C = z.shape
    K, F = C - 1, B * (C - 1) * vol
    nws = int(L.lib().mivp_cldice_ws(B, C, i3(dims), n))
    bpb = max(1, min(256, (vol + 1023) // 1024))
    assert nws == (2 * n + 7) * F + B * K * (4 * bpb + 4 + 3)
    ws, loss, dz = Guarded((nws,)), Guarded((1,)), Guarded((B, vol, C), onto)
    zd, yd = Guarded(z.shape, z), Guarded(y.shape, y)
    wd = None if weight is None else torch.tensor([weight], dtype=F32, device=DEV)
    gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    acc = 0 if onto is None else 1
    d3, ibt, ign, has = i3(dims), int(batch), 0 if ig is None else ig, 0 if ig is None else 1
    if form == "fused":
        L.call("mivp_cldice_loss", L.ptr(zd.t), L.ptr(yd.t), B, C, d3, n, smooth, ibt, ign, has, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(loss.t), L.ptr(dz.t), acc, L.stream())
    else:
        L.call("mivp_cldice_loss", L.ptr(zd.t), L.ptr(yd.t), B, C, d3, n, smooth, ibt, ign, has, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(loss.t), None, 0, L.stream())
        L.call("mivp_cldice_loss_grad", L.ptr(zd.t), L.ptr(yd.t), B, C, d3, n, smooth, ibt, ign, has, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(gs), L.ptr(dz.t), acc, L.stream())
    torch.cuda.synchronize()
    raw = ws.done("workspace", written=False)
    assert_same_bits(zd.done("logits"), z, "logits are read only")
    assert_same_bits(yd.done("labels"), y, "labels are read only")
    return float(loss.done("loss value")[0]), dz.done("dlogits"), raw[:F].reshape(B, K, *dims).copy()


def term_failures(z, y, dims, n, smooth, batch, ig, got, what, need_share=False, kernels=True):
    loss, dz, p = got
    B, vol, C = z.shape
    fails = []
    valid = R.valid_mask(y, C, ig)
    p64 = R.planar(R.softmax(z.astype(np.float64)) * valid[..., None], dims)
    p32 = R.planar(R.softmax(z) * valid[..., None].astype(np.float32), dims)
    ep = max(float(np.abs(p32.astype(np.float64) - p64).max()), R.U32)
    perr = float(np.abs(p.astype(np.float64) - p64).max())
    print(f"[cldice-p] {what}: E32 {ep:.3e} kernel {perr:.3e} ratio {perr / ep:.3f}")
    if not perr <= R.LOSS_MARGIN * ep:
        fails.append(f"{what}: planar p off by {perr:.3e} > {R.LOSS_MARGIN} x {ep:.3e}")
    pv = np.moveaxis(p.reshape(B, C - 1, vol), 1, -1)
    if not np.array_equal(bits(pv[~valid]), np.zeros_like(bits(pv[~valid]))):
        fails.append(f"{what}: planar p is not +0 at an invalid voxel")
    want, g64, _ = R.term(z, y, dims, n, smooth, batch, ig, np.float64, p)
    _, g32, _ = R.term(z, y, dims, n, smooth, batch, ig, np.float32, p)
    if not abs(loss - want) <= R.LOSS_VALUE_BAR * max(1.0, abs(want)):
        fails.append(f"{what}: loss {loss!r}, float64 {want!r}")
    if need_share:
        share = float((np.abs(g64).max(-1) > 0)[valid].mean())
        print(f"[cldice-share] {what}: {share:.3f} of the valid voxels have a non-zero reference gradient")
        assert share >= 0.5, what
    if kernels and not np.array_equal(bits(dz[~valid]), np.zeros_like(bits(dz[~valid]))):
        fails.append(f"{what}: an invalid voxel's gradient is not +0 in every bit")
    if np.abs(dz[~valid]).max(initial=0.0) != 0:                   # (autograd's zeros through a product with 0 may be -0)
        fails.append(f"{what}: an invalid voxel's gradient is not zero")
    return fails + within(dz, g64, g32, what)


TERM_CONFIGS = ((1, 2, 255, False), (3, 3, -1, True), (3, 8, None, False), (3, 3, 255, False))


@pytest.mark.parametrize("config", TERM_CONFIGS, ids=lambda c: f"B{c[0]}-C{c[1]}-ig{c[2]}-batch{int(c[3])}")
@pytest.mark.parametrize("dims", R.SHAPES, ids=ids_shape)
def test_term_value_and_gradient(dims, config):
    B, C, ig, batch = config
    fails = []
    for n in (1, 3):
        for kind in ("noise", "tube", "pm30", "grid16"):
            if n == 1 and kind in ("pm30", "grid16"):
                continue
            z, y = R.term_case(kind, B, C, dims, ig)
            invalid = ~R.valid_mask(y, C, ig)
            assert bool(invalid.any()) or math.prod(dims) < 16
            what = f"{ids_shape(dims)} B {B} C {C} ig {ig} batch {batch} n {n} {kind}"
            got = term_call(z, y, dims, n, 1.0, batch, ig)
            share = kind in ("noise", "tube") and math.prod(dims) >= 300 and n == 3 and C <= 3
            fails += term_failures(z, y, dims, n, 1.0, batch, ig, got, what, need_share=share)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dims", ((5, 7, 9), (6, 7, 8)), ids=ids_shape)
def test_term_structure(dims):
    """Weight and lambda, the split form with a gscale, accumulate onto a known dz, everything ignored, a second run."""
    B, C, ig, n = 3, 3, 255, 3
    z, y = R.term_case("noise", B, C, dims, ig)
    what = ids_shape(dims)
    l_f, g_f, p_f = term_call(z, y, dims, n, 0.5, False, ig, 1.0, 0.37)
    l_1, g_1, _ = term_call(z, y, dims, n, 0.5, False, ig)
    fails = term_failures(z, y, dims, n, 0.5, False, ig, (l_1, g_1, p_f), what + " smooth 0.5")
    assert abs(l_f - 0.37 * l_1) <= 4e-7 * abs(l_1)                 # three roundings: f32(0.37) and both values
    fails += within(g_f, 0.37 * g_1.astype(np.float64), np.float32(0.37) * g_1, what + " weight 0.37 against weight 1")
    l_2, g_2, _ = term_call(z, y, dims, n, 0.5, False, ig, 1.0, 0.37)
    assert l_2 == l_f
    assert_same_bits(g_2, g_f, what + ": a second identical call")
    l_l, g_l, _ = term_call(z, y, dims, n, 0.5, False, ig, 0.5, 0.74)                  # 0.5 x 0.74 = 0.37 exactly in f32
    assert_same_bits(g_l, g_f, what + ": lambda 0.5 x weight 0.74")
    for gs in (None, 1.0):
        l_s, g_s, _ = term_call(z, y, dims, n, 0.5, False, ig, 1.0, 0.37, form="split", gscale=gs)
        assert l_s == l_f
        assert_same_bits(g_s, g_f, what + f": split form, gscale {gs}")
    l_k, g_k, _ = term_call(z, y, dims, n, 0.5, False, ig, 1.0, None, form="split", gscale=-2.5)
    fails += within(g_k, -2.5 * g_1.astype(np.float64), np.float32(-2.5) * g_1, what + " gscale -2.5")
    onto = (R.rng(9).standard_normal(z.shape) * float(np.abs(g_f).max())).astype(np.float32)
    for form in ("fused", "split"):
        l_a, g_a, _ = term_call(z, y, dims, n, 0.5, False, ig, 1.0, 0.37, form=form, onto=onto)
        assert l_a == l_f
        assert_same_bits(g_a, onto + g_f, what + f": accumulate onto a known dz, {form}")
    l_0, g_0, p_0 = term_call(z, np.full_like(y, float(ig)), dims, n, 0.5, False, ig)
    assert abs(l_0) <= 1e-7 and not g_0.any() and not p_0.any()    # Tprec = Tsens = s / s: cl = 0
    assert not fails, "\n".join(fails)


# =============================================================================================
# the wrappers
# =============================================================================================
@pytest.mark.parametrize("dims", ((5, 7, 9), (11, 10, 21)), ids=ids_shape)
def test_soft_skeleton_wrapper(dims):
    x = R.fields("tube", 6, dims).reshape(2, 3, *dims)
    g = R.rng(8).uniform(-1, 1, x.shape).astype(np.float32)
    want_s, want_g = skel_call(x.reshape(6, *dims), 3, g.reshape(6, *dims))
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = losses.soft_skeleton(xt, 3)
    assert "SkeletonFn" in type(out.grad_fn).__name__
    out.backward(torch.from_numpy(g).to(DEV), retain_graph=True)
    assert_same_bits(out, want_s.reshape(x.shape), "soft_skeleton against the entry")
    assert_same_bits(xt.grad, want_g.reshape(x.shape), "its gradient against the entry")
    with pytest.raises(RuntimeError, match="second backward"):
        out.backward(torch.from_numpy(g).to(DEV))
    assert_same_bits(losses.soft_skeleton(xt.detach(), 3), want_s.reshape(x.shape), "without a gradient: two fields of workspace")
    # any other layout takes the plain-torch composition: the same bits forward, the share-equally gradient
    xs = torch.from_numpy(x).to(DEV).transpose(3, 4).contiguous().transpose(3, 4).requires_grad_(True)
    out = losses.soft_skeleton(xs, 3)
    assert "SkeletonFn" not in type(out.grad_fn).__name__
    out.backward(torch.from_numpy(g).to(DEV))
    assert_same_bits(out, want_s.reshape(x.shape), "the torch composition on the GPU")
    g64 = R.soft_skeleton_bwd(x.astype(np.float64), 3, g.astype(np.float64))
    fails = within(xs.grad.cpu().numpy(), g64, R.soft_skeleton_bwd(x, 3, g), "torch composition gradient")
    assert not fails, "\n".join(fails)


def seg_run(spec, z, y, B, C, dims, module=None, up=1.0, **kw):
    base = torch.from_numpy(z).view(B, *dims, C).to(DEV).requires_grad_(True)
    yd = torch.from_numpy(y).view(B, 1, *dims).to(DEV)
    logits = base.permute(0, 4, 1, 2, 3)
    got = module(logits, yd) if module is not None else (spec(logits, yd) if callable(spec) else losses.seg_loss(logits, yd, spec, **kw))
    (got * up).backward()
    torch.cuda.synchronize()
    return got.detach().cpu().numpy().astype(np.float32).reshape(1), base.grad.cpu().numpy().reshape(B, -1, C), got


@pytest.mark.parametrize("batch", (False, True))
@pytest.mark.parametrize("dims", ((5, 7, 9), (6, 7, 8)), ids=ids_shape)
def test_wrappers_add_the_term(dims, batch):
    B, C, ig, n, lam = 3, 3, 255, 2, 1.5
    z, y = R.term_case("tube", B, C, dims, ig)
    want_l, want_g, _ = term_call(z, y, dims, n, 0.5, batch, ig)
    l_c, g_c, out = seg_run(lambda lg, yd: losses.cldice_loss(lg, yd, iterations=n, smooth=0.5, batch=batch, ignore_index=ig),
                            z, y, B, C, dims)
    assert "ClDiceFn" in type(out.grad_fn).__name__
    assert float(l_c[0]) == want_l
    assert_same_bits(g_c, want_g, "cldice_loss against the entry")
    yi = torch.from_numpy(np.where(R.valid_mask(y, C, None), y, float(ig))).view(B, *dims).long().to(DEV)
    zt = torch.from_numpy(z).view(B, *dims, C).to(DEV)
    l_i = losses.cldice_loss(zt.permute(0, 4, 1, 2, 3), yi, iterations=n, smooth=0.5, batch=batch, ignore_index=ig)
    _, _, p = term_call(z, np.where(R.valid_mask(y, C, None), y, float(ig)).astype(np.float32), dims, n, 0.5, batch, ig)
    ref_i, _, _ = R.term(z, np.where(R.valid_mask(y, C, None), y, float(ig)), dims, n, 0.5, batch, ig, np.float64, p)
    assert abs(float(l_i) - ref_i) <= R.LOSS_VALUE_BAR
    # channels-first logits: the plain-torch composition
    plain = torch.from_numpy(z).view(B, *dims, C).permute(0, 4, 1, 2, 3).contiguous().to(DEV).requires_grad_(True)
    got = losses.cldice_loss(plain, torch.from_numpy(y).view(B, 1, *dims).to(DEV), iterations=n, smooth=0.5, batch=batch,
                             ignore_index=ig)
    assert "ClDiceFn" not in type(got.grad_fn).__name__
    got.backward()
    fails = term_failures(z, y, dims, n, 0.5, batch, ig,
                          (float(got.detach()), plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(B, -1, C).numpy(), p_of(z, y, dims, n, batch, ig)),
                          f"torch path {dims}", kernels=False)
    # seg_loss: the sum of the separately computed terms, with an incoming gradient
    opts = dict(alpha=0.3, beta=0.7, batch=batch, include_background=False, focal_gamma=2.0, ignore_index=ig,
                class_weights=(0.5, 2.0, 1.0))
    cl = dict(lambda_cldice=lam, cldice_iterations=n, cldice_smooth=0.5)
    l_base, g_base, out = seg_run(losses.SegLossSpec(**opts), z, y, B, C, dims, up=2.5)
    assert type(out.grad_fn).__name__.startswith("_SegLossFn")
    l_bd, g_bd, _ = seg_run(losses.SegLossSpec(lambda_boundary=0.5, **opts), z, y, B, C, dims, up=2.5)
    scale = 2.5 * lam
    for name, spec, l_rest, g_rest in (
            ("region + voxel + clDice", losses.SegLossSpec(**opts, **cl), l_base, g_base),
            ("region + voxel + boundary + clDice", losses.SegLossSpec(lambda_boundary=0.5, **opts, **cl), l_bd, g_bd),
            ("clDice alone", losses.SegLossSpec(lambda_region=0.0, lambda_voxel=0.0, batch=batch, ignore_index=ig, **cl), 0.0, 0.0)):
        l_all, g_all, out = seg_run(spec, z, y, B, C, dims, up=2.5)
        assert "SegTermsFn" in type(out.grad_fn).__name__
        total = float(l_rest if np.isscalar(l_rest) else l_rest[0]) + lam * want_l
        assert abs(float(l_all[0]) - total) <= R.LOSS_VALUE_BAR * max(1.0, abs(total)), name
        # the yardstick is the f32 sum of the two gradients minus the rest: it carries the one rounding of the add
        diff = g_all.astype(np.float64) - g_rest
        fails += within(diff, scale * want_g.astype(np.float64), (np.float32(scale) * want_g + np.float32(g_rest)).astype(np.float64) - g_rest,
                        f"seg_loss {name} minus the rest {dims}")
        mod = losses.SegLoss(spec).to(DEV)
        l_m, g_m, _ = seg_run(spec, z, y, B, C, dims, module=mod, up=2.5)
        assert_same_bits(l_m, l_all, name + ": SegLoss value")
        assert_same_bits(g_m, g_all, name + ": SegLoss gradient")
        mod.set_cldice_weight(2.0)
        l_w, g_w, _ = seg_run(spec, z, y, B, C, dims, module=mod, up=2.5)
        fails += within(g_w.astype(np.float64) - g_rest, 2.0 * scale * want_g.astype(np.float64),
                        (np.float32(2.0 * scale) * want_g + np.float32(g_rest)).astype(np.float64) - g_rest,
                        f"seg_loss {name}, cldice weight 2")
    # lambda_cldice = 0: the bits of the path without the field
    out_l, out_g, out = seg_run(None, z, y, B, C, dims, module=losses.SegLoss(losses.SegLossSpec(lambda_cldice=0.0, **opts)).to(DEV), up=2.5)
    assert type(out.grad_fn).__name__.startswith("_SegLossFn")
    assert_same_bits(out_l, l_base, "lambda_cldice = 0: value")
    assert_same_bits(out_g, g_base, "lambda_cldice = 0: gradient")
    assert not fails, "\n".join(fails)


def p_of(z, y, dims, n, batch, ig):
    return term_call(z, y, dims, n, 0.5, batch, ig)[2]


def test_recorded_step_follows_new_operands_and_a_new_weight():
    """A SegLoss with region + voxel + boundary + clDice, value + backward, in one graph; replays with new logits, labels
    and clDice weight have the bits of the eager call on the same content."""
    B, C, dims, ig = 3, 3, (6, 7, 8), 255
    z, y = R.term_case("tube", B, C, dims, ig)
    z2, y2 = R.term_case("noise", B, C, dims, ig, seed=3)
    spec = losses.SegLossSpec(alpha=0.3, beta=0.7, include_background=False, ignore_index=ig, lambda_boundary=0.5,
                              lambda_cldice=0.75, cldice_iterations=3)
    mod = losses.SegLoss(spec).to(DEV)
    zs = torch.from_numpy(z).view(B, *dims, C).to(DEV).requires_grad_(True)
    ys = torch.from_numpy(y).view(B, 1, *dims).to(DEV).clone()

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
            mod.set_cldice_weight(0.1)
    grad_g = zs.grad
    for zn, yn, wn in ((z, y, 1.0), (z2, y2, 0.37), (z, y2, 0.0), (z2, y, 2.0)):
        with torch.no_grad():
            zs.copy_(torch.from_numpy(zn).view(B, *dims, C))
        ys.copy_(torch.from_numpy(yn).view(B, 1, *dims))
        mod.set_cldice_weight(wn)
        graph.replay()
        torch.cuda.synchronize()
        got_l, got_g = loss_g.detach().cpu().clone().reshape(1), grad_g.detach().cpu().clone()
        ze = torch.from_numpy(zn).view(B, *dims, C).to(DEV).requires_grad_(True)
        want = mod(ze.permute(0, 4, 1, 2, 3), torch.from_numpy(yn).view(B, 1, *dims).to(DEV))
        want.backward()
        assert_same_bits(got_l, want.detach().cpu().reshape(1), f"replayed value, weight {wn}")
        assert_same_bits(got_g, ze.grad.cpu(), f"replayed gradient, weight {wn}")
