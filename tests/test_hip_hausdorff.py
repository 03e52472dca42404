"""Direct parity tests of the Hausdorff distance-transform term (csrc/hausdorff.hip): the weight maps and the value /
gradient passes against tests/hausdorff_ref.py (float64, CPU), and of the wrappers above them.

The entry points are called through ``_lib.call`` on their own operands: every output and the workspace of exactly ``*_ws``
size sit between guard words that must come back untouched, and the outputs start as the guard pattern (a NaN), so an
element that was never written is seen as well (the helpers of tests/test_hip_distmap.py).

Bars (tests/test_hausdorff_host.py shows on the CPU that f32 meets them on these very cases and that plausible kernel bugs do
not):
  maps, unit spacing, alpha 2   equal bits with the integer reference; the four squared fields in the workspace equal bits with
                                surface.distance_transform_sq of the same masks (+inf where a side has no voxel)
  maps, other spacing / alpha   LOSS_MARGIN x E32 x max |Wm64| per element, E32 from the f32 numpy run of the same formula
  value                         VALUE_BAR max(1, A), A = the float64 value without its weight
  gradient                      rel-L2 < 1e-4, per element LOSS_MARGIN x E32 x max |g64|; +0 in every bit at invalid voxels

Measured on an MI355X (kernel error / E32, the bar is 8): the numbers are in DESIGN 5.12."""
import math
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hausdorff_ref as R  # noqa: E402
from test_hip_distmap import DEV, Guarded, assert_same_bits, bits  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import losses, surface
from mivp_amd._host import i3

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BOOLS = (False, True)
# every label case of distmap_ref with a kind of logits: all three kinds meet the degenerate cases absent / full
MAP_CASES = tuple((case, R.LOGIT_KINDS[i % 3]) for i, case in enumerate(R.LABEL_CASES)) + (("full", "randn"), ("absent", "pm30"))


# =============================================================================================
# the maps
# =============================================================================================
def map_call(z, y, spacing, bg, ignore, alpha=2.0):
    """(wmap [B, K, H, W, D], fields [2, 2, B, K, H, W, D]) on the CPU from logits z [B, vol, C] and labels y [B, H, W, D]
    (CPU f32), through guarded operands."""
    B, dims, C = y.shape[0], tuple(y.shape[1:]), z.shape[-1]
    K = C - (0 if bg else 1)
    vol = math.prod(dims)
    nbytes = int(L.lib().mivp_hausdorff_maps_ws(B, K, i3(dims)))
    assert nbytes == (4 * B * K * vol * 4 + 255) // 256 * 256 + 4 * B * K * vol * 8 and nbytes % 4 == 0
    ws, wmap = Guarded((nbytes // 4,)), Guarded((B, K) + dims)
    zd, yd = Guarded(tuple(z.shape), z), Guarded(tuple(y.shape), y)
    L.call("mivp_hausdorff_maps", L.ptr(zd.t), L.ptr(yd.t), B, C, int(bg), 0 if ignore is None else ignore,
           0 if ignore is None else 1, i3(dims), (L.C.c_float * 3)(*spacing), alpha, L.ptr(wmap.t), L.ptr(ws.t), L.stream())
    torch.cuda.synchronize()
    raw = ws.done("workspace", written=False)
    assert_same_bits(yd.done("labels"), y, "the labels are read only")
    assert_same_bits(zd.done("logits"), z, "the logits are read only")
    return wmap.done("wmap"), raw[:4 * B * K * vol].view((2, 2, B, K) + dims)


@lru_cache(maxsize=None)
def map_inputs(shape, case, kind):
    B, C, dims = shape
    return R.logits(kind, B, math.prod(dims), C), R.labels(case, B, C, dims)


@lru_cache(maxsize=None)
def map_ref(shape, case, kind, bg, aniso):
    R.ndi()
    z, y = map_inputs(shape, case, kind)
    return R.MapRef(z, y, R.ANISO32 if aniso else R.UNIT, bg, R.IGNORE)


@pytest.mark.parametrize("bg", BOOLS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids_shape)
def test_maps_at_unit_spacing_and_alpha_2_are_the_integers(shape, bg):
    B, C, dims = shape
    for case, kind in MAP_CASES:
        z, y = map_inputs(shape, case, kind)
        ref = map_ref(shape, case, kind, bg, False)
        got, fields = map_call(z, y, R.UNIT, bg, R.IGNORE)
        what = f"{R.ids_shape(shape)} {case} {kind} bg {bg}"
        want = ref.wm(2.0)
        assert float(want.max()) < 2 ** 24
        assert_same_bits(got, torch.from_numpy(want.astype(np.float32)), what + ": wmap")
        if not bg or (case, kind) not in MAP_CASES[:3] + MAP_CASES[-2:]:
            continue
        # the squared fields behind it: those of the single-volume transform on the same seeds
        for src, masks in enumerate((ref.P, ref.G)):
            for b in range(B):
                for k in range(C):
                    M = torch.from_numpy(masks[b, k]).to(DEV)
                    for side, seeds in enumerate((M, ~M)):
                        single = surface.distance_transform_sq(seeds.to(torch.uint8), R.UNIT).cpu()
                        assert_same_bits(fields[src, side, b, k], single, f"{what}: field source {src} side {side} ({b}, {k})")


@pytest.mark.parametrize("bg", BOOLS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids_shape)
def test_maps_at_anisotropic_spacing_and_other_alpha(shape, bg):
    fails = []
    for aniso, alpha in ((True, 2.0), (False, 1.0), (False, 3.0), (True, 1.0), (True, 3.0)):
        worst = 0.0
        for case, kind in MAP_CASES:
            z, y = map_inputs(shape, case, kind)
            ref = map_ref(shape, case, kind, bg, aniso)
            got, _ = map_call(z, y, R.ANISO32 if aniso else R.UNIT, bg, R.IGNORE, alpha)
            want = ref.wm(alpha)
            bar, e32 = R.map_bar(want, ref.wm(alpha, np.float32))
            what = f"{R.ids_shape(shape)} {case} {kind} bg {bg} {'aniso' if aniso else 'unit'} alpha {alpha}"
            if not np.array_equal(got.numpy() == 0, want == 0):
                fails.append(f"{what}: zeros in other places")
            scale = float(np.abs(want).max())
            if scale > 0:
                worst = max(worst, float(np.abs(got.double().numpy() - want).max()) / scale / e32)
            try:
                R.assert_within_located(got, torch.from_numpy(want), bar, "bkhwd", what)
            except AssertionError as e:
                fails.append(str(e))
        print(f"[hausdorff-maps-ratio] {R.ids_shape(shape)} bg {bg} {'aniso' if aniso else 'unit'} alpha {alpha}: "
              f"worst kernel / E32 {worst:.3f} (bar {R.LOSS_MARGIN})")
    assert not fails, "\n".join(fails)


def test_maps_are_reproducible_and_samples_independent():
    B, C, dims = R.SHAPES[0]
    z, y = map_inputs(R.SHAPES[0], "bad", "randn")
    a, fa = map_call(z, y, R.ANISO32, False, R.IGNORE, 3.0)
    b, fb = map_call(z, y, R.ANISO32, False, R.IGNORE, 3.0)
    assert_same_bits(a, b, "a second identical call")
    assert_same_bits(fa, fb, "a second identical call: fields")
    z2, y2 = z.clone(), y.clone()
    z2[1], y2[1] = R.logits("ties", B, z.shape[1], C)[1], R.labels("checker", B, C, dims)[1]
    c, _ = map_call(z2, y2, R.ANISO32, False, R.IGNORE, 3.0)
    assert_same_bits(c[0], a[0], "sample 0 after sample 1 changed")
    assert not torch.equal(c[1], a[1])
    d, _ = map_call(torch.stack([z[1], z[0]]), torch.stack([y[1], y[0]]), R.ANISO32, False, R.IGNORE, 3.0)
    assert_same_bits(d[0], a[1], "sample 1 moved to slot 0")
    assert_same_bits(d[1], a[0], "sample 0 moved to slot 1")


# =============================================================================================
# the loss term
# =============================================================================================
def loss_call(z, y, wmap, bg, ig, lam=1.0, weight=None, form="fused", gscale=None, onto=None):
    """(loss, dz) on the CPU.  fused: mivp_hausdorff_loss with dlogits; split: the value call without dlogits, then
    mivp_hausdorff_loss_grad on the same workspace with ``gscale`` (None: NULL).  ``onto``: dz's content, accumulate = 1."""
    B, vol, Cc = z.shape
    n_ws = int(L.lib().mivp_hausdorff_loss_ws(B, vol))
    assert n_ws == 2 * B * max(1, min(256, (vol + 1023) // 1024)) + 4
    ws, loss, dz = Guarded((n_ws,)), Guarded((1,)), Guarded((B, vol, Cc), onto)
    zd, yd, pd = Guarded(tuple(z.shape), z), Guarded(tuple(y.shape), y), Guarded(tuple(wmap.shape), wmap)
    wd = None if weight is None else torch.tensor([weight], dtype=F32, device=DEV)
    gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    acc = 0 if onto is None else 1
    ibg, ign, has = int(bg), 0 if ig is None else ig, 0 if ig is None else 1
    if form == "fused":
        assert gscale is None
        L.call("mivp_hausdorff_loss", L.ptr(zd.t), L.ptr(yd.t), L.ptr(pd.t), B, vol, Cc, ibg, ign, has, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(loss.t), L.ptr(dz.t), acc, L.stream())
    else:
        L.call("mivp_hausdorff_loss", L.ptr(zd.t), L.ptr(yd.t), L.ptr(pd.t), B, vol, Cc, ibg, ign, has, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(loss.t), None, 0, L.stream())
        L.call("mivp_hausdorff_loss_grad", L.ptr(zd.t), L.ptr(yd.t), L.ptr(pd.t), B, vol, Cc, ibg, ign, has, lam, L.ptr(wd),
               L.ptr(ws.t), L.ptr(gs), L.ptr(dz.t), acc, L.stream())
    torch.cuda.synchronize()
    ws.done("workspace", written=False)
    for gd, src, name in ((zd, z, "logits"), (yd, y, "labels"), (pd, wmap, "wmap")):
        assert_same_bits(gd.done(name), src, f"{name} are read only")
    return loss.done("loss value")[0], dz.done("dlogits")


def failures(got_loss, got_dz, ref, what, k=1.0):
    """Print the case's figures, then return the list of bars it misses (k: the incoming gradient)."""
    out = []
    want = float(ref.l64)
    print(f"[hausdorff-value] {what}: loss {float(got_loss)!r} float64 {want!r} off {abs(float(got_loss) - want):.3e} "
          f"bar {R.VALUE_BAR * max(1.0, ref.A):.3e}")
    if not abs(float(got_loss) - want) <= R.VALUE_BAR * max(1.0, ref.A):
        out.append(f"{what}: loss {float(got_loss)!r}, float64 {want!r} (A {ref.A:.3e})")
    if ref.zero or k == 0.0:
        if not bool(got_dz.double().abs().max() == 0):
            out.append(f"{what}: a zero gradient is owed, max |dz| {float(got_dz.abs().max()):.3e}")
        return out
    g64 = k * ref.g64
    err = float((got_dz.double() - g64).abs().max()) / (abs(k) * ref.scale)
    print(f"[hausdorff-ratio] {what}: E32 {ref.e32:.3e} kernel {err:.3e} ratio {err / ref.e32:.3f} bar {ref.bar_norm:.3e}")
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
    R.ndi()
    z, y, wmap, ig = R.loss_case(shape, bg, sat)
    invalid = ~R.is_class(y, z.shape[-1], ig)
    assert bool(invalid.any())
    fails = []
    for w in (None, 0.37, 0.0):
        what = f"{R.ids_shape(shape)} bg {bg} {'+-30' if sat else 'randn'} weight {w}"
        ref = R.HdRef(z, y, wmap, bg, ig, w)
        loss, dz = loss_call(z, y, wmap, bg, ig, 1.0, w)
        fails += failures(loss, dz, ref, what)
        if w != 0.0 and not torch.equal(bits(dz[invalid]), torch.zeros_like(bits(dz[invalid]))):
            fails.append(f"{what}: an invalid voxel's gradient is not +0 in every bit")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=R.ids_shape)
def test_structure(shape):
    """Everything ignored; accumulate onto a known dz; the split form with a gscale against the fused form; lambda; equal
    calls; a sample's gradient pattern without its batch neighbours."""
    R.ndi()
    z, y, wmap, ig = R.loss_case(shape, False)
    what = R.ids_shape(shape)
    ref = R.HdRef(z, y, wmap, False, ig, 0.37)
    l_f, g_f = loss_call(z, y, wmap, False, ig, 1.0, 0.37)
    l_r, g_r = loss_call(z, y, wmap, False, ig, 1.0, 0.37)
    assert_same_bits(g_r, g_f, what + ": a second identical call")
    assert_same_bits(l_r.reshape(1), l_f.reshape(1), what + ": a second identical call, value")
    # every voxel ignored: value 0 and a zero gradient
    l_0, g_0 = loss_call(z, torch.full_like(y, float(ig)), wmap, False, ig, 1.0, None)
    assert float(l_0) == 0.0 and torch.equal(bits(g_0), torch.zeros_like(bits(g_0))), what
    # accumulate = 1: dz + g in the bits
    onto = torch.randn(z.shape, generator=R.gen(5), dtype=F32) * float(g_f.abs().max())
    l_a, g_a = loss_call(z, y, wmap, False, ig, 1.0, 0.37, onto=onto)
    assert_same_bits(g_a, onto + g_f, what + ": accumulate onto a known dz, fused")
    l_s, g_s = loss_call(z, y, wmap, False, ig, 1.0, 0.37, form="split", gscale=None, onto=onto)
    assert_same_bits(g_s, onto + g_f, what + ": accumulate onto a known dz, split")
    assert_same_bits(l_a.reshape(1), l_f.reshape(1), what + ": value")
    # split against fused
    for gs in (1.0, None):
        l_k, g_k = loss_call(z, y, wmap, False, ig, 1.0, 0.37, form="split", gscale=gs)
        assert_same_bits(g_k, g_f, what + f": split with gscale {gs} against fused")
        assert_same_bits(l_k.reshape(1), l_f.reshape(1), what + ": value")
    fails = []
    for gs in (-2.5, 0.0):
        l_k, g_k = loss_call(z, y, wmap, False, ig, 1.0, 0.37, form="split", gscale=gs)
        assert_same_bits(l_k.reshape(1), l_f.reshape(1), what + f": value, gscale {gs}")
        fails += failures(l_k, g_k, ref, what + f" gscale {gs}", gs)
    # lambda_hausdorff multiplies like the weight: 0.5 x 0.74 = 0.37 exactly in f32's product
    l_l, g_l = loss_call(z, y, wmap, False, ig, 0.5, 0.74)
    fails += failures(l_l, g_l, R.HdRef(z, y, wmap, False, ig, float(np.float32(0.5) * np.float32(0.74))), what + " lambda 0.5")
    # a sample alone: N is the batch's, so sample 0's gradient alone is the batched one times N / N_0 -- within the bars
    if z.shape[0] > 1:
        n_all, n_0 = float(R.is_class(y, z.shape[-1], ig).sum()), float(R.is_class(y[:1], z.shape[-1], ig).sum())
        l_1, g_1 = loss_call(z[:1].contiguous(), y[:1].contiguous(), wmap[:1].contiguous(), False, ig, 1.0, 0.37)
        one = R.HdRef(z[:1], y[:1], wmap[:1], False, ig, 0.37)
        fails += failures(l_1, g_1, one, what + " sample 0 alone")
        assert float((g_1.double() * (n_0 / n_all) - g_f[:1].double()).abs().max()) <= 2 * ref.bar_abs
    assert not fails, "\n".join(fails)


# =============================================================================================
# the wrappers
# =============================================================================================
def seg_run(fn, z, y, B, C, dims, up=1.0):
    base = z.view(B, *dims, C).to(DEV).requires_grad_(True)
    yd = y.view(B, 1, *dims).to(DEV)
    got = fn(base.permute(0, 4, 1, 2, 3), yd)
    (got * up).backward()
    torch.cuda.synchronize()
    return got.detach().cpu(), base.grad.cpu().view(B, -1, C)


@pytest.mark.parametrize("bg", BOOLS)
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2]], ids=R.ids_shape)
def test_public_functions(shape, bg):
    """``hausdorff_weight_maps`` on the device against the entry and the CPU restatement; ``hausdorff_dt_loss`` on the kernels
    (maps built inside, and ``maps=``) and on the plain-torch path, against the reference and the CPU composition;
    ``HausdorffDTLoss(base=SegLoss(...))`` = the base + the term."""
    R.ndi()
    B, C, dims = shape
    z, y, wmap, ig = R.loss_case(shape, bg)
    K = wmap.shape[1]
    opts = dict(include_background=bg, ignore_index=ig)
    zc, yc = z.view(B, *dims, C).permute(0, 4, 1, 2, 3), y.view(B, 1, *dims)
    maps = losses.hausdorff_weight_maps(zc.to(DEV), yc.to(DEV), **opts)
    assert tuple(maps.shape) == (B, K) + dims and maps.dtype == F32
    assert_same_bits(maps.cpu(), map_call(z, y.view(B, *dims), R.UNIT, bg, ig)[0], "hausdorff_weight_maps against the entry")
    assert_same_bits(maps.cpu(), losses.hausdorff_weight_maps(zc, yc, **opts), "the device maps against the CPU restatement")
    assert_same_bits(maps.cpu().view(B, K, -1), wmap, "the device maps against the reference")
    yi = torch.where(R.is_class(y, C, None), y, torch.full_like(y, float(ig))).view(B, *dims).long().to(DEV)
    assert_same_bits(losses.hausdorff_weight_maps(zc.to(DEV), yi, **opts), maps, "integer labels")
    ref = R.HdRef(z, y, wmap, bg, ig, 0.37)
    w = torch.tensor([0.37], device=DEV)
    fails = []
    for given, name in ((None, "maps inside"), (maps, "maps=")):
        def fn(a, b):
            out = losses.hausdorff_dt_loss(a, b, maps=given, weight=w, **opts)
            assert "HausdorffFn" in type(out.grad_fn).__name__
            return out
        fails += failures(*seg_run(fn, z, y, B, C, dims, 2.5), ref, f"hausdorff_dt_loss {name} {dims}", 2.5)
    plain = zc.contiguous().to(DEV).requires_grad_(True)
    got = losses.hausdorff_dt_loss(plain, yc.to(DEV), weight=w, **opts)
    assert "HausdorffFn" not in type(got.grad_fn).__name__                                    # the composition, not the kernels
    (got * 0.7).backward()
    fails += failures(got.detach().cpu(), plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(B, -1, C), ref, f"channels-first {dims}", 0.7)
    # against the CPU composition of the package
    cpu = zc.clone().requires_grad_(True)
    want = losses.hausdorff_dt_loss(cpu, yc, weight=torch.tensor([0.37]), **opts)
    want.backward()
    l_k, g_k = seg_run(lambda a, b: losses.hausdorff_dt_loss(a, b, weight=w, **opts), z, y, B, C, dims)
    assert abs(float(l_k) - float(want.detach())) <= 2 * R.VALUE_BAR * max(1.0, ref.A)
    R.assert_within_located(g_k, cpu.grad.permute(0, 2, 3, 4, 1).reshape(B, -1, C).double(), 2 * ref.bar_abs, "bvc", "kernels against the CPU composition")
    # the module around a base loss
    sopts = dict(alpha=0.3, beta=0.7, include_background=bg, focal_gamma=2.0, ignore_index=ig, class_weights=(0.5, 2.0, 1.0, 3.0)[:C])
    base = losses.SegLoss(**sopts).to(DEV)
    lam = 1.5
    mod = losses.HausdorffDTLoss(base=base, lambda_hausdorff=lam, **opts).to(DEV)
    assert mod.weight.is_cuda
    l_base, g_base = seg_run(base, z, y, B, C, dims, 2.5)
    l_all, g_all = seg_run(mod, z, y, B, C, dims, 2.5)
    fails += failures(l_all - l_base, g_all - g_base, R.HdRef(z, y, wmap, bg, ig, lam), f"module minus its base {dims}", 2.5)
    assert len(mod._maps_ws) == 1
    mod.set_weight(2.0)
    l_two, g_two = seg_run(mod, z, y, B, C, dims, 2.5)
    fails += failures(l_two - l_base, g_two - g_base, R.HdRef(z, y, wmap, bg, ig, lam * 2.0), "weight 2", 2.5)
    assert len(mod._maps_ws) == 1                                                             # the scratch is the shape's, kept
    alone = losses.HausdorffDTLoss(lambda_hausdorff=lam, **opts).to(DEV)
    fails += failures(*seg_run(alone, z, y, B, C, dims), R.HdRef(z, y, wmap, bg, ig, lam), f"the term alone {dims}")
    # (the differences carry one rounding of the sum per element on top of the term's own error; the bars stay the term's)
    assert not fails, "\n".join(fails)


def test_recorded_step_follows_new_logits_labels_and_weight():
    """HausdorffDTLoss around a SegLoss, value + backward, in one graph on one stream; replays with new logits (the prediction's
    masks move), new labels (class 2 disappears from sample 0) and a new weight have the bits of the eager call."""
    R.ndi()
    shape = R.SHAPES[0]
    B, C, dims = shape
    z, y, wmap, ig = R.loss_case(shape, False)
    base = losses.SegLoss(alpha=0.3, beta=0.7, include_background=False, ignore_index=ig)
    mod = losses.HausdorffDTLoss(base=base, lambda_hausdorff=0.5, alpha=3.0, ignore_index=ig, spacing=R.ANISO).to(DEV)
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
            mod.set_weight(0.1)
    grad_g = zs.grad
    z2 = R.logits("ties", B, z.shape[1], C, seed=11)
    y2 = R.labels("blobs", B, C, dims, seed=9)
    y2[0][y2[0] == 2.0] = 0.0
    y2[1, 0, 0, :3] = 255.0
    assert not bool((y2[0] == 2.0).any()) and bool((y2[1] == 2.0).any())
    for zn, yn, wn in ((z, y.view(B, *dims), 1.0), (z2, y2, 0.37), (z, y2, 0.0), (z2, y.view(B, *dims), 2.0)):
        with torch.no_grad():
            zs.copy_(zn.view(B, *dims, C))
        ys.copy_(yn.view(B, 1, *dims))
        mod.set_weight(wn)
        graph.replay()
        torch.cuda.synchronize()
        got_l, got_g = loss_g.detach().cpu().clone(), grad_g.detach().cpu().clone()
        ze = zn.view(B, *dims, C).to(DEV).requires_grad_(True)
        want = mod(ze.permute(0, 4, 1, 2, 3), yn.view(B, 1, *dims).to(DEV))
        want.backward()
        assert_same_bits(got_l.reshape(1), want.detach().cpu().reshape(1), f"replayed value, weight {wn}")
        assert_same_bits(got_g, ze.grad.cpu(), f"replayed gradient, weight {wn}")


def test_train_step_loss_takes_the_module_as_seg_loss():
    """conf.seg_loss = HausdorffDTLoss(base=SegLoss(...)) through train.step_loss: the module's own value and gradient."""
    R.ndi()
    from types import SimpleNamespace
    from mivp_amd import train
    shape = R.SHAPES[2]
    B, C, dims = shape
    z, y, wmap, ig = R.loss_case(shape, False)
    mod = losses.HausdorffDTLoss(base=losses.SegLoss(ignore_index=ig, include_background=False), ignore_index=ig).to(DEV)
    conf = SimpleNamespace(training_mode="downstream", seg_loss=mod, include_background=False)
    l_a, g_a = seg_run(lambda a, b: train.step_loss({"downstream": a}, conf, b), z, y, B, C, dims)
    l_b, g_b = seg_run(mod, z, y, B, C, dims)
    assert_same_bits(l_a.reshape(1), l_b.reshape(1), "step_loss value")
    assert_same_bits(g_a, g_b, "step_loss gradient")
