"""Direct parity tests of the Lovasz-Softmax term (csrc/lovasz.hip) and of the device-wide key sort under it
(csrc/sort_common.hpp) against numpy.sort and tests/lovasz_ref.py (float64, CPU), and of the wrappers above them.

The entry points are called through ``_lib.call`` on their own operands between guard words (the helpers of
tests/test_hip_distmap.py); the workspace has exactly ``*_ws`` bytes.

Bars (tests/test_lovasz_host.py checks the restatement itself on the CPU):
  sort       the bits of numpy.sort per segment
  keys       |e(key) - e64| <= 4 x E_u (the yardstick of tests/segtopk_ref.py); the foreground flags, G and the valid counts exact
  value      VALUE_BAR max(1, A), A = the float64 value without its weight
  gradient   per element LOSS_MARGIN x E32 x max |g64| against the restatement ORDERED BY THE KERNEL'S OWN KEYS (a float32
             near-tie cannot reorder the reference, and no element is left out); rel-L2 < 1e-4; +0 in every bit when every voxel
             is ignored

Measured on an MI355X (kernel error / E32, the bar is 8): the numbers are in DESIGN 5.13."""
import itertools
import math
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lovasz_ref as R  # noqa: E402
from test_hip_distmap import DEV, Guarded, assert_same_bits, bits  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import losses

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BOOLS = (False, True)


def words(g, a):
    """Fill a Guarded tensor with the 32-bit words of numpy array ``a``."""
    g.t.view(torch.int32).copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(g.t.shape)))


def as_u32(t):
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)


# =============================================================================================
# the sort
# =============================================================================================
def sort_call(keys):
    """keys u32 numpy [S, n] -> the entry's result, through guarded operands."""
    S, n = keys.shape
    nbytes = int(L.lib().mivp_sort_u32_ws(S, n))
    assert nbytes > 0 and nbytes % 4 == 0
    kd, ws = Guarded((S, n)), Guarded((nbytes // 4,))
    words(kd, keys)
    L.call("mivp_sort_u32", L.ptr(kd.t), S, n, L.ptr(ws.t), L.stream())
    torch.cuda.synchronize()
    ws.done("workspace", written=False)
    return as_u32(kd.done("keys", written=False))


def sort_lengths():
    T = int(L.lib().mivp_sort_tile())
    return (1, 2, 255, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)


@pytest.mark.parametrize("content", ["random", "four", "equal"])
def test_sort_is_numpy_sort(content):
    rng = np.random.default_rng(5)
    for n in sort_lengths():
        if content == "random":
            keys = rng.integers(0, 2 ** 32, (1, n), dtype=np.uint32)
        elif content == "four":
            keys = np.array([0xFFFFFFFF, 0, 0x7F000001, 0x00FF00FF], np.uint32)[rng.integers(0, 4, (1, n))]
        else:
            keys = np.full((1, n), 0x3C00FF01, np.uint32)
        got = sort_call(keys)
        assert np.array_equal(got, np.sort(keys, axis=1)), f"{content} n = {n}: first difference at " \
            f"{int(np.argmax(got != np.sort(keys, axis=1)))}"


def test_sort_keeps_segments_apart():
    T = int(L.lib().mivp_sort_tile())
    rng = np.random.default_rng(6)
    for n in (1, 2 * T + 5):
        keys = np.stack([rng.integers(0, 2 ** 32, n, dtype=np.uint32),
                         np.array([7, 0xFFFFFFFF, 0x80000000, 7 << 8], np.uint32)[rng.integers(0, 4, n)],
                         np.full(n, 0x01020304, np.uint32)])
        got = sort_call(keys)
        for s in range(3):
            assert np.array_equal(got[s], np.sort(keys[s])), f"n = {n}, segment {s}"
        assert np.array_equal(sort_call(keys), got), "a second identical call"


# =============================================================================================
# keys, value and gradient
# =============================================================================================
def abi_opts(o):
    ig = o["ignore_index"]
    return (int(o["include_background"]), 0 if ig is None else ig, 0 if ig is None else 1, int(o["per_image"]))


def seg_shape(z, o):
    B, vol, C = z.shape
    K = C - (0 if o["include_background"] else 1)
    return (B * K, vol) if o["per_image"] else (K, B * vol)


def keys_call(z, y, o):
    """(keys u32 [S, N], counts [S, 2]) of mivp_lovasz_keys."""
    B, vol, C = z.shape
    S, N = seg_shape(z, o)
    kd, cd = Guarded((S, N)), Guarded((S, 2))
    zd, yd = Guarded(tuple(z.shape), z), Guarded(tuple(y.shape), y)
    bg, ign, has, pi = abi_opts(o)
    L.call("mivp_lovasz_keys", L.ptr(zd.t), L.ptr(yd.t), B, vol, C, bg, ign, has, pi, L.ptr(kd.t), L.ptr(cd.t), L.stream())
    torch.cuda.synchronize()
    assert_same_bits(zd.done("logits"), z, "the logits are read only")
    assert_same_bits(yd.done("labels"), y, "the labels are read only")
    return as_u32(kd.done("keys", written=False)), as_u32(cd.done("counts")).astype(np.int64)


def loss_call(z, y, o, lam=1.0, weight=None, form="fused", gscale=None, onto=None):
    """(loss, dz, sorted keys [S, N]) on the CPU.  fused: mivp_lovasz_loss with dlogits; split: the value call without dlogits,
    then mivp_lovasz_loss_grad on the same workspace with ``gscale`` (None: NULL).  ``onto``: dz's content, accumulate = 1."""
    B, vol, C = z.shape
    S, N = seg_shape(z, o)
    bg, ign, has, pi = abi_opts(o)
    nbytes = int(L.lib().mivp_lovasz_ws(B, C, bg, pi, vol))
    assert nbytes > 0 and nbytes % 256 == 0
    ws, loss, dz = Guarded((nbytes // 4,)), Guarded((1,)), Guarded((B, vol, C), onto)
    zd, yd = Guarded(tuple(z.shape), z), Guarded(tuple(y.shape), y)
    wd = None if weight is None else torch.tensor([weight], dtype=F32, device=DEV)
    gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    acc = 0 if onto is None else 1
    al = 1 if o["classes"] == "all" else 0
    if form == "fused":
        assert gscale is None
        L.call("mivp_lovasz_loss", L.ptr(zd.t), L.ptr(yd.t), B, vol, C, bg, ign, has, pi, al, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(loss.t), L.ptr(dz.t), acc, L.stream())
    else:
        L.call("mivp_lovasz_loss", L.ptr(zd.t), L.ptr(yd.t), B, vol, C, bg, ign, has, pi, al, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(loss.t), None, 0, L.stream())
        L.call("mivp_lovasz_loss_grad", L.ptr(zd.t), L.ptr(yd.t), B, vol, C, bg, ign, has, pi, al, lam, L.ptr(wd), L.ptr(ws.t),
               L.ptr(gs), L.ptr(dz.t), acc, L.stream())
    torch.cuda.synchronize()
    raw = ws.done("workspace", written=False)
    assert_same_bits(zd.done("logits"), z, "the logits are read only")
    assert_same_bits(yd.done("labels"), y, "the labels are read only")
    return loss.done("loss value")[0], dz.done("dlogits"), as_u32(raw[:S * N]).reshape(S, N)


@lru_cache(maxsize=None)
def inputs(shape, content, lab):
    B, C, dims = shape
    return R.logits(content, B, math.prod(dims), C), R.label_case(lab, B, C, dims)


def opts(classes="present", per_image=False, bg=True, ig=R.IGNORE):
    return dict(classes=classes, per_image=per_image, include_background=bg, ignore_index=ig)


def failures(got_loss, got_dz, ref, what, k=1.0):
    """Print the case's figures, then return the list of bars it misses (k: the incoming gradient)."""
    out = []
    print(f"[lovasz-value] {what}: loss {float(got_loss)!r} float64 {ref.l64!r} off {abs(float(got_loss) - ref.l64):.3e} "
          f"bar {R.VALUE_BAR * max(1.0, ref.A):.3e}")
    if not abs(float(got_loss) - ref.l64) <= R.VALUE_BAR * max(1.0, ref.A):
        out.append(f"{what}: loss {float(got_loss)!r}, float64 {ref.l64!r} (A {ref.A:.3e})")
    if ref.zero or k == 0.0:
        if not bool(got_dz.double().abs().max() == 0):
            out.append(f"{what}: a zero gradient is owed, max |dz| {float(got_dz.abs().max()):.3e}")
        return out
    g64 = k * ref.g64
    err = float((got_dz.double() - g64).abs().max()) / (abs(k) * ref.scale)
    print(f"[lovasz-ratio] {what}: E32 {ref.e32:.3e} kernel {err:.3e} ratio {err / ref.e32:.3f} bar {ref.bar_norm:.3e}")
    l2 = R.rel_l2(got_dz, g64)
    if not l2 < R.LOSS_L2_BAR:
        out.append(f"{what}: gradient rel-L2 {l2:.3e}")
    try:
        R.assert_within_located(got_dz, g64, abs(k) * ref.bar_abs, "bvc", what)
    except AssertionError as e:
        out.append(str(e))
    return out


@pytest.mark.parametrize("per_image", BOOLS)
@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids_shape)
def test_keys_flags_and_counts(shape, content, per_image):
    fails = []
    for lab, bg in (("blobs", True), ("ignored", False), ("none", True)):
        z, y = inputs(shape, content, lab)
        o = opts(per_image=per_image, bg=bg)
        c0 = 0 if bg else 1
        keys, counts = keys_call(z, y, o)
        eu, e64, valid = R.e_u(z, y, R.IGNORE)
        _, _, hot, _ = R.softmax_errors(z, y, R.IGNORE)
        e_k, fg_k, valid_k = R.key_errors(keys)
        what = f"{R.ids_shape(shape)} {content} {lab} per_image {per_image} bg {bg}"
        assert np.array_equal(valid_k, R.to_segments(np.repeat(valid[..., None], z.shape[-1], -1), c0, per_image)), what
        assert np.array_equal(fg_k, R.to_segments(hot, c0, per_image)), what + ": foreground flags"
        assert np.array_equal(counts[:, 0], fg_k.sum(1)) and np.array_equal(counts[:, 1], valid_k.sum(1)), what + ": counts"
        if valid_k.any():
            off = float(np.abs(e_k - R.to_segments(e64, c0, per_image))[valid_k].max())
            print(f"[lovasz-keys] {what}: E_u {eu:.3e} kernel {off:.3e} ratio {off / eu:.3f} (bar {R.KEY_BAND})")
            if not off <= R.KEY_BAND * eu:
                fails.append(f"{what}: keys off by {off:.3e}, band {R.KEY_BAND * eu:.3e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("lab", ["blobs", "absent", "ignored", "none"])
@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.ids_shape)
def test_value_and_gradient(shape, content, lab):
    z, y = inputs(shape, content, lab)
    fails = []
    for per_image, classes in itertools.product(BOOLS, ("present", "all")):
        bg = not (per_image and classes == "all")
        o = opts(classes, per_image, bg)
        what = f"{R.ids_shape(shape)} {content} {lab} per_image {per_image} classes {classes} bg {bg}"
        keys, counts = keys_call(z, y, o)
        ref = R.LvRef(z, y, keys=keys, weight=0.37, **o)
        assert np.array_equal(ref.counts, counts), what
        loss, dz, sorted_keys = loss_call(z, y, o, 1.0, 0.37)
        assert np.array_equal(sorted_keys, np.sort(keys, axis=1)), what + ": the workspace holds the sorted keys"
        fails += failures(loss, dz, ref, what)
        if lab == "none":
            assert float(loss) == 0.0 and torch.equal(bits(loss.reshape(1)), torch.zeros(1, dtype=torch.int32)), what
            assert torch.equal(bits(dz), torch.zeros_like(bits(dz))), what + ": every gradient word is +0.0"
        else:
            invalid = ~R.is_class(y, z.shape[-1], R.IGNORE)
            assert torch.equal(bits(dz[invalid]), torch.zeros_like(bits(dz[invalid]))), what + ": invalid voxels"
        if lab == "absent" and per_image and bg:                 # class 1 of sample 0 has no voxel, class 1 of sample 1 has
            assert counts[1, 0] == 0 and counts[z.shape[-1] + 1, 0] > 0 and ref.A > 0, what
    assert not fails, "\n".join(fails)


def test_structure():
    """Equal calls; accumulate onto a known dz; the split form with a gscale against the fused form; lambda; NULL weight."""
    shape = R.SHAPES[1]
    z, y = inputs(shape, "randn", "ignored")
    o = opts("present", True)
    what = R.ids_shape(shape)
    keys, _ = keys_call(z, y, o)
    ref = R.LvRef(z, y, keys=keys, weight=0.37, **o)
    l_f, g_f, k_f = loss_call(z, y, o, 1.0, 0.37)
    l_r, g_r, k_r = loss_call(z, y, o, 1.0, 0.37)
    assert_same_bits(g_r, g_f, what + ": a second identical call")
    assert_same_bits(l_r.reshape(1), l_f.reshape(1), what + ": a second identical call, value")
    assert np.array_equal(k_r, k_f)
    onto = torch.randn(z.shape, generator=R.gen(5), dtype=F32) * float(g_f.abs().max())
    l_a, g_a, _ = loss_call(z, y, o, 1.0, 0.37, onto=onto)
    assert_same_bits(g_a, onto + g_f, what + ": accumulate onto a known dz, fused")
    l_s, g_s, _ = loss_call(z, y, o, 1.0, 0.37, form="split", onto=onto)
    assert_same_bits(g_s, onto + g_f, what + ": accumulate onto a known dz, split")
    for gs in (1.0, None):
        l_k, g_k, _ = loss_call(z, y, o, 1.0, 0.37, form="split", gscale=gs)
        assert_same_bits(g_k, g_f, what + f": split with gscale {gs} against fused")
        assert_same_bits(l_k.reshape(1), l_f.reshape(1), what + ": value")
    fails = []
    for gs in (-2.5, 0.0):
        l_k, g_k, _ = loss_call(z, y, o, 1.0, 0.37, form="split", gscale=gs)
        assert_same_bits(l_k.reshape(1), l_f.reshape(1), what + f": value, gscale {gs}")
        fails += failures(l_k, g_k, ref, what + f" gscale {gs}", gs)
    l_l, g_l, _ = loss_call(z, y, o, 0.5, 0.74)
    fails += failures(l_l, g_l, R.LvRef(z, y, keys=keys, weight=float(np.float32(0.5) * np.float32(0.74)), **o), what + " lambda 0.5")
    l_n, g_n, _ = loss_call(z, y, o, 1.0, None)
    fails += failures(l_n, g_n, R.LvRef(z, y, keys=keys, **o), what + " weight NULL")
    l_0, g_0, _ = loss_call(z, y, o, 1.0, 0.0)
    fails += failures(l_0, g_0, R.LvRef(z, y, keys=keys, weight=0.0, **o), what + " weight 0")
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


@pytest.mark.parametrize("per_image", BOOLS)
def test_public_functions(per_image):
    """``lovasz_softmax_loss`` on the kernels against the entry, on the plain-torch path against the reference;
    ``LovaszSoftmaxLoss(base=SegLoss(...))`` = the base + the term."""
    shape = R.SHAPES[0]
    B, C, dims = shape
    z, y = inputs(shape, "randn", "ignored")
    o = opts("present", per_image)
    keys, _ = keys_call(z, y, o)
    ref = R.LvRef(z, y, keys=keys, weight=0.37, **o)
    w = torch.tensor([0.37], device=DEV)

    def fn(a, b):
        out = losses.lovasz_softmax_loss(a, b, weight=w, **o)
        assert "LovaszFn" in type(out.grad_fn).__name__
        return out
    l_k, g_k = seg_run(fn, z, y, B, C, dims, 2.5)
    l_e, g_e, _ = loss_call(z, y, o, 1.0, 0.37, form="split", gscale=2.5)
    assert_same_bits(l_k.reshape(1), l_e.reshape(1), "lovasz_softmax_loss against the entry, value")
    assert_same_bits(g_k, g_e, "lovasz_softmax_loss against the entry, gradient")
    fails = failures(l_k, g_k, ref, f"lovasz_softmax_loss per_image {per_image}", 2.5)
    zc = z.view(B, *dims, C).permute(0, 4, 1, 2, 3)
    plain = zc.contiguous().to(DEV).requires_grad_(True)
    got = losses.lovasz_softmax_loss(plain, y.view(B, 1, *dims).to(DEV), weight=w, **o)
    assert "LovaszFn" not in type(got.grad_fn).__name__                                       # the composition, not the kernels
    (got * 0.7).backward()
    plain_ref = R.LvRef(z, y, weight=0.37, **o)                                               # its own (float32) order: no ties here
    fails += failures(got.detach().cpu(), plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(B, -1, C), plain_ref, "channels-first", 0.7)
    base = losses.SegLoss(alpha=0.3, beta=0.7, focal_gamma=2.0, ignore_index=R.IGNORE, class_weights=(0.5, 2.0, 1.0)).to(DEV)
    mod = losses.LovaszSoftmaxLoss(base=base, lambda_lovasz=1.5, **o).to(DEV)
    assert mod.weight.is_cuda
    l_base, g_base = seg_run(base, z, y, B, C, dims, 2.5)
    l_all, g_all = seg_run(mod, z, y, B, C, dims, 2.5)
    fails += failures(l_all - l_base, g_all - g_base, R.LvRef(z, y, keys=keys, weight=1.5, **o), "module minus its base", 2.5)
    mod.set_weight(2.0)
    l_two, g_two = seg_run(mod, z, y, B, C, dims, 2.5)
    fails += failures(l_two - l_base, g_two - g_base, R.LvRef(z, y, keys=keys, weight=3.0, **o), "weight 2", 2.5)
    assert len(mod._ws) == 1                                                                  # the workspace is the shape's, kept
    assert not fails, "\n".join(fails)


def test_recorded_step_follows_new_logits_labels_and_weight():
    """LovaszSoftmaxLoss around a SegLoss, value + backward, in one graph on one stream; replays with new logits, new labels
    (class 2 disappears from sample 0, then from the batch) and a new weight have the bits of the eager call."""
    shape = R.SHAPES[0]
    B, C, dims = shape
    z, y = inputs(shape, "randn", "ignored")
    base = losses.SegLoss(alpha=0.3, beta=0.7, ignore_index=R.IGNORE)
    for per_image in BOOLS:
        mod = losses.LovaszSoftmaxLoss(base=base, lambda_lovasz=0.5, per_image=per_image, ignore_index=R.IGNORE).to(DEV)
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
        z2 = R.logits("pm30", B, z.shape[1], C, seed=11)
        y2 = R.label_case("blobs", B, C, dims, seed=9).clone()
        y2[0][y2[0] == 2.0] = 0.0
        y3 = y2.clone()
        y3[y3 == 2.0] = 1.0
        assert bool((y == 2.0).any()) and not bool((y2[0] == 2.0).any()) and bool((y2[1] == 2.0).any()) and not bool((y3 == 2.0).any())
        for zn, yn, wn in ((z, y, 1.0), (z2, y2, 0.37), (z, y3, 0.0), (z2, y3, 2.0), (z, y, 2.0)):
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
    """conf.seg_loss = LovaszSoftmaxLoss(base=SegLoss(...)) through train.step_loss: the module's own value and gradient."""
    from types import SimpleNamespace
    from mivp_amd import train
    shape = R.SHAPES[0]
    B, C, dims = shape
    z, y = inputs(shape, "randn", "ignored")
    mod = losses.LovaszSoftmaxLoss(base=losses.SegLoss(ignore_index=R.IGNORE), ignore_index=R.IGNORE).to(DEV)
    conf = SimpleNamespace(training_mode="downstream", seg_loss=mod, include_background=True)
    l_a, g_a = seg_run(lambda a, b: train.step_loss({"downstream": a}, conf, b), z, y, B, C, dims)
    l_b, g_b = seg_run(mod, z, y, B, C, dims)
    assert_same_bits(l_a.reshape(1), l_b.reshape(1), "step_loss value")
    assert_same_bits(g_a, g_b, "step_loss gradient")
