"""CPU: the float64 references of the Hausdorff distance-transform term (tests/hausdorff_ref.py), the bars that
tests/test_hip_hausdorff.py applies to csrc/hausdorff.hip, and the package's host side.

1. the map reference (scipy) against all-pairs distances at unit and anisotropic spacing, its degenerate masks, exact ties;
2. the loss reference's hand-written gradient against autograd in float64; f32 torch inside every bar on every case the GPU
   file runs; plausible kernel bugs outside them;
3. the package on the CPU: the numpy maps and the torch composition against the references, ``HausdorffDTLoss`` around a
   base loss, the argument checks, the header and the ABI, ``SegLossSpec`` untouched;
4. what the term is for: of two predictions with the same false-positive volume and the same Dice, the one whose island
   lies far from the object costs more."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hausdorff_ref as R  # noqa: E402

from conftest import ROOT  # noqa: E402

F32, F64 = torch.float32, torch.float64
BOOLS = (False, True)
SMALL = ((2, 3, (6, 5, 7)), (1, 2, (1, 1, 9)))


# =============================================================================================
# 1. the map reference
# =============================================================================================
@pytest.mark.parametrize("spacing", [R.UNIT, R.ANISO32], ids=["unit", "aniso"])
@pytest.mark.parametrize("case", R.LABEL_CASES)
def test_map_reference_is_the_all_pairs_distance(case, spacing):
    R.ndi()
    for B, C, dims in SMALL:
        y = R.labels(case, B, C, dims)
        vol = dims[0] * dims[1] * dims[2]
        for kind in R.LOGIT_KINDS:
            z = R.logits(kind, B, vol, C)
            for bg in BOOLS:
                a = R.MapRef(z, y, spacing, bg, R.IGNORE)
                b = R.MapRef(z, y, spacing, bg, R.IGNORE, edt=R.D.edt_brute(spacing))
                for alpha in (1.0, 2.0, 3.0):
                    wa, wb = a.wm(alpha), b.wm(alpha)
                    assert float(np.abs(wa - wb).max()) <= 1e-12 * max(1.0, float(np.abs(wb).max())), (case, kind, dims, bg, alpha)
                if spacing[0] == 1.0:
                    assert np.array_equal(np.rint(a.wm(2.0)), np.rint(b.wm(2.0))) and float(np.abs(a.wm(2.0) - np.rint(a.wm(2.0))).max()) < 1e-9


def test_masks_ties_and_degenerate_fields():
    R.ndi()
    B, C, dims = R.SHAPES[0]
    vol = dims[0] * dims[1] * dims[2]
    z = R.logits("ties", B, vol, C)
    pred = R.pred_classes(z)
    assert bool((pred[:, 0::7] == 0).all()) and bool((pred[:, 1::7] == C - 2).all()) and bool((pred[:, 2::7] == 0).all())
    assert torch.equal(pred, torch.argmax(z.double(), -1))        # torch.argmax documents the first maximum as well
    y = R.labels("full", B, C, dims)
    ref = R.MapRef(z, y, R.UNIT, True, R.IGNORE)
    assert ref.G[0, 1].all() and not ref.fg2[0, 1].any()           # the whole sample: field 0
    assert not ref.G[0, 0].any() and not ref.fg2[0, 0].any()       # empty: field 0
    zc = z.clone()
    zc[0, :, 1] = 9.0                                              # the prediction of sample 0 is class 1 everywhere
    deg = R.MapRef(zc, y, R.UNIT, True, R.IGNORE)
    assert deg.P[0, 1].all() and not deg.fp2[0].any() and deg.fp2[1].any()
    assert not deg.wm(2.0)[0].any() and not deg.wm(3.0)[0].any()   # both masks degenerate in every class of sample 0
    bad = R.labels("bad", B, C, dims)
    refb = R.MapRef(z, bad, R.UNIT, False, R.IGNORE)
    assert not refb.G[:, :, ~R.is_class(bad, C, R.IGNORE).numpy()[0]][0].any()    # an invalid label is in no G ...
    assert refb.P.any(1).reshape(-1)[(pred.reshape(-1) >= 1).numpy()].all()       # ... the prediction has a class at every voxel
    # a one-voxel mask: the field is the distance to that voxel outside it, and the distance to its nearest neighbour inside
    M = np.zeros(dims, bool)
    M[2, 3, 10] = True
    f = R.field_sq(M, R.ANISO32)
    assert abs(f[2, 3, 10] - min(R.ANISO32) ** 2) < 1e-12
    assert abs(f[0, 0, 0] - ((2 * R.ANISO32[0]) ** 2 + (3 * R.ANISO32[1]) ** 2 + (10 * R.ANISO32[2]) ** 2)) < 1e-9


# =============================================================================================
# 2. the loss reference and the bars
# =============================================================================================
def loss_cases():
    for shape in R.SHAPES:
        for bg in BOOLS:
            for sat in BOOLS:
                yield shape, bg, sat


def test_hand_written_gradient_is_autograd_in_float64():
    R.ndi()
    for shape, bg, sat in loss_cases():
        z, y, wmap, ig = R.loss_case(shape, bg, sat)
        w = float(np.float32(0.37))
        l64, g64, A = R.hausdorff_ref(z, y, wmap, bg, ig, 0.37)
        zz = z.double().requires_grad_(True)
        C, c0 = z.shape[-1], 0 if bg else 1
        ok = R.is_class(y, C, ig)
        valid = ok.double()
        onehot = ((y.double().unsqueeze(-1) == torch.arange(C, dtype=F64)) & ok.unsqueeze(-1)).double()
        err = torch.softmax(zz, -1) - onehot
        want = w * ((err * err * R.D.phit_of(wmap.double(), C, c0)).sum(-1) * valid).sum() / ((C - c0) * valid.sum())
        want.backward()
        assert abs(float(l64 - want.detach())) <= 1e-12 * max(1.0, A)
        assert float((g64 - zz.grad).abs().max()) <= 1e-12 * float(zz.grad.abs().max()), (shape, bg, sat)
        assert not bool(g64[valid == 0].abs().max() > 0) and bool((valid == 0).any())


def f32_inside(ref, what):
    assert abs(float(ref.l32) - float(ref.l64)) <= R.VALUE_BAR * max(1.0, ref.A), what
    assert R.rel_l2(ref.g32, ref.g64) < R.LOSS_L2_BAR, what
    assert ref.bar_norm <= 1e-4, (what, ref.bar_norm)              # no per-element bar looser than the aggregate one
    R.assert_within_located(ref.g32, ref.g64, ref.bar_abs, "bvc", what)


def test_f32_torch_meets_the_bars_on_every_gpu_case():
    R.ndi()
    worst = 0.0
    for shape, bg, sat in loss_cases():
        z, y, wmap, ig = R.loss_case(shape, bg, sat)
        for w in (None, 0.37):
            ref = R.HdRef(z, y, wmap, bg, ig, w)
            f32_inside(ref, f"{R.ids_shape(shape)} bg {bg} saturated {sat} weight {w}")
            worst = max(worst, ref.bar_norm)
        zero = R.HdRef(z, y, wmap, bg, ig, 0.0)
        assert zero.zero and float(zero.l64) == 0.0 and not bool(zero.g32.abs().max() > 0)
    print(f"loosest per-element bar: {worst:.2e} of max |g|")
    z, y, wmap, ig = R.loss_case(R.SHAPES[0], False, all_ignored=True)
    ref = R.HdRef(z, y, wmap, False, ig)
    assert ref.zero and float(ref.l64) == 0.0 and float(ref.l32) == 0.0


def test_f32_numpy_maps_meet_their_own_bar():
    """The yardstick of the map tests: the f32 evaluation is inside LOSS_MARGIN x E32 by construction; E32 stays a few
    unit roundoffs, so the bar is a statement about f32, not a loose one."""
    R.ndi()
    worst = 0.0
    for shape in R.SHAPES:
        B, C, dims = shape
        z = R.logits("randn", B, dims[0] * dims[1] * dims[2], C)
        ref = R.MapRef(z, R.labels("blobs", B, C, dims), R.ANISO32, True, R.IGNORE)
        for alpha in (1.0, 2.0, 3.0):
            bar, e32 = R.map_bar(ref.wm(alpha), ref.wm(alpha, np.float32))
            worst = max(worst, e32)
    print(f"largest E32 of the maps: {worst / R.U32:.2f} unit roundoffs")
    assert worst <= 8 * R.U32


def assert_located_fails(bad_l, bad_g, ref, what):
    print(f"{what}: value off by {abs(float(bad_l) - float(ref.l64)):.2e}, rel_l2 {R.rel_l2(bad_g, ref.g64):.2e}; "
          f"per-element bar {ref.bar_norm:.2e} of max |g|")
    assert not abs(float(bad_l) - float(ref.l64)) <= R.VALUE_BAR * max(1.0, ref.A), what
    with pytest.raises(AssertionError, match="leave the bound of the float64 reference"):
        R.assert_within_located(bad_g, ref.g64, ref.bar_abs, "bvc", what)


@pytest.mark.parametrize("bg", BOOLS)
def test_plausible_kernel_bugs_miss_the_bars(bg):
    R.ndi()
    z, y, wmap, ig = R.loss_case(R.SHAPES[0], bg)
    ref = R.HdRef(z, y, wmap, bg, ig)
    assert_located_fails(*R.hausdorff_ref(z, y, wmap, bg, ig, all_voxels=True)[:2], ref, "mean over all voxels")
    assert_located_fails(*R.hausdorff_ref(z, y, wmap, bg, ig, shift=1)[:2], ref, "wmap[c] for wmap[c - c0]")
    assert_located_fails(*R.hausdorff_ref(z, y, wmap, bg, ig, no_target=True)[:2], ref, "p^2 for (p - g)^2")


# =============================================================================================
# 3. the package on the CPU
# =============================================================================================
@pytest.mark.parametrize("spacing", [R.UNIT, R.ANISO32], ids=["unit", "aniso"])
def test_numpy_maps_of_the_package_are_the_reference(spacing):
    R.ndi()
    from mivp_amd import losses
    for B, C, dims in SMALL + (R.SHAPES[2],):
        vol = dims[0] * dims[1] * dims[2]
        for case, kind in (("blobs", "randn"), ("bad", "ties"), ("full", "pm30"), ("absent", "ties")):
            z, y = R.logits(kind, B, vol, C), R.labels(case, B, C, dims)
            for bg in BOOLS:
                ref = R.MapRef(z, y, spacing, bg, R.IGNORE)
                for alpha in (2.0, 1.0, 3.0):
                    got = losses.hausdorff_weight_maps(z.view(B, *dims, C).permute(0, 4, 1, 2, 3), y.view(B, 1, *dims), alpha=alpha,
                                                       spacing=spacing, include_background=bg, ignore_index=R.IGNORE)
                    want = ref.wm(alpha)
                    assert got.dtype == F32 and tuple(got.shape) == want.shape
                    if alpha == 2.0 and spacing[0] == 1.0:
                        assert np.array_equal(got.numpy(), want.astype(np.float32)), (case, kind, dims, bg)
                    else:
                        assert float(np.abs(got.double().numpy() - want).max()) <= 2 * R.U32 * max(1.0, float(want.max()))


@pytest.mark.parametrize("bg", BOOLS)
def test_cpu_composition_is_the_reference(bg):
    R.ndi()
    from mivp_amd import losses
    shape = R.SHAPES[2]
    B, C, dims = shape
    z, y, wmap, ig = R.loss_case(shape, bg)
    ref = R.HdRef(z, y, wmap, bg, ig, 0.37)
    K = wmap.shape[1]
    for maps in (None, wmap.view(B, K, *dims)):
        for dtype, tol in ((F64, 1e-10), (F32, None)):
            base = z.to(dtype).view(B, *dims, C).clone().requires_grad_(True)
            got = losses.hausdorff_dt_loss(base.permute(0, 4, 1, 2, 3), y.view(B, 1, *dims), include_background=bg, ignore_index=ig,
                                           maps=maps, weight=torch.tensor([0.37]))
            got.backward()
            grad = base.grad.view(B, -1, C)
            if tol is not None:
                assert got.dtype == F64 and abs(float(got.detach()) - float(ref.l64)) <= tol * max(1.0, ref.A)
                assert float((grad - ref.g64).abs().max()) <= tol * ref.scale
            else:
                assert got.dtype == F32 and abs(float(got.detach()) - float(ref.l64)) <= R.VALUE_BAR * max(1.0, ref.A)
                R.assert_within_located(grad, ref.g64, ref.bar_abs, "bvc", "f32 package composition")
    # the maps are a constant: the gradient above is the reference's, which differentiates the softmax alone


def test_module_is_the_base_plus_the_term():
    R.ndi()
    from mivp_amd import losses
    shape = R.SHAPES[2]
    B, C, dims = shape
    z, y, wmap, ig = R.loss_case(shape, False)
    zz = z.view(B, *dims, C).permute(0, 4, 1, 2, 3)
    yy = y.view(B, 1, *dims)
    base = losses.SegLoss(ignore_index=ig, include_background=False)
    opts = dict(alpha=2.0, include_background=False, ignore_index=ig)
    mod = losses.HausdorffDTLoss(base=base, lambda_hausdorff=0.5, **opts)
    term = losses.hausdorff_dt_loss(zz, yy, **opts)
    assert torch.allclose(mod(zz, yy), base(zz, yy) + 0.5 * term, rtol=1e-6, atol=0)
    alone = losses.HausdorffDTLoss(lambda_hausdorff=0.5, **opts)
    assert torch.allclose(alone(zz, yy), 0.5 * term, rtol=1e-6, atol=0)
    assert tuple(mod.weight.shape) == (1,) and float(mod.weight) == 1.0
    assert "weight" in dict(mod.named_buffers()) and "weight" not in mod.state_dict()
    mod.set_weight(0.25)
    assert float(mod.weight) == 0.25
    assert torch.allclose(mod(zz, yy), base(zz, yy) + 0.125 * term, rtol=1e-6, atol=0)
    zg = zz.clone().requires_grad_(True)
    mod(zg, yy).backward()
    z1, z2 = zz.clone().requires_grad_(True), zz.clone().requires_grad_(True)
    base(z1, yy).backward()
    losses.hausdorff_dt_loss(z2, yy, **opts).backward()
    assert torch.allclose(zg.grad, z1.grad + 0.125 * z2.grad, rtol=1e-5, atol=1e-9)
    with pytest.raises(ValueError, match="weight"):
        mod.set_weight(float("nan"))
    # through train.step_loss, as conf.seg_loss
    from types import SimpleNamespace
    from mivp_amd import train
    conf = SimpleNamespace(training_mode="downstream", seg_loss=mod, include_background=False)
    assert torch.equal(train.step_loss({"downstream": zz}, conf, yy), mod(zz, yy))


def test_public_functions_check_their_arguments():
    from mivp_amd import losses
    z, y = torch.zeros(2, 2, 3, 4, 5), torch.zeros(2, 1, 3, 4, 5)
    for fn in (losses.hausdorff_dt_loss, losses.hausdorff_weight_maps):
        with pytest.raises(ValueError, match="logits"):
            fn(z[0], y)
        with pytest.raises(ValueError, match="classes"):
            fn(z[:, :1], y)
        with pytest.raises(ValueError, match="classes"):
            fn(torch.zeros(2, 9, 3, 4, 5), y)
        with pytest.raises(ValueError, match="target"):
            fn(z, y[:, :, :2])
        with pytest.raises(ValueError, match="include_background"):
            fn(z, y, include_background=1)
        with pytest.raises(ValueError, match="ignore_index"):
            fn(z, y, ignore_index=1.5)
        with pytest.raises(ValueError, match="spacing"):
            fn(z, y, spacing=(1.0, -1.0, 1.0))
        for alpha in (0.0, -1.0, 4.5, float("nan"), "2", True):
            with pytest.raises(ValueError, match="alpha"):
                fn(z, y, alpha=alpha)
    with pytest.raises(ValueError, match="maps"):
        losses.hausdorff_dt_loss(z, y, maps=torch.zeros(2, 2, 3, 4, 5))          # K = 1 without the background
    with pytest.raises(ValueError, match="weight"):
        losses.hausdorff_dt_loss(z, y, weight=torch.ones(2))
    assert float(losses.hausdorff_dt_loss(z, y, maps=torch.zeros(2, 1, 3, 4, 5))) == 0.0
    for bad, name in ((dict(lambda_hausdorff=-1.0), "lambda_hausdorff"), (dict(lambda_hausdorff=float("inf")), "lambda_hausdorff"),
                      (dict(lambda_hausdorff=1e39), "lambda_hausdorff"), (dict(alpha=5.0), "alpha"), (dict(spacing=(1.0, 1.0)), "spacing"),
                      (dict(include_background="no"), "include_background"), (dict(ignore_index=2.5), "ignore_index")):
        with pytest.raises(ValueError, match=name):
            losses.HausdorffDTLoss(**bad)
    with pytest.raises(TypeError, match="base"):
        losses.HausdorffDTLoss(base=lambda a, b: a)


def test_header_declares_the_entries_and_the_abi_stays_18():
    from mivp_amd import _lib, losses
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    P = _lib.parse_header()
    want = {"mivp_hausdorff_maps_ws": (3, _lib.C.c_size_t), "mivp_hausdorff_maps": (13, _lib.C.c_int),
            "mivp_hausdorff_loss_ws": (2, _lib.C.c_size_t), "mivp_hausdorff_loss": (16, _lib.C.c_int),
            "mivp_hausdorff_loss_grad": (16, _lib.C.c_int)}
    for name, (n, ret) in want.items():
        assert len(P[name][1]) == n and P[name][0] is ret, name
    assert sorted(n for n in P if n.startswith("mivp_hausdorff")) == sorted(want)
    assert len(P["mivp_hausdorff_loss"][1]) == len(P["mivp_boundary_loss"][1])
    assert len(P["mivp_hausdorff_loss_grad"][1]) == len(P["mivp_boundary_loss_grad"][1])
    # the term is no field of the spec: its slots end as they did
    assert losses.SegLossSpec.__slots__ == ("alpha", "beta", "batch", "include_background", "focal_gamma", "class_weights",
                                            "ignore_index", "lambda_region", "lambda_voxel", "top_k", "lambda_boundary",
                                            "boundary_spacing", "lambda_cldice", "cldice_iterations", "cldice_smooth")
    assert not any("hausdorff" in s for s in losses.SegLossSpec.__slots__)


def test_entries_refuse_what_the_host_refuses():
    """MIVP_REQUIRE returns before anything is launched or dereferenced: the pointers are never read."""
    from mivp_amd import _lib as L
    from mivp_amd._host import i3
    lib = L.lib()
    assert int(lib.mivp_hausdorff_maps_ws(2, 3, i3((5, 6, 7)))) == (4 * 2 * 3 * 210 * 4 + 255) // 256 * 256 + 4 * 2 * 3 * 210 * 8
    for B, K, dims in ((0, 1, (5, 6, 7)), (1, 0, (5, 6, 7)), (1, 9, (5, 6, 7)), (1, 1, (65536, 1, 1)), (1, 1, (1, 65536, 1)),
                       (1, 1, (0, 4, 4)), (2, 2, (1024, 1024, 256)), (1, 1, (1024, 1024, 512))):
        assert int(lib.mivp_hausdorff_maps_ws(B, K, i3(dims))) == 0, (B, K, dims)
    for B, vol, rows in ((3, 63, 3), (2, 2053, 6), (2, 66 * 64 * 64, 512)):
        assert int(lib.mivp_hausdorff_loss_ws(B, vol)) == 2 * rows + 4
    p = 4096                                                       # a non-NULL address that no accepted call would be given
    sp = (L.C.c_float * 3)(1.0, 1.0, 1.0)
    for B, C, bg, dims, spc, alpha in ((0, 2, 0, (4, 4, 4), sp, 2.0), (1, 1, 1, (4, 4, 4), sp, 2.0), (1, 9, 0, (4, 4, 4), sp, 2.0),
                                       (1, 2, 0, (65536, 1, 1), sp, 2.0), (1, 2, 0, (4, 4, 4), (L.C.c_float * 3)(1.0, 0.0, 1.0), 2.0),
                                       (1, 2, 0, (4, 4, 4), (L.C.c_float * 3)(1.0, float("inf"), 1.0), 2.0),
                                       (1, 2, 0, (4, 4, 4), sp, 0.0), (1, 2, 0, (4, 4, 4), sp, 4.5), (1, 2, 0, (4, 4, 4), sp, float("nan")),
                                       (2, 2, 0, (1024, 1024, 256), sp, 2.0)):
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_hausdorff_maps", p, p, B, C, bg, 0, 0, i3(dims), spc, alpha, p, p, None)
    for B, vol, C, lam in ((0, 8, 2, 1.0), (2, 0, 2, 1.0), (2, 8, 1, 1.0), (2, 8, 9, 1.0), (2, 8, 2, -1.0), (2, 8, 2, float("nan"))):
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_hausdorff_loss", p, p, p, B, vol, C, 0, 0, 0, lam, None, p, p, None, 0, None)
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_hausdorff_loss_grad", p, p, p, B, vol, C, 0, 0, 0, lam, None, p, None, p, 0, None)
    with pytest.raises(RuntimeError, match="contract violated"):
        L.call("mivp_hausdorff_loss", p, p, None, 2, 8, 2, 0, 0, 0, 1.0, None, p, p, None, 0, None)


# =============================================================================================
# 4. what the term is for
# =============================================================================================
def test_a_far_false_positive_costs_more_than_a_near_one_at_equal_dice():
    """One object, two predictions that add a 2 x 2 x 2 false-positive island to the exact object: one touching it, one 20
    voxels away.  Same false-positive volume and the same soft Dice; the Hausdorff term alone tells them apart."""
    from mivp_amd import losses
    dims = (8, 8, 40)
    y = torch.zeros((1, 1) + dims)
    y[0, 0, 2:6, 2:6, 4:8] = 1.0
    near, far = y.clone(), y.clone()
    near[0, 0, 3:5, 3:5, 8:10] = 1.0                               # adjacent to the object's face at d = 8
    far[0, 0, 3:5, 3:5, 28:30] = 1.0                               # 20 voxels further along D
    assert float((near - y).sum()) == float((far - y).sum()) == 8.0

    def logits_of(mask):                                           # confident two-class logits of a hard mask
        return torch.cat([-6.0 * (2.0 * mask - 1.0), 6.0 * (2.0 * mask - 1.0)], 1).double()

    from oracle.loss_ref import dice_loss                          # the CPU restatement of losses.dice_loss (a GPU kernel)
    d_near, d_far = (dice_loss(logits_of(m), y, include_background=False) for m in (near, far))
    assert abs(float(d_near) - float(d_far)) <= 1e-12              # the same multiset of terms, summed in another order
    h_near, h_far = (losses.hausdorff_dt_loss(logits_of(m), y) for m in (near, far))
    assert float(h_far) > float(h_near) > 0.0
    assert float(h_far) > 50.0 * float(h_near)                     # squared distances: 1 .. 4 voxels against 21 .. 22
    exact = losses.hausdorff_dt_loss(logits_of(y), y)
    assert float(exact) < float(h_near)
