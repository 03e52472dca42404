"""CPU: the float64 references of the signed distance maps and the boundary term (tests/distmap_ref.py), the bars that
tests/test_hip_distmap.py applies to csrc/distmap.hip, and the package's host side.

1. the map reference (scipy) against all-pairs distances on small volumes, and its two zero cases;
2. the loss reference's hand-written gradient against autograd in float64; plain f32 torch inside every bar on every case
   the GPU file runs; three plausible kernel bugs outside them;
3. the package on the CPU: the plain-torch path of ``boundary_loss`` with ``dist=``, ``SegLossSpec`` validation, the
   argument checks of the two public functions, the header and the ABI."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distmap_ref as R  # noqa: E402

from conftest import ROOT  # noqa: E402

F32, F64 = torch.float32, torch.float64
BOOLS = (False, True)


# =============================================================================================
# 1. the map reference
# =============================================================================================
@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), R.ANISO], ids=["unit", "aniso"])
@pytest.mark.parametrize("case", R.LABEL_CASES)
def test_map_reference_is_the_all_pairs_distance(case, spacing):
    R.ndi()
    for B, C, dims in ((2, 3, (6, 5, 7)), (1, 2, (1, 1, 9))):
        y = R.labels(case, B, C, dims)
        for bg in BOOLS:
            a = R.MapRef(y, C, spacing, bg, R.IGNORE)
            b = R.MapRef(y, C, spacing, bg, R.IGNORE, edt=R.edt_brute(spacing))
            assert np.array_equal(a.zero, b.zero) and np.array_equal(a.inside, b.inside)
            assert float(np.abs(a.phi - b.phi).max()) <= 1e-12 * max(1.0, float(np.abs(b.phi).max())), (case, dims, bg)
            if spacing[0] == 1.0:
                assert np.array_equal(np.rint(a.d2), np.rint(b.d2)) and float(np.abs(a.d2 - np.rint(a.d2)).max()) < 1e-9


def test_label_cases_are_what_their_names_say():
    R.ndi()
    B, C, dims = R.SHAPES[0]
    ref = lambda case, bg=False: R.MapRef(R.labels(case, B, C, dims), C, (1, 1, 1), bg, R.IGNORE)  # noqa: E731
    absent = ref("absent")
    assert absent.zero[0, 0] and not absent.zero[1, 0] and not absent.phi[0, 0].any()
    full = ref("full")
    assert full.zero[0, 0] and full.inside[0, 0].all() and not full.phi[0, 0].any() and full.zero[0, 1]
    corner = ref("corner")
    assert int(corner.inside[0, C - 2].sum()) == 1 and corner.inside[0, C - 2, -1, -1, -1]
    assert abs(corner.phi[0, C - 2, 0, 0, 0] - np.sqrt(sum((n - 1) ** 2 for n in dims))) < 1e-12
    assert corner.phi[0, C - 2, -1, -1, -1] == 0.0
    faces = ref("faces").inside[:, 0]
    assert faces[:, 0].all() and faces[:, -1].all() and faces[:, :, 0].all() and faces[:, :, -1].all()
    assert faces[..., 0].all() and faces[..., -1].all() and not faces.all()
    checker = ref("checker", True)
    assert float(np.abs(checker.phi).max()) == 1.0 and set(np.unique(checker.phi)) == {0.0, 1.0}
    y = R.labels("bad", B, C, dims)
    assert all(bool((y == v).any()) for v in (255.0, 1.5, -1.0))
    bad = ref("bad")
    assert not bad.inside[0][:, (y[0] == 255.0).numpy()].any()     # an ignored voxel is in no class: outside for every class
    assert float(bad.phi[0, 0][(y[0] == 1.5).numpy()].min()) > 0.0


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
        z, y, phi, ig = R.loss_case(shape, bg, sat)
        w = float(np.float32(0.37))
        l64, g64, A = R.boundary_ref(z, y, phi, bg, ig, 0.37)
        zz = z.double().requires_grad_(True)
        C, c0 = z.shape[-1], 0 if bg else 1
        valid = R.is_class(y, C, ig).double()
        p = torch.softmax(zz, -1)
        want = w * ((p * R.phit_of(phi.double(), C, c0)).sum(-1) * valid).sum() / ((C - c0) * valid.sum())
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
        z, y, phi, ig = R.loss_case(shape, bg, sat)
        for w in (None, 0.37):
            ref = R.BoundaryRef(z, y, phi, bg, ig, w)
            f32_inside(ref, f"{R.ids_shape(shape)} bg {bg} saturated {sat} weight {w}")
            worst = max(worst, ref.bar_norm)
        zero = R.BoundaryRef(z, y, phi, bg, ig, 0.0)
        assert zero.zero and float(zero.l64) == 0.0 and not bool(zero.g32.abs().max() > 0)
    print(f"loosest per-element bar: {worst:.2e} of max |g|")
    z, y, phi, ig = R.loss_case(R.SHAPES[0], False, all_ignored=True)
    ref = R.BoundaryRef(z, y, phi, False, ig)
    assert ref.zero and float(ref.l64) == 0.0 and float(ref.l32) == 0.0 and not bool(phi.abs().max() > 0)


def assert_located_fails(bad_l, bad_g, ref, what):
    print(f"{what}: value off by {abs(float(bad_l) - float(ref.l64)):.2e}, rel_l2 {R.rel_l2(bad_g, ref.g64):.2e}; "
          f"per-element bar {ref.bar_norm:.2e} of max |g|")
    with pytest.raises(AssertionError, match="leave the bound of the float64 reference"):
        R.assert_within_located(bad_g, ref.g64, ref.bar_abs, "bvc", what)


@pytest.mark.parametrize("bg", BOOLS)
def test_the_minus_one_applied_outside_instead_of_inside(bg):
    R.ndi()
    shape = R.SHAPES[0]
    z, y, phi, ig = R.loss_case(shape, bg)
    ref = R.BoundaryRef(z, y, phi, bg, ig)
    maps = R.MapRef(R.labels("bad", *shape, seed=3), shape[1], (1, 1, 1), bg, ig)
    d = np.sqrt(maps.d2)
    wrong = np.where(maps.inside, -d, d - 1.0) * ~maps.zero[:, :, None, None, None]
    bad_l, bad_g, _ = R.boundary_ref(z, y, torch.from_numpy(wrong).reshape(phi.shape), bg, ig)
    # the bug moves phi by -1 at every voxel of a class that is neither empty nor the sample: the value bar sees that; with
    # the background included and every class present the shift is common to all classes and the softmax gradient is blind to it
    assert not abs(float(bad_l) - float(ref.l64)) <= R.VALUE_BAR * max(1.0, ref.A)
    if bg:
        print(f"-1 outside, background included: value off by {abs(float(bad_l) - float(ref.l64)):.2e}, gradient rel_l2 "
              f"{R.rel_l2(bad_g, ref.g64):.2e}")
    else:
        assert_located_fails(bad_l, bad_g, ref, "-1 outside")


@pytest.mark.parametrize("bg", BOOLS)
def test_the_mean_over_all_voxels_instead_of_the_valid_ones(bg):
    R.ndi()
    z, y, phi, ig = R.loss_case(R.SHAPES[0], bg)
    ref = R.BoundaryRef(z, y, phi, bg, ig)
    assert_located_fails(*R.boundary_ref(z, y, phi, bg, ig, all_voxels=True)[:2], ref, "mean over all voxels")


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[4]], ids=R.ids_shape)
def test_phi_indexed_with_c_instead_of_c_minus_c0(shape):
    R.ndi()
    z, y, phi, ig = R.loss_case(shape, False)
    ref = R.BoundaryRef(z, y, phi, False, ig)
    assert_located_fails(*R.boundary_ref(z, y, phi, False, ig, shift=1)[:2], ref, "phi[c] for phi[c - c0]")


# =============================================================================================
# 3. the package on the CPU
# =============================================================================================
@pytest.mark.parametrize("bg", BOOLS)
def test_boundary_loss_on_the_cpu_with_dist_is_the_reference(bg):
    R.ndi()
    from mivp_amd import losses
    shape = R.SHAPES[2]
    B, C, dims = shape
    z, y, phi, ig = R.loss_case(shape, bg)
    ref = R.BoundaryRef(z, y, phi, bg, ig, 0.37)
    K = phi.shape[1]
    for dtype, tol in ((F64, 1e-10), (F32, None)):
        base = z.to(dtype).view(B, *dims, C).clone().requires_grad_(True)
        got = losses.boundary_loss(base.permute(0, 4, 1, 2, 3), y.view(B, 1, *dims), include_background=bg, ignore_index=ig,
                                   dist=phi.view(B, K, *dims), weight=torch.tensor([0.37]))
        got.backward()
        grad = base.grad.view(B, -1, C)
        if tol is not None:
            assert got.dtype == F64 and abs(float(got.detach()) - float(ref.l64)) <= tol * max(1.0, ref.A)
            assert float((grad - ref.g64).abs().max()) <= tol * ref.scale
        else:
            assert got.dtype == F32 and abs(float(got.detach()) - float(ref.l64)) <= R.VALUE_BAR * max(1.0, ref.A)
            R.assert_within_located(grad, ref.g64, ref.bar_abs, "bvc", "f32 package composition")
    with pytest.raises(RuntimeError, match="needs dist="):
        losses.boundary_loss(base.permute(0, 4, 1, 2, 3), y.view(B, 1, *dims))


@pytest.mark.parametrize("bad,name", [
    (dict(lambda_boundary=-0.5), "lambda_boundary"), (dict(lambda_boundary=float("nan")), "lambda_boundary"),
    (dict(lambda_boundary=float("inf")), "lambda_boundary"), (dict(lambda_boundary=1e39), "lambda_boundary"),
    (dict(lambda_boundary="1"), "lambda_boundary"), (dict(lambda_boundary=True), "lambda_boundary"),
    (dict(boundary_spacing=(1.0, 1.0)), "spacing"), (dict(boundary_spacing=(1.0, 0.0, 1.0)), "spacing"),
    (dict(boundary_spacing=(1.0, -2.0, 1.0)), "spacing"), (dict(boundary_spacing=(1.0, float("inf"), 1.0)), "spacing"),
    (dict(boundary_spacing=2.0), "spacing"), (dict(boundary_spacing=(1.0, 1e39, 1.0)), "spacing"),
    (dict(lambda_region=0.0, lambda_voxel=0.0), "lambda_region and lambda_voxel and lambda_boundary"),
    (dict(lambda_region=0, lambda_voxel=0, lambda_boundary=0), "must not all be 0"),
    (dict(top_k=0.5, lambda_boundary=0.1), "top_k together with lambda_boundary"),
])
def test_spec_refuses_each_invalid_boundary_option_by_name(bad, name):
    from mivp_amd.losses import SegLossSpec
    with pytest.raises(ValueError, match=name):
        SegLossSpec(**bad)


def test_spec_defaults_are_unchanged_and_the_new_fields_are_values():
    from mivp_amd import losses
    d = losses.SegLossSpec()
    assert (d.alpha, d.beta, d.batch, d.include_background, d.focal_gamma, d.class_weights, d.ignore_index, d.lambda_region,
            d.lambda_voxel, d.top_k) == (0.5, 0.5, False, True, 0.0, None, None, 1.0, 1.0, None)
    assert d.lambda_boundary == 0.0 and d.boundary_spacing == (1.0, 1.0, 1.0)
    a = losses.SegLossSpec(lambda_boundary=1, boundary_spacing=[0.8, 0.8, 2.5])
    assert a == losses.SegLossSpec(lambda_boundary=1.0, boundary_spacing=(0.8, 0.8, 2.5)) and hash(a) == hash(
        losses.SegLossSpec(lambda_boundary=1.0, boundary_spacing=(0.8, 0.8, 2.5))) and a != d
    assert "lambda_boundary=1.0" in repr(a) and repr(d).startswith("SegLossSpec(alpha=0.5, beta=0.5, batch=False")
    only = losses.SegLossSpec(lambda_region=0.0, lambda_voxel=0.0, lambda_boundary=0.5)      # the boundary term alone
    assert only.lambda_boundary == 0.5
    mod = losses.SegLoss(lambda_boundary=0.5)
    assert tuple(mod.boundary_weight.shape) == (1,) and float(mod.boundary_weight) == 1.0
    assert "boundary_weight" in dict(mod.named_buffers()) and "boundary_weight" not in mod.state_dict()
    mod.set_boundary_weight(0.25)
    assert float(mod.boundary_weight) == 0.25
    with pytest.raises(ValueError, match="boundary weight"):
        mod.set_boundary_weight(float("nan"))
    z, y = torch.zeros(2, 2, 2, 2, 2), torch.zeros(2, 1, 2, 2, 2)
    with pytest.raises(RuntimeError, match="built on the GPU"):
        mod(z, y)
    assert torch.equal(losses.SegLoss()(z, y), losses.seg_loss(z, y, d))          # lambda_boundary = 0: the path as before


def test_public_functions_check_their_arguments():
    from mivp_amd import losses
    y = torch.zeros(2, 1, 3, 4, 5)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        losses.signed_distance_maps(y, 2)
    for kw, err, name in ((dict(spacing=(1.0, 1.0)), ValueError, "spacing"), (dict(spacing=(1.0, 0.0, 1.0)), ValueError, "spacing"),
                          (dict(num_classes=0), ValueError, "num_classes"), (dict(num_classes=17), ValueError, "num_classes")):
        args = dict(num_classes=2)
        args.update(kw)
        with pytest.raises(err, match=name):
            losses.signed_distance_maps(y, **args)
    z = torch.zeros(2, 2, 3, 4, 5)
    with pytest.raises(ValueError, match="logits"):
        losses.boundary_loss(z[0], y)
    with pytest.raises(ValueError, match="target"):
        losses.boundary_loss(z, y[:, :, :2])
    with pytest.raises(ValueError, match="at least 2 classes"):
        losses.boundary_loss(z[:, :1], y)
    with pytest.raises(ValueError, match="include_background"):
        losses.boundary_loss(z, y, include_background=1)
    with pytest.raises(ValueError, match="ignore_index"):
        losses.boundary_loss(z, y, ignore_index=1.5)
    with pytest.raises(ValueError, match="spacing"):
        losses.boundary_loss(z, y, spacing=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="dist"):
        losses.boundary_loss(z, y, dist=torch.zeros(2, 2, 3, 4, 5))              # K = 1 without the background
    with pytest.raises(ValueError, match="weight"):
        losses.boundary_loss(z, y, dist=torch.zeros(2, 1, 3, 4, 5), weight=torch.ones(2))
    assert float(losses.boundary_loss(z, y, dist=torch.zeros(2, 1, 3, 4, 5))) == 0.0


def test_header_declares_the_entries_and_the_abi_stays_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    P = _lib.parse_header()
    want = {"mivp_distmap_ws": (3, _lib.C.c_size_t), "mivp_distmap_signed": (11, _lib.C.c_int),
            "mivp_boundary_loss_ws": (2, _lib.C.c_size_t), "mivp_boundary_loss": (16, _lib.C.c_int),
            "mivp_boundary_loss_grad": (16, _lib.C.c_int)}
    for name, (n, ret) in want.items():
        assert len(P[name][1]) == n and P[name][0] is ret, name
    assert sorted(n for n in P if n.startswith(("mivp_distmap", "mivp_boundary"))) == sorted(want)


def test_entries_refuse_what_the_host_refuses():
    """MIVP_REQUIRE returns before anything is launched or dereferenced: the pointers are never read."""
    from mivp_amd import _lib as L
    from mivp_amd._host import i3
    lib = L.lib()
    assert int(lib.mivp_distmap_ws(2, 3, i3((5, 6, 7)))) == (2 * 2 * 3 * 210 * 4 + 255) // 256 * 256 + 2 * 2 * 3 * 210 * 8
    for B, K, dims in ((0, 1, (5, 6, 7)), (1, 0, (5, 6, 7)), (1, 17, (5, 6, 7)), (1, 1, (65536, 1, 1)), (1, 1, (1, 65536, 1)),
                       (1, 1, (0, 4, 4)), (4, 2, (1024, 1024, 256))):
        assert int(lib.mivp_distmap_ws(B, K, i3(dims))) == 0, (B, K, dims)
    for B, vol, rows in ((3, 63, 3), (2, 2053, 6), (2, 66 * 64 * 64, 512)):
        assert int(lib.mivp_boundary_loss_ws(B, vol)) == 2 * rows + 4
    p = 4096                                                       # a non-NULL address that no accepted call would be given
    sp = (L.C.c_float * 3)(1.0, 1.0, 1.0)
    for B, C, bg, dims, spc in ((0, 2, 0, (4, 4, 4), sp), (1, 1, 0, (4, 4, 4), sp), (1, 18, 0, (4, 4, 4), sp),
                                (1, 2, 0, (65536, 1, 1), sp), (1, 2, 0, (4, 4, 4), (L.C.c_float * 3)(1.0, 0.0, 1.0)),
                                (1, 2, 0, (4, 4, 4), (L.C.c_float * 3)(1.0, float("inf"), 1.0))):
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_distmap_signed", p, B, C, bg, 0, 0, i3(dims), spc, p, p, None)
    for B, vol, C, lam in ((0, 8, 2, 1.0), (2, 0, 2, 1.0), (2, 8, 1, 1.0), (2, 8, 9, 1.0), (2, 8, 2, -1.0), (2, 8, 2, float("nan"))):
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_boundary_loss", p, p, p, B, vol, C, 0, 0, 0, lam, None, p, p, None, 0, None)
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_boundary_loss_grad", p, p, p, B, vol, C, 0, 0, 0, lam, None, p, None, p, 0, None)
    with pytest.raises(RuntimeError, match="contract violated"):
        L.call("mivp_boundary_loss", p, p, None, 2, 8, 2, 0, 0, 0, 1.0, None, p, p, None, 0, None)
