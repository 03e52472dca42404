"""CPU: the float64 reference of the Tversky + weighted cross-entropy loss (tests/segloss_ref.py), the bars that
tests/test_hip_segloss.py applies to csrc/segloss.hip, and the package's host side.

1. the reference against independent definitions in float64, to 1e-12: ``F.cross_entropy(weight=, ignore_index=)`` at
   gamma = 0, the sibling loss's Dice (``dice_focal_ref64(gamma=-1)``) at alpha = beta = 0.5, and the closed-form gradient
   against autograd for every option;
2. plain f32 torch stays inside every bound on 100 % of the elements of every case the GPU file runs (the cases are imported
   from segloss_ref.py), and no per-element bar is looser than 1e-4 of max |g| (2.3e-4 where the logits saturate, see there);
3. the bars see what a plausible kernel bug does: each corruption is applied to the float64 closed form through its hooks
   and must make the located check fail;
4. the package on the CPU: ``seg_loss`` takes the plain-torch composition and agrees with the reference, ``SegLossSpec``
   refuses each invalid option by name, ``train.step_loss`` with and without ``conf.seg_loss``, the header and the ABI."""
import os
import sys
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_optim_ref as R0  # noqa: E402
import segloss_ref as R  # noqa: E402

from conftest import ROOT  # noqa: E402

F32, F64 = torch.float32, torch.float64
ids_dims = lambda d: "x".join(str(v) for v in d)  # noqa: E731


def tight(got, want, what, tol=1e-12):
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: off by {err:.3e} (scale {scale:.3e})"


# =============================================================================================
# 1. the reference against independent definitions
# =============================================================================================
@pytest.mark.parametrize("ignore", R.IGNORES)
@pytest.mark.parametrize("weighted", [False, True])
def test_voxel_term_is_torch_cross_entropy_at_gamma_zero(weighted, ignore):
    B, vol, C = 3, 63, 4
    w = R.WEIGHTS8[:C] if weighted else None
    o = R.opts(class_weights=w, ignore_index=ignore, lambda_region=0.0)
    z, y = R.seg_inputs(B, vol, C, 3, "plain" if ignore is None else "sample_ignored", ignore)
    l64, g64 = R.seg_loss_ref64(z, y, o)
    zz = z.double().clone().requires_grad_(True)
    want = F.cross_entropy(zz.reshape(-1, C), y.reshape(-1).long(), weight=None if w is None else torch.tensor(w, dtype=F64),
                           ignore_index=-100 if ignore is None else ignore, reduction="mean")
    want.backward()
    assert abs(float(l64) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want)))
    tight(g64, zz.grad, f"cross-entropy gradient, weights {weighted}, ignore {ignore}")
    if ignore is not None:
        assert not bool(g64[1].abs().max() > 0) and not bool(g64[y == ignore].abs().max() > 0)


@pytest.mark.parametrize("bg", [True, False])
@pytest.mark.parametrize("C", [2, 5])
def test_region_term_is_the_projects_dice_at_alpha_beta_half(C, bg):
    z, y = R.seg_inputs(3, 315, C, 4)
    l64, g64 = R.seg_loss_ref64(z, y, R.opts(include_background=bg, lambda_voxel=0.0))
    want_l, want_g = R0.dice_focal_ref64(z, y, bg, -1.0)
    assert abs(float(l64 - want_l)) <= 1e-12
    tight(g64, want_g, f"Dice gradient C {C} bg {bg}")


@pytest.mark.parametrize("C", R.PRODUCT_CLASSES)
@pytest.mark.parametrize("ignore", R.IGNORES)
def test_closed_form_is_the_autograd_gradient_for_every_option(ignore, C):
    z, y = R.ladder_case((5, 7, 9), C, R.opts(ignore_index=ignore))
    for o in R.product_options(C, ignore):
        _, g64 = R.seg_loss_ref64(z, y, o)
        closed = R.seg_grad_closed(z, y, o)
        assert float((closed - g64).abs().max()) <= 1e-12 * float(g64.abs().max()), R.opts_name(o)


def test_closed_form_on_the_special_operands():
    for i, (name, C, kind, o) in enumerate(R.special_cases()):
        z, y = R.special_inputs(i, 315)
        l64, g64 = R.seg_loss_ref64(z, y, o)
        closed = R.seg_grad_closed(z, y, o)
        assert bool(torch.isfinite(g64).all()) and bool(torch.isfinite(l64)), name
        assert float((closed - g64).abs().max()) <= 1e-12 * max(float(g64.abs().max()), 1e-300), name
        invalid = ~R.valid_mask(y, C, o["ignore_index"])
        assert not bool(g64[invalid].abs().max() > 0) if bool(invalid.any()) else True, name


def test_special_operands_are_what_their_names_say():
    cases = {name: (i, C, kind, o) for i, (name, C, kind, o) in enumerate(R.special_cases())}
    i, C, _, o = cases["batch ignored"]
    z, y = R.special_inputs(i, 336)
    ref = R.SegRef(z, y, o)
    assert ref.zero and float(ref.l64) == 0.0 and float(ref.l32) == 0.0 and bool((y == 255).all())
    i, C, _, o = cases["only zero-weight classes, voxel alone"]
    z, y = R.special_inputs(i, 336)
    ref = R.SegRef(z, y, o)
    valid = R.valid_mask(y, C, 255)
    assert ref.zero and float(ref.l64) == 0.0 and bool(valid.any()) and float(y[valid].max()) <= 1.0
    i, C, _, o = cases["only zero-weight classes"]
    ref = R.SegRef(*R.special_inputs(i, 336), o)
    assert not ref.zero                                            # the region term still trains
    i, C, _, o = cases["sample ignored"]
    z, y = R.special_inputs(i, 315)
    assert bool((y[1] == 255).all()) and not bool(R.SegRef(z, y, o).g64[1].abs().max() > 0)
    i, C, _, o = cases["absent class"]
    z, y = R.special_inputs(i, 315)
    assert float(R.seg_stats(z, y, o)[2][:, C - 2].sum()) == 0.0
    i, C, _, o = cases["bad labels"]
    z, y = R.special_inputs(i, 315)
    frac = float((~R.is_class(y, C)).double().mean())
    assert 0.2 < frac < 0.45 and bool((y == 0.5).any()) and bool((y == float(C)).any()) and bool((y < 0).any())
    i, C, _, o = cases["saturated g1"]
    z, y = R.special_inputs(i, 315)
    assert float(z.abs().max()) == 30.0 and 0.2 < float((z.abs() == 30.0).double().mean()) < 0.3
    i, C, _, o = cases["quad and tail ignored"]
    for vol in R.SPECIAL_VOLS:
        z, y = R.special_inputs(i, vol)
        ig = y == 255
        tail = vol % 4 or 4
        assert bool(ig[1, 4:8].all()) and bool(ig[:, vol - tail:].all()) and int(ig.sum()) == 4 + 3 * tail


# =============================================================================================
# 2. f32 torch inside every bound, on the GPU file's cases
# =============================================================================================
# The yardstick is autograd in f32.  Where |log p_y| reaches 60 (logits at +-30) the focal factor's backward adds terms of size
# gamma |log p_y| <= 120 that cancel to O(1): a few roundings of 120 x 2^-24 = 7e-6 each, so E32 may reach ~3e-5 there and the
# per-element bar 8 E32 ~ 2.5e-4.  Everywhere else the per-element bar has to be tighter than the aggregate 1e-4.
SATURATED_BAR = 8 * 4 * 120 * R.U32


def f32_inside(z, y, o, what, bar_cap=1e-4):
    ref = R.SegRef(z, y, o)
    assert bool(torch.isfinite(ref.g32).all()) and bool(torch.isfinite(ref.l32)), what
    assert abs(float(ref.l32) - float(ref.l64)) <= R.LOSS_VALUE_BAR * max(1.0, abs(float(ref.l64))), what
    if ref.zero:
        assert not bool(ref.g32.abs().max() > 0), what
        return 0.0
    assert ref.bar_norm <= bar_cap, (what, ref.bar_norm)
    assert R.rel_l2(ref.g32, ref.g64) < R.LOSS_L2_BAR, what
    R.assert_within_located(ref.g32, ref.g64, ref.bar_abs, "bvc", what)
    return ref.bar_norm


@pytest.mark.parametrize("dims", R.SCALAR_VOLS + R.VEC_VOLS, ids=ids_dims)
def test_f32_torch_meets_the_bars_on_the_ladder(dims):
    worst = 0.0
    for C in R.CLASSES:
        for o in R.ladder_options(C):
            z, y = R.ladder_case(dims, C, o)
            worst = max(worst, f32_inside(z, y, o, f"{dims} C {C} {R.opts_name(o)}"))
    print(f"{dims}: loosest per-element bar over C, options: {worst:.2e} of max |g|")


@pytest.mark.parametrize("ignore", R.IGNORES)
@pytest.mark.parametrize("dims", R.PRODUCT_DIMS, ids=ids_dims)
@pytest.mark.parametrize("C", R.PRODUCT_CLASSES)
def test_f32_torch_meets_the_bars_on_the_full_product(C, dims, ignore):
    z, y = R.ladder_case(dims, C, R.opts(ignore_index=ignore))
    for o in R.product_options(C, ignore):
        f32_inside(z, y, o, f"{dims} C {C} {R.opts_name(o)}")


def test_f32_torch_meets_the_bars_on_the_special_operands():
    for vol in R.SPECIAL_VOLS:
        for i, (name, C, kind, o) in enumerate(R.special_cases()):
            f32_inside(*R.special_inputs(i, vol), o, f"{name} vol {vol}", SATURATED_BAR if kind == "saturated" else 1e-4)
    for vol in R.FORMS_VOLS:
        f32_inside(*R.forms_case(vol), f"forms {vol}")
    for dims in R.WRAPPER_DIMS:
        f32_inside(*R.wrapper_case(dims), f"wrappers {dims}")


@pytest.mark.parametrize("C", R.PRODUCT_CLASSES)
def test_f32_torch_meets_the_bars_on_several_partial_rows(C):
    for vol, _ in R.PARTIAL_ROW_VOLS:
        for o in (R.opts(), R.big_options(C)):
            z, y = R.seg_inputs(2, vol, C, vol + C, "plain" if o["ignore_index"] is None else "ignored", o["ignore_index"])
            f32_inside(z, y, o, f"vol {vol} C {C} {R.opts_name(o)}")


@pytest.mark.parametrize("vol", [R.CAP_VOL, R.GRID_CAP_DIMS[0] * R.GRID_CAP_DIMS[1] * R.GRID_CAP_DIMS[2]], ids=["cap", "grid"])
def test_f32_torch_meets_the_bars_on_the_large_cases(vol):
    o = R.big_options()
    z, y = R.seg_inputs(2, vol, 2, vol + 2, "ignored", o["ignore_index"])
    f32_inside(z, y, o, f"vol {vol}")


# =============================================================================================
# 3. corruptions
# =============================================================================================
def corruption_case(o, B=3, vol=315, C=3, seed=9, kind=None):
    ig = o["ignore_index"]
    z, y = R.seg_inputs(B, vol, C, seed, kind or ("plain" if ig is None else "ignored"), ig)
    ref = R.SegRef(z, y, o)
    good = R.seg_grad_closed(z, y, o)
    R.assert_within_located(good, ref.g64, ref.bar_abs, "bvc", "the closed form against its own bar")
    return z, y, ref


def assert_located_fails(bad, ref, what):
    print(f"{what}: rel_l2 {R.rel_l2(bad, ref.g64):.2e}; per-element bar {ref.bar_norm:.2e} of max |g|")
    with pytest.raises(AssertionError, match="leave the bound of the float64 reference"):
        R.assert_within_located(bad, ref.g64, ref.bar_abs, "bvc", what)


W3 = (0.5, 2.0, 1.0)


def one_ignored_voxel(y, ig):
    at = torch.nonzero(y == ig)
    assert at.shape[0] > 10
    return tuple(int(v) for v in at[at.shape[0] // 2])


def test_one_ignored_voxel_counted_in_P():
    o = R.opts(0.3, 0.7, False, True, 1.0, W3, 255)
    z, y, ref = corruption_case(o)
    mask = R.valid_mask(y, 3, 255).clone()
    mask[one_ignored_voxel(y, 255)] = True
    bad = R.seg_grad_closed(z, y, o, stats=R.seg_stats(z, y, o, p_valid=mask))
    assert_located_fails(bad, ref, "an ignored voxel in P")


def test_one_ignored_voxel_receives_the_cross_entropy_gradient_of_class_0():
    o = R.opts(0.5, 0.5, False, True, 0.0, W3, 255)
    z, y, ref = corruption_case(o)
    at = one_ignored_voxel(y, 255)
    mask = R.valid_mask(y, 3, 255).clone()
    mask[at] = True
    bad = R.seg_grad_closed(z, y, o, voxel_valid=mask)
    changed = torch.nonzero((bad - ref.g64).abs().amax(-1) > 1e-15)
    assert changed.shape[0] == 1 and tuple(int(v) for v in changed[0]) == at
    assert_located_fails(bad, ref, "an ignored voxel trained as class 0")


def test_normalising_by_the_valid_voxel_count_instead_of_the_weight_sum():
    o = R.opts(0.5, 0.5, False, True, 2.0, W3, -1)
    z, y, ref = corruption_case(o)
    count = float(R.valid_mask(y, 3, -1).sum())
    bad = R.seg_grad_closed(z, y, o, wsum=count)
    assert_located_fails(bad, ref, "count instead of the weight sum")
    # with unit weights the two are the same number: the corruption needs the weighted cases to be seen
    o1 = R.opts(0.5, 0.5, False, True, 2.0, None, -1)
    ref1 = R.SegRef(z, y, o1)
    R.assert_within_located(R.seg_grad_closed(z, y, o1, wsum=count), ref1.g64, ref1.bar_abs, "bvc", "unit weights")


def test_the_weight_of_the_neighbouring_class():
    o = R.opts(0.3, 0.7, True, False, 1.0, W3, None)
    z, y, ref = corruption_case(o)
    bad = R.seg_grad_closed(z, y, o, voxel_weights=W3[1:] + W3[:1])
    assert_located_fails(bad, ref, "the neighbouring class's weight")


def test_batch_statistics_taken_from_the_voxels_own_sample():
    o = R.opts(0.3, 0.7, True, True, 0.0, None, 255)
    z, y, ref = corruption_case(o)
    own = R.seg_stats(z, y, dict(o, batch=False))
    bad = R.seg_grad_closed(z, y, o, stats=own, sample_of=torch.arange(3).unsqueeze(1).expand(3, 315))
    assert_located_fails(bad, ref, "per-sample sums under batch")


def test_alpha_and_beta_exchanged():
    o = R.opts(0.3, 0.7, False, False, 2.0, W3, 255)
    z, y, ref = corruption_case(o)
    bad = R.seg_grad_closed(z, y, dict(o, alpha=0.7, beta=0.3))
    assert_located_fails(bad, ref, "alpha and beta exchanged")


def test_region_constants_of_the_neighbouring_sample_for_one_quad():
    o = R.opts(0.3, 0.7, False, True, 1.0, (0.5, 2.0), 255)
    B, vol = 2, 2052
    z, y, ref = corruption_case(o, B=B, vol=vol, C=2, seed=10)
    y = y.clone()
    y[1, :4] = torch.tensor([0.0, 1.0, 1.0, 0.0])                  # the quad behind the sample boundary is valid
    ref = R.SegRef(z, y, o)
    sample_of = torch.arange(B).unsqueeze(1).expand(B, vol).clone()
    sample_of[1, :4] = 0
    bad = R.seg_grad_closed(z, y, o, sample_of=sample_of)
    changed = (bad - R.seg_grad_closed(z, y, o)).abs().amax(-1) > 0
    assert int(changed.sum()) == 4 and bool(changed[1, :4].all())
    err = R.rel_l2(bad, ref.g64)
    assert err < R.LOSS_L2_BAR, "the corruption is louder than the aggregate bar: it would not need the located one"
    assert_located_fails(bad, ref, "wrong sample's region constants")


def test_an_unwritten_tail_of_an_odd_volume():
    o = R.opts(0.3, 0.7, False, True, 1.0, (0.5, 2.0), 255)
    z, y, ref = corruption_case(o, B=3, vol=1027, C=2, seed=11)
    tail_valid = R.valid_mask(y, 2, 255)[:, 1027 - 3:]
    assert bool(tail_valid.any())
    for stale in (float("nan"), 0.0):                              # what the buffer held before: the tests' NaN, or zeros
        bad = ref.g64.clone()
        bad[:, 1027 - 3:] = stale
        assert_located_fails(bad, ref, f"unwritten tail ({stale})")


# =============================================================================================
# 4. the package on the CPU
# =============================================================================================
def spec_of(o):
    from mivp_amd.losses import SegLossSpec
    return SegLossSpec(**o)


def package_grad(z, y, o, dims, dtype=F64, module=False):
    from mivp_amd import losses
    B, vol, C = z.shape
    base = z.to(dtype).view(B, *dims, C).clone().requires_grad_(True)
    logits = base.permute(0, 4, 1, 2, 3)
    target = y.view(B, 1, *dims)
    got = losses.SegLoss(spec_of(o))(logits, target) if module else losses.seg_loss(logits, target, spec_of(o))
    got.backward()
    return got.detach(), base.grad.view(B, vol, C)


@pytest.mark.parametrize("C", [2, 5, 8])
def test_seg_loss_on_the_cpu_is_the_reference(C):
    dims = (5, 7, 9)
    for k, o in enumerate(R.ladder_options(C)):
        z, y = R.ladder_case(dims, C, o)
        l64, g64 = R.seg_loss_ref64(z, y, o)
        got_l, got_g = package_grad(z, y, o, dims, module=bool(k % 2))
        assert got_l.dtype == F64 and abs(float(got_l - l64)) <= 1e-10 * max(1.0, abs(float(l64))), R.opts_name(o)
        tight(got_g, g64, R.opts_name(o), 1e-10 * float(g64.abs().max()))


def test_seg_loss_on_the_cpu_special_operands():
    for i, (name, C, kind, o) in enumerate(R.special_cases()):
        z, y = R.special_inputs(i, 315)
        l64, g64 = R.seg_loss_ref64(z, y, o)
        got_l, got_g = package_grad(z, y, o, (5, 7, 9))
        assert bool(torch.isfinite(got_l)) and abs(float(got_l - l64)) <= 1e-10 * max(1.0, abs(float(l64))), name
        tight(got_g, g64, name, 1e-10 * max(float(g64.abs().max()), 1e-30))
        invalid = ~R.valid_mask(y, C, o["ignore_index"])
        if bool(invalid.any()):
            assert not bool(got_g[invalid].abs().max() > 0), name
    # f32 logits, a [B, H, W, D] integer target and a weight tensor given at the call
    from mivp_amd import losses
    z, y, o = R.wrapper_case((5, 7, 9))
    base = z.view(3, 5, 7, 9, 4).clone().requires_grad_(True)
    got = losses.seg_loss(base.permute(0, 4, 1, 2, 3), y.view(3, 5, 7, 9).long(), spec_of(dict(o, class_weights=None)),
                          class_weights=torch.tensor(o["class_weights"]))
    got.backward()
    ref = R.SegRef(z, y, o)
    assert got.dtype == F32 and abs(float(got) - float(ref.l64)) <= R.LOSS_VALUE_BAR * max(1.0, abs(float(ref.l64)))
    R.assert_within_located(base.grad.view(3, 315, 4), ref.g64, ref.bar_abs, "bvc", "f32 package composition")


@pytest.mark.parametrize("bad,name", [
    (dict(alpha=-0.1), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(beta=-1), "beta"), (dict(beta=float("inf")), "beta"),
    (dict(beta="0.5"), "beta"), (dict(batch=1), "batch"), (dict(include_background="yes"), "include_background"),
    (dict(focal_gamma=0.5), "focal_gamma"), (dict(focal_gamma=-1.0), "focal_gamma"), (dict(focal_gamma=True), "focal_gamma"),
    (dict(class_weights=(1.0, -1.0)), r"class_weights\[1\]"), (dict(class_weights=(1.0,)), "class_weights"),
    (dict(class_weights=(1.0,) * 9), "class_weights"), (dict(class_weights=(1.0, float("nan"), 1.0)), r"class_weights\[1\]"),
    (dict(ignore_index=1.5), "ignore_index"), (dict(ignore_index=True), "ignore_index"), (dict(ignore_index=2 ** 24 + 1), "ignore_index"),
    (dict(lambda_region=-1.0), "lambda_region"), (dict(lambda_voxel=float("nan")), "lambda_voxel"),
    (dict(lambda_region=0.0, lambda_voxel=0.0), "lambda_region and lambda_voxel"), (dict(alpha=1e39), "alpha"),
])
def test_spec_refuses_each_invalid_option_by_name(bad, name):
    from mivp_amd.losses import SegLossSpec
    with pytest.raises(ValueError, match=name):
        SegLossSpec(**bad)


def test_spec_is_an_immutable_value_and_seg_loss_checks_its_operands():
    from mivp_amd import losses
    a, b = losses.SegLossSpec(0.3, 0.7, class_weights=[1, 2.0], ignore_index=-1), losses.SegLossSpec(0.3, 0.7, class_weights=(1.0, 2.0), ignore_index=-1)
    assert a == b and hash(a) == hash(b) and a != losses.SegLossSpec() and "alpha=0.3" in repr(a)
    assert losses.SegLossSpec(focal_gamma=1).focal_gamma == 1.0 and losses.SegLossSpec(lambda_voxel=0).lambda_voxel == 0.0
    with pytest.raises(AttributeError):
        a.alpha = 0.5
    z, y = torch.zeros(2, 2, 2, 2, 2), torch.zeros(2, 1, 2, 2, 2)
    with pytest.raises(TypeError, match="SegLossSpec"):
        losses.seg_loss(z, y, dict(alpha=0.5))
    with pytest.raises(ValueError, match="class_weights"):
        losses.seg_loss(z, y, losses.SegLossSpec(class_weights=(1.0, 2.0, 3.0)))
    with pytest.raises(ValueError, match="class_weights"):
        losses.seg_loss(z, y, losses.SegLossSpec(), class_weights=torch.ones(3))
    with pytest.raises(ValueError, match="target"):
        losses.seg_loss(z, y[:, :, :1], losses.SegLossSpec())
    with pytest.raises(ValueError, match="logits"):
        losses.seg_loss(z[0], y, losses.SegLossSpec())
    with pytest.raises(TypeError):
        losses.SegLoss(losses.SegLossSpec(), alpha=0.3)
    mod = losses.SegLoss(alpha=0.3, beta=0.7, class_weights=(1.0, 2.0))
    assert mod.spec == losses.SegLossSpec(0.3, 0.7, class_weights=(1.0, 2.0)) and "class_weights" in dict(mod.named_buffers())
    assert losses.SegLoss().class_weights is None


def test_step_loss_with_and_without_a_seg_loss():
    from mivp_amd import losses, train
    g = R.gen(5)
    B, C, dims = 2, 2, (4, 4, 4)
    logits = torch.randn((B, C) + dims, generator=g)
    y = torch.randint(0, C, (B, 1) + dims, generator=g).float()
    y[0, 0, 0] = 255.0
    conf = Namespace(training_mode="downstream", include_background=True)
    plain = train.step_loss({"downstream": logits}, conf, y.clamp(max=1.0))
    assert torch.equal(plain, train.dice_focal_loss(logits, y.clamp(max=1.0), True, 4.0))
    mod = losses.SegLoss(alpha=0.3, beta=0.7, ignore_index=255, class_weights=(1.0, 2.0))
    conf.seg_loss = mod
    got = train.step_loss({"downstream": logits}, conf, y)
    assert torch.equal(got, losses.seg_loss(logits, y, mod.spec)) and not torch.equal(got, plain)
    want, _ = R.seg_loss_ref64(logits.permute(0, 2, 3, 4, 1).reshape(B, -1, C), y.reshape(B, -1), R.opts(0.3, 0.7, ignore_index=255,
                                                                                                       class_weights=(1.0, 2.0)))
    assert abs(float(got) - float(want)) <= R.LOSS_VALUE_BAR
    del conf.seg_loss
    assert torch.equal(train.step_loss({"downstream": logits}, conf, y.clamp(max=1.0)), plain)
    # the supervised modes read out["seg_pred"]; without the attribute they are the GPU-only Dice as before
    sup = Namespace(training_mode="supervised_learning_all", include_background=True, seg_loss=mod)
    assert torch.equal(train.step_loss({"seg_pred": logits}, sup, y), got)
    del sup.seg_loss
    with pytest.raises(RuntimeError, match="dice_loss runs on the GPU"):
        train.step_loss({"seg_pred": logits}, sup, y)
    ssl = Namespace(training_mode="self_supervised_learning_all", include_background=True, seg_loss=mod)
    with pytest.raises(ValueError, match="students_teacher_step"):
        train.step_loss({"seg_pred": logits}, ssl, y)


def test_header_declares_the_entries_and_the_abi_stays_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    P = _lib.parse_header()
    assert len(P["mivp_seg_loss_ws"][1]) == 2 and P["mivp_seg_loss_ws"][0] is _lib.C.c_size_t
    assert len(P["mivp_seg_loss"][1]) == 19 and len(P["mivp_seg_loss_grad"][1]) == 19
    assert not [n for n in P if n.startswith("mivp_seg_loss") and n not in ("mivp_seg_loss_ws", "mivp_seg_loss", "mivp_seg_loss_grad")]


def test_entries_refuse_the_options_the_host_refuses():
    """MIVP_REQUIRE returns before anything is launched or dereferenced: the pointers are never read."""
    from mivp_amd import _lib as L
    for B, vol, want in ((3, 63, 3 * 2 + 1), (2, 2053, 2 * 4 + 1), (2, R.CAP_VOL, 2 * 257 + 1), (5, 4, 5 * 2 + 1)):
        assert int(L.lib().mivp_seg_loss_ws(B, vol)) == want * 26
    p = 4096                                                       # a non-NULL address that no accepted call would be given
    good = dict(B=2, vol=8, C=3, alpha=0.5, beta=0.5, gamma=0.0, lr=1.0, lv=1.0)
    for change in (dict(C=9), dict(C=1), dict(B=0), dict(vol=0), dict(alpha=-0.5), dict(beta=float("nan")), dict(gamma=0.5),
                   dict(gamma=-1.0), dict(lr=-1.0), dict(lr=0.0, lv=0.0), dict(lv=float("inf"))):
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_seg_loss", p, p, a["B"], a["vol"], a["C"], 1, 0, a["alpha"], a["beta"], a["gamma"], None, 0, 0, a["lr"],
                   a["lv"], p, p, None, None)
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_seg_loss_grad", p, p, a["B"], a["vol"], a["C"], 1, 0, a["alpha"], a["beta"], a["gamma"], None, 0, 0,
                   a["lr"], a["lv"], p, None, p, None)
    with pytest.raises(RuntimeError, match="contract violated"):
        L.call("mivp_seg_loss", None, p, 2, 8, 3, 1, 0, 0.5, 0.5, 0.0, None, 0, 0, 1.0, 1.0, p, p, None, None)
