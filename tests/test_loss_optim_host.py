"""CPU proof of the bars that tests/test_hip_loss_optim.py applies to the loss, optimizer and metric-count kernels.

Two things are shown here, on the float64 references of tests/loss_optim_ref.py alone:

  * the references define the bars: plain f32 torch on the CPU (``torch.optim.AdamW(foreach=False)``, ``tau t + om s``, the
    loss formulas run in f32) stays inside every bound on 100 % of the elements of every case the GPU file uses, and the
    per-element loss bar is never looser than 1e-4 in the normalised max norm;
  * the bars see what a plausible kernel bug does: each corruption below is applied to the float64 reference and must make
    the located check fail.  Where the suite had an aggregate check for the quantity before (rel-L2 < 1e-4 on the loss
    gradient, max |a - b| / max |a| < 2e-6 on the AdamW parameters, allclose(rtol 1e-6, atol 1e-7) on the EMA) and that check
    is blind to the corruption, that is asserted too.  Three corruptions are loud enough for the old bars (an unwritten
    tail, a dropped focal column, a tensor tail that is not stepped): those were never a matter of the bar but of cases
    nobody ran (no odd volume, no size 1024 k + 1), and only the located failure is asserted for them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_optim_ref as R  # noqa: E402

F32, F64 = torch.float32, torch.float64
OLD_ADAM_BAR = 2e-6


def old_adam_check(got, want):
    return float((got - want).abs().max() / want.abs().max())


def old_ema_check(got, want):
    return bool(torch.allclose(got.float(), want.float(), rtol=1e-6, atol=1e-7))


def loss_refs(z, y, inc_bg, gamma):
    l64, g64 = R.dice_focal_ref64(z, y, inc_bg, gamma)
    _, g32 = R.dice_focal_ref64(z, y, inc_bg, gamma, dtype=F32)
    bar_abs, bar_norm = R.loss_grad_bar(g32, g64)
    return l64, g64, g32, bar_abs, bar_norm


def assert_located_fails(bad, g64, bar_abs, what):
    with pytest.raises(AssertionError, match="leave the bound of the float64 reference"):
        R.assert_within_located(bad, g64, bar_abs, "bvc", what)


# =============================================================================================
# the references define the bars
# =============================================================================================
@pytest.mark.parametrize("dims", R.SCALAR_VOLS + R.VEC_VOLS, ids=lambda d: "x".join(str(v) for v in d))
def test_loss_bar_of_every_grid_case_is_tighter_than_the_old_one_and_the_two_derivations_agree(dims):
    vol = dims[0] * dims[1] * dims[2]
    B = 5 if vol == 4 else 3
    worst = 0.0
    for C in R.LOSS_CLASSES:
        z, y = R.loss_inputs(B, vol, C, 1000 * C + vol)
        for inc_bg, gamma in R.LOSS_MODES:
            _, g64, g32, bar_abs, bar_norm = loss_refs(z, y, inc_bg, gamma)
            worst = max(worst, bar_norm)
            assert bar_norm <= 1e-4, (dims, C, inc_bg, gamma, bar_norm)
            R.assert_within_located(g32, g64, bar_abs, "bvc", "the f32 reference against its own bar")
            closed = R.dice_focal_grad_closed(z, y, inc_bg, gamma)
            assert float((closed - g64).abs().max()) <= 1e-12 * float(g64.abs().max()), (dims, C, inc_bg, gamma)
    print(f"vol {vol}: loosest per-element bar over C, modes: {worst:.2e} of max |g|")


@pytest.mark.parametrize("kind,C,gamma", [("sample_bg", 2, 4.0), ("absent", 5, 4.0), ("saturated", 3, 4.0), ("plain", 4, 0.0),
                                          ("saturated", 2, -1.0)])
def test_loss_bar_of_the_awkward_cases(kind, C, gamma):
    for vol in (315, 336):
        z, y = R.loss_inputs(3, vol, C, 77 + vol, kind)
        for inc_bg in (1, 0):
            l64, g64, g32, bar_abs, bar_norm = loss_refs(z, y, inc_bg, gamma)
            assert bool(torch.isfinite(g64).all()) and bool(torch.isfinite(g32).all()) and np.isfinite(float(l64))
            assert bar_norm <= 1e-4, (kind, vol, inc_bg, bar_norm)
            closed = R.dice_focal_grad_closed(z, y, inc_bg, gamma)
            assert float((closed - g64).abs().max()) <= 1e-12 * float(g64.abs().max())
    if kind == "sample_bg":
        I, P, T = R.dice_stats(z, y)
        assert float(T[1, 1]) == 0.0 and float(I[1, 1]) == 0.0 and float(P[1, 1]) > 0.0
    if kind == "absent":
        assert float(R.dice_stats(z, y)[2][:, C - 2].sum()) == 0.0
    if gamma == 0.0:                                              # gamma = 0: every focal weight is 1, the term is the plain BCE mean
        zz = z.double()
        t = (y.unsqueeze(-1) == torch.arange(C)).double()
        bce = torch.nn.functional.binary_cross_entropy_with_logits(zz[..., 0:], t[..., 0:])
        l_dice, _ = R.dice_focal_ref64(z, y, 1, -1.0)
        l_all, _ = R.dice_focal_ref64(z, y, 1, 0.0)
        assert abs(float(l_all - l_dice - bce)) < 1e-12


def adam_torch_f32(case, groups=R.ADAM_GROUPS):
    """torch.optim.AdamW(foreach=False) in f32 on the CPU, step by step: yields [(p, exp_avg, exp_avg_sq) | None]."""
    params = [torch.nn.Parameter(p.clone()) for p in case["p0"]]
    opt = torch.optim.AdamW([dict(params=[q for q, gi in zip(params, case["group_of"]) if gi == k], **grp)
                             for k, grp in enumerate(groups)], foreach=False)
    for row in case["grads"]:
        for q, gr in zip(params, row):
            q.grad = None if gr is None else gr.clone()
        opt.step()
        yield [None if i == case["no_grad"] else (q.detach().clone(), opt.state[q]["exp_avg"].clone(),
                                                  opt.state[q]["exp_avg_sq"].clone()) for i, q in enumerate(params)]


@pytest.mark.parametrize("which", ["ladder", "many"])
def test_adamw_bound_holds_f32_torch_on_every_element(which):
    case = R.adam_case() if which == "ladder" else R.adam_many_case()
    ref = R.adam_reference(case)
    used, tight = 0.0, 0.0
    for step, got in enumerate(adam_torch_f32(case)):
        for i, (st, tr) in enumerate(zip(ref[step], got)):
            if st is None:
                assert tr is None
                continue
            for name, val, bound, t32 in (("p", st.p, st.ep, tr[0]), ("exp_avg", st.m, st.em, tr[1]),
                                          ("exp_avg_sq", st.v, st.ev, tr[2])):
                R.assert_within_located(t32.reshape(-1), val.reshape(-1), bound.reshape(-1), "i",
                                        f"f32 torch AdamW, step {step + 1}, tensor {i}, {name}")
                live = val.abs() > 0
                if bool(live.any()):
                    used = max(used, float(((t32.double() - val).abs() / bound)[live].max()))
                    tight = max(tight, float((bound / val.abs())[live & (val.abs() > 1e-3 * val.abs().max())].max()))
    print(f"{which}: f32 torch uses at most {used:.2f} of its bound; the loosest bound is {tight:.2e} of the value")
    assert 0.02 < used <= 1.0                                    # not vacuous: rounding does reach a visible part of it
    assert tight < 1e-3                                          # (an element whose update cancels keeps an absolute bound)


def test_adamw_reference_matches_the_old_aggregate_bar_and_the_optimizer_row():
    """The float64 reference is the operation torch performs: its f32 result meets the suite's old parameter bar; and the
    row the reference takes is the row FusedAdamW._hyper builds."""
    case = R.adam_case()
    ref = R.adam_reference(case)
    for step, got in enumerate(adam_torch_f32(case)):
        for st, tr in zip(ref[step], got):
            if st is not None:
                assert old_adam_check(tr[0].double(), st.p) < OLD_ADAM_BAR
    from mivp_amd.optim import FusedAdamW
    params = [torch.nn.Parameter(torch.zeros(2)) for _ in R.ADAM_GROUPS]
    opt = FusedAdamW([dict(params=[q], **grp) for q, grp in zip(params, R.ADAM_GROUPS)])
    stepping = {id(q) for q in params}
    for step in (1, 2, 3):
        rows = opt._hyper(stepping)
        want = np.stack([R.adam_hyper_row(step=step, **grp) for grp in R.ADAM_GROUPS])
        assert rows.dtype == np.float32 and np.array_equal(rows, want), step


@pytest.mark.parametrize("tau", R.EMA_TAUS)
def test_ema_bound_holds_f32_torch_on_every_element(tau):
    teachers, students = R.ema_case()
    om = R.ema_om(tau)
    for i, (t, s) in enumerate(zip(teachers, students)):
        ref, bound = R.ema_ref64(t, s, tau)
        got = tau * t + om * s                                    # f32 tensors times Python scalars: f32 arithmetic
        assert got.dtype == F32
        R.assert_within_located(got.reshape(-1), ref.reshape(-1), bound.reshape(-1), "i", f"f32 torch EMA tau={tau} tensor {i}")
        assert float((bound / (ref.abs() + t.abs().double() + s.abs().double() + 1e-30)).max()) < 4 * R.U32
        if tau == 1.0:
            assert torch.equal(ref, t.double())
        if tau == 0.0:
            assert torch.equal(ref, s.double())


# =============================================================================================
# corruptions: the loss gradient
# =============================================================================================
def test_dice_constants_of_the_neighbouring_sample_for_one_group_of_four_voxels():
    """``stats + b * K`` with b off by one for the first four voxels of sample 1 (the group behind a sample boundary)."""
    B, vol, C = 2, 66 * 64 * 64, 2
    z, y = R.loss_inputs(B, vol, C, 5)
    _, g64, _, bar_abs, bar_norm = loss_refs(z, y, 1, 4.0)
    sample_of = torch.arange(B).unsqueeze(1).expand(B, vol).clone()
    sample_of[1, :4] = 0
    bad = R.dice_focal_grad_closed(z, y, 1, 4.0, sample_of=sample_of)
    changed = (bad - R.dice_focal_grad_closed(z, y, 1, 4.0)).abs().amax(-1) > 0
    assert int(changed.sum()) == 4 and bool(changed[1, :4].all())
    err = R.rel_l2(bad, g64)
    print(f"rel_l2 {err:.2e} (old bar {R.LOSS_L2_BAR:g}); per-element bar {bar_norm:.2e} of max |g|")
    assert err < R.LOSS_L2_BAR, "the corruption is louder than the old bar: shrink the corruption"
    assert_located_fails(bad, g64, bar_abs, "wrong sample's Dice constants")


def test_last_voxels_of_an_odd_volume_left_unwritten():
    B, vol, C = 3, 1027, 2
    z, y = R.loss_inputs(B, vol, C, 6)
    _, g64, _, bar_abs, _ = loss_refs(z, y, 1, 4.0)
    for stale in (float("nan"), 0.0):                             # what the buffer held before: the tests' NaN, or zeros
        bad = g64.clone()
        bad[:, vol - vol % 4:] = stale
        assert_located_fails(bad, g64, bar_abs, f"unwritten tail ({stale})")


def test_one_focal_class_column_dropped_without_background():
    """``c > c0`` instead of ``c >= c0`` in the focal branch: class 1 keeps its Dice gradient and loses its focal term."""
    B, vol, C = 3, 315, 5
    z, y = R.loss_inputs(B, vol, C, 7)
    _, g64, _, bar_abs, _ = loss_refs(z, y, 0, 4.0)
    bad = R.dice_focal_grad_closed(z, y, 0, 4.0, focal_classes=range(2, C))
    assert torch.equal(bad[..., 2:], R.dice_focal_grad_closed(z, y, 0, 4.0)[..., 2:])
    print(f"rel_l2 {R.rel_l2(bad, g64):.2e}")
    assert_located_fails(bad, g64, bar_abs, "dropped focal column")


def test_the_located_report_names_sample_voxel_and_class(capsys):
    z, y = R.loss_inputs(3, 63, 4, 8)
    _, g64, _, bar_abs, _ = loss_refs(z, y, 1, 4.0)
    bad = g64.clone()
    bad[2, 62, 3] += 2 * bar_abs
    bad[0, 0, 1] -= 2 * bar_abs
    with pytest.raises(AssertionError) as ei:
        R.assert_within_located(bad.float(), g64, bar_abs, "bvc", "demo")
    text = str(ei.value)
    assert "2 of" in text and "(2, 62, 3)" in text and "(0, 0, 1)" in text and "bound" in text
    assert "demo" in capsys.readouterr().out
    R.assert_within_located(g64.float(), g64, bar_abs, "bvc")


# =============================================================================================
# corruptions: AdamW and EMA
# =============================================================================================
def test_adamw_tail_of_a_tensor_of_1024k_plus_1_elements_not_stepped():
    case = R.adam_case()
    i = R.LADDER.index(3 * 1024 + 1)
    st = R.adamw_ref64(R.AdamState(case["p0"][i]), case["grads"][0][i], R.adam_hyper_row(step=1, **R.ADAM_GROUPS[case["group_of"][i]]))
    for name, val, bound, start in (("p", st.p, st.ep, case["p0"][i].double()), ("exp_avg", st.m, st.em, torch.zeros_like(st.m)),
                                    ("exp_avg_sq", st.v, st.ev, torch.zeros_like(st.v))):
        bad = val.clone()
        bad[-1] = start[-1]
        with pytest.raises(AssertionError, match=r"1 of .* leave the bound"):
            R.assert_within_located(bad, val, bound, "i", name)


def test_adamw_tensor_stepped_with_the_neighbouring_groups_row():
    """Two groups that differ in their betas alone: after one step the bias-corrected update, and with it the parameter, is
    the same to rounding, so the old parameter-only comparison passes; exp_avg and exp_avg_sq are wrong in every element."""
    g = R.gen(21)
    p0, gr = torch.randn(1025, generator=g), torch.randn(1025, generator=g)
    own = dict(R.ADAM_GROUPS[0])
    other = dict(own, betas=(R.f32_of(0.8), R.f32_of(0.99)))
    want = R.adamw_ref64(R.AdamState(p0), gr, R.adam_hyper_row(step=1, **own))
    bad = R.adamw_ref64(R.AdamState(p0), gr, R.adam_hyper_row(step=1, **other))
    err = old_adam_check(bad.p, want.p)
    print(f"old parameter check {err:.2e} (bar {OLD_ADAM_BAR:g})")
    assert err < OLD_ADAM_BAR
    for name, b, w, bound in (("exp_avg", bad.m, want.m, want.em), ("exp_avg_sq", bad.v, want.v, want.ev)):
        with pytest.raises(AssertionError, match="leave the bound"):
            R.assert_within_located(b, w, bound, "i", name)
    # and with groups that differ in everything, the parameter check of the new tests sees it at once
    bad = R.adamw_ref64(R.AdamState(p0), gr, R.adam_hyper_row(step=1, **R.ADAM_GROUPS[1]))
    with pytest.raises(AssertionError, match="leave the bound"):
        R.assert_within_located(bad.p, want.p, want.ep, "i", "p")


def test_ema_with_one_minus_tau_formed_in_float64():
    """om = 1 - tau on the host in double (0.004) instead of f32(1 - f32(0.996)) = 0.0040000081: 2e-6 of the student term."""
    tau = 0.996
    teachers, students = R.ema_case()
    t, s = teachers[R.LADDER.index(2048)], students[R.LADDER.index(2048)]
    ref, bound = R.ema_ref64(t, s, tau)
    bad = R.f32_of(tau) * t.double() + (1.0 - tau) * s.double()
    assert abs(R.ema_om(tau) - (1.0 - tau)) > 5e-9
    assert old_ema_check(bad, ref), "the corruption is louder than the old bar"
    with pytest.raises(AssertionError, match="leave the bound"):
        R.assert_within_located(bad, ref, bound, "i", "EMA")


# =============================================================================================
# corruptions: the counts
# =============================================================================================
def test_counts_with_the_last_maximum_tie_rule():
    B, vol, C = 3, 315, 5
    z, y = R.seg_case(B, vol, C, 31)
    ref = R.seg_counts_ref(z, y, C)
    ties = (z == z.amax(1, keepdim=True)).sum(1) > 1
    assert float(ties.double().mean()) > 0.3 and bool((z == z[:, :1]).all(1).any())
    last = R.seg_counts_ref(torch.flip(z, dims=(1,)), (C - 1) - y, C).flip(0)       # classes mirrored: last maximum wins
    assert torch.equal(last[:, 2], ref[:, 2]) and int(last[:, 1].sum()) == int(ref[:, 1].sum()) == B * vol
    with pytest.raises(AssertionError, match="differ from the float64 reference"):
        R.assert_equal_located(last, ref, "ck", "last-maximum rule")
    # labels that match no class add to the prediction column alone
    outside = ((y < 0) | (y >= C) | (y != y.round()))
    assert bool(outside.any()) and int(ref[:, 2].sum()) == int((~outside).sum())


def test_counts_with_the_channels_first_stride_of_the_wrong_sample():
    """logits[(b + c) vol + s] instead of logits[(b C + c) vol + s]: right for sample 0, wrong from sample 1 on."""
    B, vol, C = 3, 315, 5
    z, y = R.seg_case(B, vol, C, 32)
    ref = R.seg_counts_ref(z, y, C)
    flat = z.reshape(B * C, vol)
    wrong = torch.stack([torch.stack([flat[b + c] for c in range(C)]) for b in range(B)])
    assert torch.equal(wrong[0], z[0]) and not torch.equal(wrong[1], z[1])
    with pytest.raises(AssertionError, match="differ from the float64 reference"):
        R.assert_equal_located(R.seg_counts_ref(wrong, y, C), ref, "ck", "wrong sample stride")
    assert torch.equal(R.seg_counts_ref(z[:1], y[:1], C), R.seg_counts_ref(wrong[:1], y[:1], C))   # B = 1 cannot see it
