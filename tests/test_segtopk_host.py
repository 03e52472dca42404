"""CPU: the float64 reference of the top-k cross-entropy (tests/segtopk_ref.py), the condition under which
tests/test_hip_segtopk.py may compare a kernel's selection with it, and the package's host side.

1. the reference against ``torch.topk`` + autograd in float64 on tie-free cases (value and gradient to 1e-12), its closed
   form, the tie rule, and ``top_k = 1`` against the existing voxel term;
2. every case of the GPU file is decidable (no u within the band of tau except designed ties), and f32 torch meets the bars;
3. the bars see planted errors: k off by one, ``>=`` on ties, tau per sample, invalid voxels in N, the weight sum as the
   normaliser;
4. the package on the CPU: ``seg_loss`` with ``top_k`` (the torch composition) for every C, ``SegLossSpec`` validation,
   ``top_k=None`` unchanged, ``train.step_loss``, ``top_k_stats``, the header and the entries' argument checks."""
import math
import os
import sys
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segloss_ref as R  # noqa: E402
import segtopk_ref as T  # noqa: E402

from conftest import ROOT  # noqa: E402

F32, F64 = torch.float32, torch.float64


def tight(got, want, what, tol=1e-12):
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"{what}: off by {err:.3e} (scale {scale:.3e})"


# =============================================================================================
# 1. the reference
# =============================================================================================
@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("top_k", [0.05, 0.3, 1.0])
def test_reference_is_torch_topk_with_autograd_on_tie_free_cases(top_k, ignore, gamma):
    B, vol, C = 3, 315, 4
    z, y = T.topk_inputs(B, vol, C, 3, "plain" if ignore is None else "ignored", ignore)
    o = T.opts(top_k, class_weights=R.WEIGHTS8[:C], ignore_index=ignore, focal_gamma=gamma, lambda_region=0.0)
    l64, g64, sel = T.topk_loss(z, y, o)
    assert sel.n_eq == 1 and sel.n_gt == sel.k - 1
    zz = z.double().clone().requires_grad_(True)
    ce = F.cross_entropy(zz.reshape(-1, C), y.reshape(-1).long(), weight=torch.tensor(o["class_weights"], dtype=F64),
                         ignore_index=-100 if ignore is None else ignore, reduction="none")
    if gamma:
        p = zz.reshape(-1, C).softmax(-1)
        hot = F.one_hot(R.class_index(y, C).reshape(-1), C).double()
        ce = ce * (p * (1.0 - hot)).sum(-1) ** gamma
    keep = R.valid_mask(y, C, ignore).reshape(-1)
    want = torch.topk(ce[keep], T.k_of(top_k, int(keep.sum())))[0].mean()
    want.backward()
    assert abs(float(l64) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    tight(g64, zz.grad, f"top_k {top_k} ignore {ignore} gamma {gamma}")
    tight(T.topk_grad_closed(z, y, o), g64, "closed form")
    if ignore is not None:
        assert not bool(g64[~R.valid_mask(y, C, ignore)].abs().max() > 0)


def test_closed_form_is_the_autograd_gradient_on_every_gpu_case():
    for name, z, y, o in T.all_gpu_cases():
        _, g64, sel = T.topk_loss(z, y, o)
        closed = T.topk_grad_closed(z, y, o)
        assert float((closed - g64).abs().max()) <= 1e-12 * max(float(g64.abs().max()), 1e-300), name
        assert abs(float(sel.s.sum()) - (sel.k if sel.N else 0)) <= 1e-9 * sel.k, name


def test_tie_rule():
    # all equal: rho = k / N, sum s = k
    z, y = T.topk_inputs(2, 64, 3, 13, "zeros")
    for top_k in (0.01, 0.3, 1.0):
        _, u, valid = T.u_of(z, y, T.opts(top_k))
        sel = T.Select(u, valid, top_k)
        assert sel.N == 128 and sel.k == max(1, math.floor(top_k * 128)) and sel.n_gt == 0 and sel.n_eq == 128
        assert sel.rho == sel.k / 128 and abs(float(sel.s.sum()) - sel.k) < 1e-12
        l64, _, _ = T.topk_loss(z, y, T.opts(top_k, lambda_region=0.0))
        assert abs(float(l64) - math.log(3.0)) < 1e-12
    # a tie group straddling k: u = 5, 3, 3, 3, 3, 1 and k = 3 -> s = 1, 1/2 x 4, 0
    u = torch.tensor([[3.0, 1.0, 3.0, 5.0, 3.0, 3.0]], dtype=F64)
    sel = T.Select(u, torch.ones_like(u, dtype=torch.bool), 0.5)
    assert (sel.N, sel.k, float(sel.tau), sel.n_gt, sel.n_eq, sel.rho) == (6, 3, 3.0, 1, 4, 0.5)
    assert sel.s.tolist() == [[0.5, 0.0, 0.5, 1.0, 0.5, 0.5]] and float(sel.s.sum()) == 3.0
    assert float(T.voxel_value(u, sel)) == (5.0 + 2 * 3.0) / 3 == float(torch.topk(u[0], 3)[0].mean())
    # exact sums on the designed ties of the GPU cases
    for name, z, y, o in T.select_cases():
        if "five" in name:
            sel = T.assert_case_is_decidable(z, y, o, name)
            assert sel.n_gt + sel.rho * sel.n_eq == pytest.approx(sel.k, abs=1e-9) and 0 < sel.rho <= 1


def test_top_k_one_without_weights_is_the_existing_voxel_term():
    for ignore, gamma in ((None, 0.0), (255, 2.0)):
        z, y = T.topk_inputs(3, 315, 3, 8, "plain" if ignore is None else "ignored", ignore)
        o = T.opts(1.0, ignore_index=ignore, focal_gamma=gamma, alpha=0.3, beta=0.7)
        l64, g64, _ = T.topk_loss(z, y, o)
        want_l, want_g = R.seg_loss_ref64(z, y, T.base_opts(o))
        assert abs(float(l64 - want_l)) <= 1e-12
        tight(g64, want_g, f"top_k 1 ignore {ignore}")


# =============================================================================================
# 2. the GPU file's cases: decidable, and f32 torch inside the bars
# =============================================================================================
def test_every_gpu_case_is_decidable():
    cases = T.all_gpu_cases()
    assert len(cases) > 60
    for name, z, y, o in cases:
        T.assert_case_is_decidable(z, y, o, f"{name} top_k {o['top_k']:.6g}")


def test_the_select_cases_hold_what_the_issue_lists():
    cases = T.select_cases()
    seen = {(z.shape[0], z.shape[1]) for _, z, _, _ in cases}
    assert {(b, v) for b in (1, 2, 3) for v in (1, 63, 64, 2053)} <= seen and (2, 8000) in seen
    assert {z.shape[2] for _, z, _, _ in cases} == set(range(2, 9))
    kinds = {"k1": 0, "kN": 0, "first": 0, "inside": 0, "last": 0, "zero_u": 0, "empty": 0, "levels": set()}
    for name, z, y, o in cases:
        _, u64, valid = T.u_of(z, y, o)
        sel = T.Select(u64, valid, o["top_k"])
        if sel.N == 0:
            kinds["empty"] += 1
            continue
        kinds["k1"] += sel.k == 1
        kinds["kN"] += sel.k == sel.N
        if sel.n_eq >= 3:
            place = sel.k - sel.n_gt
            kinds["first"] += place == 1
            kinds["last"] += place == sel.n_eq
            kinds["inside"] += 1 < place < sel.n_eq
        kinds["zero_u"] += bool((u64[valid] == 0).any())
        if "wide" in name:
            keys = u64[valid].to(F32).view(torch.int32)
            kinds["levels"] |= {int(v) for v in (keys >> 20).unique()}
    assert all(kinds[k] > 0 for k in ("k1", "kN", "first", "inside", "last", "zero_u", "empty")), kinds
    assert len(kinds["levels"]) > 60                              # level-1 bins in use: the keys span many exponents
    _, z, y, _ = next(c for c in cases if c[0].startswith("bad labels"))
    assert bool((y == 0.5).any()) and bool((y == 4.0).any()) and bool((y < 0).any())


def f32_inside(z, y, o, what):
    ref = T.TopkRef(z, y, o)
    assert bool(torch.isfinite(ref.g32).all()) and bool(torch.isfinite(ref.l32)), what
    assert abs(float(ref.l32) - float(ref.l64)) <= T.LOSS_VALUE_BAR * max(1.0, abs(float(ref.l64))), what
    if ref.zero:
        assert not bool(ref.g32.abs().max() > 0), what
        return
    assert T.rel_l2(ref.g32, ref.g64) < T.LOSS_L2_BAR, what
    T.assert_within_located(ref.g32, ref.g64, ref.bar_abs, "bvc", what)


def test_f32_torch_meets_the_bars_on_the_gpu_cases():
    for name, z, y, o in T.product_cases() + [(f"forms {v}",) + T.forms_case(v) for v in T.FORMS_VOLS]:
        f32_inside(z, y, o, name)
    for name, z, y, o in T.select_cases()[::4]:
        f32_inside(z, y, o, name)


# =============================================================================================
# 3. planted errors
# =============================================================================================
def planted_case(ignore=255, kind="ignored", top_k=0.3, weights=(0.5, 2.0, 1.0), seed=9):
    z, y = T.topk_inputs(3, 315, 3, seed, kind, ignore)
    o = T.opts(top_k, alpha=0.3, beta=0.7, class_weights=weights, ignore_index=ignore)
    ref = T.TopkRef(z, y, o)
    T.assert_within_located(T.topk_grad_closed(z, y, o), ref.g64, ref.bar_abs, "bvc", "the closed form against its own bar")
    _, u, valid = T.u_of(z, y, o)
    return z, y, o, ref, u, valid


def assert_located_fails(bad, ref, what):
    print(f"{what}: rel_l2 {T.rel_l2(bad, ref.g64):.2e}; per-element bar {ref.bar_norm:.2e} of max |g|")
    with pytest.raises(AssertionError, match="leave the bound of the float64 reference"):
        T.assert_within_located(bad, ref.g64, ref.bar_abs, "bvc", what)


@pytest.mark.parametrize("shift", [-1, 1])
def test_k_off_by_one(shift):
    z, y, o, ref, u, valid = planted_case()
    sel = T.Select(u, valid, o["top_k"], k_shift=shift)
    assert sel.k == ref.sel.k + shift
    assert_located_fails(T.topk_grad_closed(z, y, o, sel=sel), ref, f"k {shift:+d}")


def test_every_tied_voxel_selected_instead_of_the_shared_weight():
    z, y, o, ref, u, valid = planted_case(ignore=None, kind="five", weights=None, top_k=0.4)
    assert ref.sel.n_eq >= 3 and 0 < ref.sel.rho < 1
    sel = T.Select(u, valid, o["top_k"], ties_all=True)
    assert float(sel.s.sum()) > sel.k
    assert_located_fails(T.topk_grad_closed(z, y, o, sel=sel), ref, ">= on ties")
    # and the first-come form: the first k - n_gt tied voxels in memory order take weight 1, the others 0
    s = ref.sel.s.clone()
    tied = torch.nonzero(s.reshape(-1) == ref.sel.rho).reshape(-1)
    s.view(-1)[tied] = 0.0
    s.view(-1)[tied[:ref.sel.k - ref.sel.n_gt]] = 1.0
    first = T.Select(u, valid, o["top_k"])
    first.s = s
    assert float(s.sum()) == ref.sel.k
    assert_located_fails(T.topk_grad_closed(z, y, o, sel=first), ref, "memory-order ties")


def test_tau_taken_per_sample():
    z, y, o, ref, u, valid = planted_case(kind="sample_ignored")
    sel = T.Select(u, valid, o["top_k"], per_sample=True)
    assert sel.N == ref.sel.N and not torch.equal(sel.s, ref.sel.s)
    assert_located_fails(T.topk_grad_closed(z, y, o, sel=sel), ref, "per-sample tau")
    z, y, o, ref, u, valid = planted_case(ignore=None, kind="wide")          # equal counts, unequal difficulty
    sel = T.Select(u, valid, o["top_k"], per_sample=True)
    assert_located_fails(T.topk_grad_closed(z, y, o, sel=sel), ref, "per-sample tau, equal counts")


def test_invalid_voxels_counted_in_N():
    z, y, o, ref, u, valid = planted_case()
    sel = T.Select(u, valid, o["top_k"], count_invalid=True)
    assert sel.N == 3 * 315 > ref.sel.N and sel.k > ref.sel.k
    assert_located_fails(T.topk_grad_closed(z, y, o, sel=sel), ref, "invalid voxels in N")


def test_normalising_by_the_weight_sum_instead_of_k():
    z, y, o, ref, u, valid = planted_case()
    w = torch.tensor(o["class_weights"], dtype=F64)[R.class_index(y, 3)]
    wsum = float((ref.sel.s * w * valid).sum())
    assert abs(wsum - ref.sel.k) > 1.0
    assert_located_fails(T.topk_grad_closed(z, y, o, norm=wsum), ref, "weight sum as the normaliser")
    bad_l, _, _ = T.topk_loss(z, y, o, norm=wsum)
    assert abs(float(bad_l - ref.l64)) > T.LOSS_VALUE_BAR * max(1.0, abs(float(ref.l64)))


# =============================================================================================
# 4. the package on the CPU
# =============================================================================================
def package_grad(z, y, o, dims, dtype=F64, module=False):
    from mivp_amd import losses
    B, vol, C = z.shape
    base = z.to(dtype).view(B, *dims, C).clone().requires_grad_(True)
    mod = losses.SegLoss(losses.SegLossSpec(**o))
    got = mod(base.permute(0, 4, 1, 2, 3), y.view(B, 1, *dims)) if module else \
        losses.seg_loss(base.permute(0, 4, 1, 2, 3), y.view(B, 1, *dims), mod.spec)
    got.backward()
    return got.detach(), base.grad.view(B, vol, C), mod


@pytest.mark.parametrize("C", range(2, 9))
def test_seg_loss_with_top_k_on_the_cpu_is_the_reference(C):
    dims = (5, 7, 9)
    for i, (gamma, ignore, wts, batch) in enumerate(((0.0, 255, True, False), (2.0, None, True, True), (2.0, -1, False, False),
                                                      (0.0, None, False, True))):
        z, y = T.topk_inputs(3, 315, C, 100 + C, "plain" if ignore is None else "ignored", ignore)
        o = T.opts(0.25, alpha=0.3, beta=0.7, batch=batch, focal_gamma=gamma, class_weights=R.WEIGHTS8[:C] if wts else None,
                   ignore_index=ignore, lambda_voxel=0.5)
        l64, g64, sel = T.topk_loss(z, y, o)
        got_l, got_g, mod = package_grad(z, y, o, dims, module=bool(i % 2))
        assert got_l.dtype == F64 and abs(float(got_l - l64)) <= 1e-10 * max(1.0, abs(float(l64))), T.opts_name(o)
        tight(got_g, g64, T.opts_name(o), 1e-10 * float(g64.abs().max()))
        if i % 2:
            st = mod.top_k_stats()
            assert (st["N"], st["k"], st["n_gt"], st["n_eq"]) == (sel.N, sel.k, sel.n_gt, sel.n_eq)
            assert abs(st["tau"] - float(sel.tau)) <= 1e-12


def test_seg_loss_with_top_k_on_the_cpu_ties_and_special_operands():
    for name, z, y, o in T.select_cases():
        B, vol, C = z.shape
        if vol > 400:
            continue
        l64, g64, sel = T.topk_loss(z, y, o)
        got_l, got_g, _ = package_grad(z, y, o, (1, 1, vol))
        assert abs(float(got_l - l64)) <= 1e-10 * max(1.0, abs(float(l64))), name
        tight(got_g, g64, name, 1e-10 * max(float(g64.abs().max()), 1e-30))
        invalid = ~R.valid_mask(y, C, o["ignore_index"])
        if bool(invalid.any()):
            assert not bool(got_g[invalid].abs().max() > 0), name


@pytest.mark.parametrize("bad", [0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), True, "0.1", (0.1,)])
def test_spec_refuses_an_invalid_top_k_by_name(bad):
    from mivp_amd.losses import SegLossSpec
    with pytest.raises(ValueError, match="top_k"):
        SegLossSpec(top_k=bad)


def test_spec_with_top_k():
    from mivp_amd import losses
    with pytest.raises(ValueError, match="top_k.*lambda_voxel"):
        losses.SegLossSpec(top_k=0.1, lambda_voxel=0.0)
    a, b = losses.SegLossSpec(top_k=0.1), losses.SegLossSpec(top_k=0.1)
    assert a == b and hash(a) == hash(b) and a != losses.SegLossSpec() and a != losses.SegLossSpec(top_k=0.2)
    assert "top_k=0.1" in repr(a) and "top_k=None" in repr(losses.SegLossSpec()) and losses.SegLossSpec(top_k=1).top_k == 1.0
    assert losses.SegLossSpec() == losses.SegLossSpec(top_k=None) and hash(losses.SegLossSpec()) == hash(losses.SegLossSpec(top_k=None))
    assert repr(a).index("lambda_voxel") < repr(a).index("top_k")              # the added field comes last
    with pytest.raises(AttributeError):
        a.top_k = 0.5
    with pytest.raises(RuntimeError, match="top_k_stats"):
        losses.SegLoss(top_k=0.1).top_k_stats()


def test_top_k_none_gives_the_results_of_a_spec_without_the_argument():
    from mivp_amd import losses
    z, y, o = R.wrapper_case((5, 7, 9))
    out = []
    for spec in (losses.SegLossSpec(**o), losses.SegLossSpec(top_k=None, **o)):
        base = z.view(3, 5, 7, 9, 4).clone().requires_grad_(True)
        got = losses.seg_loss(base.permute(0, 4, 1, 2, 3), y.view(3, 1, 5, 7, 9), spec)
        got.backward()
        out.append((got.detach(), base.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_step_loss_with_a_top_k_seg_loss():
    from mivp_amd import losses, train
    g = T.gen(5)
    B, C, dims = 2, 2, (4, 4, 4)
    logits = torch.randn((B, C) + dims, generator=g)
    y = torch.randint(0, C, (B, 1) + dims, generator=g).float()
    y[0, 0, 0] = 255.0
    mod = losses.SegLoss(top_k=0.1, ignore_index=255)
    conf = Namespace(training_mode="downstream", include_background=True, seg_loss=mod)
    got = train.step_loss({"downstream": logits}, conf, y)
    z = logits.permute(0, 2, 3, 4, 1).reshape(B, -1, C)
    want, _, sel = T.topk_loss(z, y.reshape(B, -1), T.opts(0.1, ignore_index=255))
    assert abs(float(got) - float(want)) <= T.LOSS_VALUE_BAR
    st = mod.top_k_stats()
    assert (st["N"], st["k"]) == (sel.N, sel.k) == (128 - 16, 11)
    plain = train.step_loss({"downstream": logits}, Namespace(training_mode="downstream", include_background=True,
                                                               seg_loss=losses.SegLoss(ignore_index=255)), y)
    assert float(got) > float(plain)                              # the mean over the hardest voxels


def test_header_declares_the_top_k_entries_and_the_abi_stays_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    P = _lib.parse_header()
    assert len(P["mivp_seg_topk_ws"][1]) == 2 and P["mivp_seg_topk_ws"][0] is _lib.C.c_size_t
    for name in ("mivp_seg_topk", "mivp_seg_topk_grad"):
        assert len(P[name][1]) == 20 and P[name][1][15] is _lib.C.c_double and P[name][1].count(_lib.C.c_double) == 1
        assert not name.startswith("mivp_seg_loss")
    assert len(P["mivp_seg_loss"][1]) == 19 and len(P["mivp_seg_loss_grad"][1]) == 19
    assert "#define MIVP_SEG_TOPK_RECORD_WORDS 16" in text and "#define MIVP_SEG_TOPK_KEYS_OFFSET 5136" in text


def test_entries_refuse_the_options_the_host_refuses():
    """MIVP_REQUIRE returns before anything is launched or dereferenced: the pointers are never read."""
    from mivp_amd import _lib as L
    for B, vol in ((3, 63), (2, 2053), (1, 1), (2, 8000)):
        base = (int(L.lib().mivp_seg_loss_ws(B, vol)) + 3) // 4 * 4
        assert int(L.lib().mivp_seg_topk_ws(B, vol)) == base + 5136 + (B * vol + 3) // 4 * 4
    p = 4096                                                       # a non-NULL address that no accepted call would be given
    good = dict(B=2, vol=8, C=3, alpha=0.5, beta=0.5, gamma=0.0, lr=1.0, lv=1.0, top_k=0.1)
    for change in (dict(C=9), dict(C=1), dict(B=0), dict(vol=0), dict(alpha=-0.5), dict(beta=float("nan")), dict(gamma=0.5),
                   dict(lr=-1.0), dict(lv=float("inf")), dict(top_k=0.0), dict(top_k=1.5), dict(top_k=float("nan")),
                   dict(top_k=-0.1), dict(lv=0.0), dict(B=2, vol=2 ** 30), dict(B=1, vol=2 ** 31)):
        a = dict(good, **change)
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_seg_topk", p, p, a["B"], a["vol"], a["C"], 1, 0, a["alpha"], a["beta"], a["gamma"], None, 0, 0, a["lr"],
                   a["lv"], a["top_k"], p, p, None, None)
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_seg_topk_grad", p, p, a["B"], a["vol"], a["C"], 1, 0, a["alpha"], a["beta"], a["gamma"], None, 0, 0,
                   a["lr"], a["lv"], a["top_k"], p, None, p, None)
    with pytest.raises(RuntimeError, match="contract violated"):
        L.call("mivp_seg_topk", None, p, 2, 8, 3, 1, 0, 0.5, 0.5, 0.0, None, 0, 0, 1.0, 1.0, 0.1, p, p, None, None)
