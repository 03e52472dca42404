"""CPU: the float64 restatement of the Lovasz-Softmax term (tests/lovasz_ref.py), and the package's host side.

1. the restatement against a brute force on N <= 7 errors: the Lovasz extension has one value for every tie-consistent order
   (so their mean is that value) and the restatement's; its gradient is finite differences where no errors are tied; the tie
   rule adds up to its group's total; against the authors' ``lovasz_grad`` recurrence;
2. the package on the CPU: the torch composition against the restatement, the module around a base loss, the argument checks
   of the Python surface and of every new entry, the header and the ABI."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lovasz_ref as R  # noqa: E402

from conftest import ROOT  # noqa: E402

F32, F64 = torch.float32, torch.float64
BOOLS = (False, True)
# (errors, foreground flags): no ties; ties inside and across the two kinds; all equal; no foreground; no background; one voxel
SMALL = (
    ([0.9, 0.1, 0.55, 0.3, 0.7, 0.2, 0.45], [1, 0, 0, 1, 0, 1, 0]),
    ([0.5, 0.5, 0.5, 0.25, 0.25, 0.75, 0.75], [1, 0, 0, 1, 1, 0, 1]),
    ([0.5, 0.5, 0.5, 0.5, 0.5, 0.5], [1, 0, 1, 0, 0, 1]),
    ([1.0, 1.0, 0.0, 0.0, 0.5], [0, 1, 1, 0, 0]),
    ([0.3, 0.3, 0.6, 0.1], [0, 0, 0, 0]),
    ([0.3, 0.3, 0.6, 0.1], [1, 1, 1, 1]),
    ([0.4], [1]),
    ([0.4], [0]),
)


def consistent_orders(e):
    """Every permutation that lists the errors in descending order (ties in any order)."""
    return [p for p in itertools.permutations(range(len(e))) if all(e[p[i]] >= e[p[i + 1]] for i in range(len(p) - 1))]


# =============================================================================================
# 1. the restatement
# =============================================================================================
@pytest.mark.parametrize("case", range(len(SMALL)))
def test_value_is_one_for_every_order_and_the_tie_rule_adds_up(case):
    e, g = np.array(SMALL[case][0]), np.array(SMALL[case][1], bool)
    orders = consistent_orders(e)
    assert len(orders) >= 1
    values = [R.extension(e[list(p)], g[list(p)])[0] for p in orders]
    s = R.tie_weights(R.order_keys(e, g), g)
    mine = float(np.dot(s, e))
    assert abs(float(np.mean(values)) - mine) < 1e-14
    assert max(abs(v - mine) for v in values) < 1e-14
    # a group's weights add up to its difference of J, for every order the group's total is the same
    G = int(g.sum())
    for val in np.unique(e):
        grp = e == val
        F0, K0 = int((g & (e > val)).sum()), int((~g & (e > val)).sum())
        F1, K1 = F0 + int((g & grp).sum()), K0 + int((~g & grp).sum())
        assert abs(s[grp].sum() - (R.jaccard(F1, K1, G) - R.jaccard(F0, K0, G))) < 1e-14
        # foreground first: 1 / (G + K0) each; the background shares the rest equally
        assert np.allclose(s[grp & g], 1.0 / (G + K0), rtol=0, atol=1e-15) if (grp & g).any() else True
        assert len(set(np.round(s[grp & ~g], 15))) <= 1
    # the mean over the orders of the per-position differences gives each group the same total
    mean_w = np.zeros(len(e))
    for p in orders:
        mean_w[list(p)] += R.extension(e[list(p)], g[list(p)])[1]
    mean_w /= len(orders)
    for val in np.unique(e):
        assert abs(mean_w[e == val].sum() - s[e == val].sum()) < 1e-13


def test_gradient_is_finite_differences_without_ties():
    e, g = np.array(SMALL[0][0]), np.array(SMALL[0][1], bool)
    assert len(consistent_orders(e)) == 1
    s = R.tie_weights(R.order_keys(e, g), g)

    def value(x):
        o = np.argsort(-x, kind="stable")
        return R.extension(x[o], g[o])[0]

    h = 1e-6
    for i in range(len(e)):
        d = np.zeros(len(e))
        d[i] = h
        assert abs((value(e + d) - value(e - d)) / (2 * h) - s[i]) < 1e-8


def lovasz_grad_authors(gt_sorted):
    """The recurrence of the authors' ``lovasz_grad`` on labels sorted by descending error."""
    gts = gt_sorted.sum()
    intersection = gts - np.cumsum(gt_sorted)
    union = gts + np.cumsum(1.0 - gt_sorted)
    jaccard = 1.0 - intersection / union
    if len(gt_sorted) > 1:
        jaccard[1:] = jaccard[1:] - jaccard[:-1]
    return jaccard


@pytest.mark.parametrize("seed", range(4))
def test_against_the_authors_recurrence(seed):
    rng = np.random.default_rng(seed)
    n = 300
    e = rng.random(n) if seed % 2 == 0 else rng.integers(0, 5, n) / 4.0       # odd seeds: five distinct errors
    g = rng.random(n) < 0.3
    o = np.argsort(-e, kind="stable")
    grad = lovasz_grad_authors(g[o].astype(np.float64))
    s = R.tie_weights(R.order_keys(e, g), g)
    assert abs(float(np.dot(e[o], grad)) - float(np.dot(s, e))) < 1e-12
    if seed % 2 == 0:
        assert np.abs(grad - s[o]).max() < 1e-12


def case(shape, content, lab, seed=3):
    B, C, dims = shape
    return R.logits(content, B, math.prod(dims), C, seed), R.label_case(lab, B, C, dims, seed)


def test_reference_gradient_is_autograd_of_its_value_without_ties():
    """d (sum_i s_i e_i) / dz with s held fixed is what the closed form dz_k = p_k (q_k - sum p q) states."""
    z, y = case(R.SHAPES[0], "randn", "ignored")
    for per_image, classes in itertools.product(BOOLS, ("present", "all")):
        ref = R.LvRef(z, y, classes=classes, per_image=per_image, include_background=True, ignore_index=R.IGNORE, weight=0.37)
        h = 1e-6
        g = ref.g64
        for (b, v, c) in ((0, 5, 0), (1, 100, 2), (0, 33, 1)):
            zp, zm = z.to(F64).clone(), z.to(F64).clone()
            zp[b, v, c] += h
            zm[b, v, c] -= h
            lp = R.lovasz_ref(zp, y, classes, per_image, True, R.IGNORE, 0.37)[0]
            lm = R.lovasz_ref(zm, y, classes, per_image, True, R.IGNORE, 0.37)[0]
            assert abs((lp - lm) / (2 * h) - float(g[b, v, c])) < 1e-7, (per_image, classes, b, v, c)


# =============================================================================================
# 2. the package on the CPU
# =============================================================================================
@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("lab", ["blobs", "absent", "ignored", "none"])
def test_cpu_composition_is_the_reference(content, lab):
    from mivp_amd import losses
    shape = R.SHAPES[0]
    B, C, dims = shape
    z, y = case(shape, content, lab)
    for per_image, classes, bg in itertools.product(BOOLS, ("present", "all"), BOOLS):
        opts = dict(classes=classes, per_image=per_image, include_background=bg, ignore_index=R.IGNORE)
        ref = R.LvRef(z, y, weight=0.37, **opts)
        zc = z.to(F64).view(B, *dims, C).permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
        got = losses.lovasz_softmax_loss(zc, y.view(B, 1, *dims), weight=torch.tensor([float(np.float32(0.37))], dtype=F64), **opts)
        assert abs(float(got.detach()) - ref.l64) < 1e-12, opts
        if got.requires_grad:
            got.backward()
            grad = zc.grad.permute(0, 2, 3, 4, 1).reshape(B, -1, C)
        else:
            grad = torch.zeros_like(ref.g64)
        assert float((grad - ref.g64).abs().max()) < 1e-13, opts
        if lab == "none":
            assert float(got.detach()) == 0.0 and ref.zero


def test_module_is_the_base_plus_the_term():
    from mivp_amd import losses
    shape = R.SHAPES[0]
    B, C, dims = shape
    z, y = case(shape, "randn", "ignored")
    zc, yc = z.view(B, *dims, C).permute(0, 4, 1, 2, 3), y.view(B, 1, *dims)
    base = losses.SegLoss(ignore_index=R.IGNORE)
    mod = losses.LovaszSoftmaxLoss(base=base, lambda_lovasz=0.5, per_image=True, ignore_index=R.IGNORE)
    assert "weight" not in mod.state_dict()
    term = losses.lovasz_softmax_loss(zc, yc, per_image=True, ignore_index=R.IGNORE)
    assert abs(float(mod(zc, yc)) - float(base(zc, yc) + 0.5 * term)) < 1e-6
    mod.set_weight(2.0)
    assert abs(float(mod(zc, yc)) - float(base(zc, yc) + term)) < 1e-6
    alone = losses.LovaszSoftmaxLoss(per_image=True, ignore_index=R.IGNORE)
    assert abs(float(alone(zc, yc)) - float(term)) < 1e-7
    assert "lambda_lovasz=0.5" in repr(mod)
    with pytest.raises(ValueError, match="weight"):
        mod.set_weight(float("nan"))


def test_public_functions_check_their_arguments():
    from mivp_amd import losses
    z, y = torch.zeros(2, 3, 4, 4, 4), torch.zeros(2, 1, 4, 4, 4)
    for fn in (losses.lovasz_softmax_loss, lambda a, b, **kw: losses.LovaszSoftmaxLoss(**kw)(a, b)):
        with pytest.raises(ValueError, match="logits"):
            fn(z[0], y)
        with pytest.raises(ValueError, match="classes"):
            fn(torch.zeros(2, 1, 4, 4, 4), y)
        with pytest.raises(ValueError, match="classes"):
            fn(torch.zeros(2, 9, 4, 4, 4), y)
        with pytest.raises(ValueError, match="target"):
            fn(z, y[:1])
        with pytest.raises(ValueError, match="classes"):
            fn(z, y, classes="some")
        with pytest.raises(ValueError, match="per_image"):
            fn(z, y, per_image=1)
        with pytest.raises(ValueError, match="include_background"):
            fn(z, y, include_background=0)
        with pytest.raises(ValueError, match="ignore_index"):
            fn(z, y, ignore_index=2.5)
    with pytest.raises(ValueError, match="weight"):
        losses.lovasz_softmax_loss(z, y, weight=torch.ones(2))
    with pytest.raises(ValueError, match="weight"):
        losses.lovasz_softmax_loss(z, y, weight=0.5)
    for bad in (-1.0, float("nan"), float("inf"), 1e39, True):
        with pytest.raises(ValueError, match="lambda_lovasz"):
            losses.LovaszSoftmaxLoss(lambda_lovasz=bad)
    with pytest.raises(TypeError, match="base"):
        losses.LovaszSoftmaxLoss(base=lambda a, b: a.sum())


def test_header_declares_the_entries_and_the_abi_stays_18():
    from mivp_amd import _lib, losses
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    P = _lib.parse_header()
    want = {"mivp_sort_tile": (0, _lib.C.c_int), "mivp_sort_u32_ws": (2, _lib.C.c_size_t), "mivp_sort_u32": (5, _lib.C.c_int),
            "mivp_lovasz_ws": (5, _lib.C.c_size_t), "mivp_lovasz_keys": (12, _lib.C.c_int), "mivp_lovasz_loss": (17, _lib.C.c_int),
            "mivp_lovasz_loss_grad": (17, _lib.C.c_int)}
    for name, (n, ret) in want.items():
        assert len(P[name][1]) == n and P[name][0] is ret, name
    assert sorted(n for n in P if n.startswith(("mivp_lovasz", "mivp_sort"))) == sorted(want)
    assert not any("lovasz" in s for s in losses.SegLossSpec.__slots__)


def test_entries_refuse_what_the_host_refuses():
    """MIVP_REQUIRE returns before anything is launched or dereferenced: the pointers are never read."""
    from mivp_amd import _lib as L
    lib = L.lib()
    tile = int(lib.mivp_sort_tile())
    assert tile >= 256 and tile % 256 == 0
    assert int(lib.mivp_sort_u32_ws(3, 10)) > 3 * 10 * 4 and int(lib.mivp_sort_u32_ws(3, 10)) % 256 == 0
    for S, n in ((0, 8), (1, 0), (65536, 1), (2, 2 ** 30), (1, 2 ** 31)):
        assert int(lib.mivp_sort_u32_ws(S, n)) == 0, (S, n)
    small = int(lib.mivp_lovasz_ws(2, 3, 1, 0, 210))
    assert small >= 3 * 3 * 420 * 4 and small % 256 == 0
    assert int(lib.mivp_lovasz_ws(2, 3, 0, 1, 210)) > 0
    for B, C, vol in ((0, 3, 8), (2, 1, 8), (2, 9, 8), (2, 3, 0), (65536, 2, 1), (4, 8, 2 ** 27), (1, 2, 2 ** 31)):
        for per_image in (0, 1):
            assert int(lib.mivp_lovasz_ws(B, C, 1, per_image, vol)) == 0, (B, C, vol, per_image)
    p = 4096                                                       # a non-NULL address that no accepted call would be given
    for S, n in ((0, 8), (1, 0), (65536, 1), (2, 2 ** 30)):
        with pytest.raises(RuntimeError, match="contract violated"):
            L.call("mivp_sort_u32", p, S, n, p, None)
    with pytest.raises(RuntimeError, match="contract violated"):
        L.call("mivp_sort_u32", None, 1, 8, p, None)
    for B, vol, C, lam in ((0, 8, 2, 1.0), (2, 0, 2, 1.0), (2, 8, 1, 1.0), (2, 8, 9, 1.0), (2, 8, 2, -1.0), (2, 8, 2, float("nan")),
                           (2, 8, 2, float("inf")), (65536, 8, 2, 1.0), (4, 2 ** 27, 8, 1.0)):
        for per_image in (0, 1):
            with pytest.raises(RuntimeError, match="contract violated"):
                L.call("mivp_lovasz_loss", p, p, B, vol, C, 1, 0, 0, per_image, 0, lam, None, p, p, None, 0, None)
            with pytest.raises(RuntimeError, match="contract violated"):
                L.call("mivp_lovasz_loss_grad", p, p, B, vol, C, 1, 0, 0, per_image, 0, lam, None, p, None, p, 0, None)
            if lam == 1.0:
                with pytest.raises(RuntimeError, match="contract violated"):
                    L.call("mivp_lovasz_keys", p, p, B, vol, C, 1, 0, 0, per_image, p, p, None)
    with pytest.raises(RuntimeError, match="contract violated"):
        L.call("mivp_lovasz_loss", p, p, 2, 8, 2, 1, 0, 0, 0, 0, 1.0, None, None, p, None, 0, None)
