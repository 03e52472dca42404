"""CPU tests of the clDice term's restatement (tests/cldice_ref.py), of the bars tests/test_hip_cldice.py holds the kernels
to, and of the plain-torch path and the argument checks of ``soft_skeleton`` / ``cldice_loss`` / ``SegLossSpec``
(DESIGN 4.36 / 5.8)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cldice_ref as R  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import losses

GRID_SHAPES = ((1, 1, 4), (2, 2, 2), (3, 3, 7), (5, 7, 9), (6, 7, 8))


# ---------------------------------------------------------------------------------------------
# the clDice authors' soft_skel as a torch max-pool composition
# ---------------------------------------------------------------------------------------------
def soft_erode(img):
    p1 = -F.max_pool3d(-img, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    p2 = -F.max_pool3d(-img, (1, 3, 1), (1, 1, 1), (0, 1, 0))
    p3 = -F.max_pool3d(-img, (1, 1, 3), (1, 1, 1), (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def soft_open(img):
    return F.max_pool3d(soft_erode(img), (3, 3, 3), (1, 1, 1), (1, 1, 1))


def soft_skel(img, iter_):
    skel = F.relu(img - soft_open(img))
    for _ in range(iter_):
        img = soft_erode(img)
        delta = F.relu(img - soft_open(img))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32 if a.dtype == np.float32 else np.int64),
                                                                        b.view(np.int32 if b.dtype == np.float32 else np.int64))


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("dims", R.SHAPES, ids=str)
def test_restatement_is_the_max_pool_composition_in_every_bit(dims, n):
    for kind in R.KINDS:
        x = R.fields(kind, 3, dims)
        want = soft_skel(torch.from_numpy(x).unsqueeze(0), n)[0].numpy()
        assert same_bits(R.soft_skeleton(x, n), want), (kind, dims, n)


@pytest.mark.parametrize("dims", ((3, 3, 7), (5, 7, 9), (6, 7, 8)), ids=str)
def test_restatement_backward_is_autograd_where_nothing_ties(dims):
    x = R.rng(3, *dims).random((2,) + dims)                            # float64 noise: no two values equal
    assert np.unique(x).size == x.size
    g = R.rng(4, *dims).uniform(-1, 1, x.shape)
    xt = torch.from_numpy(x).unsqueeze(0).requires_grad_(True)
    soft_skel(xt, 3).backward(torch.from_numpy(g).unsqueeze(0))
    got = R.soft_skeleton_bwd(x, 3, g)
    assert np.abs(got - xt.grad[0].numpy()).max() <= 1e-14
    assert np.abs(got).max() > 0.1


def test_ties_share_equally_on_two_hand_cases():
    """1 x 1 x 4: x = (1, .5, .5, 1), g = (1, 2, 3, 4), n = 1.  E_1 = E_2 = O_0 = O_1 = .5, so d_0 = (.5, 0, 0, .5), d_1 = 0,
    A_1 = 0, A_0 = (1, 0, 0, 4).  O_0(0) = max(E_1(0), E_1(1)) ties twice: G_1 = (-1/2, -1/2, -2, -2).  E_1(0) = min(x_0, x_1)
    selects voxel 1; E_1(1) and E_1(2) tie voxels 1 and 2; E_1(3) selects voxel 2:
      G_0 = (1, -1/2 - 1/4 - 1, -1/4 - 1 - 2, 4) = (1, -1.75, -3.25, 4).
    2 x 2 x 2: x = 1 at the corner, .5 elsewhere, g = 2 at the corner, n = 1.  E_1 = .5 everywhere, d_0 = .5 at the corner only,
    A_0 = 2 there; O_0(corner) ties all 8 voxels: G_1 = -1/4 everywhere.  Tie counts of E_1: 3 at the corner (its three
    neighbours) and at each neighbour (itself and two voxels two steps away), 4 elsewhere, so with q = -1/4:
      corner 2;  one and two steps away q (1/3 + 1/3 + 1/4 + 1/4) and q (1/4 + 2/3 + 1/4) = -7/24;  the far corner q."""
    x = np.array([1.0, 0.5, 0.5, 1.0]).reshape(1, 1, 4)
    g = np.array([1.0, 2.0, 3.0, 4.0]).reshape(1, 1, 4)
    for dt in (np.float64, np.float32):
        got = R.soft_skeleton_bwd(x.astype(dt), 1, g.astype(dt))
        assert np.array_equal(got.ravel(), np.array([1.0, -1.75, -3.25, 4.0], dt))
    x = np.full((2, 2, 2), 0.5)
    x[0, 0, 0] = 1.0
    g = R.rng(1).uniform(-1, 1, (2, 2, 2))
    g[0, 0, 0] = 2.0
    want = np.empty((2, 2, 2))
    for h, w, d in np.ndindex(2, 2, 2):
        want[h, w, d] = (2.0, -7.0 / 24.0, -7.0 / 24.0, -0.25)[h + w + d]
    got = R.soft_skeleton_bwd(x, 1, g)
    assert np.abs(got - want).max() <= 1e-16
    first = R.soft_skeleton_bwd(x, 1, g, R.Bugs(first_index=True))
    assert np.abs(first - want).max() > 0.1                            # the first-index rule is another gradient


@pytest.mark.parametrize("n", (1, 2, 3))
@pytest.mark.parametrize("dims", GRID_SHAPES, ids=str)
def test_sixteenth_grid_is_exact_in_float32(dims, n):
    x = R.fields("grid16", 3, dims)
    assert same_bits(R.soft_skeleton(x, n).astype(np.float64), R.soft_skeleton(x.astype(np.float64), n))


# ---------------------------------------------------------------------------------------------
# planted kernel bugs leave the bars of tests/test_hip_cldice.py
# ---------------------------------------------------------------------------------------------
def backward_misses(x, n, g, bugs):
    """Whether the float32 backward with ``bugs`` leaves the bars against the float64 definition."""
    g64 = R.soft_skeleton_bwd(x.astype(np.float64), n, g.astype(np.float64))
    bad = R.soft_skeleton_bwd(x, n, g, bugs).astype(np.float64)
    if not np.abs(g64).max() > 0:
        return bool(np.abs(bad).max() > 0)
    e32, scale = R.yardstick(R.soft_skeleton_bwd(x, n, g), g64)
    return bool(np.abs(bad - g64).max() > R.LOSS_MARGIN * e32 * scale) or R.rel_l2(bad, g64) >= R.LOSS_L2_BAR


def test_the_definition_itself_meets_the_bars():
    for kind in R.KINDS:
        x = R.fields(kind, 2, (6, 7, 8))
        g = R.rng(5).uniform(-1, 1, x.shape).astype(np.float32)
        assert not backward_misses(x, 3, g, R.NONE), kind


@pytest.mark.parametrize("bug", ("erode_cube", "halo_zero", "one_iteration_less"))
def test_forward_bugs_change_the_bits(bug):
    x = R.fields("tube", 2, (6, 7, 8))
    assert not same_bits(R.soft_skeleton(x, 3, R.Bugs(**{bug: True})), R.soft_skeleton(x, 3))
    g = R.rng(5).uniform(-1, 1, x.shape).astype(np.float32)
    assert backward_misses(x, 3, g, R.Bugs(**{bug: True}))


def test_backward_bugs_leave_the_bars():
    g = R.rng(5).uniform(-1, 1, (2, 6, 7, 8)).astype(np.float32)
    assert backward_misses(R.fields("grid16", 2, (6, 7, 8)), 3, g, R.Bugs(first_index=True))
    assert backward_misses(R.fields("binary", 2, (6, 7, 8)), 3, g, R.Bugs(first_index=True))
    assert backward_misses(R.fields("ones", 2, (6, 7, 8)), 3, g, R.Bugs(relu_grad_at_zero=True))     # zero is owed
    assert backward_misses(R.fields("grid16", 2, (6, 7, 8)), 3, g, R.Bugs(relu_grad_at_zero=True))


def test_reference_gradient_of_the_term_is_not_vacuous():
    for kind in ("noise", "tube"):
        z, y = R.term_case(kind, 2, 3, (6, 7, 8), R.IGNORE)
        value, dz, p = R.term(z, y, (6, 7, 8), 3, 1.0, False, R.IGNORE)
        valid = R.valid_mask(y, 3, R.IGNORE)
        share = float((np.abs(dz).max(-1) > 0)[valid].mean())
        assert share >= 0.5, (kind, share)
        assert 0.0 < value < 1.0
        assert np.all(dz[~valid] == 0)


# ---------------------------------------------------------------------------------------------
# the plain-torch path of the package
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", ((2, 2, 2), (5, 7, 9)), ids=str)
def test_torch_path_of_soft_skeleton(dims):
    for kind in ("noise", "grid16", "binary", "ones"):
        x = R.fields(kind, 4, dims).reshape(2, 2, *dims)
        got = losses.soft_skeleton(torch.from_numpy(x), 3)
        assert same_bits(got.numpy(), R.soft_skeleton(x, 3)), kind
        g = R.rng(6).uniform(-1, 1, x.shape)
        xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        out = losses.soft_skeleton(xt, 3)
        assert type(out.grad_fn).__name__ != "_SkeletonFnBackward"
        out.backward(torch.from_numpy(g))
        assert np.abs(xt.grad.numpy() - R.soft_skeleton_bwd(x.astype(np.float64), 3, g)).max() <= 1e-14, kind


@pytest.mark.parametrize("batch", (False, True))
def test_torch_path_of_cldice_loss(batch):
    dims, B, C = (5, 7, 9), 2, 3
    z, y = R.term_case("grid16", B, C, dims, R.IGNORE)
    want, dz, _ = R.term(z, y, dims, 2, 0.5, batch, R.IGNORE)
    zt = torch.from_numpy(z.astype(np.float64)).reshape(B, *dims, C).permute(0, 4, 1, 2, 3).requires_grad_(True)
    w = torch.tensor([0.37], dtype=torch.float64)
    got = losses.cldice_loss(zt, torch.from_numpy(y).reshape(B, 1, *dims), iterations=2, smooth=0.5, batch=batch,
                             ignore_index=R.IGNORE, weight=w)
    got.backward()
    assert abs(float(got.detach()) - 0.37 * want) <= 1e-13
    grad = zt.grad.permute(0, 2, 3, 4, 1).reshape(B, -1, C).numpy()
    assert np.abs(grad - 0.37 * dz).max() <= 1e-14
    spec = losses.SegLossSpec(lambda_region=0.0, lambda_voxel=0.0, lambda_cldice=2.0, cldice_iterations=2, cldice_smooth=0.5,
                              batch=batch, ignore_index=R.IGNORE)
    alone = losses.seg_loss(zt.detach(), torch.from_numpy(y).reshape(B, 1, *dims), spec, cldice_weight=w)
    assert abs(float(alone) - 2.0 * 0.37 * want) <= 1e-13
    both = losses.SegLossSpec(lambda_cldice=2.0, cldice_iterations=2, cldice_smooth=0.5, batch=batch, ignore_index=R.IGNORE)
    rest = losses.SegLossSpec(batch=batch, ignore_index=R.IGNORE)
    tgt = torch.from_numpy(y).reshape(B, 1, *dims)
    total = losses.seg_loss(zt.detach(), tgt, both, cldice_weight=w)
    assert abs(float(total) - float(losses.seg_loss(zt.detach(), tgt, rest)) - 2.0 * 0.37 * want) <= 1e-12


# ---------------------------------------------------------------------------------------------
# options and the ABI
# ---------------------------------------------------------------------------------------------
def test_spec_defaults_are_unchanged_and_the_new_fields_are_checked():
    spec = losses.SegLossSpec()
    assert (spec.lambda_cldice, spec.cldice_iterations, spec.cldice_smooth) == (0.0, 3, 1.0)
    assert losses.SegLossSpec.__slots__[-3:] == ("lambda_cldice", "cldice_iterations", "cldice_smooth")
    assert losses.SegLossSpec.__slots__[-4] == "boundary_spacing"
    assert spec == losses.SegLossSpec(lambda_cldice=0.0) and hash(spec) == hash(losses.SegLossSpec(cldice_iterations=3))
    assert repr(losses.SegLossSpec(lambda_cldice=0.5)).startswith(repr(spec).split("lambda_cldice")[0])
    with pytest.raises(ValueError, match="must not all be 0"):
        losses.SegLossSpec(lambda_region=0.0, lambda_voxel=0.0)
    losses.SegLossSpec(lambda_region=0.0, lambda_voxel=0.0, lambda_cldice=1.0)
    losses.SegLossSpec(lambda_boundary=1.0, lambda_cldice=1.0)
    for bad in (0, 17, 2.0, True, None):
        with pytest.raises(ValueError, match="cldice_iterations"):
            losses.SegLossSpec(cldice_iterations=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e39, 1e-50, True):
        with pytest.raises(ValueError, match="cldice_smooth"):
            losses.SegLossSpec(cldice_smooth=bad)
    for bad in (-1.0, float("nan"), 1e39):
        with pytest.raises(ValueError, match="lambda_cldice"):
            losses.SegLossSpec(lambda_cldice=bad)
    with pytest.raises(ValueError, match="top_k together with lambda_cldice"):
        losses.SegLossSpec(top_k=0.5, lambda_cldice=1.0)


def test_wrapper_argument_checks():
    z, y = torch.zeros(1, 2, 2, 2, 2), torch.zeros(1, 1, 2, 2, 2)
    with pytest.raises(ValueError, match="iterations"):
        losses.cldice_loss(z, y, iterations=0)
    with pytest.raises(ValueError, match="smooth"):
        losses.cldice_loss(z, y, smooth=0.0)
    with pytest.raises(ValueError, match="batch"):
        losses.cldice_loss(z, y, batch=1)
    with pytest.raises(ValueError, match="ignore_index"):
        losses.cldice_loss(z, y, ignore_index=0.5)
    with pytest.raises(ValueError, match="weight"):
        losses.cldice_loss(z, y, weight=torch.ones(2))
    with pytest.raises(ValueError, match="target"):
        losses.cldice_loss(z, y[..., :1])
    with pytest.raises(ValueError, match="at least 2 classes"):
        losses.cldice_loss(z[:, :1], y)
    with pytest.raises(ValueError, match=r"\[B, K, H, W, D\]"):
        losses.soft_skeleton(torch.zeros(2, 2, 2), 3)
    with pytest.raises(ValueError, match="iterations"):
        losses.soft_skeleton(torch.zeros(1, 1, 2, 2, 2), 17)
    mod = losses.SegLoss(lambda_cldice=1.0)
    mod.set_cldice_weight(0.25)
    assert float(mod.cldice_weight) == 0.25 and "cldice_weight" not in mod.state_dict()
    with pytest.raises(ValueError):
        mod.set_cldice_weight(float("nan"))


def test_the_entries_joined_abi_18():
    assert L.ABI_VERSION == 18
    protos = L.parse_header()
    assert len(protos["mivp_seg_loss"][1]) == 19
    assert len(protos["mivp_boundary_loss"][1]) == 16
    assert len(protos["mivp_cldice_loss"][1]) == 17 and len(protos["mivp_cldice_loss_grad"][1]) == 17
    assert len(protos["mivp_cldice_skeleton"][1]) == 8 and len(protos["mivp_cldice_skeleton_grad"][1]) == 8
    assert protos["mivp_cldice_ws"][0] is L.C.c_size_t and protos["mivp_cldice_skeleton_ws"][0] is L.C.c_size_t
