"""CPU checks of tests/uphead_ref.py, the float64 reference of the low-resolution head kernels: the reference is
consistent with itself (the plane decomposition reproduces the composite op, the adjoint is the transpose of the gather),
every case of tests/test_hip_uphead.py finds a draw density that meets conditions (a) to (d) on the reference alone, and
the two comparisons (bit equality, bf16 interval) fail on a one-element error planted at a corner voxel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_ref as E  # noqa: E402
import uphead_ref as R  # noqa: E402

SMALL = ("S1", "S2", "S3", "S4")


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("cout", [1, 2])
def test_plane_decomposition_reproduces_the_composite_op(name, cout):
    """planes_ref -> clamped .25 / .75 interpolation -> masked taps == conv3d(up(x) * scale + shift, w, b), exactly."""
    c = R.forward_case(name, 8, cout)
    E.assert_equal_located(R.gather_planes(c.planes, c.b), c.ref, "bchwd", f"decomposition {name}")


@pytest.mark.parametrize("name", SMALL)
def test_adjoint_is_the_transpose_of_the_gather(name):
    """<dy, gather(Y)> == <D, Y> exactly, for integer planes Y."""
    B, h, w, d = R.SHAPES[name]
    c = R.adjoint_case(name, 2)
    Y = E.draw(E.gen(11), (27, B, 2, h, w, d), (-3, -2, -1, 1, 2, 3))
    lhs = float((c.dy * R.gather_planes(Y)).sum())
    rhs = float((c.D * Y.permute(1, 3, 4, 5, 0, 2).reshape(B * h * w * d, 54)).sum())
    assert abs(lhs) < 2 ** 53 / 64 and lhs == rhs, (lhs, rhs)
    assert float(c.D.abs().sum()) > 0


def test_gram_of_the_reference_has_the_claimed_row_sums():
    """U^T U 1 = 8 at every cell (the columns of U sum to 2 per axis): a sanity check of gx that restates no Gram weight."""
    for name in SMALL:
        B, h, w, d = R.SHAPES[name]
        (_, _, gx), _ = R.stats_ref(torch.ones((B, 1, h, w, d), dtype=torch.float64))
        assert torch.equal(gx, torch.full_like(gx, 8.0)), name


def test_every_case_meets_the_conditions_on_the_reference_alone():
    """Each builder picks its density with first_exact and asserts (a) to (d) itself; the densities are printed."""
    lines = []
    for label, build in R.all_cases():
        c = build()
        lines.append(f"{label}: density {c.dens}")
    print("\n".join(lines))
    assert len(lines) == len(R.all_cases())
    # the D reference of every adjoint case is a bf16 number everywhere: no case falls back to the interval form
    for name in R.SHAPES:
        assert bool(E.is_bf16(R.adjoint_case(name, 2).D).all())
    # and the training-mode dx is the one output that is not: it needs the interval form
    assert any(not bool(E.is_bf16(R.dx_case(name, C, R.dx_cout(C), True).ref).all()) for name, C in R.shape_c_pairs())


def test_equality_fails_on_one_planted_error_at_a_corner_voxel():
    c = R.forward_case("S3", 8, 2)
    ref = R.cl64(c.ref)
    B, H, W, D, _ = ref.shape
    bad = ref.clone()
    bad[B - 1, H - 1, 0, D - 1, 1] += 1
    with pytest.raises(AssertionError) as ei:
        E.assert_equal_located(bad.float(), ref, "bhwdc", "planted")
    text = str(ei.value)
    assert "1 of" in text and f"({B - 1}, {H - 1}, 0, {D - 1}, 1)" in text and "'corner': 1" in text
    E.assert_equal_located(ref.float(), ref, "bhwdc")


def test_interval_fails_on_one_planted_error_at_a_corner_voxel():
    c = R.dx_case("S3", 8, 1, True)
    ref = c.ref
    B, h, w, d, _ = ref.shape
    stored = ref.float().bfloat16()
    R.assert_interval_located(stored, ref)                       # round to nearest lies inside
    assert not bool(E.is_bf16(ref).all())
    at = (B - 1, 0, w - 1, d - 1, 3)
    assert float(ref[at]) != 0
    up = torch.nextafter(stored[at], torch.tensor(float("inf"), dtype=torch.bfloat16))
    down = torch.nextafter(stored[at], torch.tensor(float("-inf"), dtype=torch.bfloat16))
    bad = stored.clone()
    bad[at] = up if abs(float(up) - float(ref[at])) > abs(float(down) - float(ref[at])) else down    # the farther neighbour
    if abs(float(bad[at]) - float(ref[at])) <= float(R.bf16_half_spacing(ref[at])):                  # a tie: go one further
        bad[at] = torch.nextafter(bad[at], bad[at] * 4)
    with pytest.raises(AssertionError) as ei:
        R.assert_interval_located(bad, ref, "planted")
    text = str(ei.value)
    assert "1 of" in text and str(at) in text and "'corner': 1" in text
    nan = stored.clone()
    nan[at] = float("nan")
    with pytest.raises(AssertionError):
        R.assert_interval_located(nan, ref)


def test_half_spacing():
    v = torch.tensor([0.0, 1.0, 1.5, 2.0, -3.0, 255.0, 256.0, 1.0 / 512], dtype=torch.float64)
    want = torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 0.5, 1.0, 2.0 ** -17], dtype=torch.float64)
    assert torch.equal(R.bf16_half_spacing(v), want)
