"""CPU proof that the exact-integer comparison of tests/exact_ref.py sees local indexing mistakes that the global
rel-L2 bars of the GPU tests do not.  Everything runs on the float64 reference: each test corrupts the reference the way a
kernel with one wrong index would, then asserts that ``assert_equal_located`` fails while ``rel_l2`` stays under the bar
the GPU tests apply to that tensor (4e-3 for a bf16 conv output, 1e-5 for a gemm_tn result).  Where a corruption was too
loud for the bar at the chosen shape the corruption was shrunk (fewer taps, fewer rows), never the bar.
Conditions (a) and (b) of the method are unit-tested at the end on inputs that violate them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_ref as E  # noqa: E402
from conftest import rel_l2  # noqa: E402

CONV_BAR = 4e-3          # tests/test_hip_ops.py: bf16 conv outputs
GEMM_BAR = 1e-5          # tests/test_hip_wgrad.py: gemm_tn results


@pytest.fixture(scope="module")
def halo_case():
    """The 144 -> 48, (9, 13, 21), B = 2 conv of the halo-brick test, with an affine prologue and bias: integer draws."""
    cin, cout, dims = 144, 48, (9, 13, 21)

    def make(dens):                                            # half-integers (scale 0.5) are bf16 numbers only below 128
        g = E.gen(1)
        x = E.draw(g, (2, cin, *dims), (-2, -1, 1, 2), 0.5)
        w = E.draw(g, (cout, cin, 3, 3, 3), (-1, 1), dens)
        bias = E.draw(g, (cout,), (-3, -2, -1, 1, 2, 3))
        scale = E.draw(g, (cin,), (1, 2, -1, 0.5))
        shift = E.draw(g, (cin,), (-3, -2, -1, 1, 2, 3))
        ref, bound = E.conv3d_ref(x, w, bias, scale, shift)
        return ref, bound, True, (x, w, bias, scale, shift, ref, bound)

    x, w, bias, scale, shift, ref, bound = E.first_exact(make, (0.06, 0.03, 0.015))
    E.assert_exact_inputs(ref, bound, True, "halo_case")
    xin = E.affine_input(x, scale, shift)
    xpad = torch.nn.functional.pad(xin, (1, 1, 1, 1, 1, 1))
    return {"x": x, "w": w, "bias": bias, "scale": scale, "shift": shift, "ref": ref, "xpad": xpad, "dims": dims}


def _assert_seen_by_exact_only(bad, ref, layout, bar):
    err = rel_l2(bad, ref)
    print(f"rel_l2 {err:.2e} (bar {bar:g}), {int((bad != ref).sum())} of {ref.numel()} elements wrong")
    assert err < bar, f"the corruption is louder than the old bar ({err:.2e} >= {bar}): shrink the corruption"
    with pytest.raises(AssertionError, match="differ from the float64 reference"):
        E.assert_equal_located(bad, ref, layout)
    return err


def test_plain_draw_matches_the_issue_figures():
    """x from {-2,-1,1,2} and w from {-1,1}, both at density 0.5, at 144 -> 48, (9,13,21): conditions (a) and (b) hold."""
    g = E.gen(0)
    x = E.draw(g, (2, 144, 9, 13, 21), (-2, -1, 1, 2), 0.5)
    w = E.draw(g, (48, 144, 3, 3, 3), (-1, 1), 0.5)
    ref, bound = E.conv3d_ref(x, w)
    E.assert_exact_inputs(ref, bound, True)
    assert float(ref.abs().max()) <= 256 and float((ref != 0).double().mean()) > 0.95


def test_dropped_tap_at_a_corner_voxel(halo_case):
    c = halo_case
    H, W, D = c["dims"]
    b, h, w, d = 1, H - 1, W - 1, D - 1
    win = E.conv_window(c["xpad"], b, h, w, d).clone()
    assert float(win[:, 0, 0, 0].abs().sum()) > 0
    win[:, 0, 0, 0] = 0                                        # tap (-1, -1, -1): inside the volume at the far corner
    bad = c["ref"].clone()
    bad[b, :, h, w, d] = torch.einsum("oiabc,iabc->o", c["w"], win) + c["bias"]
    _assert_seen_by_exact_only(bad, c["ref"], "bchwd", CONV_BAR)


def test_halo_cell_holding_shift_instead_of_zero(halo_case):
    c = halo_case
    xpad = c["xpad"].clone()
    xpad[0, :, 0, 0, 0] = c["shift"]                           # the padding cell (-1, -1, -1): affine applied to a zero
    bad = torch.nn.functional.conv3d(xpad, c["w"], c["bias"])
    assert int((bad != c["ref"]).any(1).sum()) == 1            # only voxel (0, 0, 0, 0) reads that cell
    _assert_seen_by_exact_only(bad, c["ref"], "bchwd", CONV_BAR)


def test_window_crossing_into_the_next_batch_element(halo_case):
    c = halo_case
    H, W, D = c["dims"]
    b, h, w, d = 0, H - 1, 5, 7
    win = E.conv_window(c["xpad"], b, h, w, d).clone()
    assert float(win[:, 2].abs().sum()) == 0                   # the plane below the volume is padding
    # in channels-last memory the voxel "below" (b, H-1, w, d) is (b+1, 0, w, d); shrunk to the centre tap of that plane
    win[:, 2, 1, 1] = E.conv_window(c["xpad"], b + 1, 0, w, d)[:, 1, 1, 1]
    bad = c["ref"].clone()
    bad[b, :, h, w, d] = torch.einsum("oiabc,iabc->o", c["w"], win) + c["bias"]
    _assert_seen_by_exact_only(bad, c["ref"], "bchwd", CONV_BAR)


def test_swapped_taps_in_one_channel_group_at_the_last_ragged_brick_row():
    """48 -> 144, (5, 9, 17), B = 3: three output-channel groups of 48; h = 4 is the ragged last row of 4-high bricks.
    One k-step of the halo kernel holds taps (2j, 2j+1) x 16 input channels: swap those two taps for one 16-channel chunk
    in group 1 at one voxel of that row."""
    g = E.gen(2)
    cin, cout, dims = 48, 144, (5, 9, 17)
    x = E.draw(g, (3, cin, *dims), (-2, -1, 1, 2), 0.5)
    w = E.draw(g, (cout, cin, 3, 3, 3), (-1, 1), 0.25)
    ref, bound = E.conv3d_ref(x, w)
    E.assert_exact_inputs(ref, bound, True)
    xpad = torch.nn.functional.pad(x, (1, 1, 1, 1, 1, 1))
    b, h, wv, d = 2, 4, 4, 9
    wbad = w[48:96].clone()
    t0, t1 = E.taps()[12], E.taps()[13]                        # k-step 6: taps 12 and 13 (the centre tap)
    wbad[:, 16:32, t0[0], t0[1], t0[2]] = w[48:96, 16:32, t1[0], t1[1], t1[2]]
    wbad[:, 16:32, t1[0], t1[1], t1[2]] = w[48:96, 16:32, t0[0], t0[1], t0[2]]
    bad = ref.clone()
    bad[b, 48:96, h, wv, d] = torch.einsum("oiabc,iabc->o", wbad, E.conv_window(xpad, b, h, wv, d))
    _assert_seen_by_exact_only(bad, ref, "bchwd", CONV_BAR)


def test_gemm_tn_last_columns_taken_from_the_neighbouring_block():
    """N = 520 = 8 blocks of 64 + 8 columns: the last 4 columns of the ragged block come from the block before it.
    The 1e-5 bar of the gemm_tn tests is so tight that only a result with a large common part can hide a wrong element:
    operands 1 + a sparse {-1, +1} term (every entry of the result is close to T), corruption shrunk to one row."""
    g = E.gen(3)
    T, M, N = 4097, 520, 520
    a = 1.0 + E.draw(g, (T, M), (-1, 1), 0.004)
    b = 1.0 + E.draw(g, (T, N), (-1, 1), 0.004)
    ref, bound = E.matmul_tn_ref(a, b)
    E.assert_exact_inputs(ref, bound, False)
    bad = ref.clone()
    bad[M - 1, N - 4:] = ref[M - 1, N - 4 - 64:N - 64]
    assert int((bad != ref).sum()) >= 1
    _assert_seen_by_exact_only(bad, ref, "mn", GEMM_BAR)


def test_located_report_names_voxel_channel_and_position(halo_case, capsys):
    ref = halo_case["ref"].permute(0, 2, 3, 4, 1).contiguous()
    bad = ref.clone()
    bad[1, 0, 0, 20, 5] += 1                                   # a corner
    bad[0, 3, 0, 7, 2] += 1                                    # a face
    bad[0, 3, 4, 7, 2] += 1                                    # interior
    with pytest.raises(AssertionError) as ei:
        E.assert_equal_located(bad.float(), ref, "bhwdc", what="demo")
    text = str(ei.value)
    assert "3 of" in text and "(1, 0, 0, 20, 5)" in text and "(0, 3, 0, 7, 2)" in text
    assert "'corner': 1" in text and "'face': 1" in text and "'interior': 1" in text and "'edge': 0" in text
    assert "demo" in capsys.readouterr().out
    E.assert_equal_located(ref.bfloat16(), ref, "bhwdc")        # equal through a bf16 store: condition (b) held


def test_condition_a_rejects_sums_that_can_round():
    g = E.gen(4)
    x = E.draw(g, (1, 16, 3, 3, 3), (4096,))
    w = E.draw(g, (16, 16, 3, 3, 3), (4096,))
    ref, bound = E.conv3d_ref(x, w)
    assert float(bound.max()) >= 2 ** 24
    with pytest.raises(AssertionError, match=r"condition \(a\)"):
        E.assert_exact_inputs(ref, bound, False)
    a = torch.full((2 ** 12, 1), 2.0 ** 6, dtype=torch.float64)
    ref, bound = E.matmul_tn_ref(a, a)                          # 2**12 * 2**12 = 2**24 exactly: not below the limit
    with pytest.raises(AssertionError, match=r"condition \(a\)"):
        E.assert_exact_inputs(ref, bound, False)
    with pytest.raises(AssertionError, match="absolute-value form"):
        E.assert_exact_inputs(ref, bound - 1, False)


def test_condition_b_rejects_values_a_bf16_store_would_round():
    ref = torch.tensor([1.0, 256.0, 257.0, -3.5], dtype=torch.float64)
    E.assert_exact_inputs(ref, ref.abs(), False)
    with pytest.raises(AssertionError, match=r"condition \(b\).*1 of 4"):
        E.assert_exact_inputs(ref, ref.abs(), True)
    with pytest.raises(AssertionError):
        E.assert_bf16_operands(torch.tensor([0.1], dtype=torch.float64))
    E.assert_bf16_operands(torch.tensor([0.75, -192.0, 2.0 ** 20], dtype=torch.float64), None)
    # the density search never hands back a case that violates a condition
    with pytest.raises(AssertionError, match="no density"):
        E.first_exact(lambda dens: (ref, ref.abs(), True, None))
    assert E.first_exact(lambda dens: (ref * 0 + dens, ref * 0 + dens, True, dens), (0.1, 0.5)) == 0.5


def test_ulp_distance():
    r = torch.tensor([1.0, -3.0, 1e-3], dtype=torch.float64)
    g32 = r.float()
    up = torch.nextafter(g32, torch.full_like(g32, float("inf")))
    assert torch.equal(E.ulp_distance(g32, r), torch.zeros(3, dtype=torch.float64))
    d = E.ulp_distance(up, r)
    assert float(d.max()) <= 1.0 + 1e-9 and float(d.min()) >= 0.5
