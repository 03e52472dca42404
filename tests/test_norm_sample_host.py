"""CPU checks of tests/norm_sample_ref.py, run before any kernel:

1. the bounds are honest: plain f32 torch in each kernel's operation order stays inside every bound on all elements of the cases
   the GPU tests use, and the closed float64 form of the backward agrees with autograd;
2. the bounds see plausible bugs the rel-L2 bars of tests/test_hip_ops.py (4e-3 / 6e-3 / 3e-3) and of
   test_sampling_kernel_on_channels_last_bf16_latent (1e-6 / 3e-3) do not: each injection prints its rel-L2 beside the count of
   located violations;
3. the host tables of losses._axis_np are right over the whole domain."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_sample_ref as R  # noqa: E402
from mivp_amd.losses import _axis_np

F64, F32 = R.F64, R.F32
OLD_BARS = dict(bn_fwd=4e-3, bn_dx=6e-3, bn_dw=3e-3, sample_fwd=1e-6, sample_bwd=3e-3)


def violations(got, ref, bound):
    g = got.to(F64)
    return int((~((g - ref).abs() <= bound)).sum())


def inside(got, ref, bound, layout, what):
    R.assert_within_located(got, ref, bound, layout, what)
    return R.used(got, ref, bound)


def fed(o, lrelu=True):
    st = R.bn_forward(o.x, o.w, o.b)
    return st, st.scale32, st.shift32, st.mean32, st.rstd32


# ---------------------------------------------------------------------------------------------- 1. honest bounds
@pytest.mark.parametrize("case", R.BN_SMALL + R.BN_STATS_CAP, ids=R.bn_id)
def test_f32_statistics_stay_inside_their_bounds(case):
    n, C = case
    o = R.bn_operands(n, C, seed=n + C)
    st, sc, sh, mu, rs = fed(o)
    assert not bool(R.gate_undecided(o.x, sc, sh).any())
    nblk, G = R.stats_nblk(n, C), C // 8
    k = R.chain_len(n * G, nblk, G)
    ref, mag = R.bn_sums(o.x)
    part = R.emul_bn_stats(o.x, nblk)
    assert not bool(part[R.live_blocks(n * G):].any())
    f1 = inside(part.to(F64).sum(0), ref, R.SLACK * k * R.U32 * mag, "c", f"f32 bn_stats {case}")
    c = R.bn_backward_closed(o.x, o.dy, o.w, o.b, True)
    part = R.emul_bwd_stats(o.x, o.dy, sc, sh, mu, rs, True, nblk)
    f2 = inside(part.to(F64).sum(0), torch.cat([c.S1, c.S2]), R.bwd_sums_bounds(c, k), "c", f"f32 bn_bwd_stats {case}")
    print(f"[host] {R.bn_id(case)} k={k}: bn_stats uses {f1:.3f} of its bound, bn_bwd_stats {f2:.3f}")


@pytest.mark.parametrize("case", R.BN_SMALL + R.BN_APPLY_CAP, ids=R.bn_id)
def test_f32_elementwise_kernels_stay_inside_their_bounds(case):
    n, C = case
    o = R.bn_operands(n, C, seed=n + C)
    st, sc, sh, mu, rs = fed(o)
    assert not bool(R.gate_undecided(o.x, sc, sh).any())
    for lrelu in (True, False):
        y, e32 = R.affine_ref(o.x, sc, sh, lrelu)
        f1 = inside(R.emul_affine(o.x, sc, sh, lrelu), y, R.with_bf16(y, e32), "nc", f"f32 affine_act {case} lrelu={lrelu}")
        c = R.bn_backward_closed(o.x, o.dy, o.w, o.b, lrelu)
        sums = R.r32(torch.cat([c.S1, c.S2]))
        dx = R.emul_bwd_apply(o.x, o.dy, sc, sh, mu, rs, sums, lrelu)
        f2 = inside(dx, c.dx, R.with_bf16(c.dx, R.bwd_dx_bound(c, o.x)), "nc", f"f32 bn_bwd_apply {case} lrelu={lrelu}")
        ce = R.bn_backward_closed(o.x, o.dy, o.w, o.b, lrelu, train=False)
        dxe = R.emul_bwd_apply(o.x, o.dy, sc, sh, mu, rs, torch.zeros(2 * C, dtype=F64), lrelu)
        f3 = inside(dxe, ce.dx, R.with_bf16(ce.dx, R.bwd_dx_bound(ce, o.x, train=False)), "nc", f"f32 eval dx {case} lrelu={lrelu}")
        print(f"[host] {R.bn_id(case)} lrelu={lrelu}: affine {f1:.3f}, dx {f2:.3f}, eval dx {f3:.3f} of the bounds")


@pytest.mark.parametrize("C", (8, 48, 144))
@pytest.mark.parametrize("lrelu", (True, False))
def test_closed_form_backward_is_autograd(C, lrelu):
    o = R.bn_operands(R.SMALL_N, C, seed=C)
    R.plant_symmetric_zero_channel(o)
    c = R.bn_backward_closed(o.x, o.dy, o.w, o.b, lrelu)
    dx, dg, db = R.bn_backward_autograd(o.x, o.dy, o.w, o.b, lrelu)
    for name, a, b in (("dx", c.dx, dx), ("dgamma", c.S2, dg), ("dbeta", c.S1, db)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
    if lrelu:                                                               # torch's rule at z == 0: the 0.01 slope
        zero = c.z[:, 0] == 0
        assert int(zero.sum()) >= 2 and bool((c.gz[zero, 0] == R.SLOPE * o.dy[zero, 0]).all())


@pytest.mark.parametrize("C", R.FINALIZE_C)
@pytest.mark.parametrize("nblk", R.FINALIZE_NBLK)
def test_f32_finalize_stays_inside_its_bounds(nblk, C):
    part, count = R.finalize_part(nblk, C, seed=nblk * 100 + C)
    g = R.gen(nblk + C)
    w, b = (1 + 0.3 * torch.randn(C, generator=g)).to(F64), (0.3 * torch.randn(C, generator=g)).to(F64)
    rm, rv = torch.randn(C, generator=g).to(F64), (0.5 + torch.rand(C, generator=g)).to(F64)
    for wv, bv, run in ((w, b, True), (None, b, True), (w, None, True), (w, b, False)):
        ref = R.finalize_ref(part, count, wv, bv, R.EPS, R.MOMENTUM, rm if run else None, rv if run else None)
        got = R.emul_finalize(part, count, wv, bv, R.EPS, R.MOMENTUM, rm if run else None, rv if run else None)
        for name in ("scale", "shift", "mean", "rstd") + (("rmean", "rvar") if run else ()):
            inside(getattr(got, name), getattr(ref, name), getattr(ref, "b_" + name), "c", f"f32 bn_finalize nblk={nblk} C={C} {name}")


def test_clamp_case_is_negative_in_double_either_way():
    part, count, v, plain, fused = R.clamp_part()
    assert plain < 0 and fused < 0
    ref = R.finalize_ref(part, count, None, None, R.EPS, R.MOMENTUM, None, None)
    assert float(ref.raw_var[0]) < 0 and float(ref.var[0]) == 0.0
    assert abs(float(ref.rstd[0]) - 1 / math.sqrt(R.EPS)) <= 1e-12 / math.sqrt(R.EPS)
    # without the clamp rstd moves by -var / (2 eps): far outside one f32 rounding
    assert -plain / (2 * R.EPS) > 1000 * R.U32


def axis_tabs(dims, out, jitter):
    crop = R.crop_of(dims, jitter)
    return [_axis_np(n, lo, nc, od) for n, (lo, nc), od in zip(dims, crop, out)]


def sample_cases():
    m = R.SAMPLE_MAIN
    return [(m["B"], 8, m["dims"], m["out"], m["jitter"])] + [(2, 8, d, o, j) for d, o, j in R.SAMPLE_EDGES] + \
        [(1, 8, d, o, j) for d, o, j in R.sample_extremes()]


@pytest.mark.parametrize("case", sample_cases(), ids=lambda c: f"B{c[0]}_{c[2][0]}x{c[2][1]}x{c[2][2]}_to_{c[3][0]}x{c[3][1]}x{c[3][2]}_j{c[4]}")
def test_f32_sampling_stays_inside_its_bounds(case):
    B, C, dims, out, jitter = case
    vol, vol_fed = R.sample_volume(B, C, dims, seed=sum(dims), jitter=jitter, nan_outside=True)
    tabs = axis_tabs(dims, out, jitter)
    ref, bound = R.sample_fwd_ref(vol, out, jitter)
    f1 = inside(R.emul_sample_fwd(vol_fed, [t[:3] for t in tabs], out), ref, bound, "bnc", f"f32 sample fwd {case}")
    gout = torch.randn(ref.shape, generator=R.gen(7), dtype=F32).to(F64)
    g, gb, touched = R.sample_bwd_ref(vol.shape, out, jitter, gout)
    got = R.emul_sample_bwd(gout, [(t[3], t[4], t[5], t[6]) for t in tabs], dims, out)
    f2 = inside(got, g, R.with_bf16(g, gb), "bhwdc", f"f32 sample bwd {case}")
    assert not bool(got[~touched].any())
    print(f"[host] sample {case[2]}->{case[3]} j={jitter}: fwd {f1:.3f}, bwd {f2:.3f} of the bounds")


# ---------------------------------------------------------------------------------------------- 2. injected bugs
def test_injected_bugs_leave_the_bounds_and_not_the_old_bars(capsys):
    rows = []
    n, C = R.SMALL_N, 48
    o = R.bn_operands(n, C, seed=n + C)
    planted = R.plant_symmetric_zero_channel(o)
    st, sc, sh, mu, rs = fed(o)
    assert not bool(R.gate_undecided(o.x, sc, sh).any())
    grid = R.apply_grid(n, C)
    y, e32 = R.affine_ref(o.x, sc, sh, True)
    by = R.with_bf16(y, e32)
    c = R.bn_backward_closed(o.x, o.dy, o.w, o.b, True)
    sums = R.r32(torch.cat([c.S1, c.S2]))
    bdx = R.with_bf16(c.dx, R.bwd_dx_bound(c, o.x))
    assert violations(R.emul_affine(o.x, sc, sh, True, grid), y, by) == 0
    assert violations(R.emul_bwd_apply(o.x, o.dy, sc, sh, mu, rs, sums, True, grid), c.dx, bdx) == 0

    def row(name, got, ref, bound, bar, expect=None):
        v = violations(got, ref, bound)
        l2 = R.rel_l2(torch.nan_to_num(got.to(F64)), ref)
        rows.append((name, l2, bar, v, got.numel()))
        assert v > 0, name
        if expect is not None:
            assert v == expect, (name, v, expect)
        return l2

    l2 = row("neighbour group's constants, one block, affine_act C=48", R.emul_affine(o.x, sc, sh, True, grid, "neighbour_group"), y, by,
             OLD_BARS["bn_fwd"])
    row("neighbour group's constants, one block, bn_bwd_apply C=48",
        R.emul_bwd_apply(o.x, o.dy, sc, sh, mu, rs, sums, True, grid, "neighbour_group"), c.dx, bdx, OLD_BARS["bn_dx"])
    row("unwritten tail of items % 256, affine_act", R.emul_affine(o.x, sc, sh, True, grid, "tail"), y, by, OLD_BARS["bn_fwd"],
        expect=(n * 6 % 256) * 8)
    row("gate < instead of <= on planted zeros, bn_bwd_apply", R.emul_bwd_apply(o.x, o.dy, sc, sh, mu, rs, sums, True, grid, "strict_gate"),
              c.dx, bdx, OLD_BARS["bn_dx"], expect=len(planted))
    row("1/n from the per-batch voxel count, bn_bwd_apply", R.emul_bwd_apply(o.x, o.dy, sc, sh, mu, rs, sums, True, grid, "per_batch_n", n // 2),
        c.dx, bdx, OLD_BARS["bn_dx"])
    part = R.emul_bn_stats(o.x, R.stats_nblk(n, C)).to(F64)
    ref = R.finalize_ref(part, float(n), o.w, o.b, R.EPS, R.MOMENTUM, None, None)
    bad = R.emul_finalize(part, float(n), o.w, o.b, R.EPS, R.MOMENTUM, None, None, "unbiased_scale")
    l2u = row("unbiased variance in scale, bn_finalize (n = 210)", bad.scale, ref.scale, ref.b_scale, OLD_BARS["bn_fwd"], expect=C)
    assert l2u < OLD_BARS["bn_fwd"]                                         # 1 / (2 n) = 2.4e-3 of scale
    # sampling
    dims, out, jitter = R.SAMPLE_EDGES[1]
    vol, vol_fed = R.sample_volume(2, 8, dims, seed=5, jitter=jitter, nan_outside=True)
    tabs = [list(t[:3]) for t in axis_tabs(dims, out, jitter)]
    sref, sb = R.sample_fwd_ref(vol, out, jitter)
    assert violations(R.emul_sample_fwd(vol_fed, tabs, out), sref, sb) == 0
    loose = [(lo, np.minimum(lo + 1, n - 1).astype(np.int32), w) for (lo, hi, w), n in zip(tabs, dims)]      # clamped at the volume only
    row("hi not clamped at the crop's end (NaN outside the crop)", R.emul_sample_fwd(vol_fed, loose, out), sref, sb, OLD_BARS["sample_fwd"])
    m = R.SAMPLE_MAIN
    vol = R.sample_volume(m["B"], 8, m["dims"], seed=6)
    tabs = [t[:3] for t in axis_tabs(m["dims"], m["out"], m["jitter"])]
    sref, sb = R.sample_fwd_ref(vol, m["out"], m["jitter"])
    row("batch stride H W D instead of C H W D (B = 2)", R.emul_sample_fwd(vol, tabs, m["out"], "batch_stride"), sref, sb,
        OLD_BARS["sample_fwd"], expect=sref[1:].numel())
    one = R.emul_sample_fwd(vol[:1], tabs, m["out"], "batch_stride")
    assert violations(one, sref[:1], sb[:1]) == 0                           # invisible at B = 1
    with capsys.disabled():
        print("\n[injected] bug | rel-L2 | old bar | located violations / elements")
        for name, l2, bar, v, total in rows:
            print(f"[injected] {name} | {l2:.2e} | {bar:.0e} ({'passes' if l2 < bar else 'fails'}) | {v} / {total}")
    assert l2 < 1.0


# ---------------------------------------------------------------------------------------------- 3. the tables, whole domain
@pytest.mark.parametrize("rf", (2, 4, 8, 16))
def test_axis_tables_over_the_whole_domain(rf):
    g = R.gen(rf)
    top, seen = int(math.ceil(rf)), 0
    for n in range(1, 41):
        n_out = max(int(n // rf), 1)
        axis = torch.randn(n, generator=g, dtype=F64)
        for j0 in range(top):
            for j1 in range(top):
                nc = n - j0 - j1
                if nc < 1:
                    continue
                lo, hi, w, i1, w1, i2, w2 = _axis_np(n, j0, nc, n_out)     # must not raise "more than two samples touch a voxel"
                what = f"n={n} rf={rf} jitter=({j0}, {j1}) n_out={n_out}"
                assert lo.min() >= j0 and hi.max() <= j0 + nc - 1 and bool(((hi == lo) | (hi == lo + 1)).all()), what
                assert w.dtype == np.float32 and bool(((w >= 0) & (w < 1)).all()), what
                vol = axis.view(1, 1, n, 1, 1)
                ref = R.grid_sample_ref(vol, (n_out, 1, 1), (j0, j1, 0, 0, 0, 0)).reshape(n_out)
                a = axis.numpy()
                w64 = w.astype(np.float64)
                got = torch.from_numpy((1.0 - w64) * a[lo] + w64 * a[hi])
                tol = torch.from_numpy(2.0 ** -25 * np.abs(a[hi] - a[lo]) + 1e-14 * (np.abs(a[lo]) + np.abs(a[hi])))
                R.assert_within_located(got, ref, tol, "i", "forward taps against grid_sample (reflection padding), " + what)
                # the positions never leave [0, n_crop - 1]: the clamp and the reflection are both the identity there
                pos = R.axis_positions(nc, n_out)
                assert float(pos.min()) >= 0.0 and float(pos.max()) <= nc - 1.0, what
                # the backward tables are the exact transpose of the forward ones
                fwd = np.zeros((n_out, n), np.float32)
                for i in range(n_out):
                    fwd[i, lo[i]] += np.float32(1.0) - w[i]
                    fwd[i, hi[i]] += w[i]
                bwd = np.zeros((n, n_out), np.float32)
                for c in range(n):
                    assert i1[c] >= 0 or (w1[c] == 0 and i2[c] < 0), what
                    assert i2[c] != i1[c] or i2[c] < 0, what
                    if i1[c] >= 0:
                        bwd[c, i1[c]] = w1[c]
                    if i2[c] >= 0:
                        bwd[c, i2[c]] = w2[c]
                assert np.array_equal(bwd, fwd.T), "backward tables are not the transpose of the forward ones, " + what
                seen += 1
    assert seen > 40
