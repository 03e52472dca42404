"""Direct located parity tests of the BatchNorm pieces (mivp_bn_stats, mivp_bn_finalize, mivp_affine_act, mivp_bn_bwd_stats,
mivp_bn_bwd_apply) and of the point sampling (mivp_sample_points_fwd / _bwd) against tests/norm_sample_ref.py (float64, CPU).

Every entry is called through ``_lib.call`` on its own operands; outputs are NaN-prefilled buffers with a guard tail; each case
asserts its input conditions on the reference before it looks at the kernel; every bound is derived in the header of
tests/norm_sample_ref.py and shown honest on the CPU by tests/test_norm_sample_host.py.  ``[margin]`` lines print the largest used
fraction of each bound (DESIGN 5.14 quotes them)."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_sample_ref as R  # noqa: E402
from test_hip_prompt_path import DEV, Out, assert_same_bits, bits, dev  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import losses, ops

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EINVAL = r"failed with code -1"


def margin(entry, case, frac):
    print(f"[margin] {entry} {case}: {frac:.3f} of the bound")


def inside(got, ref, bound, layout, entry, case):
    R.assert_within_located(got, ref, bound, layout, f"{entry} {case}")
    margin(entry, case, R.used(got, ref, bound))


def fed(o):
    """The f32 scale / shift / mean_rstd the reference itself rounds, on the device, and the float64 statistics."""
    st = R.bn_forward(o.x, o.w, o.b)
    assert not bool(R.gate_undecided(o.x, st.scale32, st.shift32).any()), "an element's LeakyReLU gate is undecided in f32"
    return st, dev(st.scale32), dev(st.shift32), dev(torch.cat([st.mean32, st.rstd32]))


# =============================================================================================
# mivp_bn_stats, mivp_bn_bwd_stats
# =============================================================================================
STATS = R.BN_SMALL + R.BN_STATS_CAP


@pytest.mark.parametrize("case", STATS, ids=[f"{R.bn_id(c)}-{R.path(c[0], c[1], R.stats_nblk(*c), 1024)}" for c in STATS])
def test_statistics_kernels(case):
    n, Cc = case
    G, nblk = Cc // 8, R.stats_nblk(n, Cc)
    assert nblk == ops._nblk(n * G, G) and (nblk * 256) % G == 0
    k = R.chain_len(n * G, nblk, G)
    o = R.bn_operands(n, Cc, seed=n + Cc)
    R.plant_symmetric_zero_channel(o)
    st, sc, sh, mr = fed(o)
    x, dy = dev(o.x, BF16), dev(o.dy, BF16)
    what = f"{R.bn_id(case)} nblk={nblk} k={k}"
    live = R.live_blocks(n * G)

    def run(entry, launch):
        outs = []
        for _ in range(2):
            part = Out((nblk, 2 * Cc))
            launch(part.t)
            torch.cuda.synchronize()
            outs.append(part.done(f"{entry} {what}"))
        assert_same_bits(outs[0], outs[1], f"{entry} {what}: a repeated call")
        dead = outs[0][live:]
        assert not bool(bits(dead).any()), f"{entry} {what}: rows of blocks beyond the live items must be +0"
        return outs[0].to(F64).sum(0)

    ref, mag = R.bn_sums(o.x)
    got = run("bn_stats", lambda part: L.call("mivp_bn_stats", L.ptr(x), n, Cc, nblk, L.ptr(part), L.stream()))
    inside(got, ref, R.SLACK * k * R.U32 * mag, "c", "bn_stats", what)
    for lrelu in (1, 0):
        dxa, dg, db = R.bn_backward_autograd(o.x, o.dy, o.w, o.b, bool(lrelu))
        c = R.bn_backward_closed(o.x, o.dy, o.w, o.b, bool(lrelu))
        if lrelu:
            zero = c.z[:, 0] == 0
            assert int(zero.sum()) >= 4 and bool((c.gz[zero, 0] == R.SLOPE * o.dy[zero, 0]).all())
        got = run("bn_bwd_stats", lambda part: L.call("mivp_bn_bwd_stats", L.ptr(x), L.ptr(dy), n, Cc, L.ptr(sc), L.ptr(sh), L.ptr(mr),
                                                      lrelu, nblk, L.ptr(part), L.stream()))
        inside(got, torch.cat([db, dg]), R.bwd_sums_bounds(c, k), "c", f"bn_bwd_stats lrelu={lrelu}", what)


# =============================================================================================
# mivp_affine_act, mivp_bn_bwd_apply
# =============================================================================================
APPLY = R.BN_SMALL + R.BN_APPLY_CAP


@pytest.mark.parametrize("case", APPLY, ids=[f"{R.bn_id(c)}-{R.path(c[0], c[1], R.apply_grid(*c), 4096)}" for c in APPLY])
def test_affine_act(case):
    n, Cc = case
    o = R.bn_operands(n, Cc, seed=n + Cc)
    st = R.bn_forward(o.x, o.w, o.b)
    scale, shift = st.scale32.clone(), st.shift32.clone()
    planted = R.plant_zeros(o.x, scale, shift, rows=(0, 3, n - 1))
    x, sc, sh = dev(o.x, BF16), dev(scale), dev(shift)
    for lrelu in (1, 0):
        ref, e32 = R.affine_ref(o.x, scale, shift, bool(lrelu))
        z = o.x * scale + shift
        assert not bool(((z != 0) & (z.abs() <= e32)).any()), "an element has 0 < |z64| <= e32"
        assert all(float(z[p]) == 0.0 for p in planted)
        y = Out((n, Cc), BF16)
        L.call("mivp_affine_act", L.ptr(x), n, Cc, L.ptr(sc), L.ptr(sh), lrelu, L.ptr(y.t), L.stream())
        torch.cuda.synchronize()
        got = y.done(f"affine_act {R.bn_id(case)}")
        inside(got, ref, R.with_bf16(ref, e32), "nc", f"affine_act lrelu={lrelu}", R.bn_id(case))
        for p in planted:
            assert float(got[p]) == 0.0, f"affine_act {R.bn_id(case)} lrelu={lrelu}: planted zero at {p} came back {float(got[p])!r}"


@pytest.mark.parametrize("case", APPLY, ids=[f"{R.bn_id(c)}-{R.path(c[0], c[1], R.apply_grid(*c), 4096)}" for c in APPLY])
def test_bn_bwd_apply(case):
    n, Cc = case
    o = R.bn_operands(n, Cc, seed=n + Cc)
    rows = R.plant_symmetric_zero_channel(o)
    st, sc, sh, mr = fed(o)
    x, dy = dev(o.x, BF16), dev(o.dy, BF16)
    for lrelu in (1, 0):
        dxa, dg, db = R.bn_backward_autograd(o.x, o.dy, o.w, o.b, bool(lrelu))
        c = R.bn_backward_closed(o.x, o.dy, o.w, o.b, bool(lrelu))
        ce = R.bn_backward_closed(o.x, o.dy, o.w, o.b, bool(lrelu), train=False)
        assert all(float(c.z[r, 0]) == 0.0 for r in rows)
        if lrelu:                                                           # torch's rule: the 0.01 slope at z == 0 (eval form: dx alone)
            assert all(float(ce.dx[r, 0]) == float(st.scale[0] * (R.SLOPE * o.dy[r, 0])) for r in rows)
        sums = dev(torch.cat([db, dg]))
        zeros = torch.zeros(2 * Cc, dtype=F32, device=DEV)
        for form, s, ref, cc, train in (("train", sums, dxa, c, True), ("eval", zeros, ce.dx, ce, False)):
            outs = []
            for _ in range(2):
                dx = Out((n, Cc), BF16)
                L.call("mivp_bn_bwd_apply", L.ptr(x), L.ptr(dy), n, Cc, L.ptr(sc), L.ptr(sh), L.ptr(mr), L.ptr(s), lrelu, L.ptr(dx.t),
                       L.stream())
                torch.cuda.synchronize()
                outs.append(dx.done(f"bn_bwd_apply {form} {R.bn_id(case)}"))
            assert_same_bits(outs[0], outs[1], f"bn_bwd_apply {form} {R.bn_id(case)}: a repeated call")
            inside(outs[0], ref, R.with_bf16(ref, R.bwd_dx_bound(cc, o.x, train)), "nc", f"bn_bwd_apply {form} lrelu={lrelu}", R.bn_id(case))


# =============================================================================================
# mivp_bn_finalize
# =============================================================================================
class InOut(Out):
    """A guarded buffer the kernel updates in place."""

    def __init__(self, values):
        super().__init__(tuple(values.shape))
        self.t.copy_(values.to(F32))


def finalize(part, count, w, b, rm, rv, with_mr, Cc, what):
    nblk = part.shape[0]
    scale, shift = Out((Cc,)), Out((Cc,))
    mr = Out((2 * Cc,))
    rmo, rvo = (InOut(rm), InOut(rv)) if rm is not None else (None, None)
    part_d = dev(part)
    w_d, b_d = (None if w is None else dev(w)), (None if b is None else dev(b))
    L.call("mivp_bn_finalize", L.ptr(part_d), nblk, Cc, float(count), L.ptr(w_d), L.ptr(b_d), R.EPS, R.MOMENTUM,
           None if rmo is None else L.ptr(rmo.t), None if rvo is None else L.ptr(rvo.t), L.ptr(scale.t), L.ptr(shift.t),
           L.ptr(mr.t) if with_mr else None, L.stream())
    torch.cuda.synchronize()
    got = dict(scale=scale.done(what), shift=shift.done(what))
    if with_mr:
        m = mr.done(what)
        got["mean"], got["rstd"] = m[:Cc], m[Cc:]
    else:
        assert bool(torch.isnan(mr.flat).all()), what + ": mean_rstd is NULL, its neighbour buffer was written"
    if rmo is not None:
        got["rmean"], got["rvar"] = rmo.done(what), rvo.done(what)
    return got


@pytest.mark.parametrize("Cc", R.FINALIZE_C)
@pytest.mark.parametrize("nblk", R.FINALIZE_NBLK)
def test_bn_finalize(nblk, Cc):
    part, count = R.finalize_part(nblk, Cc, seed=nblk * 100 + Cc)
    g = R.gen(nblk + Cc)
    w, b = (1 + 0.3 * torch.randn(Cc, generator=g)).to(F64), (0.3 * torch.randn(Cc, generator=g)).to(F64)
    rm, rv = torch.randn(Cc, generator=g).to(F64), (0.5 + torch.rand(Cc, generator=g)).to(F64)
    forms = (("all", w, b, True, True), ("w_null", None, b, True, True), ("b_null", w, None, True, True),
             ("mean_rstd_null", w, b, True, False), ("running_null", w, b, False, True))
    worst = 0.0
    for form, wv, bv, run, with_mr in forms:
        what = f"bn_finalize nblk={nblk} C={Cc} {form}"
        ref = R.finalize_ref(part, count, wv, bv, R.EPS, R.MOMENTUM, rm if run else None, rv if run else None)
        got = finalize(part, count, wv, bv, rm if run else None, rv if run else None, with_mr, Cc, what)
        for name, val in got.items():
            R.assert_within_located(val, getattr(ref, name), getattr(ref, "b_" + name), "c", f"{what} {name}")
            worst = max(worst, R.used(val, getattr(ref, name), getattr(ref, "b_" + name)))
    margin("bn_finalize", f"nblk={nblk} C={Cc}", worst)


def test_bn_finalize_count_one_and_clamp():
    x = torch.tensor([[0.75, -1.5, 2.0, 0.0, 3.0, -0.125, 1.0, 100.0]], dtype=F64)
    part = torch.cat([x, x * x], 1)
    rm, rv = torch.zeros(8, dtype=F64), torch.ones(8, dtype=F64)
    ref = R.finalize_ref(part, 1.0, None, None, R.EPS, R.MOMENTUM, rm, rv)
    assert bool((ref.var == 0).all())                                        # one voxel: the unbiased variance is the biased one, 0
    got = finalize(part, 1.0, None, None, rm, rv, True, 8, "bn_finalize count=1")
    for name, val in got.items():
        R.assert_within_located(val, getattr(ref, name), getattr(ref, "b_" + name), "c", f"bn_finalize count=1 {name}")
    assert bool(torch.isfinite(got["rvar"]).all())
    part, count, v, plain, fused = R.clamp_part()
    assert plain < 0 and fused < 0                                           # negative in double, contracted or not
    ref = R.finalize_ref(part, count, None, None, R.EPS, R.MOMENTUM, None, None)
    got = finalize(part, count, None, None, None, None, True, 1, "bn_finalize clamp")
    want = torch.tensor([1.0 / math.sqrt(R.EPS)], dtype=F64)
    R.assert_within_located(got["rstd"], want, R.U32 * want, "c", "bn_finalize clamp: rstd must be 1 / sqrt(eps)")
    R.assert_within_located(got["scale"], want, R.U32 * want, "c", "bn_finalize clamp: scale (w NULL)")
    R.assert_within_located(got["shift"], ref.shift, ref.b_shift, "c", "bn_finalize clamp: shift")


# =============================================================================================
# the ops wrappers against the entries called one by one
# =============================================================================================
def test_wrappers_are_the_entries():
    n, Cc = R.SMALL_N, 48
    o = R.bn_operands(n, Cc, seed=n + Cc)
    R.plant_symmetric_zero_channel(o)
    st, sc, sh, mr = fed(o)
    x5, dy5 = dev(o.x, BF16).view(2, *R.SMALL_DIMS, Cc), dev(o.dy, BF16).view(2, *R.SMALL_DIMS, Cc)
    w, b = dev(o.w), dev(o.b)
    rm, rv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
    s_w, h_w, m_w = ops.bn_batch_stats(x5, w, b, R.EPS, rm, rv, R.MOMENTUM)
    nblk = R.stats_nblk(n, Cc)
    part = Out((nblk, 2 * Cc))
    L.call("mivp_bn_stats", L.ptr(x5), n, Cc, nblk, L.ptr(part.t), L.stream())
    rm2, rv2 = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
    s_e, h_e, m_e = torch.empty_like(s_w), torch.empty_like(h_w), torch.empty_like(m_w)
    L.call("mivp_bn_finalize", L.ptr(part.t), nblk, Cc, float(n), L.ptr(w), L.ptr(b), R.EPS, R.MOMENTUM, L.ptr(rm2), L.ptr(rv2),
           L.ptr(s_e), L.ptr(h_e), L.ptr(m_e), L.stream())
    torch.cuda.synchronize()
    for name, a, bb in (("scale", s_w, s_e), ("shift", h_w, h_e), ("mean_rstd", m_w, m_e), ("running_mean", rm, rm2), ("running_var", rv, rv2)):
        assert_same_bits(a, bb, f"ops.bn_batch_stats {name}")
    # the chained statistics against the float64 reference: scale / shift carry bn_stats' error on top of bn_finalize's roundings
    ref = R.finalize_ref(part.done("bn_stats").to(F64), float(n), o.w, o.b, R.EPS, R.MOMENTUM, None, None)
    inside(s_w, ref.scale, ref.b_scale, "c", "ops.bn_batch_stats scale (from its own part)", "C=48")
    for lrelu in (True, False):
        y = Out((2, *R.SMALL_DIMS, Cc), BF16)
        L.call("mivp_affine_act", L.ptr(x5), n, Cc, L.ptr(sc), L.ptr(sh), 1 if lrelu else 0, L.ptr(y.t), L.stream())
        assert_same_bits(ops.affine_act(x5, sc, sh, lrelu), y.t, f"ops.affine_act lrelu={lrelu}")
        dx_t, dg_t, db_t = ops.bn_backward(x5, dy5, sc, sh, mr, lrelu)
        dx_e, dg_e, db_e = ops.bn_backward_eval(x5, dy5, sc, sh, mr, lrelu)
        assert_same_bits(dg_t.contiguous(), dg_e.contiguous(), "dgamma of the training and the eval form")
        assert_same_bits(db_t.contiguous(), db_e.contiguous(), "dbeta of the training and the eval form")
        sums = torch.cat([db_t, dg_t]).contiguous()
        for form, s, want in (("train", sums, dx_t), ("eval", torch.zeros_like(sums), dx_e)):
            dx = Out((2, *R.SMALL_DIMS, Cc), BF16)
            L.call("mivp_bn_bwd_apply", L.ptr(x5), L.ptr(dy5), n, Cc, L.ptr(sc), L.ptr(sh), L.ptr(mr), L.ptr(s), 1 if lrelu else 0,
                   L.ptr(dx.t), L.stream())
            torch.cuda.synchronize()
            assert_same_bits(want, dx.t, f"ops.bn_backward{'_eval' if form == 'eval' else ''} lrelu={lrelu}")
        # and the whole wrapper against autograd: the sums now carry bn_bwd_stats' own error, one more rounding budget each
        dxa, dg, db = R.bn_backward_autograd(o.x, o.dy, o.w, o.b, lrelu)
        c = R.bn_backward_closed(o.x, o.dy, o.w, o.b, lrelu)
        k = R.chain_len(n * 6, nblk, 6) + nblk                                  # reduce_rows adds the nblk rows in f32
        inside(torch.cat([db_t, dg_t]), torch.cat([db, dg]), R.bwd_sums_bounds(c, k), "c", f"ops.bn_backward sums lrelu={lrelu}", "C=48")


# =============================================================================================
# point sampling
# =============================================================================================
def tables(dims, out, jitter):
    """The package's host tables of the three axes on the device: [(lo, hi, w, i1, w1, i2, w2)] * 3."""
    crop = R.crop_of(dims, jitter)
    return [tuple(torch.from_numpy(a).to(DEV) for a in losses._axis_np(n, lo, nc, od)) for n, (lo, nc), od in zip(dims, crop, out)]


def sample_fwd(src, is_bf16, clast, B, dims, Cc, out, tabs, what):
    od = (C.c_int32 * 3)(*out)
    res = Out((B, out[0] * out[1] * out[2], Cc))
    L.call("mivp_sample_points_fwd", L.ptr(src), is_bf16, clast, B, dims[0], dims[1], dims[2], Cc, od,
           losses._ptr3([t[0] for t in tabs], C.c_int32), losses._ptr3([t[1] for t in tabs], C.c_int32),
           losses._ptr3([t[2] for t in tabs], C.c_float), L.ptr(res.t), L.stream())
    torch.cuda.synchronize()
    return res.done(what)


def sample_bwd(gout_d, B, dims, Cc, out, tabs, what):
    od = (C.c_int32 * 3)(*out)
    g = Out((B, *dims, Cc), BF16)
    L.call("mivp_sample_points_bwd", L.ptr(gout_d), B, dims[0], dims[1], dims[2], Cc, od,
           losses._ptr3([t[3] for t in tabs], C.c_int32), losses._ptr3([t[5] for t in tabs], C.c_int32),
           losses._ptr3([t[4] for t in tabs], C.c_float), losses._ptr3([t[6] for t in tabs], C.c_float), L.ptr(g.t), L.stream())
    torch.cuda.synchronize()
    return g.done(what)


def layout(fed_vol, dtype, clast):
    """The device buffer of one instantiation from the channels-first float64 volume."""
    t = fed_vol.permute(0, 2, 3, 4, 1) if clast else fed_vol
    return dev(t.contiguous(), dtype)


def check_sampling(B, Cc, dims, out, jitter, combos, seed, backward=True):
    vol, fed_vol = R.sample_volume(B, Cc, dims, seed, jitter, nan_outside=True)           # NaN outside the crop: never read
    tabs = tables(dims, out, jitter)
    ref, bound = R.sample_fwd_ref(vol, out, jitter)
    case = f"B{B}_C{Cc}_{dims}->{out}_j{jitter}"
    for dtype, clast in combos:
        name = f"sample_fwd<{'bf16' if dtype == BF16 else 'f32'},{'clast' if clast else 'cfirst'}>"
        got = sample_fwd(layout(fed_vol, dtype, clast), 1 if dtype == BF16 else 0, clast, B, dims, Cc, out, tabs, f"{name} {case}")
        inside(got, ref, bound, "bnc", name, case)
    if backward and Cc % 8 == 0:
        gout = torch.randn(ref.shape, generator=R.gen(seed + 1), dtype=F32).to(F64)
        g, gb, touched = R.sample_bwd_ref(vol.shape, out, jitter, gout)
        (a0, n0), (a1, n1), (a2, n2) = R.crop_of(dims, jitter)
        outside = torch.ones(touched.shape, dtype=torch.bool)
        outside[:, a0:a0 + n0, a1:a1 + n1, a2:a2 + n2] = False
        assert not bool((touched & outside).any()) and bool((g[~touched] == 0).all())
        got = sample_bwd(dev(gout), B, dims, Cc, out, tabs, f"sample_bwd {case}")
        inside(got, g, R.with_bf16(g, gb), "bhwdc", "sample_bwd", case)
        assert not bool(bits(got)[~touched].any()), f"sample_bwd {case}: a voxel no sample touches must be +0"


ALL4 = [(BF16, 1), (BF16, 0), (F32, 1), (F32, 0)]


@pytest.mark.parametrize("Cc", (3, 8, 48))
def test_sampling_all_instantiations(Cc):
    m = R.SAMPLE_MAIN
    check_sampling(m["B"], Cc, m["dims"], m["out"], m["jitter"], ALL4, seed=Cc)


@pytest.mark.parametrize("dims,out,jitter", R.SAMPLE_EDGES + R.sample_extremes(),
                         ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else "j0")
def test_sampling_edges_and_extremes(dims, out, jitter):
    crop = R.crop_of(dims, jitter)
    if dims == (16, 9, 8):
        assert [c[1] for c in crop] == [2, 1, 1]                            # crop == out, one-voxel crops on two axes
        t = losses._axis_np(16, 7, 2, 2)
        assert list(t[2]) == [0.0, 0.0] and list(t[0]) == [7, 8]            # upper taps with weight exactly 0
    check_sampling(2, 8, dims, out, jitter, [(BF16, 1), (F32, 0)], seed=sum(dims) + sum(out))


def test_sampling_wrapper_layouts_and_jitter_slot():
    m = R.SAMPLE_MAIN
    B, Cc, dims, out = m["B"], 8, m["dims"], m["out"]
    j1, j2 = m["jitter"], (0, 3, 2, 1, 1, 0)
    vol = R.sample_volume(B, Cc, dims, seed=11)
    gout = torch.randn((B, out[0] * out[1] * out[2], Cc), generator=R.gen(12), dtype=F32)
    slot = losses.JitterSlot()
    slot.load(dims, out, j1, torch.device(DEV))
    ptrs = [b.data_ptr() for b in slot.bufs]
    for step, jit in enumerate((j1, j2)):
        if step:
            slot.reload(jit)
            assert ptrs == [b.data_ptr() for b in slot.bufs], "JitterSlot.reload reallocated its tables"
        ref, bound = R.sample_fwd_ref(vol, out, jit)
        g, gb, _ = R.sample_bwd_ref(vol.shape, out, jit, gout.to(F64))
        base = dev(vol.permute(0, 2, 3, 4, 1).contiguous(), BF16)           # the model's layout: channels-last bf16 storage
        res = {}
        for how in ("cached", "slot"):
            leaf = base.clone().requires_grad_(True)
            y = losses.sample_points(leaf.permute(0, 4, 1, 2, 3), out, jit if how == "cached" else None, slot if how == "slot" else None)
            y.backward(dev(gout))
            torch.cuda.synchronize()
            res[how] = (y.detach(), leaf.grad)
        assert_same_bits(res["cached"][0], res["slot"][0], f"sample_points through a JitterSlot, jitter {jit}")
        assert_same_bits(res["cached"][1], res["slot"][1], f"sample_points gradient through a JitterSlot, jitter {jit}")
        inside(res["slot"][0], ref, bound, "bnc", "sample_points(slot) fwd", f"jitter {jit}")
        inside(res["slot"][1], g, R.with_bf16(g, gb), "bhwdc", "sample_points(slot) bwd", f"jitter {jit}")
    # the f32 channels-first path the coordinate grids take, through the wrapper, with its f32 gradient view
    leaf = dev(vol).requires_grad_(True)
    y = losses.sample_points(leaf, out, j1)
    y.backward(dev(gout))
    torch.cuda.synchronize()
    ref, bound = R.sample_fwd_ref(vol, out, j1)
    g, gb, _ = R.sample_bwd_ref(vol.shape, out, j1, gout.to(F64))
    inside(y.detach(), ref, bound, "bnc", "sample_points f32 channels-first fwd", f"jitter {j1}")
    assert leaf.grad.dtype == F32 and leaf.grad.shape == leaf.shape
    inside(leaf.grad.permute(0, 2, 3, 4, 1), g, R.with_bf16(g, gb), "bhwdc", "sample_points f32 channels-first bwd", f"jitter {j1}")


def test_sampling_backward_refuses_other_channel_counts():
    m = R.SAMPLE_MAIN
    B, Cc, dims, out = 1, 3, m["dims"], m["out"]
    leaf = dev(R.sample_volume(B, Cc, dims, seed=3)).requires_grad_(True)
    y = losses.sample_points(leaf, out, m["jitter"])
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        y.backward(torch.ones_like(y))
    tabs = tables(dims, out, m["jitter"])
    gout = torch.ones((B, out[0] * out[1] * out[2], Cc), device=DEV)
    od = (C.c_int32 * 3)(*out)
    g = Out((B, *dims, 8), BF16)
    with pytest.raises(RuntimeError, match=EINVAL):
        L.call("mivp_sample_points_bwd", L.ptr(gout), B, dims[0], dims[1], dims[2], Cc, od,
               losses._ptr3([t[3] for t in tabs], C.c_int32), losses._ptr3([t[5] for t in tabs], C.c_int32),
               losses._ptr3([t[4] for t in tabs], C.c_float), losses._ptr3([t[6] for t in tabs], C.c_float), L.ptr(g.t), L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(g.flat).all()), "a refused call wrote to its output"


@pytest.mark.parametrize("dtype,clast", [(BF16, 1), (F32, 0)], ids=["bf16_clast", "f32_cfirst"])
def test_sampling_forward_grid_cap_with_identity_tables(dtype, clast):
    """Identity tables (lo = hi = i, w = 0) make the forward a copy: out[b, voxel, c] = vol[b, c, voxel], exactly."""
    B, Cc, dims = 2, 8, (128, 128, 65)
    N = dims[0] * dims[1] * dims[2]
    assert 65536 * 256 < B * N * Cc < 65536 * 256 * 2                        # the grid cap and a partial second trip
    g = torch.Generator(device=DEV).manual_seed(5)
    shape = (B, *dims, Cc) if clast else (B, Cc, *dims)
    src = torch.randn(shape, generator=g, device=DEV, dtype=F32).to(dtype)
    tabs = []
    for n in dims:
        i = torch.arange(n, dtype=torch.int32, device=DEV)
        tabs.append((i, i.clone(), torch.zeros(n, dtype=F32, device=DEV)))
    od = (C.c_int32 * 3)(*dims)
    res = torch.full((B * N * Cc + 64,), float("nan"), dtype=F32, device=DEV)
    L.call("mivp_sample_points_fwd", L.ptr(src), 1 if dtype == BF16 else 0, clast, B, dims[0], dims[1], dims[2], Cc, od,
           losses._ptr3([t[0] for t in tabs], C.c_int32), losses._ptr3([t[1] for t in tabs], C.c_int32),
           losses._ptr3([t[2] for t in tabs], C.c_float), L.ptr(res), L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(res[B * N * Cc:]).all()), "the kernel wrote behind its output buffer"
    want = (src if clast else src.permute(0, 2, 3, 4, 1)).reshape(B, N, Cc).float()
    assert torch.equal(res[:B * N * Cc].view(B, N, Cc), want)
