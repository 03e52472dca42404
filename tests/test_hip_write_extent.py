"""Write extent of the model's output kernels (DESIGN.md "Write extent"): every wrapper of mivp_amd.ops and the Swin block of
mivp_amd.swin_ops run under tests/guarded.py -- each output, partial-sum buffer and workspace the wrappers allocate sits between
two canary bands, every case runs twice (canary 0xA5, then 0x5A) -- and must

  (a) leave every band intact (no store outside an allocation, in front of it or behind it),
  (b) store every element of every tensor it returns (the two-pattern rule), apart from the exception masks written next to
      the case, each computed from the descriptor with one line saying why,
  (c) leave its inputs untouched (BatchNorm running statistics and gemm_tn's accumulator are outputs by contract),

and return the same bits in both runs.  The values are held to the float64 / exact reference that already exists for the
wrapper, by that file's own assertion: where an existing parity test calls the wrapper, its body IS the case (run through
``guarded.twice_calls``, which spies on the wrappers it calls); the few wrappers without one get a body here.  A kernel that
is wrong only when its output sits inside a guarded buffer is therefore caught too."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_ref as E  # noqa: E402
import guarded as G  # noqa: E402
import norm_sample_ref as NR  # noqa: E402
import uphead_ref as UR  # noqa: E402
import test_hip_exact as X  # noqa: E402
import test_hip_swin_bwd as SB  # noqa: E402
import test_hip_uphead as U  # noqa: E402
from conftest import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def mods():
    import mivp_amd  # noqa: F401
    from mivp_amd import ops, swin_ops
    return ops, swin_ops


def extent(body, what, allow=None):
    """Run ``body`` (which calls wrappers and asserts their values itself) under the guard, twice."""
    calls, g = G.twice_calls(body, *mods(), allow=allow, what=what)
    return calls, g


def names(calls):
    return {c.name for c in calls}


# =============================================================================================
# convolution: im2col and halo paths, data-gradient packs, weight gradients
# =============================================================================================
@pytest.mark.parametrize("cin,cout", [(8, 2), (24, 36), (48, 96)])
def test_conv3d_im2col(cin, cout):
    """test_hip_exact.test_im2col_conv: B in {1, 3} x dims (1,1,1), (1,2,40), (3,3,3), (5,6,7) x (bf16 | f32 output; bias;
    residual + affine prologue), split-K workspace included where the grid is small."""
    calls, g = extent(lambda: X.test_im2col_conv(cin, cout), f"conv3d im2col {cin}->{cout}")
    assert sum(c.name == "conv3d" for c in calls) == 32
    split = any(r.site.startswith("ops.py") and "(conv3d)" in r.site and r.dtype == F32 and len(r.shape) == 1 for r in g.records)
    assert split == (cin > 8), "the split-K workspace"        # Cin = 8: Kp = 224 is 7 k-steps, below the 8 of one slice


@pytest.mark.parametrize("cin,cout", [X.HALO_PAIRS[0], X.HALO_PAIRS[-1]])
def test_conv3d_halo(cin, cout):
    """test_hip_exact.test_halo_brick_channels_all_geometries at B = 3: every brick code at (7, 9, 19), ragged for all five,
    plain (bias, residual when cin == cout) and with the fused affine prologue."""
    calls, g = extent(lambda: X.test_halo_brick_channels_all_geometries(cin, cout, 3), f"conv3d halo {cin}->{cout}")
    assert sum(c.name == "conv3d" for c in calls) == 2 * len(X.BRICK_CODES)
    assert sum("(halo_pack)" in r.site for r in g.records) == 2 * len(X.BRICK_CODES)


@pytest.mark.parametrize("cout", [2, 5, 24])
def test_dgrad_packs(cout):
    calls, _ = extent(lambda: X.test_dgrad_packs_through_both_kernels(cout), f"dgrad packs cout={cout}")
    assert {"pack_conv_weight_dgrad", "pack_conv_weight_dgrad16", "conv3d"} <= names(calls)


@pytest.mark.parametrize("cout", [2, 5, 8])
def test_conv3d_wgrad_small_and_rows(cout):
    """The per-workgroup partial buffers (``part``) of both kernels sit between bands.  gs [3][80][64] of conv3d_wgrad_rows is
    internal: rows 72..79 of each plane are padding the wrapper never reads (band check only)."""
    def small():
        ops, _ = mods()
        for cin, B, dims in ((8, 1, (1, 1, 1)), (48, 2, (5, 6, 7)), (8, 1, (9, 13, 20)), (24, 3, (1, 2, 40))):   # the body of
            c = X.wgrad_case(60 + cout + cin, B, cin, cout, dims, True)                     # test_conv3d_wgrad_small, any cout <= 8
            dw, db = ops.conv3d_wgrad_small(X.cl(c.x), X.dev(c.sc), X.dev(c.sh), False, X._pad_channels(X.cl(c.dy), 8), cout)
            E.assert_equal_located(dw, c.dw, "oiabc", f"wgrad_small dW cin={cin} cout={cout} dims={dims}")
            E.assert_equal_located(db, c.db, "o", f"wgrad_small db cin={cin} cout={cout} dims={dims}")
    calls, _ = extent(small, f"conv3d_wgrad_small cout={cout}")
    assert [c.name for c in calls].count("conv3d_wgrad_small") == 4
    calls, _ = extent(lambda: X.test_conv3d_wgrad_rows(cout), f"conv3d_wgrad_rows cout={cout}")
    assert "conv3d_wgrad_rows" in names(calls)


@pytest.mark.parametrize("cin,cin_p,cout,ld", [(6, 8, 16, 16), (48, 48, 5, 8)])
def test_conv3d_wgrad(cin, cin_p, cout, ld):
    calls, _ = extent(lambda: X.test_conv3d_wgrad(cin, cin_p, cout, ld), f"conv3d_wgrad {cin}->{cout}")
    assert names(calls) == {"conv3d_wgrad"}


# =============================================================================================
# gemm_tn (output and split workspace), transposed conv, pointwise conv, head conv
# =============================================================================================
@pytest.mark.parametrize("T", [1, 31, 129])
def test_gemm_tn_rows(T):
    calls, g = extent(lambda: X.test_gemm_tn_rows(T), f"gemm_tn rows T={T}")
    assert [c.name for c in calls].count("gemm_tn") == 25
    assert sum("(gemm_tn)" in r.site for r in g.records) > 25                # every call's workspace, and the outputs not handed in


def test_gemm_tn_head_split_and_conv_taps():
    extent(lambda: X.test_gemm_tn_head_split(3, 43), "gemm_tn head-split (3, 43)")
    extent(lambda: X.test_gemm_tn_conv_taps(2, (2, 3, 5)), "gemm_tn conv taps B=2 (2, 3, 5)")


@pytest.mark.parametrize("stride", [(2, 2, 2), (2, 2, 1)])
@pytest.mark.parametrize("cin,cout", [(16, 8), (96, 48)])
def test_conv_transpose(cin, cout, stride):
    calls, _ = extent(lambda: X.test_conv_transpose_k2s2(cin, cout, stride), f"convt {cin}->{cout} stride={stride}")
    assert {"convt_forward", "convt_dgrad", "convt_wgrad"} <= names(calls)


@pytest.mark.parametrize("n_vox", [1, 255, 257])
@pytest.mark.parametrize("Cc", [8, 48])
def test_pointwise_conv(Cc, n_vox):
    """dyb [n, 4] bf16 of pointwise_conv_backward is internal (band check only)."""
    calls, _ = extent(lambda: X.test_pointwise_conv(Cc, n_vox), f"pointwise C={Cc} n_vox={n_vox}")
    assert {"pointwise_conv", "pointwise_conv_backward"} <= names(calls)


@pytest.mark.parametrize("cin,cout,dims", [(48, 2, (5, 6, 17)), (32, 1, (1, 1, 1)), (16, 2, (9, 4, 33))])
def test_head_conv(cin, cout, dims):
    calls, _ = extent(lambda: X.test_head_conv(cin, cout, dims), f"head_conv {cin}->{cout} dims={dims}")
    assert "head_conv" in names(calls)


# =============================================================================================
# upsample + concat, patch embedding, patch merging
# =============================================================================================
UPCAT = [((2, 2, 2), (1, 1, 1), (2, 2, 2), 16, 8),             # first row of test_upcat's list
         ((2, 2, 1), (2, 3, 24), (4, 6, 24), 384, 192),       # last row
         ((2, 2, 2), (3, 4, 2), (5, 7, 4), 16, 8)]            # odd output dims (cropped)


@pytest.mark.parametrize("scale,idims,sdims,cx,cs", UPCAT)
def test_upcat(scale, idims, sdims, cx, cs):
    calls, _ = extent(lambda: X.test_upcat(scale, idims, sdims, cx, cs), f"upcat {idims}->{sdims} cx={cx} cs={cs}")
    assert {"upcat", "upcat_backward", "upcat_stats", "upcat_affine"} <= names(calls)


@pytest.mark.parametrize("dims,Cc", [((6, 10, 14), 48), ((2, 2, 2), 8)])
def test_patch_embed_and_backward(dims, Cc):
    """B = 2, Cin = 3.  Forward against F.batch_norm(F.conv3d(.., stride 2)) as tests/test_hip_ops.test_patch_embed does
    (rel-L2 4e-3, running statistics 1e-4).  Backward against autograd of the same: dz and the im2col patches are bf16
    (2^-9 per element, about 1.1e-3 rel-L2 each), the sums f32 -- dx, dgamma, dbeta by test_batchnorm_train_fwd_bwd's bars
    (6e-3, 3e-3, 3e-3), dW and dbias by the bf16-operand bar of the merge weight gradients (6e-3)."""
    B, cin = 2, 3
    g = torch.Generator().manual_seed(Cc)
    x = torch.rand(B, cin, *dims, generator=g).requires_grad_(True)
    w = (torch.randn(Cc, cin, 2, 2, 2, generator=g) * 0.3).requires_grad_(True)
    b = (torch.randn(Cc, generator=g) * 0.1).requires_grad_(True)
    bw = (1 + 0.2 * torch.randn(Cc, generator=g)).requires_grad_(True)
    bb = (0.1 * torch.randn(Cc, generator=g)).requires_grad_(True)
    rm, rv = torch.zeros(Cc), torch.ones(Cc)
    n_out = B * math_prod(dims) // 8
    want = F.batch_norm(F.conv3d(x, w, b, stride=2), rm, rv, bw, bb, True, 0.1, 1e-6)
    gout = SB.r16(torch.randn(want.shape, generator=g))
    want.backward(gout)
    xd, wd, bd, bwd, bbd = (t.detach().to(DEV) for t in (x, w, b, bw, bb))
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, BF16)
    cf = lambda t: t.float().cpu().permute(0, 4, 1, 2, 3)

    def body():
        ops, _ = mods()
        rmd, rvd = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
        y, stats = ops.patch_embed(xd, wd, bd, bwd, bbd, 1e-6, rmd, rvd, return_stats=True)      # kernel modes 0 and 1
        dw, db, dgamma, dbeta, dx = ops.patch_embed_backward(xd, wd, bd, dy, stats, need_dx=True)
        torch.cuda.synchronize()
        assert rel_l2(cf(y), want.detach()) < 4e-3
        assert rel_l2(rmd.cpu(), rm) < 1e-4 and rel_l2(rvd.cpu(), rv) < 1e-4
        assert rel_l2(dbeta.cpu(), bb.grad) < 3e-3
        assert all(bool(torch.isfinite(t).all()) for t in (dw, db, dgamma, dx))
        if n_out > 2:
            # (at dims (2, 2, 2) the batch is two voxels per channel: y = beta +- gamma whatever the input, so dx, dW, dbias and
            # dgamma are zero in exact arithmetic and what either side returns is rounding noise -- no relative bar exists)
            assert rel_l2(dx.cpu(), x.grad) < 6e-3
            assert rel_l2(dgamma.cpu(), bw.grad) < 3e-3
            assert rel_l2(dw.cpu(), w.grad) < 6e-3
            assert float((db.cpu() - b.grad).abs().max()) < 6e-3 * float(dbeta.abs().max())     # dbias is zero behind a BatchNorm
    calls, _ = extent(body, f"patch_embed dims={dims} C={Cc}")
    assert names(calls) == {"patch_embed", "patch_embed_backward"}


def math_prod(v):
    out = 1
    for n in v:
        out *= n
    return out


@pytest.mark.parametrize("Cc,dims,last", [(48, (8, 8, 8), True), (192, (4, 6, 5), False)])
def test_patch_merge_and_backward(Cc, dims, last):
    """test_hip_swin_bwd.test_patch_merge_backward_real_channels: patch_merge (as y_fwd) and patch_merge_backward without and
    with need_w.  wg_dn / wg_x [T, kC] are internal (band check only)."""
    calls, _ = extent(lambda: SB.test_patch_merge_backward_real_channels(Cc, dims, last), f"patch_merge C={Cc} dims={dims}")
    assert [c.name for c in calls] == ["patch_merge_backward", "patch_merge_backward"]
    import test_hip_ops as TO
    calls, _ = extent(lambda: TO.test_patch_merge_real_channels(Cc, dims, last), f"patch_merge fwd C={Cc} dims={dims}")
    assert names(calls) == {"patch_merge"}


# =============================================================================================
# BatchNorm pieces, instance norm, pooling, element-wise
# =============================================================================================
BN_SHAPES = [(8, 2, (3, 3, 2)), (16, 3, (9, 13, 21))]


@pytest.mark.parametrize("Cc,B,dims", BN_SHAPES)
def test_bn_partial_sums_and_backward_statistics(Cc, B, dims):
    calls, _ = extent(lambda: X.test_bn_partial_sums_and_affine(Cc, B, dims), f"bn partial sums C={Cc} dims={dims}")
    assert {"bn_partial_sums", "bn_batch_stats"} <= names(calls)
    calls, _ = extent(lambda: X.test_bn_backward_statistics(Cc, B, dims), f"bn backward statistics C={Cc} dims={dims}")
    assert names(calls) == {"bn_backward"}


@pytest.mark.parametrize("Cc,B,dims", BN_SHAPES)
def test_affine_act_and_bn_backward_forms(Cc, B, dims):
    """affine_act, bn_backward and bn_backward_eval against tests/norm_sample_ref.py, by the assertions of
    tests/test_hip_norm_sample.py (test_affine_act, test_bn_bwd_apply, test_wrappers_are_the_entries): the derived intervals."""
    import test_hip_norm_sample as TN
    n = B * math_prod(dims)
    o = NR.bn_operands(n, Cc, seed=n + Cc)
    rows = NR.plant_symmetric_zero_channel(o)
    st, sc, sh, mr = TN.fed(o)
    x5, dy5 = TN.dev(o.x, BF16).view(B, *dims, Cc), TN.dev(o.dy, BF16).view(B, *dims, Cc)
    G8, nblk = Cc // 8, NR.stats_nblk(n, Cc)
    k = NR.chain_len(n * G8, nblk, G8) + nblk                  # reduce_rows adds the nblk rows in f32

    def body():
        ops, _ = mods()
        for lrelu in (True, False):
            ref, e32 = NR.affine_ref(o.x, st.scale32, st.shift32, lrelu)
            y = ops.affine_act(x5, sc, sh, lrelu)
            TN.inside(y.view(n, Cc), ref, NR.with_bf16(ref, e32), "nc", f"ops.affine_act lrelu={lrelu}", NR.bn_id((n, Cc)))
            dxa, dg, db = NR.bn_backward_autograd(o.x, o.dy, o.w, o.b, lrelu)
            c = NR.bn_backward_closed(o.x, o.dy, o.w, o.b, lrelu)
            ce = NR.bn_backward_closed(o.x, o.dy, o.w, o.b, lrelu, train=False)
            dx_t, dg_t, db_t = ops.bn_backward(x5, dy5, sc, sh, mr, lrelu)
            dx_e, dg_e, db_e = ops.bn_backward_eval(x5, dy5, sc, sh, mr, lrelu)
            TN.assert_same_bits(dg_t.contiguous(), dg_e.contiguous(), "dgamma of the training and the eval form")
            TN.assert_same_bits(db_t.contiguous(), db_e.contiguous(), "dbeta of the training and the eval form")
            TN.inside(torch.cat([db_t, dg_t]), torch.cat([db, dg]), NR.bwd_sums_bounds(c, k), "c", f"ops.bn_backward sums lrelu={lrelu}",
                      NR.bn_id((n, Cc)))
            TN.inside(dx_e.view(n, Cc), ce.dx, NR.with_bf16(ce.dx, NR.bwd_dx_bound(ce, o.x, False)), "nc",
                      f"ops.bn_backward_eval dx lrelu={lrelu}", NR.bn_id((n, Cc)))
            # the training dx is formed from the wrapper's own sums: bit-equal to the entry fed those sums (its interval: test_bn_bwd_apply)
            L = TN.L
            sums = torch.cat([db_t, dg_t]).contiguous()
            dx = TN.Out((n, Cc), BF16)
            L.call("mivp_bn_bwd_apply", L.ptr(x5), L.ptr(dy5), n, Cc, L.ptr(sc), L.ptr(sh), L.ptr(mr), L.ptr(sums), 1 if lrelu else 0,
                   L.ptr(dx.t), L.stream())
            torch.cuda.synchronize()
            TN.assert_same_bits(dx_t.view(n, Cc), dx.done("bn_bwd_apply"), f"ops.bn_backward dx lrelu={lrelu}")
    calls, _ = extent(body, f"affine_act / bn_backward C={Cc} dims={dims}")
    assert names(calls) == {"affine_act", "bn_backward", "bn_backward_eval"}


@pytest.mark.parametrize("Cc,B,dims", BN_SHAPES)
def test_instance_norm_and_pool(Cc, B, dims):
    """instance_norm_act (+ backward) is the per-sample chain of bn_batch_stats / affine_act / bn_backward: bit-equal to those
    wrappers called on each sample (whose own references are above).  global_avg_pool of small integers: the column sums
    are exact, so the result is the float64 mean to the two f32 roundings of the division."""
    g = E.gen(Cc + dims[2])
    x = E.draw(g, (B, Cc, *dims), (-2, -1, 1, 2, 3), 0.75)
    dy = E.draw(g, (B, Cc, *dims), X.X_VALS, 0.5)
    xd, dyd = X.cl(x), X.cl(dy)
    n = math_prod(dims)

    def body():
        ops, _ = mods()
        y, saved = ops.instance_norm_act(xd)
        dx = ops.instance_norm_act_backward(xd, dyd, saved)
        pooled = ops.global_avg_pool(xd)
        one, zero = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        for b in range(B):
            st = ops.bn_batch_stats(xd[b:b + 1], one, zero, 1e-5)
            for got, want in zip(saved[b], st):
                assert G.same_bits(got, want)
            assert G.same_bits(y[b:b + 1], ops.affine_act(xd[b:b + 1], *st[:2], True))
            assert G.same_bits(dx[b:b + 1], ops.bn_backward(xd[b:b + 1], dyd[b:b + 1].contiguous(), *st, True)[0])
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()).all())
        s = x.sum((2, 3, 4))
        E.assert_exact_inputs(s, x.abs().sum((2, 3, 4)), False, "global_avg_pool sums")
        # sums / float(n) is a product with the rounded reciprocal on the device: two f32 roundings, (1 + 2^-24)^2 - 1 < 3 * 2^-24
        off = (pooled.double().cpu() - s / n).abs()
        assert bool((off <= 3 * 2.0 ** -24 * (s / n).abs()).all()), f"global_avg_pool C={Cc} dims={dims}: {float(off.max())}"
    calls, _ = extent(body, f"instance_norm / global_avg_pool C={Cc} dims={dims}")
    assert {"instance_norm_act", "instance_norm_act_backward", "global_avg_pool"} <= names(calls)


@pytest.mark.parametrize("numel", [1, 255, 257])
def test_cast_and_add(numel):
    """cast_bf16 is round-to-nearest-even of f32; add_bf16 the bf16 rounding of the f32 sum of two bf16 numbers (exact in
    f32: 8-bit significands, so the sum is the float64 sum): both bit-equal to torch's own casts.  mivp_add_bf16 takes
    multiples of 8 elements only (its contract in mivp.h): at these lengths it must refuse and write nothing -- the bands
    and the untouched inputs are what is checked -- and it runs at the next multiple of 8."""
    g = torch.Generator().manual_seed(numel)
    n8 = (numel + 7) // 8 * 8
    t = (torch.randn(numel, generator=g) * torch.exp2(torch.randint(-12, 12, (numel,), generator=g).float())).to(DEV)
    a, b = torch.randn(n8, generator=g).to(DEV, BF16), torch.randn(n8, generator=g).to(DEV, BF16)
    a_odd, b_odd = a[:numel].clone(), b[:numel].clone()

    def body():
        ops, _ = mods()
        assert G.same_bits(ops.cast_bf16(t), t.to(BF16))
        assert G.same_bits(ops.add_bf16(a, b), (a.double() + b.double()).to(BF16))
        with pytest.raises(RuntimeError, match="failed with code -1"):
            ops.add_bf16(a_odd, b_odd)
    calls, g = extent(body, f"cast_bf16 / add_bf16 numel={numel}")
    assert [c.name for c in calls] == ["cast_bf16", "add_bf16"]
    refused = g.records[-1]
    assert refused.shape == (numel,) and bool(g.canary(refused.view).all()), "a refused call wrote to its output"


# =============================================================================================
# low-resolution head
# =============================================================================================
UPHEAD_SHAPES = ["S1", "S2", "S3"]      # the two smallest; S3: T = 680 tokens, no multiple of the 512-token taps workgroup, the 64-token
#                                         dx workgroup or the 4 x 4 x 16 adjoint brick, two samples


@pytest.mark.parametrize("name", UPHEAD_SHAPES)
def test_uphead_forward_and_statistics(name):
    Cc, cout = 48, 2
    B, h, w, d = UR.SHAPES[name]

    def body():
        ops, _ = mods()
        U.test_forward_exact(name, Cc, cout)                                   # uphead_fold + uphead_forward (and its fp16 workspace)
        c = UR.stats_case(name, Cc)
        x = U.cl(c.x)
        bw, bb = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        scale, shift, mr, gx = ops.uphead_batch_stats(x, bw, bb, 1e-5, keep_gx=True)
        part, gx_direct = U.run_stats(U._lib(), x, True)
        assert U.same_bits(gx, gx_direct)
        E.assert_equal_located(gx, UR.cl64(c.gx), "bhwdc", f"uphead_batch_stats gx {name}")
        s3 = ops.bn_finalize(part, part.shape[0], Cc, 8 * B * h * w * d, bw, bb, 1e-5, None, None)
        for got, want in zip((scale, shift, mr), s3):
            assert U.same_bits(got, want)
        a = UR.adjoint_case(name, cout)
        dy = U.cl(a.dy, F32)
        Gm, S, D = ops.uphead_gs(x, dy, cout, keep_d=True, raw=True)
        U.check_adjoint(D, a, (B, h, w, d), cout, f"uphead_gs D {name}")
        D64 = D.double().cpu()
        ref, bound = E.matmul_tn_ref(D64[:, :27 * cout], c.x.permute(0, 2, 3, 4, 1).reshape(-1, Cc))
        E.assert_exact_inputs(ref, bound, False, "uphead_gs G")
        E.assert_equal_located(Gm, ref, "mn", f"uphead_gs G {name}")
        E.assert_equal_located(S[:27 * cout], D64[:, :27 * cout].sum(0), "c", f"uphead_gs S {name}")
        G2, S2 = ops.uphead_gs(x, dy, cout)                                    # the co-major form, ldD = round_up(27 * cout, 8)
        E.assert_equal_located(G2, ref.view(27, cout, Cc).permute(1, 0, 2), "otc", f"uphead_gs G co-major {name}")
    calls, _ = extent(body, f"uphead forward / statistics {name}")
    assert {"uphead_fold", "uphead_forward", "uphead_batch_stats", "uphead_gs"} <= names(calls)


@pytest.mark.parametrize("name", UPHEAD_SHAPES)
@pytest.mark.parametrize("training", [True, False])
def test_uphead_gradients(name, training):
    """head_grads_fused and uphead_dx against the C entries called one by one on NaN-prefilled buffers (bit-equal), whose
    own exact references are tests/test_hip_uphead.py's; at S3 also the whole chain of that file."""
    Cc, cout = 48, 2
    B, h, w, d = UR.SHAPES[name]
    c = UR.head_grads_case(Cc, cout)
    s = UR.stats_case(name, Cc)
    a = UR.adjoint_case(name, cout)

    def body():
        ops, _ = mods()
        L = U._lib()
        torch.manual_seed(11)                                  # the chain draws its conv weights from the global generator
        if name == "S3":
            U.test_chain_is_bit_equal_to_its_pieces(training)
        U.test_head_grads_exact(Cc, cout, 8)
        x, dy = U.cl(s.x), U.cl(a.dy, F32)
        wt, scale, mr = U.dev(c.w), U.dev(c.scale), U.dev(c.mean_rstd)
        Gm, S, D = ops.uphead_gs(x, dy, cout, keep_d=True, raw=True)
        dW, db, dgamma, dbeta = ops.head_grads_fused(Gm, S, wt, scale, U.dev(c.shift), mr)
        gx = ops.uphead_batch_stats(x, torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV), 1e-5, keep_gx=True)[3] if training else None
        dx = ops.uphead_dx(x, D, wt, scale, mr, dgamma, dbeta, training, gx)
        wc = torch.full((U.round_up(Cc, 16), 64), U.NAN, dtype=BF16, device=DEV)
        coef = torch.full((4, Cc), U.NAN, dtype=F32, device=DEV)
        L.call("mivp_uphead_dx_prep", L.ptr(wt), L.ptr(scale), L.ptr(mr), L.ptr(dgamma) if training else None,
               L.ptr(dbeta) if training else None, 8.0 * B * h * w * d, 1 if training else 0, cout, Cc, L.ptr(wc), L.ptr(coef), L.stream())
        want = torch.full(x.shape, U.NAN, dtype=BF16, device=DEV)
        L.call("mivp_uphead_dx", L.ptr(D), L.ptr(wc), L.ptr(x), L.ptr(coef), L.ptr(gx), B, h, w, d, Cc, L.ptr(want), L.stream())
        torch.cuda.synchronize()
        assert U.same_bits(dx, want) and bool(torch.isfinite(dx.float()).all())
    calls, _ = extent(body, f"uphead gradients {name} training={training}")
    assert {"head_grads_fused", "uphead_dx", "uphead_gs"} <= names(calls)


# =============================================================================================
# Swin block: forward (save=True) and backward, every q / k / v / o / lse buffer, saved activation, partial and gradient
# =============================================================================================
def block_inputs(window, Cc, heads, n_prompt, dims, seed=5, B=2):
    """The inputs of test_hip_swin_bwd.test_block_weight_gradients_real_sizes (oracle.unetr_ref._block_state, non-trivial norms
    and biases, SB._rounded_state)."""
    from oracle.unetr_ref import _block_state
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    _block_state(sd, "", Cc, heads, list(window), 64, max(n_prompt, 1), n_prompt > 0, gen)
    for k in list(sd):
        if "norm.weight" in k:
            sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=gen)
        if "norm.bias" in k or k.endswith("proj.bias") or k.endswith("mlp.bias"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=gen)
    sd = SB._rounded_state(sd)
    x = SB.r16(torch.randn(B, Cc, *dims, generator=gen))
    prm = 0.5 * torch.randn(n_prompt, Cc, generator=gen) if n_prompt else None
    gout = SB.r16(torch.randn(B, Cc, *dims, generator=gen))
    return sd, x, prm, gout


def pad_rows(desc, shape, axis):
    """Mask of the window slots Nq <= r < Nqp along ``axis`` of a [.., Nqp, ..] buffer."""
    m = torch.zeros(shape, dtype=torch.bool)
    idx = [slice(None)] * len(shape)
    idx[axis] = slice(int(desc.Nq), int(desc.Nqp))
    m[tuple(idx)] = True
    return m


def swin_allow(call):
    """Elements of the Swin block's buffers that are unwritten by design (DESIGN.md "Write extent")."""
    return {}


def run_weight_grads(sd, x, prm, gout, window, shift, heads, toy):
    res = SB._run_block_weight_grads(sd, x, prm, gout, window, shift, heads)
    for k, err in res.items():
        # test_block_weight_gradients_real_sizes: 1.5e-2; _golden_shapes (toy windows: table gradients over a handful of windows): 3e-2
        assert err < (3e-2 if (toy and "content" in k) else 1.5e-2), (k, err)


def run_data_grads(sd, x, prm, gout, window, shift, heads, need_dx=True):
    res = SB._run_block(sd, x, prm, gout, window, shift, heads, need_dx)        # test_block_backward_real_sizes
    for k, (err, _) in res.items():
        assert err < 1.5e-2, (k, err)


SWIN = [
    ((3, 3, 2), (6, 6, 4), 16, 4, 8, (1, 1, 1), "head_dim 4, tiny windows"),
    ((5, 5, 3), (10, 10, 6), 48, 4, 16, (2, 2, 1), "75 queries: the phantom sixth query tile"),
    ((5, 5, 3), (10, 10, 6), 48, 4, 30, (2, 2, 1), "ragged second prompt tile"),
    ((2, 4, 4), (2, 4, 4), 128, 16, 0, (0, 0, 0), "16-token kernels, 32-slot window"),
    ((2, 2, 4), (2, 2, 4), 96, 8, 0, (0, 0, 0), "16-token kernels, 16-slot window"),
    ((7, 7, 7), (12, 12, 24), 96, 4, 0, (3, 3, 3), "padded volume, head_dim 24"),
    ((7, 7, 7), (14, 14, 14), 48, 4, 64, (3, 3, 3), "model stage 1 with prompts"),
    ((7, 7, 7), (6, 6, 24), 192, 4, 64, (3, 3, 3), "head_dim 48, chunked LDS"),
]


@pytest.mark.parametrize("window,dims,Cc,heads,n_prompt,shift,why", SWIN, ids=[f"C{c[2]}_{'x'.join(map(str, c[1]))}_p{c[4]}" for c in SWIN])
def test_swin_block(window, dims, Cc, heads, n_prompt, shift, why):
    """swin_block_forward(save=True) + swin_block_backward(need_w=True), and the data-gradient form (need_w=False: the one-pass
    attention backward where it applies), against autograd over the oracle by test_hip_swin_bwd's own bars."""
    sd, x, prm, gout = block_inputs(window, Cc, heads, n_prompt, dims)
    toy = tuple(window) != (7, 7, 7)
    calls, _ = extent(lambda: run_weight_grads(sd, x, prm, gout, window, shift, heads, toy), f"swin block need_w {why}", swin_allow)
    assert [c.name for c in calls] == ["weights_from_state", "swin_block_forward", "swin_block_backward"]
    calls, _ = extent(lambda: run_data_grads(sd, x, prm, gout, window, shift, heads), f"swin block data gradients {why}", swin_allow)
    assert [c.name for c in calls] == ["weights_from_state", "swin_block_forward", "swin_block_backward"]


BIG = ((7, 7, 7), (14, 14, 14), 48, 4, 64, (3, 3, 3))


def test_swin_block_prompt_only_backward():
    """need_dx=False: mivp_win_attn_bwd_prompt (first prompted block behind a frozen stem)."""
    window, dims, Cc, heads, n_prompt, shift = BIG
    sd, x, prm, gout = block_inputs(window, Cc, heads, n_prompt, dims)
    extent(lambda: run_data_grads(sd, x, prm, gout, window, shift, heads, need_dx=False), "swin block need_dx=False", swin_allow)


def test_swin_block_two_pass_backward():
    """USE_FUSED_ATTN_BWD=False: the dq-owner + dkv-owner pair without the weight-gradient outputs, and delta + dkv for need_dx=False."""
    _, swin_ops = mods()
    window, dims, Cc, heads, n_prompt, shift = BIG
    sd, x, prm, gout = block_inputs(window, Cc, heads, n_prompt, dims)
    swin_ops.USE_FUSED_ATTN_BWD = False
    try:
        extent(lambda: run_data_grads(sd, x, prm, gout, window, shift, heads), "swin block two-pass", swin_allow)
        extent(lambda: run_data_grads(sd, x, prm, gout, window, shift, heads, need_dx=False), "swin block two-pass need_dx=False", swin_allow)
    finally:
        swin_ops.USE_FUSED_ATTN_BWD = True


def test_swin_block_dropout():
    """Dropout (0.1, 0.1, seed, seed), need_w=True: the body of test_block_dropout_matches_oracle_under_the_same_masks (the
    kernels' masks exported and handed to the oracle; 6e-3 forward, 1.5e-2 gradients) on the model-size block."""
    from mivp_amd import _lib as L
    from oracle import swin_ref as S
    _, swin_ops = mods()
    window, dims, Cc, heads, n_prompt, shift = BIG
    sd, x, prm, gout = block_inputs(window, Cc, heads, n_prompt, dims, B=1)
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV, BF16)
    dy = gout.permute(0, 2, 3, 4, 1).contiguous().to(DEV, BF16)
    pd = prm.to(DEV)
    ts = ((sd["pe.weights_token"] @ sd["pe.enc_token.0"].t())[:, :n_prompt] * (64 ** -0.5)).to(DEV)

    def body():
        w = swin_ops.weights_from_state(sd, "", heads, 64, 0, torch.device(DEV), need_bwd=True)
        y, saved = swin_ops.swin_block_forward(xc, pd, w, ts, window, shift, save=True, dropout=(0.1, 0.1, 1234, 987))
        dx, dprompt, dts, wg = swin_ops.swin_block_backward(saved, w, pd, dy, True, True, need_w=True)
        d = saved.desc
        B, P, Nq, Nqp, Nkp = d.B, d.P, d.Nq, d.Nqp, d.Nkp
        ak = torch.empty((B * P * heads, Nqp, Nkp), dtype=torch.uint8, device=DEV)
        pk = torch.empty((B * P * Nqp, Cc), dtype=torch.uint8, device=DEV)
        L.call("mivp_dropout_masks", C.byref(d), L.ptr(ak), L.ptr(pk), L.stream())
        torch.cuda.synchronize()
        ak = ak.cpu().view(B, P, heads, Nqp, Nkp).float()
        cols = list(range(Nq)) + list(range(Nqp, Nqp + n_prompt))
        attn_keep = ak[:, :, :, :Nq][..., cols] * float(d.attn_drop_scale)
        proj_keep = pk.cpu().view(B, P, Nqp, Cc)[:, :, :Nq].float() * float(d.proj_drop_scale)
        sdo = {k: v.clone() for k, v in sd.items()}
        for k, v in sdo.items():
            if v.is_floating_point() and "pe." not in k:
                v.requires_grad_(True)
        xo, po = x.clone().requires_grad_(True), prm.clone().requires_grad_(True)
        want = S.swin_block(xo, po, sdo, "", window, shift, heads, 64, attn_keep, proj_keep)
        want.backward(gout)
        assert rel_l2(y.float().cpu().permute(0, 4, 1, 2, 3), want.detach()) < 6e-3
        assert rel_l2(dx.float().cpu().permute(0, 4, 1, 2, 3), xo.grad) < 1.5e-2
        assert rel_l2(dprompt.cpu(), po.grad) < 1.5e-2
        for short, key in SB.WEIGHT_KEYS.items():
            assert rel_l2(wg[short].cpu().reshape(sdo[key].shape), sdo[key].grad) < 1.5e-2, key
    extent(body, "swin block dropout", swin_allow)
