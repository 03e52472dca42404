"""Per-kernel exact parity of the low-resolution head kernels (csrc/uphead.hip) against the float64 reference of
tests/uphead_ref.py: every kernel is called at the level where the test chooses scale, shift, mean and rstd itself
(``ops.uphead_fold`` / ``ops.uphead_forward`` and the C entries), so nothing measured is folded in and the result has to
equal the reference bit for bit at every element (conditions (a) to (d): tests/uphead_ref.py).  The one
output that cannot be a bf16 number, the training-mode dx, is held to half a bf16 spacing of the float64 value.
Shapes S1 to S6 are the smallest that cross the ST_SEG = 16 statistics seams, the 4 x 4 x 16 adjoint bricks, a second
(partially live) 512-token k_uphead_taps workgroup and the batch boundary; C runs 8 ... 56 on S3."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_ref as E  # noqa: E402
import uphead_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")


def _ops():
    import mivp_amd  # noqa: F401
    from mivp_amd import ops
    return ops


def _lib():
    from mivp_amd import _lib as L
    return L


def cl(t, dtype=BF16):
    """float64 [B, C, h, w, d] -> channels-last device tensor (the cast is exact: operands are bf16 numbers)."""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)


def dev(t, dtype=torch.float32):
    return None if t is None else t.contiguous().to(DEV, dtype)


def same_bits(a, b):
    """Bit-identical tensors (NaN payloads included)."""
    assert a.dtype == b.dtype and a.shape == b.shape
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def round_up(v, m):
    return (v + m - 1) // m * m


# ---------------------------------------------------------------------------------------------
# 1. k_uphead_fold
# ---------------------------------------------------------------------------------------------
def _fold_want(w, scale, shift, mp):
    """float64 [mp, 64]: row tap * Cout + co = (w * scale | sum_c w * shift | 0 ...), rows >= 27 * Cout zero."""
    cout, C = w.shape[:2]
    wt = w.reshape(cout, C, 27)
    want = torch.zeros((mp, 64), dtype=torch.float64)
    want[:27 * cout, :C] = (wt * scale.view(1, -1, 1)).permute(2, 0, 1).reshape(27 * cout, C)
    want[:27 * cout, C] = (wt * shift.view(1, -1, 1)).sum(1).t().reshape(27 * cout)
    return want


@pytest.mark.parametrize("C", [8, 48, 56])
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_fold_dyadic_is_exact(C, cout):
    ops = _ops()
    g = E.gen(100 + 10 * C + cout)
    w = E.draw(g, (cout, C, 3, 3, 3), R.W_VALS)
    scale, shift = E.draw(g, (C,), R.DYADIC), E.draw(g, (C,), R.SHIFT_VALS)
    mp = round_up(27 * cout, 16)
    wf = ops.uphead_fold(dev(w), dev(scale), dev(shift))
    torch.cuda.synchronize()
    assert tuple(wf.shape) == (2, mp, 64)
    want = _fold_want(w, scale, shift, mp)
    E.assert_bf16_operands(want)
    E.assert_equal_located(wf[0], want, "rk", f"fold hi C={C} Cout={cout}")
    E.assert_equal_located(wf[1], torch.zeros_like(want), "rk", f"fold lo C={C} Cout={cout}")


def test_fold_hi_lo_pair_of_a_non_dyadic_weight():
    """hi = bf16(v), lo = bf16(v - hi) with v - hi exact in f32: |hi + lo - v| = |lo - (v - hi)| is one bf16 rounding,
    at most one bf16 spacing at lo (two roundings in all).  v = w * scale is a single f32 product (the same in torch
    float32); the shift column is an f32 sum of C products in the kernel's own order: C * 2^-24 * sum |w * shift| more."""
    ops = _ops()
    C, cout = 48, 2
    g = E.gen(7)
    w = torch.randn((cout, C, 3, 3, 3), generator=g, dtype=torch.float32)
    scale = 1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float32)
    shift = 0.3 * torch.randn(C, generator=g, dtype=torch.float32)
    wf = ops.uphead_fold(w.to(DEV), scale.to(DEV), shift.to(DEV)).cpu()
    wt = w.reshape(cout, C, 27)
    v = torch.zeros((64, 64), dtype=torch.float64)
    v[:54, :C] = (wt * scale.view(1, -1, 1)).permute(2, 0, 1).reshape(54, C).double()      # f32 products, then widened
    prod = (wt * shift.view(1, -1, 1)).double()
    v[:54, C] = prod.sum(1).t().reshape(54)
    slack = torch.zeros_like(v)
    slack[:54, C] = C * 2.0 ** -24 * prod.abs().sum(1).t().reshape(54)
    hi, lo = wf[0].double(), wf[1].double()
    err = (hi + lo - v).abs()
    bar = 2 * R.bf16_half_spacing(lo) + slack
    bad = torch.nonzero(~(err <= bar))
    assert bad.numel() == 0, f"{len(bad)} elements, first (row, column) {tuple(int(i) for i in bad[0])}: " \
                             f"err {float(err[tuple(bad[0])])} bar {float(bar[tuple(bad[0])])}"
    assert float((hi - v).abs().max()) > 0 and float(lo.abs().max()) > 0      # the case does exercise the lo plane
    assert torch.equal(hi[54:], torch.zeros(10, 64, dtype=torch.float64)) and torch.equal(lo[:, C + 1:], torch.zeros(64, 63 - C, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------
# 2. k_uphead_taps + k_uphead_gather
# ---------------------------------------------------------------------------------------------
FWD_CASES = [(n, C, co) for n, C in R.shape_c_pairs() for co in (1, 2)] + [("S3", C, co) for C in (8, 48) for co in (3, 4)]


@pytest.mark.parametrize("name,C,cout", FWD_CASES)
def test_forward_exact(name, C, cout):
    """k_uphead_taps<MT, Cout> (MT = 2, 4, 6, 7) and k_uphead_gather<Cout>: bit for bit at every output voxel."""
    ops = _ops()
    c = R.forward_case(name, C, cout)
    wf = ops.uphead_fold(dev(c.w), dev(c.scale), dev(c.shift))
    y = ops.uphead_forward(cl(c.x), wf, dev(c.b), cout)
    torch.cuda.synchronize()
    E.assert_equal_located(y, R.cl64(c.ref), "bhwdc", f"forward {name} C={C} Cout={cout}")


def test_forward_without_bias():
    ops, L = _ops(), _lib()
    name, C, cout = "S3", 48, 2
    B, h, w, d = R.SHAPES[name]
    c = R.forward_case(name, C, cout, False)
    x = cl(c.x)
    wf = ops.uphead_fold(dev(c.w), dev(c.scale), dev(c.shift))
    ws = torch.empty(L.lib().mivp_uphead_fwd_ws(B, h, w, d, cout) // 2, dtype=torch.float16, device=DEV)
    y = torch.full((B, 2 * h, 2 * w, 2 * d, cout), NAN, dtype=torch.float32, device=DEV)
    L.call("mivp_uphead_fwd", L.ptr(x), L.ptr(wf), None, B, h, w, d, C, cout, L.ptr(ws), L.ptr(y), L.stream())
    torch.cuda.synchronize()
    E.assert_equal_located(y, R.cl64(c.ref), "bhwdc", "forward without bias")


# ---------------------------------------------------------------------------------------------
# 3. k_uphead_stats
# ---------------------------------------------------------------------------------------------
def run_stats(L, x, keep_gx):
    B, h, w, d, C = x.shape
    nblk = L.lib().mivp_uphead_nblk(B, h, w, d, C)
    part = torch.full((nblk, 2 * C), NAN, dtype=torch.float32, device=DEV)
    gx = torch.full(x.shape, NAN, dtype=torch.float32, device=DEV) if keep_gx else None
    L.call("mivp_uphead_stats", L.ptr(x), B, h, w, d, C, L.ptr(part), L.ptr(gx), L.stream())
    torch.cuda.synchronize()
    return part, gx


@pytest.mark.parametrize("name,C", R.shape_c_pairs())
def test_stats_exact(name, C):
    """sum(Ux), sum((Ux)^2) per channel (block partials summed in float64) and gx = U^T U x at every cell: the tridiagonal
    Gram claim, its clamped ends and the ST_SEG seams against autograd of the upsample."""
    L = _lib()
    c = R.stats_case(name, C)
    x = cl(c.x)
    part, gx = run_stats(L, x, True)
    tot = part.double().sum(0).cpu()
    E.assert_equal_located(tot[:C], c.s1, "c", f"stats sum {name} C={C}")
    E.assert_equal_located(tot[C:], c.s2, "c", f"stats sum of squares {name} C={C}")
    E.assert_equal_located(gx, R.cl64(c.gx), "bhwdc", f"stats gx {name} C={C}")
    part2, _ = run_stats(L, x, False)
    assert same_bits(part, part2), "the partial sums depend on whether gx is kept"


# ---------------------------------------------------------------------------------------------
# 4. k_uphead_adjoint<Cout>, k_uphead_adjoint_brick
# ---------------------------------------------------------------------------------------------
def run_adjoint(L, dy, dims, cout, ld):
    """dy channels-last f32 [B, 2h, 2w, 2d, stride] on the device -> D [T, ld] bf16 (pre-filled with NaN)."""
    B, h, w, d = dims
    D = torch.full((B * h * w * d, ld), NAN, dtype=BF16, device=DEV)
    L.call("mivp_uphead_adjoint", L.ptr(dy), dy.shape[-1], B, h, w, d, cout, L.ptr(D), ld, L.stream())
    torch.cuda.synchronize()
    return D


def check_adjoint(D, c, dims, cout, what):
    B, h, w, d = dims
    K = 27 * cout
    E.assert_equal_located(D[:, :K].reshape(B, h, w, d, K), c.D.view(B, h, w, d, K), "bhwdc", what)
    pad = D[:, K:].reshape(B, h, w, d, D.shape[1] - K)
    E.assert_equal_located(pad, torch.zeros(pad.shape, dtype=torch.float64), "bhwdc", what + " (columns beyond 27 * Cout)")


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_adjoint_brick_and_generic_cout2(name):
    """Cout = 2: the brick kernel at ldD = 64 and 56 (contiguous dy), the generic kernel on dy padded to 8 channels;
    all equal adjoint_ref, zero beyond column 53, and the generic result is bit-equal to the brick's."""
    L = _lib()
    dims = R.SHAPES[name]
    c = R.adjoint_case(name, 2)
    dy = cl(c.dy, torch.float32)
    brick = run_adjoint(L, dy, dims, 2, 64)
    check_adjoint(brick, c, dims, 2, f"adjoint brick ldD=64 {name}")
    check_adjoint(run_adjoint(L, dy, dims, 2, 56), c, dims, 2, f"adjoint brick ldD=56 {name}")
    dy8 = torch.full((*dy.shape[:-1], 8), NAN, dtype=torch.float32, device=DEV)
    dy8[..., :2] = dy
    generic = run_adjoint(L, dy8, dims, 2, 64)
    check_adjoint(generic, c, dims, 2, f"adjoint generic dy_stride=8 {name}")
    assert same_bits(generic, brick)


@pytest.mark.parametrize("name", ["S3", "S4"])
@pytest.mark.parametrize("cout,ld", [(1, 32), (1, 64), (3, 88), (4, 112)])
def test_adjoint_generic(name, cout, ld):
    L = _lib()
    dims = R.SHAPES[name]
    c = R.adjoint_case(name, cout)
    D = run_adjoint(L, cl(c.dy, torch.float32), dims, cout, ld)
    check_adjoint(D, c, dims, cout, f"adjoint generic Cout={cout} ldD={ld} {name}")


# ---------------------------------------------------------------------------------------------
# 5. k_uphead_dx<CT>
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C", R.shape_c_pairs())
@pytest.mark.parametrize("training", [False, True])
def test_dx(name, C, training):
    """Hand-made wc and coef.  Eval (k1 = k2 = 0): bit equal.  Training: within half a bf16 spacing of the float64 value.
    gx given and gx = NULL (the in-kernel 27-point Gram gather) must agree bit for bit; every element is written."""
    L = _lib()
    B, h, w, d = R.SHAPES[name]
    cout = R.dx_cout(C)
    c = R.dx_case(name, C, cout, training)
    K = 27 * cout
    D = torch.zeros((B * h * w * d, 64), dtype=torch.float64)
    D[:, :K] = c.D
    wc = torch.zeros((round_up(C, 16), 64), dtype=torch.float64)
    wc[:C, :K] = c.wc
    D, wc, coef, x = D.to(DEV, BF16), wc.to(DEV, BF16), dev(c.coef), cl(c.x)
    gram = R.cl64(c.gram).to(DEV, torch.float32)
    assert torch.equal(gram.double().cpu(), R.cl64(c.gram))
    got = []
    for gx in (gram, None):
        dx = torch.full(x.shape, NAN, dtype=BF16, device=DEV)
        L.call("mivp_uphead_dx", L.ptr(D), L.ptr(wc), L.ptr(x), L.ptr(coef), L.ptr(gx), B, h, w, d, C, L.ptr(dx), L.stream())
        torch.cuda.synchronize()
        what = f"dx {name} C={C} training={training} gx={'given' if gx is not None else 'NULL'}"
        if training:
            R.assert_interval_located(dx, c.ref, what)
        else:
            E.assert_equal_located(dx, c.ref, "bhwdc", what)
        got.append(dx)
    assert same_bits(got[0], got[1]), "dx differs between the kept gx and the in-kernel Gram gather"


# ---------------------------------------------------------------------------------------------
# 6. k_uphead_dx_prep
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,cout", [(8, 1), (24, 2), (56, 2)])
@pytest.mark.parametrize("training", [False, True])
def test_dx_prep(C, cout, training):
    L = _lib()
    g = E.gen(300 + C + cout)
    w = torch.randn((cout, C, 3, 3, 3), generator=g, dtype=torch.float32)
    scale, mean_rstd = torch.randn(C, generator=g), torch.randn(2 * C, generator=g)
    dgamma, dbeta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    n_hr = 8.0 * 2 * 5 * 4 * 17
    cp = round_up(C, 16)
    wc = torch.full((cp, 64), NAN, dtype=BF16, device=DEV)
    coef = torch.full((4, C), NAN, dtype=torch.float32, device=DEV)
    wd, sd, md, gd, bd = (t.to(DEV) for t in (w, scale, mean_rstd, dgamma, dbeta))
    L.call("mivp_uphead_dx_prep", L.ptr(wd), L.ptr(sd), L.ptr(md), L.ptr(gd) if training else None,
           L.ptr(bd) if training else None, n_hr, 1 if training else 0, cout, C, L.ptr(wc), L.ptr(coef), L.stream())
    torch.cuda.synchronize()
    want = torch.zeros((cp, 64), dtype=torch.float32)
    want[:C, :27 * cout] = w.reshape(cout, C, 27).permute(1, 2, 0).reshape(C, 27 * cout)          # [c][tap * Cout + co]
    E.assert_equal_located(wc, want.to(BF16), "ck", f"dx_prep wc C={C} Cout={cout}")
    inv_n = torch.tensor(1.0 / n_hr, dtype=torch.float64).float()
    zero = torch.zeros(C)
    want_coef = torch.stack([scale, dbeta * inv_n if training else zero,
                             mean_rstd[C:] * dgamma * inv_n if training else zero, mean_rstd[:C]])
    E.assert_equal_located(coef, want_coef, "rc", f"dx_prep coef C={C} training={training}")


# ---------------------------------------------------------------------------------------------
# 7. k_head_grads
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 56])
@pytest.mark.parametrize("cout", [1, 2])
@pytest.mark.parametrize("ld_extra", [0, 8])
def test_head_grads_exact(C, cout, ld_extra):
    """Tap-major G with row stride C + ld_extra through ops.head_grads_fused, then the co-major layout through the C entry."""
    ops, L = _ops(), _lib()
    c = R.head_grads_case(C, cout)
    w, scale, shift, mr = dev(c.w), dev(c.scale), dev(c.shift), dev(c.mean_rstd)
    G = torch.full((27 * cout, C + ld_extra), NAN, dtype=torch.float32, device=DEV)
    G[:, :C] = dev(c.G.permute(1, 0, 2).reshape(27 * cout, C))
    S = torch.full((64,), NAN, dtype=torch.float32, device=DEV)
    S[:27 * cout] = dev(c.S.t().reshape(-1))
    tap_major = ops.head_grads_fused(G, S, w, scale, shift, mr)
    co_major = tuple(torch.full_like(t, NAN) for t in tap_major)
    Gc, Sc = dev(c.G), dev(c.S)
    L.call("mivp_head_grads", L.ptr(Gc), 27 * C, C, L.ptr(Sc), 27, 1, L.ptr(w), L.ptr(scale), L.ptr(shift), L.ptr(mr),
           cout, C, L.ptr(co_major[0]), L.ptr(co_major[1]), L.ptr(co_major[2]), L.ptr(co_major[3]), L.stream())
    torch.cuda.synchronize()
    for got, lay in ((tap_major, "tap-major"), (co_major, "co-major")):
        what = f"head_grads {lay} C={C} Cout={cout} row stride {C + ld_extra if lay == 'tap-major' else C}"
        E.assert_equal_located(got[0].reshape(cout, C, 27), c.ref[0], "oct", what + " dW")
        for k, n in ((1, "db"), (2, "dgamma"), (3, "dbeta")):
            E.assert_equal_located(got[k], c.ref[k], "c", what + " " + n)


# ---------------------------------------------------------------------------------------------
# 8. the real pipeline is these pieces
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_chain_is_bit_equal_to_its_pieces(training):
    """Fn.uphead forward + backward at S3, C = 48, Cout = 2 against the same kernels called one by one as above."""
    import torch.nn as nn
    ops, L = _ops(), _lib()
    from mivp_amd import functional as Fn
    B, h, w, d = R.SHAPES["S3"]
    C, cout = 48, 2
    g = torch.Generator().manual_seed(5)
    bn, conv = nn.BatchNorm3d(C), nn.Conv3d(C, cout, 3, 1, 1)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(C, generator=g))
        bn.bias.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_var.copy_(1 + 0.2 * torch.rand(C, generator=g))
    bn.train(training)
    bn, conv = bn.to(DEV), conv.to(DEV)
    bn2 = copy.deepcopy(bn)                                     # the pieces update their own running statistics
    x = (torch.randn((B, h, w, d, C), generator=g) + 0.3).to(DEV, BF16).requires_grad_(True)
    dy = torch.randn((B, 2 * h, 2 * w, 2 * d, cout), generator=g).to(DEV)
    out = Fn.uphead(bn, conv, x)
    out.backward(dy)
    Fn.flush_counters()

    xd = x.detach()
    gx = None
    if training:
        part, gx_direct = run_stats(L, xd, True)
        scale, shift, mean_rstd, gx = ops.uphead_batch_stats(
            xd, bn2.weight.detach().float().contiguous(), bn2.bias.detach().float().contiguous(), bn2.eps, bn2.running_mean,
            bn2.running_var, Fn.bn_momentum(bn2), True)
        assert same_bits(gx, gx_direct)
        assert same_bits(bn.running_mean, bn2.running_mean) and same_bits(bn.running_var, bn2.running_var)
    else:
        scale, shift, mean_rstd = ops.bn_eval_affine(bn2.weight.detach(), bn2.bias.detach(), bn2.running_mean, bn2.running_var, bn2.eps)
    y = ops.uphead_forward(xd, ops.uphead_fold(conv.weight, scale, shift), conv.bias, cout)
    assert same_bits(out.detach(), y)
    G, S, D = ops.uphead_gs(xd, dy, cout, keep_d=True, raw=True)
    assert same_bits(D, run_adjoint(L, dy, (B, h, w, d), cout, 64))
    dW, db, dgamma, dbeta = ops.head_grads_fused(G, S, conv.weight, scale, shift, mean_rstd)
    dx = ops.uphead_dx(xd, D, conv.weight, scale, mean_rstd, dgamma, dbeta, training, gx)
    torch.cuda.synchronize()
    assert same_bits(conv.weight.grad, dW) and same_bits(conv.bias.grad, db)
    assert same_bits(bn.weight.grad, dgamma) and same_bits(bn.bias.grad, dbeta)
    assert same_bits(x.grad, dx)
    assert bool(torch.isfinite(dx.float()).all()) and float(dx.float().abs().max()) > 0
