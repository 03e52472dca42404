"""Direct located parity tests of the encoder's down-sampling path against tests/merge_ref.py (float64, CPU):
mivp_patch_embed, mivp_patch_im2col, mivp_patch_merge_fwd, mivp_patch_merge_bwd and mivp_ln_wgrad, each called through
``_lib.call`` on its own operands with hand-filled descriptors, NaN-prefilled outputs and guard tails.

Kinds of assertion (derivations in the header of tests/merge_ref.py and tests/tok_ref.py; no bar is measured):
  exact     patch_embed with integer operands: the per-channel sums of ``part`` and the bf16 output equal float64; im2col equals
            the bf16 rounding of the float64 relayout; wg_x is the gathered rows; wg_dn = dy W for integer dy and W; dbeta for
            integer dn; tokens that gather identical rows give bit-identical y rows; -2 rows of n_out are +0, -1 rows bf16(beta);
            dx has the same bits with and without the weight-gradient outputs; every output element is written, no guard is touched
  interval  y: kC u sum |a||W| + sum D |W|;  wg_dn: Cout u sum |dy||W|;  n_out: the ``ln`` interval
  derived   dgamma: T u sum |dn||xhat| + sum |dn| dxh
  err32     dx (LayerNorm backward cancels): within (8 err32 + 2^-22) max |ref| of float64
  refusal   the error code, every output untouched

The arm each case selects is restated from the launchers in merge_ref.merge_fwd_arm / merge_bwd_arm / embed_arm, asserted on the
case and part of the test id."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_ref as M  # noqa: E402
from test_hip_prompt_path import DEV, Out, assert_same_bits, bits, dev  # noqa: E402
from test_hip_tok_kernels import margin, subset_rows  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import ops

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EINVAL, EUNSUPPORTED = r"failed with code -1", r"failed with code -2"


def dims_id(dims):
    return "x".join(str(v) for v in dims)


# =============================================================================================
# mivp_patch_embed
# =============================================================================================
def embed_desc(B, Cin, dims, Cc, nblk):
    d = L.EmbedDesc()
    d.B, d.Cin, d.C, d.nblk = B, Cin, Cc, nblk
    for a in range(3):
        d.dims[a] = dims[a]
    return d


EMBED = [(c, pin, mode) for c in M.EMBED_CASES for pin in ("smallest", "wrapper") for mode in (0, 1)]


@pytest.mark.parametrize("case,pin,mode", EMBED,
                         ids=[f"{M.embed_arm(c[1], m)}-B{c[0]}_{dims_id(c[2])}_C{c[3]}_nblk_{p}" for c, p, m in EMBED])
def test_patch_embed_exact(case, pin, mode):
    B, Cin, dims, Cc = case
    n_out, G = B * math.prod(dims) // 8, Cc // 8
    nblk = M.smallest_nblk(Cc) if pin == "smallest" else ops._nblk(n_out * G, G, cap=2048)
    assert (nblk * 256) % G == 0 and (pin == "wrapper" or nblk == (3 if Cc == 48 else 1))
    if pin == "smallest" and n_out >= 2000:
        assert n_out * G > 8 * nblk * 256                                # the grid-stride walk runs many rounds
    p = M.embed_exact(*case)
    M.assert_exact_inputs((p.sums, p.y), (p.b_sums, p.b_y), (False, True), f"patch_embed {case}")
    d = embed_desc(B, Cin, dims, Cc, nblk)
    x, w, bias = dev(p.x), dev(p.w), dev(p.bias)
    what = f"patch_embed {M.embed_arm(Cin, mode)} B={B} Cin={Cin} dims={dims} C={Cc} nblk={nblk}"
    if mode == 0:
        part = Out((nblk, 2 * Cc))
        L.call("mivp_patch_embed", C.byref(d), 0, L.ptr(x), L.ptr(w), L.ptr(bias), None, None, L.ptr(part.t), None, L.stream())
        torch.cuda.synchronize()
        got = part.done(what).to(F64)
        assert torch.equal(got, got.round()), what + ": a partial sum of integers is no integer"
        M.assert_equal_located(got.sum(0), p.sums, "c", what + " (sum | sum of squares per channel)")
    else:
        y = Out((B, dims[0] // 2, dims[1] // 2, dims[2] // 2, Cc), BF16)
        scale, shift = dev(p.scale), dev(p.shift)                        # (named: an unnamed temporary is freed before the launch)
        L.call("mivp_patch_embed", C.byref(d), 1, L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(scale), L.ptr(shift), None, L.ptr(y.t),
               L.stream())
        torch.cuda.synchronize()
        M.assert_equal_located(y.done(what), p.y, "bhwdc", what)


@pytest.mark.parametrize("dims,nblk,why", [((6, 10, 13), 3, "odd_dim"), ((6, 10, 14), 1, "nblk_breaks_group_rule"),
                                           ((6, 10, 14), 4, "nblk_breaks_group_rule")])
def test_patch_embed_refusals(dims, nblk, why):
    B, Cin, Cc = 1, 4, 48
    assert (why == "odd_dim") == any(n & 1 for n in dims) and (why == "odd_dim") == ((nblk * 256) % (Cc // 8) == 0)
    g = torch.Generator().manual_seed(1)
    x = dev(torch.randn((B, Cin, *dims), generator=g))
    w, v = dev(torch.randn((Cc, Cin, 2, 2, 2), generator=g)), dev(torch.randn(Cc, generator=g))
    d = embed_desc(B, Cin, dims, Cc, nblk)
    part, y = Out((nblk, 2 * Cc)), Out((B, dims[0] // 2, dims[1] // 2, (dims[2] + 1) // 2, Cc), BF16)
    with pytest.raises(RuntimeError, match=EINVAL):
        L.call("mivp_patch_embed", C.byref(d), 0, L.ptr(x), L.ptr(w), L.ptr(v), None, None, L.ptr(part.t), None, L.stream())
    with pytest.raises(RuntimeError, match=EINVAL):
        L.call("mivp_patch_embed", C.byref(d), 1, L.ptr(x), L.ptr(w), L.ptr(v), L.ptr(v), L.ptr(v), None, L.ptr(y.t), L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(part.flat).all()) and bool(torch.isnan(y.flat).all()), "a refused call wrote to its output"


# =============================================================================================
# mivp_patch_im2col
# =============================================================================================
IM2COL = [(1, 1, (2, 2, 2)), (2, 4, (6, 10, 14)), (1, 3, (4, 6, 8)), (1, 4, (96, 96, 118))]


@pytest.mark.parametrize("B,Cin,dims", IM2COL, ids=[f"B{b}_Cin{c}_{dims_id(d)}" for b, c, d in IM2COL])
def test_patch_im2col_bit_equal(B, Cin, dims):
    n_out = B * math.prod(dims) // 8
    if dims == (96, 96, 118):
        assert n_out * Cin * 4 > 8192 * 256                               # beyond the grid cap: the stride loop runs
    g = torch.Generator().manual_seed(n_out)
    x = torch.randn((B, Cin, *dims), generator=g, dtype=F32) * torch.exp2(torch.randint(-20, 20, (B, Cin, *dims), generator=g).float())
    d = embed_desc(B, Cin, dims, 8, 1)
    p = Out((n_out, Cin * 8), BF16)
    x_d = dev(x)
    L.call("mivp_patch_im2col", C.byref(d), L.ptr(x_d), L.ptr(p.t), L.stream())
    torch.cuda.synchronize()
    what = f"patch_im2col B={B} Cin={Cin} dims={dims} [token][ci*8 + a*4 + b*2 + c]"
    M.check_bits_equal(p.done(what), M.stored(M.im2col(x.to(F64))), what)


# =============================================================================================
# mivp_patch_merge_fwd
# =============================================================================================
def merge_desc(B, dims, Cc, Cout, merge_last):
    d = L.MergeDesc()
    d.B, d.C, d.Cout, d.merge_last, d.ln_eps = B, Cc, Cout, 1 if merge_last else 0, 1e-6
    od = M.merge_odims(dims, merge_last)
    for a in range(3):
        d.dims[a], d.odims[a] = dims[a], od[a]
    assert M.f32_of(d.ln_eps) == M.LN_EPS
    return d


def twin_tokens(B, dims, merge_last):
    """Token 0 (in every front pad there is), an interior token, a token of another workgroup (and batch), the last live one."""
    oh, ow, od = M.merge_odims(dims, merge_last)
    T = B * oh * ow * od
    inner = (min(1, oh - 1) * ow + min(1, ow - 1)) * od + min(1, od - 1)
    far = (B - 1) * oh * ow * od + inner + (od if ow > 2 else 0)
    toks = [0, inner, T // 2 + 1, far, T - 1]
    return list(dict.fromkeys(t for t in toks if 0 <= t < T))


PAR = [(6 + (p >> 2 & 1), 4 + (p >> 1 & 1), 4 + (p & 1)) for p in range(8)]
# (B, dims, C, Cout, merge_last, offset)
FWD = ([(1, (5, 6, 4), 8, 16, False, 0.0), (1, (5, 6, 4), 8, 16, True, 0.0), (1, (5, 6, 4), 16, 32, True, 0.0),
        (1, (5, 6, 4), 24, 48, True, 0.0), (1, (5, 6, 4), 32, 64, True, 0.0), (1, (5, 6, 4), 48, 96, True, 0.0),
        (1, (5, 6, 4), 96, 192, True, 0.0), (1, (5, 6, 5), 192, 384, False, 0.0), (1, (5, 6, 5), 48, 96, False, 0.0)]
       + [(1, d, 48, 96, True, 0.0) for d in PAR] + [(1, d, 96, 192, False, 0.0) for d in PAR]
       + [(1, (13, 18, 2), 8, 20, True, 0.0),                              # T = 63, Cout % 16 = 4
          (1, (10, 25, 2), 48, 100, True, 0.0),                            # T = 65: a dead tail of 63 rows with the n0 < Cout tail
          (1, (42, 38, 30), 48, 100, True, 0.0),                           # T % 64 = 33, one workgroup row owns all seven tiles
          (2, (40, 40, 32), 48, 96, True, 0.0),                            # 12800 tokens
          (2, (64, 64, 32), 48, 96, True, 0.0),                            # gx = 512
          (1, (80, 80, 4), 192, 384, False, 0.0),                          # KS 24 with twelve tiles per workgroup
          (1, (7, 5, 5), 48, 96, True, 2.0)])                              # rows about 2 sigma off zero


def fwd_id(c):
    ks, ny, per_y = M.merge_fwd_arm(*c[:5])
    return f"KS{ks}_ny{ny}_pery{per_y}-B{c[0]}_{dims_id(c[1])}_C{c[2]}_Cout{c[3]}_last{int(c[4])}" + ("_offset" if c[5] else "")


@pytest.mark.parametrize("case", FWD, ids=[fwd_id(c) for c in FWD])
def test_patch_merge_fwd(case):
    B, dims, Cc, Cout, last, offset = case
    ks, ny, per_y = M.merge_fwd_arm(B, dims, Cc, Cout, last)
    kC = (8 if last else 4) * Cc
    assert ks == kC // 32
    pinned = {(2, (40, 40, 32)): (12, 2, 3), (2, (64, 64, 32)): (12, 1, 6), (1, (80, 80, 4)): (24, 2, 12), (1, (42, 38, 30)): (12, 1, 7)}
    if (B, dims) in pinned:
        assert (ks, ny, per_y) == pinned[(B, dims)]                        # the slab loop: three or more tiles per workgroup
    T = M.merge_tokens(B, dims, last)
    if dims in ((13, 18, 2), (10, 25, 2), (42, 38, 30)):
        assert T % 64 in (63, 1, 33) and Cout % 16 == 4
    o = M.merge_operands(B, dims, Cc, Cout, last, seed=Cc + Cout + sum(dims), offset=offset)
    twins = twin_tokens(B, dims, last)
    M.plant_twins(o.x, last, twins)
    d = merge_desc(B, dims, Cc, Cout, last)
    what = f"patch_merge_fwd KS={ks} ny={ny} per_y={per_y} B={B} dims={dims} C={Cc} Cout={Cout} merge_last={last}"
    y = Out((T, Cout), BF16)
    ins = [dev(o.x, BF16), dev(o.ln_w), dev(o.ln_b), dev(o.W, BF16)]
    L.call("mivp_patch_merge_fwd", C.byref(d), L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(ins[2]), L.ptr(ins[3]), L.ptr(y.t), L.stream())
    torch.cuda.synchronize()
    got = y.done(what)                                                    # every live row written, the guard untouched
    rows = torch.unique(torch.cat([subset_rows(T), torch.arange(max(0, T - 64), T), torch.tensor(twins)]))
    ref = M.merge_fwd(o.x, o.ln_w, o.ln_b, o.W, last, tokens=rows)
    at = {int(t): i for i, t in enumerate(rows)}
    if len(twins) > 2:
        assert len({t // 64 for t in twins}) > 1 or T <= 64               # more than one workgroup where there is more than one
    for t in twins[1:]:
        assert torch.equal(ref.rows[at[t]], ref.rows[at[twins[0]]])
        assert_same_bits(got[t], got[twins[0]], f"{what}: token {t} gathers the row of token {twins[0]}")
    assert bool((ref.inv[at[0]] < 0).any()) == any(n & 1 for n in dims)   # token 0 sits in the front pad of every odd axis
    m =M.check_interval(got[rows], ref.y, ref.bound, what + " y [row of the compared subset][channel]; subset rows: "
                         + ("all" if rows.numel() == T else "subset_rows, the last 64, the twins"))
    margin("patch_merge_fwd", f"KS{ks} ny{ny} per_y{per_y}" + (" offset" if offset else ""), y=m)


@pytest.mark.parametrize("Cc,last,ks", [(192, True, 48), (24, False, 3)])
def test_patch_merge_fwd_refusals(Cc, last, ks):
    B, dims, Cout = 1, (6, 4, 4), 2 * Cc
    assert M.merge_fwd_arm(B, dims, Cc, Cout, last)[0] is None and ((8 if last else 4) * Cc + 31) // 32 == ks
    o = M.merge_operands(B, dims, Cc, Cout, last, seed=1)
    y = Out((M.merge_tokens(B, dims, last), Cout), BF16)
    d, ins = merge_desc(B, dims, Cc, Cout, last), [dev(o.x, BF16), dev(o.ln_w), dev(o.ln_b), dev(o.W, BF16)]
    with pytest.raises(RuntimeError, match=EUNSUPPORTED):
        L.call("mivp_patch_merge_fwd", C.byref(d), L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(ins[2]), L.ptr(ins[3]), L.ptr(y.t), L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.flat).all()), "a refused call wrote to y"


# =============================================================================================
# mivp_patch_merge_bwd
# =============================================================================================
def bwd_id(c):
    ns, ny, per_y = M.merge_bwd_arm(*c[:5])
    kC = (8 if c[4] else 4) * c[2]
    cap = "cap" if ny == max(1, ((kC + 15) // 16) // 3) else "below"
    return (f"NS{ns}_ny{ny}{cap}_pery{per_y}-B{c[0]}_{dims_id(c[1])}_C{c[2]}_Cout{c[3]}_last{int(c[4])}"
            + ("_offset" if c[5] else "") + ("_zerorow" if c[6] is not None else ""))


def done_volume(out, what):
    """Out.done for a [b][h][w][d][c] volume, naming the voxels that were never written."""
    flat = out.flat.cpu()
    assert bool(torch.isnan(flat[out.n:]).all()), f"{what}: the kernel wrote behind its output buffer"
    got = flat[:out.n].view(out.t.shape)
    bad = torch.isnan(got).any(-1)
    if bool(bad.any()):
        where = [tuple(int(i) for i in row) for row in torch.nonzero(bad)]
        raise M.Located(f"{what}: {len(where)} of {bad.numel()} voxels were never written (or are NaN); first (b, h, w, d): "
                        f"{where[:8]}", where)
    return got


def run_merge_bwd(d, ins, shape, T, kC, wgrad, what):
    dx = Out(shape, BF16)
    wg_dn, wg_x = (Out((T, kC), BF16), Out((T, kC), BF16)) if wgrad else (None, None)
    dy, x, yfwd, lnw, lnb, wgam, wbet, w_t = (L.ptr(t) for t in ins)
    L.call("mivp_patch_merge_bwd", C.byref(d), dy, x, yfwd, lnw, lnb, wgam, wbet, w_t, L.ptr(dx.t), L.ptr(wg_dn.t) if wgrad else None,
           L.ptr(wg_x.t) if wgrad else None, L.stream())
    torch.cuda.synchronize()
    dxv = done_volume(dx, what + " dx")                                   # no NaN left: every voxel written, odd shapes included
    return (dxv, wg_dn.done(what + " wg_dn"), wg_x.done(what + " wg_x")) if wgrad else (dxv, None, None)


@pytest.mark.parametrize("case", M.BWD_CASES, ids=[bwd_id(c) for c in M.BWD_CASES])
def test_patch_merge_bwd(case):
    B, dims, Cc, Cout, last, offset, zero_token = case
    ns, ny, per_y = M.merge_bwd_arm(B, dims, Cc, Cout, last)
    kC = (8 if last else 4) * Cc
    assert ns == (Cout + 31) // 32
    if (B, dims) == (2, (40, 40, 32)):
        assert (ny, per_y) == (6, 4) and ny < (kC // 16) // 3
    if Cc == 8:
        assert ny == 1
    T = M.merge_tokens(B, dims, last)
    o = M.merge_operands(B, dims, Cc, Cout, last, seed=5 + Cc + Cout + sum(dims), offset=offset, zero_token=zero_token)
    f = M.merge_fwd(o.x, o.ln_w, o.ln_b, o.W, last)
    yfwd = M.bf16_rne(f.y)                                                # the float64 forward, stored: no forward kernel involved
    wgam, wbet = M.merge_wvec(o.W, o.ln_w, o.ln_b)
    if zero_token is not None:
        assert float(f.rstd[zero_token]) == M.LN_EPS ** -0.5 and not bool(f.rows[zero_token].any())
    args = (o.dy, o.x, yfwd, o.ln_w, wgam, wbet, o.W, last)
    r64, r32 = M.merge_bwd(*args), M.merge_bwd(*args, dt=F32, rnd=M.bf16_f32)
    d = merge_desc(B, dims, Cc, Cout, last)
    what = f"patch_merge_bwd NS={ns} ny={ny} per_y={per_y} B={B} dims={dims} C={Cc} Cout={Cout} merge_last={last}"
    x_d, lnw, lnb = dev(o.x, BF16), dev(o.ln_w), dev(o.ln_b)
    ins = [dev(o.dy, BF16), x_d, dev(yfwd, BF16), lnw, lnb, dev(wgam), dev(wbet), dev(o.W.t(), BF16)]
    dx, wg_dn, wg_x = run_merge_bwd(d, ins, tuple(o.x.shape), T, kC, True, what)
    M.check_bits_equal(wg_x, M.stored(r64.wg_x), what + " wg_x [token][concat channel]: the gathered rows")
    m = {"wg_dn": M.check_interval(wg_dn, r64.wg_dn, r64.b_dn, what + " wg_dn [token][concat channel]")}
    m["dx"], err32 = M.check_err32(dx, r64.dx, r32.dx, what + " dx [b][h][w][d][channel]")
    dx2, _, _ = run_merge_bwd(d, ins, tuple(o.x.shape), T, kC, False, what + " without wg_*")
    M.check_bits_equal(dx2, dx, what + " dx with wg_dn / wg_x NULL against present")
    # wg_dn = dy W, exact: integer dy and W (yfwd, wgam, wbet play no part in wg_dn)
    p = M.bwd_exact(B, dims, Cc, Cout, last)
    M.assert_exact_inputs(p.wg_dn, p.b_dn, True, what + " wg_dn, integer operands")
    zeros = torch.zeros(Cout, dtype=F32, device=DEV)
    ins = [dev(p.dy, BF16), x_d, torch.zeros((T, Cout), dtype=BF16, device=DEV), lnw, lnb, zeros, zeros, dev(p.W.t(), BF16)]
    _, wg_dn, wg_x = run_merge_bwd(d, ins, tuple(o.x.shape), T, kC, True, what + " integer operands")
    M.assert_equal_located(wg_dn, p.wg_dn, "tc", what + " wg_dn = dy W on integers [token][concat channel]")
    M.check_bits_equal(wg_x, M.stored(r64.wg_x), what + " wg_x, second call")
    margin("patch_merge_bwd", f"NS{ns} ny{ny} per_y{per_y}" + (" offset" if offset else "") + (" zero row" if zero_token is not None else ""),
           err32_e6=err32 * 1e6, **m)


# =============================================================================================
# mivp_ln_wgrad
# =============================================================================================
def run_ln_wgrad(x_d, src_d, dn_d, T, Cc, Nqp, P, vol, gamma, beta, nblk, what):
    stats = torch.empty((T, 2), dtype=F32, device=DEV)
    n, part = Out((T, Cc), BF16), Out((nblk, 2 * Cc))
    gamma_d, beta_d = dev(gamma), dev(beta)
    L.call("mivp_ln_wgrad", L.ptr(x_d), L.ptr(src_d), L.ptr(dn_d), T, Cc, Nqp, P, vol, M.LN_EPS, L.ptr(gamma_d), L.ptr(beta_d),
           L.ptr(stats), L.ptr(n.t), nblk, L.ptr(part.t), L.stream())
    torch.cuda.synchronize()
    return n.done(what + " n_out"), part.done(what + " part").to(F64).sum(0)


def check_ln_wgrad(x, src, dn, gamma, beta, B, T, Cc, Nqp, P, vol, arm):
    ref = M.ln_wgrad(x, src, dn, gamma, beta, M.LN_EPS, B=B)
    assert float(ref.b_dbeta.max()) < 2 ** 24                             # integer dn: dbeta is exact in any order
    x_d, dn_d = dev(x, BF16), dev(dn, BF16)
    src_d = None if src is None else src.to(torch.int32).to(DEV)
    G = Cc // 8
    for pin, nblk in (("smallest", M.smallest_nblk(Cc)), ("wrapper", ops._nblk(T * G, G))):
        what = f"ln_wgrad {arm} T={T} C={Cc} nblk={nblk} ({pin})"
        n, sums = run_ln_wgrad(x_d, src_d, dn_d, T, Cc, Nqp, P, vol, gamma, beta, nblk, what)
        m = {"n": M.check_interval(n, ref.n, ref.width, what + " n_out [row][channel]")}
        if src is not None:
            flat = src.repeat(B, 1).reshape(-1)
            assert not bool(bits(n)[flat == -2].any()), what + ": rows of padding slots (-2) are +0 bits"
            zero = torch.nonzero(flat == -1).reshape(-1)
            assert zero.numel() >= 2
            M.check_bits_equal(n[zero], M.stored(beta).expand(zero.numel(), Cc).contiguous(), what + " rows with source -1 = bf16(beta)")
        M.assert_equal_located(sums[:Cc], ref.dbeta, "c", what + " dbeta")
        bad = ~((sums[Cc:] - ref.dgamma).abs() <= ref.b_dgamma)
        assert not bool(bad.any()), (f"{what} dgamma leaves its bound at channels {torch.nonzero(bad).reshape(-1).tolist()[:8]}: got "
                                     f"{sums[Cc:][bad][:4].tolist()}, float64 {ref.dgamma[bad][:4].tolist()}, bound {ref.b_dgamma[bad][:4].tolist()}")
        m["dgamma"] = float(((sums[Cc:] - ref.dgamma).abs() / ref.b_dgamma.clamp(min=1e-300)).max())
        margin("ln_wgrad", f"{arm} C{Cc} T{T} nblk {pin}", **m)


@pytest.mark.parametrize("T", [1, 15, 17, 4097])
@pytest.mark.parametrize("Cc", [8, 48, 384, 768])
def test_ln_wgrad_direct(Cc, T):
    g = torch.Generator().manual_seed(Cc + T)
    x = M.randn_bf16(g, T, Cc, scale=0.8, shift=0.4)
    gamma = (torch.randn(Cc, generator=g, dtype=F32) * 0.2 + 1.0).to(F64)
    beta = (torch.randn(Cc, generator=g, dtype=F32) * 0.1).to(F64)
    dn = M.draw(g, (T, Cc), range(-3, 4))
    check_ln_wgrad(x, None, dn, gamma, beta, 1, T, Cc, 0, 0, 0, "direct")


@pytest.mark.parametrize("Cc,P,Nq", [(8, 3, 13), (48, 5, 29), (384, 2, 13)])
def test_ln_wgrad_gathered(Cc, P, Nq):
    B = 2
    vol = P * Nq + 11
    src, _ = M.make_tables(P, Nq, vol, 7 + Cc, dup=False)
    Nqp = src.shape[1]
    T = B * P * Nqp
    assert bool((src == -1).any()) and bool((src == -2).any())
    g = torch.Generator().manual_seed(Cc + P)
    x = M.randn_bf16(g, B, vol, Cc, scale=0.8, shift=0.4)
    unread = torch.ones(vol, dtype=torch.bool)
    unread[src[src >= 0]] = False
    assert bool(unread.any())
    x[:, unread] = float("nan")                                           # voxels no source names are never read
    assert not torch.equal(torch.nan_to_num(x[0]), torch.nan_to_num(x[1]))   # the batch stride vol matters
    gamma = (torch.randn(Cc, generator=g, dtype=F32) * 0.2 + 1.0).to(F64)
    beta = (torch.randn(Cc, generator=g, dtype=F32) * 0.1).to(F64)
    dn = M.draw(g, (T, Cc), range(-3, 4))
    dn[(src == -2).repeat(B, 1).reshape(-1)] = float("nan")              # dn of a padding slot is never read
    check_ln_wgrad(x, src, dn, gamma, beta, B, T, Cc, Nqp, P, vol, "gathered")
