"""Guards of tests/merge_ref.py, the float64 restatement behind tests/test_hip_merge_embed.py.  CPU only.

* merge_fwd without rounding is oracle.swin_ref.patch_merge on all eight (H, W, D) parities, merged and unmerged D;
* merge_bwd with the exact y equals autograd of that oracle function for dx, and wg_dn / wg_x reproduce autograd's dW, dgamma and
  dbeta through ln_wgrad and a plain matmul;
* ln_wgrad equals autograd of F.layer_norm on a table that holds -1 and -2 entries;
* embed_conv and im2col agree with F.conv3d and its weight gradient;
* every exact case of the GPU file meets conditions (a) and (b) of tests/exact_ref.py on all of its elements;
* an f32 / bf16 emulation of dx and of n (other summation trees than merge_ref's own emulation) passes the err32 / interval rule,
  the rows about 2 sigma off zero included; the dispatch restatements give the arms the GPU ids name."""
import os
import sys

import pytest
import torch
import torch.nn.functional as Fnn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_ref as M  # noqa: E402
from oracle import swin_ref as S  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
PARITIES = [(6 + (p >> 2 & 1), 4 + (p >> 1 & 1), 4 + (p & 1)) for p in range(8)]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def oracle_merge(x, o, merge_last):
    """oracle.swin_ref.patch_merge on channels-last x -> [T, Cout]."""
    sd = {"m.norm.weight": o.ln_w, "m.norm.bias": o.ln_b, "m.reduction.weight": o.W}
    y = S.patch_merge(x.permute(0, 4, 1, 2, 3), sd, "m.", merge_last)
    return y.permute(0, 2, 3, 4, 1).reshape(-1, o.W.shape[0])


@pytest.mark.parametrize("merge_last", [True, False])
@pytest.mark.parametrize("dims", PARITIES, ids=lambda d: "x".join(map(str, d)))
def test_merge_fwd_is_the_oracle(dims, merge_last):
    o = M.merge_operands(2, dims, 8, 24, merge_last, seed=sum(dims))
    f = M.merge_fwd(o.x, o.ln_w, o.ln_b, o.W, merge_last, eps=1e-6, rnd=M.ident)
    assert f.y.shape[0] == M.merge_tokens(2, dims, merge_last)
    assert rel(f.y, oracle_merge(o.x, o, merge_last)) < 1e-12
    pads = int((f.inv < 0).sum())
    assert (pads > 0) == any(n & 1 for n in dims)                         # the front pad is there exactly on odd shapes
    assert not bool(f.rows.reshape(f.inv.shape[0], f.inv.shape[1], -1)[f.inv < 0].any())


@pytest.mark.parametrize("merge_last", [True, False])
@pytest.mark.parametrize("dims", [PARITIES[0], PARITIES[7], PARITIES[2]], ids=lambda d: "x".join(map(str, d)))
def test_merge_bwd_with_exact_y_is_autograd(dims, merge_last):
    o = M.merge_operands(2, dims, 8, 24, merge_last, seed=3 + sum(dims))
    x = o.x.clone().requires_grad_(True)
    p = M.SimpleNamespace(ln_w=o.ln_w.clone().requires_grad_(True), ln_b=o.ln_b.clone().requires_grad_(True),
                          W=o.W.clone().requires_grad_(True))
    y = oracle_merge(x, p, merge_last)
    (y * o.dy).sum().backward()
    wgam, wbet = o.W @ o.ln_w, o.W @ o.ln_b                               # exact vectors, exact y
    b = M.merge_bwd(o.dy, o.x, y.detach(), o.ln_w, wgam, wbet, o.W, merge_last, eps=1e-6, rnd=M.ident)
    assert not bool(torch.isnan(b.dx).any())                              # every voxel is written
    assert rel(b.dx, x.grad) < 1e-11
    # the two weight-gradient operands: LayerNorm parameter gradients and dW through ln_wgrad and a plain matmul
    g = M.ln_wgrad(b.wg_x, None, b.wg_dn, o.ln_w, o.ln_b, 1e-6, rnd=M.ident)
    assert rel(g.dgamma, p.ln_w.grad) < 1e-11 and rel(g.dbeta, p.ln_b.grad) < 1e-11
    assert rel(o.dy.t() @ g.n, p.W.grad) < 1e-11


@pytest.mark.parametrize("C", [8, 48])
def test_ln_wgrad_is_autograd_with_negative_codes(C):
    B, P, Nq = 2, 3, 13
    vol = P * Nq + 11
    src, _ = M.make_tables(P, Nq, vol, 5, dup=False)
    assert bool((src == -1).any()) and bool((src == -2).any())
    g = torch.Generator().manual_seed(C)
    x = M.randn_bf16(g, B, vol, C, scale=0.8, shift=0.1)
    gamma = torch.randn(C, generator=g, dtype=F64) * 0.2 + 1.0
    beta = torch.randn(C, generator=g, dtype=F64) * 0.1
    dn = M.draw(g, (B * P * src.shape[1], C), range(-3, 4))
    dn_nan = dn.clone()
    dn_nan[(src == -2).repeat(B, 1).reshape(-1)] = float("nan")          # never read
    r = M.ln_wgrad(x, src, dn_nan, gamma, beta, 1e-6, B=B, rnd=M.ident)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rows = M.gather_rows(x, src, B).reshape(-1, C)
    n = Fnn.layer_norm(rows, (C,), gm, bt, 1e-6)
    live = ~r.pad
    (n[live] * dn[live]).sum().backward()
    assert rel(r.n[live], n[live].detach()) < 1e-12
    assert not bool(r.n[r.pad].any())
    zero = (src == -1).repeat(B, 1).reshape(-1)
    assert torch.equal(r.n[zero], beta.expand(int(zero.sum()), C))        # a zero row: n = beta, exactly
    assert rel(r.dgamma, gm.grad) < 1e-12 and rel(r.dbeta, bt.grad) < 1e-12
    assert bool((r.b_dgamma > 0).all()) and bool(torch.isfinite(r.b_dgamma).all())


@pytest.mark.parametrize("Cin", [1, 4])
def test_embed_conv_and_im2col_against_conv3d(Cin):
    g = torch.Generator().manual_seed(Cin)
    B, dims, C = 2, (4, 6, 8), 16
    x = torch.randn((B, Cin, *dims), generator=g, dtype=F64)
    w = torch.randn((C, Cin, 2, 2, 2), generator=g, dtype=F64, requires_grad=True)
    bias = torch.randn(C, generator=g, dtype=F64)
    conv, bound = M.embed_conv(x, w.detach(), bias)
    p = M.im2col(x)
    assert p.shape == (B * 2 * 3 * 4, Cin * 8)
    assert rel((p @ w.detach().reshape(C, -1).t() + bias).reshape(conv.shape), conv) < 1e-13
    assert bool((conv.abs() <= bound + 1e-12).all())
    dz = torch.randn(conv.shape, generator=g, dtype=F64)
    (Fnn.conv3d(x, w, bias, stride=2).permute(0, 2, 3, 4, 1) * dz).sum().backward()
    assert rel((dz.reshape(-1, C).t() @ p).reshape(w.shape), w.grad) < 1e-13
    s, _ = M.embed_stats(conv, bound)
    assert rel(s[:C], conv.reshape(-1, C).sum(0)) < 1e-13 and rel(s[C:], (conv ** 2).reshape(-1, C).sum(0)) < 1e-13


# =============================================================================================
# conditions (a) and (b) of every exact GPU case, on the reference alone
# =============================================================================================
@pytest.mark.parametrize("case", M.EMBED_CASES, ids=lambda c: f"B{c[0]}_Cin{c[1]}_{'x'.join(map(str, c[2]))}_C{c[3]}")
def test_embed_exact_cases_meet_the_conditions(case):
    p = M.embed_exact(*case)
    M.assert_exact_inputs((p.sums, p.y), (p.b_sums, p.b_y), (False, True), f"patch_embed {case}")
    assert bool(p.conv.abs().sum() > 0) or case[2] == (2, 2, 2)           # not a degenerate all-zero draw
    assert bool(((p.scale == 0.5) | (p.scale == 1.0) | (p.scale == 2.0)).all())


@pytest.mark.parametrize("case", M.BWD_CASES, ids=lambda c: f"B{c[0]}_{'x'.join(map(str, c[1]))}_C{c[2]}_Cout{c[3]}_last{int(c[4])}")
def test_merge_bwd_exact_cases_meet_the_conditions(case):
    p = M.bwd_exact(*case[:5])
    M.assert_exact_inputs(p.wg_dn, p.b_dn, True, f"patch_merge_bwd wg_dn {case}")
    assert float(p.wg_dn.abs().max()) > 8                                 # the integers are not trivially small


def test_dispatch_restatements_reach_the_named_arms():
    assert M.merge_fwd_arm(2, (40, 40, 32), 48, 96, True) == (12, 2, 3)
    assert M.merge_fwd_arm(2, (64, 64, 32), 48, 96, True) == (12, 1, 6)
    assert M.merge_fwd_arm(1, (80, 80, 4), 192, 384, False) == (24, 2, 12)
    assert M.merge_fwd_arm(1, (6, 5, 4), 192, 384, True)[0] is None and M.merge_fwd_arm(1, (6, 5, 4), 24, 48, False)[0] is None
    assert [M.merge_bwd_arm(1, (6, 5, 4), 48, co, True)[0] for co in (16, 64, 96, 128, 192, 384)] == [1, 2, 3, 4, 6, 12]
    assert M.merge_bwd_arm(1, (6, 5, 4), 48, 96, True)[1:] == (8, 3)                  # ny at its cap n_ct / 3
    assert M.merge_bwd_arm(2, (40, 40, 32), 48, 96, True)[1:] == (6, 4)               # below the cap
    assert M.merge_bwd_arm(2, (9, 6, 3), 8, 16, False)[1:] == (1, 2)
    assert M.smallest_nblk(48) == 3 and M.smallest_nblk(8) == 1


# =============================================================================================
# the reference alone passes its own rules
# =============================================================================================
def _tree32(rows, parts):
    """An f32 row sum through ``parts`` interleaved partial sums (another summation tree than torch's)."""
    T, K = rows.shape
    return rows.reshape(T, K // parts, parts).sum(1).sum(-1, keepdim=True)


@pytest.mark.parametrize("offset", [0.0, 2.0])
@pytest.mark.parametrize("merge_last,C,Cout", [(True, 48, 96), (False, 96, 192)])
def test_f32_emulation_of_dx_stays_inside_err32(merge_last, C, Cout, offset):
    dims = (7, 5, 5)
    o = M.merge_operands(1, dims, C, Cout, merge_last, seed=11, offset=offset)
    f = M.merge_fwd(o.x, o.ln_w, o.ln_b, o.W, merge_last)
    yfwd = M.bf16_rne(f.y)
    wgam, wbet = M.merge_wvec(o.W, o.ln_w, o.ln_b)
    args = (o.dy, o.x, yfwd, o.ln_w, wgam, wbet, o.W, merge_last)
    r64, r32 = M.merge_bwd(*args), M.merge_bwd(*args, dt=F32, rnd=M.bf16_f32)
    if offset:
        assert float((f.mean.abs() * f.rstd).max()) > 1.5                 # rows without pad parts: a mean far from zero
    # another f32 evaluation: four-lane one-pass statistics, dYn from a float64 GEMM rounded once to f32
    rows = r32.wg_x
    kC = rows.shape[-1]
    mean = _tree32(rows, 4) / kC
    var = (_tree32(rows * rows, 4) / kC - mean * mean).clamp(min=0)
    rstd = (var + M.LN_EPS) ** -0.5
    dYn = r64.wg_dn.to(F32)
    alt = rstd * (dYn * o.ln_w.to(F32) - r32.m1 - (rows - mean) * rstd * r32.m2)
    alt = M.merge_scatter(alt, r64.inv, tuple(o.x.shape))
    ratio, err32 = M.check_err32(M.stored(alt), r64.dx, r32.dx, f"dx emulation offset={offset}")
    ratio2, _ = M.check_err32(M.stored(r32.dx), r64.dx, r32.dx, "dx emulation, own tree")
    print(f"[margin] host dx emulation last={merge_last} offset={offset}: other tree {ratio:.3f}, own {ratio2:.3f}, err32 {err32:.2e}")
    assert err32 < 1e-4                                                   # the bar is a tight one, not a licence


@pytest.mark.parametrize("C", [8, 48, 768])
def test_f32_emulation_of_n_stays_inside_its_interval(C):
    g = torch.Generator().manual_seed(C)
    T = 37
    x = M.randn_bf16(g, T, C, scale=0.8, shift=1.6)                       # rows about 2 sigma off zero
    gamma = (torch.randn(C, generator=g, dtype=F32) * 0.2 + 1.0).to(F64)
    beta = (torch.randn(C, generator=g, dtype=F32) * 0.1).to(F64)
    dn = M.draw(g, (T, C), range(-3, 4))
    r64 = M.ln_wgrad(x, None, dn, gamma, beta, M.LN_EPS)
    r32 = M.ln_wgrad(x, None, dn, gamma, beta, M.LN_EPS, dt=F32, rnd=M.bf16_f32)
    m = M.check_interval(M.stored(r32.n), r64.n, r64.width, f"n emulation C={C}")
    assert bool(((r32.dgamma.to(F64) - r64.dgamma).abs() <= r64.b_dgamma).all())
    assert torch.equal(r32.dbeta.to(F64), r64.dbeta)                      # integers: exact in f32 too
    print(f"[margin] host n emulation C={C}: {m:.3f}; dgamma {float(((r32.dgamma.to(F64) - r64.dgamma).abs() / r64.b_dgamma).max()):.3f}")
    # one bf16 step outside the interval is caught, at the planted element
    bad = M.stored(r32.n).clone()
    lo = M.bf16_rne(r64.n - r64.width)
    bad[5, C - 1] = (lo[5, C - 1] * (1 - 2.0 ** -7) - 2.0 ** -20 if lo[5, C - 1] > 0 else lo[5, C - 1] * (1 + 2.0 ** -7) - 2.0 ** -20).to(BF16)
    with pytest.raises(M.Located) as e:
        M.check_interval(bad, r64.n, r64.width, "planted")
    assert e.value.where == [(5, C - 1)]


def test_one_wrong_piece_of_a_front_pad_row_is_located():
    """One 16-byte piece of one corner token taken from the neighbouring voxel: the interval check names that token's row."""
    dims, C, Cout = (7, 5, 5), 48, 96
    o = M.merge_operands(1, dims, C, Cout, True, seed=2)
    f = M.merge_fwd(o.x, o.ln_w, o.ln_b, o.W, True)
    good = M.stored(M.merge_fwd(o.x, o.ln_w, o.ln_b, o.W, True, dt=F32, rnd=M.bf16_f32).y)
    M.check_interval(good, f.y, f.bound, "emulation")
    rows = f.rows.clone()
    t, part = 1, 7                                                        # token (0, 0, 1): h and w in the front pad, part 111 is live
    assert int(f.inv[t, part]) >= 0 and int(f.inv[t, 0]) < 0
    rows[t, part * C:part * C + 8] = o.x.reshape(-1, C)[int(f.inv[t, part]) + 1, :8]
    n, *_ = M.layer_norm(rows, o.ln_w, o.ln_b, M.LN_EPS)
    bad = M.stored(M.bf16_rne(n) @ o.W.t())
    with pytest.raises(M.Located) as e:
        M.check_interval(bad, f.y, f.bound, "planted")
    assert {w[0] for w in e.value.where} == {t}


def test_print_distance_of_dx_with_stored_yfwd_from_dx_with_exact_y():
    """The backward takes m2 from the bf16-stored forward output (documented approximation): a figure, not a bar."""
    for merge_last, C, Cout in ((True, 48, 96), (False, 192, 384)):
        o = M.merge_operands(1, (7, 5, 5), C, Cout, merge_last, seed=4)
        f = M.merge_fwd(o.x, o.ln_w, o.ln_b, o.W, merge_last, rnd=M.ident)
        wgam, wbet = o.W @ o.ln_w, o.W @ o.ln_b
        exact = M.merge_bwd(o.dy, o.x, f.y, o.ln_w, wgam, wbet, o.W, merge_last, rnd=M.ident).dx
        stored = M.merge_bwd(o.dy, o.x, M.bf16_rne(f.y), o.ln_w, wgam, wbet, o.W, merge_last, rnd=M.ident).dx
        print(f"[figure] dx with bf16 yfwd against exact y, kC={(8 if merge_last else 4) * C} Cout={Cout}: "
              f"max |diff| / max |dx| = {float((stored - exact).abs().max() / exact.abs().max()):.3e}")
