"""Guards of tests/tok_ref.py, the float64 restatement behind tests/test_hip_tok_kernels.py.  CPU only.

* the hand-written backward functions equal torch.autograd over the forward functions (float64, 1e-12 relative);
* qkv_fwd -> a plain float64 window attention -> proj_mlp_fwd is oracle.swin_ref.swin_block on a golden block fixture;
* block_images (a scatter) equals frag_image (a gather) of the bf16-rounded matrices;
* sensitivity: an f32 / bf16 emulation of each kernel (the same formulas in float32 with the bf16 storage points) passes the
  assertion helpers the GPU tests use, and with one planted defect fails them AT the planted location."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tok_ref as T  # noqa: E402
from conftest import load_fixture, rel_l2  # noqa: E402
from mivp_amd import geometry  # noqa: E402
from oracle import swin_ref as S  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def case(C=16, heads=4, B=2, P=3, Nq=13, seed=1, dup=False, vol=None):
    vol = vol or P * Nq + 11
    d = T.desc(B, P, Nq, C, heads, vol)
    src, dst = T.make_tables(P, Nq, vol, seed, dup=dup)
    return d, src, dst, T.block_operands(d, seed + 100)


def keep_mask(d, seed, p):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((d.B * d.P, d.Nqp, d.C), generator=g) >= p).to(F64)


# =============================================================================================
# backward functions against autograd
# =============================================================================================
@pytest.mark.parametrize("C,heads,Nq", [(16, 4, 13), (8, 2, 29), (48, 4, 13)])
def test_qkv_bwd_is_the_autograd_of_qkv_fwd(C, heads, Nq):
    d, src, dst, o = case(C, heads, Nq=Nq)                                # padding (-1), padding slots (-2); sources distinct
    x = o.x.clone().requires_grad_(True)
    f = T.qkv_fwd(d, x, src, o.ln1_w, o.ln1_b, o.Wq, o.Wk, o.Wv, rnd=T.ident)
    rows = T.gather_rows(x, src, d.B)                                     # the residual path: + dt1 reaches x through the gather
    loss = (f.q * o.dq).sum() + (f.k / T.LOG2E * o.dk).sum() + (f.v * o.dv).sum() + (rows * o.dt1).sum()
    loss.backward()
    b = T.qkv_bwd(d, o.dq, o.dk, o.dv, o.x, src, o.ln1_w, o.Wq, o.Wk, o.Wv, o.dt1, rnd=T.ident)
    named = ~torch.isnan(b.dx)
    assert bool(named.any()) and not bool(named.all())                    # some voxels are read by nobody
    assert float(x.grad[~named].abs().max()) == 0.0                       # autograd: no gradient there; the kernel: no write
    assert rel(b.dx[named], x.grad[named]) < 1e-12
    # dn_out: the gradient with respect to the attn_norm output
    y = f.ln.detach().clone().requires_grad_(True)
    a = y
    loss = sum(((T.to_heads(a @ W.t() * sc, heads)) * g).sum()
               for W, sc, g in ((o.Wq, d.q_scale, o.dq), (o.Wk, 1.0, o.dk), (o.Wv, 1.0, o.dv)))
    loss.backward()
    assert rel(b.dn_out, y.grad) < 1e-12


@pytest.mark.parametrize("p", [0.0, 0.5, 0.3])
@pytest.mark.parametrize("C,heads,Nq", [(16, 4, 13), (40, 2, 29)])
def test_proj_mlp_bwd_is_the_autograd_of_proj_mlp_fwd(C, heads, Nq, p):
    d, src, dst, o = case(C, heads, Nq=Nq, dup=True)
    keep = keep_mask(d, 5, p) if p else None
    scale = T.f32_of(1.0 / (1.0 - p))
    ov = o.o.clone().requires_grad_(True)
    f = T.proj_mlp_fwd(d, ov, o.x, src, dst, o.Wp, o.bp, o.ln2_w, o.ln2_b, o.Wm, o.bm, keep, scale, rnd=T.ident)
    written = ~torch.isnan(f.y)
    assert bool(written.any()) and not bool(written.all())                # cropping: some voxels have no destination
    dy = torch.where(written, o.dy, torch.full_like(o.dy, float("nan")))  # dy of voxels nobody wrote is never read
    (torch.where(written, f.y, torch.zeros_like(f.y)) * o.dy).sum().backward()
    t1 = f.t1.detach()
    b = T.proj_mlp_bwd(d, torch.nan_to_num(dy), dst, t1, o.ln2_w, o.Wm, o.Wp, keep, scale, rnd=T.ident)
    assert rel(b.dO, ov.grad) < 1e-12
    # dt1, d_pj, dn_out, dyw against autograd over the second half alone
    t1v = t1.clone().requires_grad_(True)
    n, _, _, _ = T.layer_norm(t1v, o.ln2_w, o.ln2_b, d.ln_eps)
    n.retain_grad()
    t2 = t1v + n @ o.Wm.t() + o.bm
    t2.retain_grad()
    yy = T.scatter_rows(t2, dst, d.B, d.vol_out)
    (torch.where(written, yy, torch.zeros_like(yy)) * o.dy).sum().backward()
    assert rel(b.dt1, t1v.grad) < 1e-12
    assert rel(b.dn_out, n.grad) < 1e-12
    assert rel(b.dyw, t2.grad) < 1e-12
    want_pj = t1v.grad if keep is None else t1v.grad * keep * scale
    assert rel(b.d_pj, want_pj) < 1e-12


# =============================================================================================
# the restated contract is the block's
# =============================================================================================
def test_token_functions_around_a_plain_attention_are_the_oracle_block():
    fx = load_fixture("block_oddpad_shift_prompt")
    m = fx.meta
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in fx["sd"].items()}
    x = fx["in"]["x"].double()
    prompt = fx["in"]["prompt"].double()
    B, C = x.shape[:2]
    heads, hd = m["heads"], C // m["heads"]
    meta, (src, dst, _) = geometry.build_tables_numpy(x.shape[2:], m["window"], m["shift"])
    P, Nq, Nqp = meta["P"], meta["Nq"], meta["Nqp"]
    src = torch.from_numpy(src).long().view(P, Nqp)
    dst = torch.from_numpy(dst).long().view(P, Nqp)
    assert bool((src == -1).any()) and bool((dst == -1).any())           # the fixture pads and crops
    vol = x[0, 0].numel()
    d = T.desc(B, P, Nq, C, heads, vol)
    xl = x.permute(0, 2, 3, 4, 1).reshape(B, vol, C)
    w = lambda k: sd[k]
    f = T.qkv_fwd(d, xl, src, w("attn_norm.weight"), w("attn_norm.bias"), w("attn.to_q.weight"), w("attn.to_k.weight"),
                  w("attn.to_v.weight"), rnd=T.ident)
    q, k, v = f.q[:, :, :Nq], f.k[:, :, :Nq] / T.LOG2E, f.v[:, :, :Nq]   # q carries hd^-0.5 already
    yp, _, _, _ = T.layer_norm(prompt, w("attn_norm.weight"), w("attn_norm.bias"), d.ln_eps)
    hp = lambda t: t.reshape(-1, heads, hd).permute(1, 0, 2)[None].expand(B * P, -1, -1, -1)
    k = torch.cat([k, hp(yp @ w("attn.to_k.weight").t())], 2)
    v = torch.cat([v, hp(yp @ w("attn.to_v.weight").t())], 2)
    n_p = prompt.shape[0]
    geo = S.BlockGeometry(x.shape[2:], m["window"], m["shift"])
    logits = q @ k.transpose(-1, -2) + S.rel_pos_bias(sd, "", m["window"], n_p, 64)[None]
    mask = S.shift_mask(geo)
    if mask is not None:
        mask = torch.cat([mask.double(), torch.ones(P, Nq, n_p, dtype=F64)], 2)
        logits = logits * mask.repeat(B, 1, 1)[:, None]
    o = torch.zeros(B * P, Nqp, C, dtype=F64)
    o[:, :Nq] = T.from_heads(logits.softmax(-1) @ v)
    y = T.proj_mlp_fwd(d, o, xl, src, dst, w("attn.proj.weight"), w("attn.proj.bias"), w("mlp_norm.weight"), w("mlp_norm.bias"),
                       w("mlp.weight"), w("mlp.bias"), rnd=T.ident).y
    assert not bool(torch.isnan(y).any())                                 # every voxel of a real block is written
    y = y.reshape((B,) + tuple(x.shape[2:]) + (C,)).permute(0, 4, 1, 2, 3)
    want = S.swin_block(fx["in"]["x"], fx["in"]["prompt"], fx["sd"], "", m["window"], m["shift"], heads)
    assert rel_l2(y, want) < 2e-5                                         # the bar of test_oracle_golden.py::test_swin_block
    assert rel_l2(y, fx["out"]["y"]) < 2e-5


# =============================================================================================
# weight images
# =============================================================================================
@pytest.mark.parametrize("C", [8, 40, 48, 96])
@pytest.mark.parametrize("with_natural", [0, 1])
def test_block_images_are_frag_images_of_the_rounded_matrices(C, with_natural):
    g = torch.Generator().manual_seed(C)
    ws = [torch.randn((C, C), generator=g, dtype=F32) for _ in range(5)]
    img = T.block_images(C, *ws, with_natural)
    b = [t.to(BF16) for t in ws]
    ks, ct = (C + 31) // 32, (C + 15) // 16
    wqkv = torch.cat(b[:3], 0)
    flat = lambda W, k, p: T.frag_image(W, k, p).reshape(-1)
    want = dict(wqkv_rm=wqkv.reshape(-1), wqkv_f=flat(wqkv, ks, False), wproj_f=flat(b[3], ks, False),
                wmlp_f=flat(b[4], ks, True), wqkv_t=flat(wqkv.t().contiguous(), (3 * 16 * ct + 31) // 32, False),
                wmlp_t=flat(b[4].t().contiguous(), ks, False), wproj_t=flat(b[3].t().contiguous(), ks, True))
    if with_natural:
        want["wmlp_f"] = torch.cat([want["wmlp_f"], flat(b[4], ks, False)])
        want["wproj_t"] = torch.cat([want["wproj_t"], flat(b[3].t().contiguous(), ks, False)])
    assert set(img) == set(want)
    for k in want:
        T.check_bits_equal(img[k], want[k], k)
    # one element by hand: lane 16 g + r of (nt, s), natural and paired (mivp.h)
    nat, par = T.frag_image(b[3], ks, False), T.frag_image(b[3], ks, True)
    nt, s, r, gq, e = ct - 1, ks - 1, 5, 2, 6
    row, col_n, col_p = 16 * nt + r, 32 * s + 8 * gq + e, 32 * s + 16 + 4 * gq + (e - 4)
    for im, col in ((nat, col_n), (par, col_p)):
        want_v = float(b[3][row, col]) if row < C and col < C else 0.0
        assert float(im[nt, s, 16 * gq + r, e]) == want_v


# =============================================================================================
# sensitivity: the emulation passes, a planted defect fails at its place
# =============================================================================================
@pytest.fixture(scope="module")
def emu():
    """One case (C = 64: two k-steps, four heads of 16), its float64 references and the f32 / bf16 emulation of all four kernels."""
    d, src, dst, o = case(64, 4, B=2, P=3, Nq=29, seed=7, dup=True)
    scale = T.f32_of(65536.0 / (65536.0 - round(0.3 * 65536)))
    keep = keep_mask(d, 9, 0.3)
    E = lambda **kw: dict(dt=F32, rnd=T.bf16_f32, **kw)
    r = T.SimpleNamespace(d=d, src=src, dst=dst, o=o, keep=keep, scale=scale)
    r.qkv = T.qkv_fwd(d, o.x, src, o.ln1_w, o.ln1_b, o.Wq, o.Wk, o.Wv)
    r.qkv_e = T.qkv_fwd(d, o.x, src, o.ln1_w, o.ln1_b, o.Wq, o.Wk, o.Wv, **E())
    r.fwd_e = T.proj_mlp_fwd(d, o.o, o.x, src, dst, o.Wp, o.bp, o.ln2_w, o.ln2_b, o.Wm, o.bm, keep, scale, **E())
    r.t1_e = T.stored(r.fwd_e.t1)
    r.fwd = T.proj_mlp_fwd(d, o.o, o.x, src, dst, o.Wp, o.bp, o.ln2_w, o.ln2_b, o.Wm, o.bm, keep, scale, t1_stored=r.t1_e)
    r.bwd_e = T.proj_mlp_bwd(d, o.dy, dst, o.t1, o.ln2_w, o.Wm, o.Wp, keep, scale, **E())
    r.dpj_e = T.stored(r.bwd_e.d_pj)
    r.bwd = T.proj_mlp_bwd(d, o.dy, dst, o.t1, o.ln2_w, o.Wm, o.Wp, keep, scale, operand_stored=r.dpj_e)
    r.bwd32 = T.proj_mlp_bwd(d, o.dy, dst, o.t1, o.ln2_w, o.Wm, o.Wp, keep, scale, dt=F32, rnd=T.bf16_f32)
    src1, _ = T.make_tables(d.P, d.Nq, d.vol_in, 7, dup=False)            # dx is a store: distinct sources
    r.src1 = src1
    r.qb = T.qkv_bwd(d, o.dq, o.dk, o.dv, o.x, src1, o.ln1_w, o.Wq, o.Wk, o.Wv, o.dt1)
    r.qb_e = T.qkv_bwd(d, o.dq, o.dk, o.dv, o.x, src1, o.ln1_w, o.Wq, o.Wk, o.Wv, o.dt1, **E())
    return r


def fails_at(fn, planted):
    """``fn`` raises a located failure whose failing set is exactly / contains the planted elements, and names the first."""
    with pytest.raises(T.Located) as ei:
        fn()
    where = set(ei.value.where)
    assert where and where <= set(planted), (sorted(where)[:5], sorted(planted)[:5])
    assert str(min(where)) in str(ei.value)
    return where


def test_the_emulation_of_every_kernel_passes_every_check(emu):
    r, d = emu, emu.d
    for n in "qkv":
        T.check_interval(T.stored(getattr(r.qkv_e, n)), getattr(r.qkv, n), getattr(r.qkv, "b" + n), n)
    T.check_qkv_structure(d, r.src, *(T.stored(getattr(r.qkv_e, n)) for n in "qkv"), "emulation")
    T.check_interval(r.t1_e, r.fwd.t1, r.fwd.b_t1, "t1")
    T.check_interval(T.stored(r.fwd_e.y), r.fwd.y, r.fwd.b_y, "y")
    assert torch.equal(torch.isnan(r.fwd_e.y), torch.isnan(r.fwd.y))
    T.check_interval(T.stored(r.bwd_e.dn_out), r.bwd.dn_out, r.bwd.b_dn, "dn_out")
    T.check_interval(T.stored(r.bwd_e.dO), r.bwd.dO, r.bwd.b_dO, "dO")
    T.check_bits_equal(T.stored(r.bwd_e.dyw), T.stored(r.bwd.dyw), "dyw")
    T.check_err32(T.stored(r.bwd_e.dt1), r.bwd.dt1, r.bwd32.dt1, "dt1")
    T.check_err32(r.dpj_e, r.bwd.d_pj, r.bwd32.d_pj, "d_pj")
    T.check_interval(T.stored(r.qb_e.dn_out), r.qb.dn_out, r.qb.b_dn, "dn1")
    T.check_err32(T.stored(r.qb_e.dx), r.qb.dx, r.qb_e.dx, "dx")
    # a flat 2^-9 |ref| allowance for the bf16 store (instead of the interval rule) is too small for a correct emulation:
    # half an ulp of an 8-bit significand reaches 2^-8 |v| just above a power of two
    got, ref = T.stored(r.bwd_e.dt1).double(), r.bwd.dt1
    top = float(ref.abs().max())
    err32 = float((r.bwd32.dt1.double() - ref).abs().max()) / top
    assert bool(((got - ref).abs() > (8 * err32 + 2.0 ** -22) * top + 2.0 ** -9 * ref.abs()).any())
    assert bool(((got - ref).abs() <= (8 * err32 + 2.0 ** -22) * top + 2.0 ** -8 * ref.abs()).all())


def test_planted_two_token_rows_swapped_inside_one_window(emu):
    r = emu
    bp, h, a, b = 4, 2, 3, 17
    for name in "qkv":
        t = T.stored(getattr(r.qkv_e, name)).clone()
        t[bp, :, [a, b]] = t[bp, :, [b, a]]
        planted = [(bp, hh, s, j) for hh in range(4) for s in (a, b) for j in range(16)]
        where = fails_at(lambda: T.check_interval(t, getattr(r.qkv, name), getattr(r.qkv, "b" + name), name), planted)
        assert len(where) > 100                                           # essentially both rows
    t = T.stored(r.bwd_e.dO).clone()
    t[bp, [a, b]] = t[bp, [b, a]]
    fails_at(lambda: T.check_interval(t, r.bwd.dO, r.bwd.b_dO, "dO"), [(bp, s, j) for s in (a, b) for j in range(64)])


def test_planted_one_heads_channel_chunk_shifted_by_one_head(emu):
    r = emu
    bp = 1
    t = T.stored(r.qkv_e.k).clone()
    t[bp] = torch.roll(t[bp], 1, 0)                                       # head h holds head h - 1's chunk
    planted = [(bp, h, s, j) for h in range(4) for s in range(r.d.Nq) for j in range(16)]
    where = fails_at(lambda: T.check_interval(t, r.qkv.k, r.qkv.bk, "k"), planted)
    assert {w[1] for w in where} == {0, 1, 2, 3}


def test_planted_one_k_step_dropped_from_one_output_tile(emu):
    r, o = emu, emu.o
    bp, s0, n0 = 3, 16, 32                                                # token tile 16..31 of window 3, output columns 32..47
    part = (o.o[bp, s0:s0 + 16, 32:64] @ o.Wp[n0:n0 + 16, 32:64].t()) * (r.keep[bp, s0:s0 + 16, n0:n0 + 16] * r.scale)
    t1 = r.fwd_e.t1.clone()
    t1[bp, s0:s0 + 16, n0:n0 + 16] -= part.to(F32)
    planted = [(bp, s, n) for s in range(s0, s0 + 16) for n in range(n0, n0 + 16)]
    where = fails_at(lambda: T.check_interval(T.stored(t1), r.fwd.t1, r.fwd.b_t1, "t1"), planted)
    assert len(where) > 64                                                # kept elements of the tile (dropped ones are zero)
    # and in qkv_fwd: k-step 1 of output tile 2 of v, tokens 0..15 of window 0
    y = T.bf16_f32(r.qkv_e.ln)
    part = T.to_heads((y[0:1, 0:16, 32:64] @ o.Wv[32:48, 32:64].t().to(F32)), 1)      # [1][1][16][16] = head 2's columns
    v = r.qkv_e.v.clone()
    v[0, 2, 0:16] -= part[0, 0]
    planted = [(0, 2, s, j) for s in range(16) for j in range(16)]
    where = fails_at(lambda: T.check_interval(T.stored(v), r.qkv.v, r.qkv.bv, "v"), planted)
    assert len(where) > 200


def bump_one_ulp(t, idx):
    """The stored bf16 value at ``idx`` moved to its neighbour of larger magnitude."""
    t = t.clone()
    bits = t.view(torch.int16)
    bits[idx] += 1
    return t


@pytest.mark.parametrize("which", ["q", "t1", "y", "dn_out", "dO", "dn1"])
def test_planted_one_element_one_bf16_ulp_outside_its_interval(emu, which):
    r = emu
    got, ref, bound = {"q": (r.qkv_e.q, r.qkv.q, r.qkv.bq), "t1": (r.fwd_e.t1, r.fwd.t1, r.fwd.b_t1),
                       "y": (r.fwd_e.y, r.fwd.y, r.fwd.b_y), "dn_out": (r.bwd_e.dn_out, r.bwd.dn_out, r.bwd.b_dn),
                       "dO": (r.bwd_e.dO, r.bwd.dO, r.bwd.b_dO), "dn1": (r.qb_e.dn_out, r.qb.dn_out, r.qb.b_dn)}[which]
    got = T.stored(got)
    ok = ~torch.isnan(ref)
    rr = torch.where(ok, ref, torch.zeros_like(ref))
    tight = ok & (T.bf16_rne(rr - bound.nan_to_num()) == T.bf16_rne(rr + bound.nan_to_num())) & (rr.abs() > 1e-3)
    idx = tuple(int(i) for i in torch.nonzero(tight)[-1])                 # the last element whose interval holds one bf16 value
    assert fails_at(lambda: T.check_interval(bump_one_ulp(got, idx), ref, bound, which), [idx]) == {idx}


def test_planted_minus_one_and_minus_two_sources_exchanged(emu):
    r, d, o = emu, emu.d, emu.o
    wrong = r.src.clone()
    wrong[r.src == -1], wrong[r.src == -2] = -2, -1
    e = T.qkv_fwd(d, o.x, wrong, o.ln1_w, o.ln1_b, o.Wq, o.Wk, o.Wv, dt=F32, rnd=T.bf16_f32)
    rows = lambda val: [(bp, h, s, j) for bp in range(d.B * d.P) for h in range(4) for j in range(16)
                        for s in torch.nonzero(r.src[bp % d.P] == val).reshape(-1).tolist()]
    where = fails_at(lambda: T.check_interval(T.stored(e.q), r.qkv.q, r.qkv.bq, "q"), rows(-1) + rows(-2))
    assert {r.src[w[0] % d.P, w[2]].item() for w in where} == {-1, -2}
    with pytest.raises(T.Located) as ei:                                  # the exact property names a padding-slot row
        T.check_qkv_structure(d, r.src, T.stored(e.q), T.stored(e.k), T.stored(e.v), "exchanged")
    t = ei.value.where[0][0]
    assert r.src.repeat(d.B, 1).reshape(-1)[t] == -2


def test_err32_check_fails_on_a_wrong_row(emu):
    r = emu
    t = T.stored(r.bwd_e.dt1).clone()
    t[2, [1, 5]] = t[2, [5, 1]]
    fails_at(lambda: T.check_err32(t, r.bwd.dt1, r.bwd32.dt1, "dt1"), [(2, s, j) for s in (1, 5) for j in range(64)])
