"""Direct parity tests of the prompt-path and row-reduction kernels against tests/prompt_ref.py (float64, CPU).

Entries under test, each called through ``_lib.call`` on its own operands: mivp_reduce_rows / _multi, mivp_token_scores_fwd /
_bwd / _fwd_multi / _bwd_multi, mivp_prompt_kv_fwd / _fwd_multi / _bwd, mivp_relbias_aug, mivp_relbias_grad, and the batched
Python path functional.prepare_prompted_blocks against the per-block path.

Kinds of assertion (none of the bars is a measured figure):
  exact    integer-valued f32 operands whose partial sums stay below 2^24 in any order: bit-equal to the int64 result
           (row reductions, mivp_relbias_grad); relayouts and one-hots: bit-equal; batched against single calls: bit-equal
  derived  f32 sums of n terms against float64: n 2^-24 sum |a||b| per element (row reductions, token scores, yln)
  interval stored bf16 values: the rounding of some value within the derived f32 bound of the float64 reference
           (kp, vp, ka, wg_n): bit-equal unless the bound straddles a rounding boundary, then one neighbour
  err32    LayerNorm backward cancels, so dprompt / wg_ln use a bar computed at run time: the same formulas in plain f32
           torch on the CPU give err32 = max |f32 - f64| / max |f64|; the kernel's same metric must stay <= 8 err32 + 2^-22
           (both are f32 sums of at most C or heads hd terms in different trees: 8 covers the order, not a precision class)

Every output buffer starts as NaN and carries a guard tail that must come back untouched; NaN is also put into every input
element the contract says a kernel does not read."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ref as R  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import functional as Fn
from mivp_amd import swin_ops, train
from mivp_amd.swin_unetr import SwinTransformerBlock

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GUARD = 64
NAN = float("nan")
EMBED = int(train.make_conf("tiny")[0].pos_bias_embed_dim)        # the model's bias embedding width (every config: 64)


class Out:
    """An output buffer: NaN everywhere, ``GUARD`` extra elements behind it that no kernel may touch."""

    def __init__(self, shape, dtype=F32):
        self.n = int(math.prod(shape))
        self.flat = torch.full((self.n + GUARD,), NAN, dtype=dtype, device=DEV)
        self.t = self.flat[:self.n].view(*shape)

    def done(self, what):
        """The guard tail is untouched and the payload holds no NaN; returns the payload on the CPU."""
        flat = self.flat.cpu()
        assert bool(torch.isnan(flat[self.n:]).all()), f"{what}: the kernel wrote behind its output buffer"
        got = flat[:self.n].view(self.t.shape)
        bad = torch.isnan(got)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {self.n} output elements were never written (or are NaN)"
        return got


def dev(t, dtype=F32):
    return t.to(dtype).to(DEV).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not torch.equal(bits(a), bits(b)):
        bad = torch.nonzero(bits(a) != bits(b))
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} elements differ in their bits; first at {first}: "
                             f"{float(a.cpu()[first])!r} != {float(b.cpu()[first])!r}")


def assert_within(got, ref, bound, what):
    g = got.detach().to(F64).cpu()
    assert g.shape == ref.shape == bound.shape, (what, tuple(g.shape), tuple(ref.shape))
    bad = ~((g - ref).abs() <= bound)
    if bool(bad.any()):
        i = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.numel()} elements leave the derived bound; first at {i}: got "
                             f"{float(g[i])!r}, float64 {float(ref[i])!r}, bound {float(bound[i]):.3e}")


def vparr(ts):
    return (C.c_void_p * len(ts))(*[0 if t is None else t.data_ptr() for t in ts])


# =============================================================================================
# row reductions
# =============================================================================================
NS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 225, 255, 256, 257, 289, 1372)
ROWS = (1, 31, 32, 33, 95, 96, 3072)
INTS = range(-2047, 2048)                                         # 1372 * 2047 < 2^22: every partial sum is exact


def reduce_rows(x_dev, n, rows, what):
    out = Out((rows,))
    L.call("mivp_reduce_rows", L.ptr(x_dev), n, rows, L.ptr(out.t), L.stream())
    return out.done(what)


@pytest.mark.parametrize("rows", ROWS)
def test_reduce_rows_exact_and_bounded(rows):
    g = R.gen(100 + rows)
    xi = R.draw(g, (max(NS), rows), INTS)
    xr = torch.randn((max(NS), rows), generator=g, dtype=F32).double()
    xi_dev, xr_dev = dev(xi), dev(xr)
    for n in NS:                                                  # a prefix of the matrix is an [n, rows] matrix
        ref, mag = R.reduce_rows_int(xi[:n])
        assert int(mag.max()) < 2 ** 24 if n else True            # precondition of "exact", on the reference alone
        got = reduce_rows(xi_dev, n, rows, f"reduce_rows int n={n} rows={rows}")
        R.assert_equal_located(got, ref.to(F64), "r", f"reduce_rows n={n} rows={rows}")
        if n == 0:
            assert not bool(bits(got).any())                      # +0, not -0
        ref64, bound = R.reduce_rows_bound(xr[:n])
        assert_within(reduce_rows(xr_dev, n, rows, f"reduce_rows f32 n={n} rows={rows}"), ref64, bound,
                      f"reduce_rows f32 n={n} rows={rows}")


HEADS_T, NPP_T, HD_T = 4, 32, 12
SEGMENTS = [(33,), (33, 1), (33, 1, 64), (33, 1, 64, 95), (HEADS_T * NPP_T * HD_T, HEADS_T * NPP_T * HD_T, HEADS_T * NPP_T)]
MULTI_NS = (0, 1, 2, 33, 65, 257, 289)


@pytest.mark.parametrize("seg_rows", SEGMENTS, ids=lambda s: "x".join(str(v) for v in s))
def test_reduce_rows_multi(seg_rows):
    g = R.gen(sum(seg_rows))
    nseg = len(seg_rows)
    xi = [R.draw(g, (max(MULTI_NS), r), INTS) for r in seg_rows]
    xr = [torch.randn((max(MULTI_NS), r), generator=g, dtype=F32) for r in seg_rows]
    xi_dev, xr_dev = [dev(x) for x in xi], [dev(x) for x in xr]
    rows = (C.c_int64 * nseg)(*seg_rows)
    for n in MULTI_NS:
        outs = [Out((r,)) for r in seg_rows]
        L.call("mivp_reduce_rows_multi", nseg, vparr(xi_dev), rows, vparr([o.t for o in outs]), n, L.stream())
        for i, o in enumerate(outs):
            ref, mag = R.reduce_rows_int(xi[i][:n])
            assert n == 0 or int(mag.max()) < 2 ** 24
            R.assert_equal_located(o.done(f"multi int seg {i} n={n}"), ref.to(F64), "r", f"reduce_rows_multi seg {i} n={n}")
        outs = [Out((r,)) for r in seg_rows]
        L.call("mivp_reduce_rows_multi", nseg, vparr(xr_dev), rows, vparr([o.t for o in outs]), n, L.stream())
        for i, o in enumerate(outs):                              # fixed order: the same bits as the single-array entry
            got = o.done(f"multi f32 seg {i} n={n}")
            assert_same_bits(got, reduce_rows(xr_dev[i], n, seg_rows[i], "single"), f"multi vs single seg {i} n={n}")
            ref64, bound = R.reduce_rows_bound(xr[i][:n].double())
            assert_within(got, ref64, bound, f"reduce_rows_multi f32 seg {i} n={n}")


# =============================================================================================
# token scores
# =============================================================================================
TS_SHAPES = [(4, 64, EMBED), (16, 64, EMBED), (8, 30, EMBED), (2, 1, 5), (3, 7, 33)]


def ts_operands(heads, n_p, e, seed):
    g = R.gen(seed)
    mk = lambda *s: torch.randn(s, generator=g, dtype=F32).double()
    return mk(heads, e), mk(n_p, e), mk(heads, n_p)


def ts_fwd_single(W, E, scale, what):
    heads, e = W.shape
    out = Out((heads, E.shape[0]))
    Wd, Ed = dev(W), dev(E)                                       # named: a temporary's memory is reused by the next one
    L.call("mivp_token_scores_fwd", L.ptr(Wd), L.ptr(Ed), heads, E.shape[0], e, scale, L.ptr(out.t), L.stream())
    return out.done(what)


def ts_bwd_single(dts, W, E, scale, what):
    heads, e = W.shape
    dW, dE = Out((heads, e)), Out((E.shape[0], e))
    Dd, Wd, Ed = dev(dts), dev(W), dev(E)
    L.call("mivp_token_scores_bwd", L.ptr(Dd), L.ptr(Wd), L.ptr(Ed), heads, E.shape[0], e, scale, L.ptr(dW.t),
           L.ptr(dE.t), L.stream())
    return dW.done(what + " dW"), dE.done(what + " dE")


@pytest.mark.parametrize("heads,n_p,e", TS_SHAPES)
def test_token_scores_against_float64(heads, n_p, e):
    W, E, dts = ts_operands(heads, n_p, e, 7 * heads + n_p)
    # the power of two next to e^-0.5 (exactly e^-0.5 = 1/8 at the model's e = 64): the closing multiplication by scale is
    # then exact, and the bound of an n-term f32 sum (n roundings) is a bound of the whole kernel
    scale = 2.0 ** round(math.log2(e ** -0.5))
    assert scale == R.f32_of(scale) and (e != EMBED or scale == e ** -0.5)
    b_ts, b_w, b_e = R.token_scores_bounds(dts, W, E, scale)
    what = f"token_scores ({heads}, {n_p}, {e})"
    assert_within(ts_fwd_single(W, E, scale, what), R.token_scores(W, E, scale), b_ts, what + " ts")
    dW, dE = ts_bwd_single(dts, W, E, scale, what)
    rW, rE = R.token_scores_grads(dts, W, E, scale)
    assert_within(dW, rW, b_w, what + " dW")
    assert_within(dE, rE, b_e, what + " dE")


@pytest.mark.parametrize("n", [1, 2, 16])
def test_token_scores_multi_equals_single_calls(n):
    shapes = [((4, 16, 8, 2, 3)[i % 5], (64, 30, 1, 7, 16, 33)[i % 6]) for i in range(n)]
    e = EMBED
    scales = [2.0 ** -3 * (1 + i / 16) for i in range(n)]
    ops = [ts_operands(h, p, e, 50 + i) for i, (h, p) in enumerate(shapes)]
    no_grad = {16: (3, 9), 2: (1,), 1: ()}[n]                     # jobs whose dts pointer is NULL
    Wd, Ed = [dev(o[0]) for o in ops], [dev(o[1]) for o in ops]
    Dd = [None if i in no_grad else dev(o[2]) for i, o in enumerate(ops)]
    heads = (C.c_int32 * n)(*[s[0] for s in shapes])
    nps = (C.c_int32 * n)(*[s[1] for s in shapes])
    sc = (C.c_float * n)(*scales)
    ts = [Out(s) for s in shapes]
    L.call("mivp_token_scores_fwd_multi", n, vparr(Wd), vparr(Ed), heads, nps, e, sc, vparr([o.t for o in ts]), L.stream())
    dW = [Out((s[0], e)) for s in shapes]
    dE = [Out((s[1], e)) for s in shapes]
    L.call("mivp_token_scores_bwd_multi", n, vparr(Dd), vparr(Wd), vparr(Ed), heads, nps, e, sc, vparr([o.t for o in dW]),
           vparr([o.t for o in dE]), L.stream())
    for i, (W, E, dts) in enumerate(ops):
        what = f"job {i} of {n} {shapes[i]}"
        assert_same_bits(ts[i].done(what), ts_fwd_single(W, E, scales[i], what), what + " ts")
        gW, gE = dW[i].done(what + " dW"), dE[i].done(what + " dE")
        if i in no_grad:                                          # no gradient reached the block: exact zeros, written
            assert not bool(gW.any()) and not bool(gE.any()), what
        else:
            sW, sE = ts_bwd_single(dts, W, E, scales[i], what)
            assert_same_bits(gW, sW, what + " dW")
            assert_same_bits(gE, sE, what + " dE")


def test_token_scores_fn_with_a_longer_enc_token():
    heads, rows, n_p, e = 4, 64, 30, EMBED
    W, E, dts = ts_operands(heads, rows, e, 91)
    dts = dts[:, :n_p].contiguous()
    scale = R.f32_of(e ** -0.5)
    Wp, Ep = dev(W).requires_grad_(True), dev(E).requires_grad_(True)
    ts = Fn._TokenScoresFn.apply(Wp, Ep, n_p, scale)
    ts.backward(dev(dts))
    torch.cuda.synchronize()
    b_ts, b_w, b_e = R.token_scores_bounds(dts, W, E[:n_p], scale)
    assert_within(ts, R.token_scores(W, E[:n_p], scale), b_ts, "ts")
    rW, rE = R.token_scores_grads(dts, W, E[:n_p], scale)
    assert_within(Wp.grad, rW, b_w, "dW")
    assert Ep.grad.shape == (rows, e)
    assert_within(Ep.grad[:n_p], rE, b_e, "dE")
    assert not bool(bits(Ep.grad[n_p:]).any()), "rows of dE beyond n_prompt must be exactly zero"


# =============================================================================================
# prompt K / V
# =============================================================================================
W777 = (7, 7, 7)
KV_CASES = [(16, 4, 8, W777), (48, 4, 64, W777), (96, 8, 30, W777), (192, 16, 1, W777), (384, 4, 16, W777),
            (48, 4, 16, (5, 5, 3))]
KV_IDS = [f"C{c}_h{h}_np{p}_w{''.join(str(v) for v in w)}" for c, h, p, w in KV_CASES]


def kv_operands(Cc, heads, n_p, window, seed):
    """Operands as float64 tensors that hold exactly the values the device copies hold (f32, or bf16 for the weights)."""
    g = R.gen(seed)
    rnd = lambda *s: torch.randn(s, generator=g, dtype=F32)
    o = dict(prompt=(0.8 * rnd(n_p, Cc) + 0.1).double(), ln_w=(1.0 + 0.2 * rnd(Cc)).double(), ln_b=(0.1 * rnd(Cc)).double(),
             wqkv=(rnd(3 * Cc, Cc) * Cc ** -0.5).bfloat16().double(), ts=(0.3 * rnd(heads, n_p)).double(),
             tabs=[(0.3 * rnd(heads, 2 * w - 1)).double() for w in window])
    o["dev"] = dict(prompt=dev(o["prompt"]), ln_w=dev(o["ln_w"]), ln_b=dev(o["ln_b"]), wqkv=dev(o["wqkv"], BF16), ts=dev(o["ts"]),
                    tabs=[dev(t) for t in o["tabs"]])
    return o


def kv_fwd_single(d, o, what, with_yln=True):
    hd = d.C // d.heads
    kp, vp = Out((d.heads, d.Npp, hd), BF16), Out((d.heads, d.Npp, hd), BF16)
    yln = Out((d.Np, d.C)) if with_yln else None
    D = o["dev"]
    L.call("mivp_prompt_kv_fwd", C.byref(d), L.ptr(D["prompt"]), L.ptr(D["ln_w"]), L.ptr(D["ln_b"]), L.ptr(D["wqkv"]),
           L.ptr(kp.t), L.ptr(vp.t), L.ptr(yln.t if with_yln else None), L.stream())
    return kp.done(what + " kp"), vp.done(what + " vp"), (yln.done(what + " yln") if with_yln else None)


def relbias_aug(d, o, ts_dev, what):
    qa, ka = Out((d.Nqp, d.augp), BF16), Out((d.heads, d.Nkp, d.augp), BF16)
    t = o["dev"]["tabs"]
    L.call("mivp_relbias_aug", C.byref(d), L.ptr(t[0]), L.ptr(t[1]), L.ptr(t[2]), L.ptr(ts_dev), L.ptr(qa.t), L.ptr(ka.t),
           L.stream())
    return qa, ka


@pytest.mark.parametrize("Cc,heads,n_p,window", KV_CASES, ids=KV_IDS)
def test_prompt_kv_fwd(Cc, heads, n_p, window):
    d = swin_ops.prompt_desc(Cc, heads, window, n_p)
    assert d.Npp == R.round_up(n_p, 16) and (n_p, d.Npp) in [(8, 16), (64, 64), (30, 32), (1, 16), (16, 16)]
    o = kv_operands(Cc, heads, n_p, window, Cc + n_p)
    what = f"prompt_kv_fwd C={Cc} heads={heads} Np={n_p}"
    kp, vp, yln = kv_fwd_single(d, o, what)
    ref_yln, _, _, _, _ = R.prompt_kv(o["prompt"], o["ln_w"], o["ln_b"], o["wqkv"], heads, d.Npp, float(d.ln_eps))
    # two f32 reductions of C terms: C 2^-23 relative to the row's largest element
    assert_within(yln, ref_yln, (Cc * 2.0 ** -23 * ref_yln.abs().amax(1, keepdim=True)).expand_as(ref_yln), what + " yln")
    # the GEMM from the bf16 rounding of the GPU's own yln: what is left is the order of an f32 accumulation of C terms
    _, rk, rv, bk, bv = R.prompt_kv(o["prompt"], o["ln_w"], o["ln_b"], o["wqkv"], heads, d.Npp, float(d.ln_eps), y_gemm=yln)
    R.assert_rounds_from_interval(kp, rk, bk, what + " kp [heads][Npp][hd] (x log2 e)")
    R.assert_rounds_from_interval(vp, rv, bv, what + " vp [heads][Npp][hd]")
    assert not bool(bits(kp[:, n_p:]).any()) and not bool(bits(vp[:, n_p:]).any()), "rows Np..Npp-1 must be +0"
    # calling without the yln output changes nothing else
    kp2, vp2, _ = kv_fwd_single(d, o, what, with_yln=False)
    assert_same_bits(kp2, kp, what + " kp without yln")
    assert_same_bits(vp2, vp, what + " vp without yln")


@pytest.mark.parametrize("n", [2, 16])
def test_prompt_kv_fwd_multi_equals_single_calls_and_rewrites_only_the_prompt_rows(n):
    jobs = [KV_CASES[i % len(KV_CASES)] for i in range(n)]       # n = 2: Npp 16 beside Npp 64 (surplus workgroups exit)
    descs = [swin_ops.prompt_desc(c, h, w, p) for c, h, p, w in jobs]
    assert {int(d.Npp) for d in descs} >= {16, 64}
    ops = [kv_operands(c, h, p, w, 300 + i) for i, (c, h, p, w) in enumerate(jobs)]
    kps = [Out((d.heads, d.Npp, d.C // d.heads), BF16) for d in descs]
    vps = [Out((d.heads, d.Npp, d.C // d.heads), BF16) for d in descs]
    kas = []
    for d, o in zip(descs, ops):                                  # the image swin_ops.prompt_aug_image caches: ts = 0
        zero = torch.zeros((d.heads, d.Np), dtype=F32, device=DEV)
        kas.append(relbias_aug(d, o, zero, "aug image for ts = 0")[1])
        kas[-1].done("aug image for ts = 0")
    darr = (L.SwinDesc * n)(*descs)
    D = [o["dev"] for o in ops]
    L.call("mivp_prompt_kv_fwd_multi", n, darr, vparr([x["prompt"] for x in D]), vparr([x["ln_w"] for x in D]),
           vparr([x["ln_b"] for x in D]), vparr([x["wqkv"] for x in D]), vparr([x["ts"] for x in D]),
           vparr([k.t for k in kps]), vparr([v.t for v in vps]), vparr([k.t for k in kas]), L.stream())
    for i, (d, o) in enumerate(zip(descs, ops)):
        what = f"job {i} of {n} {jobs[i]}"
        kp, vp, _ = kv_fwd_single(d, o, what, with_yln=False)
        assert_same_bits(kps[i].done(what + " kp"), kp, what + " kp")
        assert_same_bits(vps[i].done(what + " vp"), vp, what + " vp")
        want = relbias_aug(d, o, o["dev"]["ts"], what)[1].done(what + " ka with the real ts")
        assert_same_bits(kas[i].done(what + " ka"), want, what + " ka: prompt rows written, nothing else touched")


# =============================================================================================
# relative-position bias: augmentation images and table gradients
# =============================================================================================
WINDOWS = [(7, 7, 7), (8, 8, 4), (5, 5, 3), (3, 3, 2), (2, 3, 5)]
WIN_IDS = ["".join(str(v) for v in w) for w in WINDOWS]


@pytest.mark.parametrize("window", WINDOWS, ids=WIN_IDS)
def test_relbias_aug(window):
    w0 = window[0]
    for n_p in (0, 8, 30, 64):
        for heads in (2, 4):
            Cc = 8 * heads
            d = swin_ops.prompt_desc(Cc, heads, window, n_p)
            dims = R.aug_dims(window, n_p)
            assert all(int(getattr(d, k)) == v for k, v in dims.items()), dims
            if window == (7, 7, 7):
                assert (d.Nq, d.Nqp) == (343, 352)
            if window == (8, 8, 4):
                assert d.Nq == d.Nqp
            if window == (3, 3, 2):
                assert d.Nqp == 32
            o = kv_operands(Cc, heads, n_p, window, 500 + 10 * n_p + heads)
            what = f"relbias_aug window={window} Np={n_p} heads={heads}"
            qa, ka = relbias_aug(d, o, o["dev"]["ts"] if n_p else None, what)
            qa, ka = qa.done(what + " qa"), ka.done(what + " ka")
            ref_qa = R.relbias_qa(window, n_p)
            R.assert_equal_located(qa, ref_qa, "na", what + " qa")
            assert not bool(bits(qa[d.Nq:]).any()) and not bool(bits(qa[:, d.aug:]).any())
            ref_ka, b = R.relbias_ka(*o["tabs"], o["ts"], window, n_p)
            R.assert_rounds_from_interval(ka, ref_ka, b, what + " ka")
            pad = torch.cat([torch.arange(d.Nq, d.Nqp), torch.arange(d.Nqp + n_p, d.Nkp)])
            assert bool((ka[:, pad, :w0].double() == R.PAD_BIAS).all()) and not bool(ka[:, pad, w0:].double().any()), what
            assert not bool(ka[:, :, d.aug:].double().any()) and not bool(ka[:, d.Nqp:d.Nqp + n_p, w0:].double().any()), what
            # the full bias rebuilt from the STORED images: three bf16 table terms per logit (one for a prompt key), each
            # the rounding (8 significant bits: 2^-8 relative) of a value within b of the float64 term
            term_tol = 2.0 ** -8 * (ref_ka.abs() + b) + b
            tol = R.bias_from_aug(ref_qa, term_tol, window, n_p) + 1e-12
            assert_within(R.bias_from_aug(qa, ka, window, n_p), R.relbias_full(*o["tabs"], o["ts"], window), tol,
                          what + " bias rebuilt from qa / ka")


@pytest.mark.parametrize("window", WINDOWS, ids=WIN_IDS)
def test_relbias_grad_exact(window):
    n_p = 8
    for heads in (2, 4):
        d = swin_ops.prompt_desc(8 * heads, heads, window, n_p)
        g = R.gen(700 + heads + sum(window))
        vals = R.draw(g, (heads, d.Nq, d.aug), range(-8, 9))
        # NaN wherever the kernel has no business reading: rows >= Nq (padding, prompt rows), columns aug..31
        dka = torch.full((heads, d.Nkp, 32), NAN, dtype=F64)
        dka[:, :d.Nq, :d.aug] = vals
        dki = torch.zeros((heads, d.Nkp, 32), dtype=torch.int64)
        dki[:, :d.Nq, :d.aug] = vals.to(torch.int64)
        ref = R.relbias_grad(dki, window)
        # an element enters a table entry at most twice, with either sign: every partial sum of any order is an integer
        # below twice the sum of all magnitudes of the head
        assert 2 * int(dki.abs().sum(dim=(1, 2)).max()) < 2 ** 24
        outs = [Out((heads, 2 * w - 1)) for w in window]
        dka_dev = dev(dka)
        L.call("mivp_relbias_grad", C.byref(d), L.ptr(dka_dev), L.ptr(outs[0].t), L.ptr(outs[1].t), L.ptr(outs[2].t),
               L.stream())
        for name, o, r in zip(("d_th", "d_tw", "d_td"), outs, ref):
            what = f"relbias_grad window={window} heads={heads} {name}"
            R.assert_equal_located(o.done(what), r.to(F64), "he", what)


# =============================================================================================
# prompt K / V backward
# =============================================================================================
@pytest.mark.parametrize("Cc,heads,n_p,window", KV_CASES, ids=KV_IDS)
def test_prompt_kv_bwd(Cc, heads, n_p, window):
    d = swin_ops.prompt_desc(Cc, heads, window, n_p)
    o = kv_operands(Cc, heads, n_p, window, 900 + Cc + n_p)
    hd, eps = Cc // heads, float(d.ln_eps)
    g = R.gen(Cc * 3 + n_p)
    dkp = torch.full((heads, d.Npp, hd), NAN, dtype=F64)          # rows >= Np belong to no prompt token: never read
    dvp = torch.full((heads, d.Npp, hd), NAN, dtype=F64)
    dkp[:, :n_p] = torch.randn((heads, n_p, hd), generator=g, dtype=F32).double()
    dvp[:, :n_p] = torch.randn((heads, n_p, hd), generator=g, dtype=F32).double()
    D = o["dev"]
    dkp_dev, dvp_dev = dev(dkp), dev(dvp)
    what = f"prompt_kv_bwd C={Cc} heads={heads} Np={n_p}"

    def run(with_w):
        dp = Out((n_p, Cc))
        wa, wn, wl = (Out((2, n_p, Cc), BF16), Out((n_p, Cc), BF16), Out((2, n_p, Cc))) if with_w else (None, None, None)
        L.call("mivp_prompt_kv_bwd", C.byref(d), L.ptr(dkp_dev), L.ptr(dvp_dev), L.ptr(D["prompt"]), L.ptr(D["ln_w"]),
               L.ptr(D["ln_b"]), L.ptr(D["wqkv"]), L.ptr(dp.t), L.ptr(wa.t if with_w else None),
               L.ptr(wn.t if with_w else None), L.ptr(wl.t if with_w else None), L.stream())
        if not with_w:
            return dp.done(what + " dprompt"), None, None, None
        return dp.done(what + " dprompt"), wa.done(what + " wg_a"), wn.done(what + " wg_n"), wl.done(what + " wg_ln")

    dp0, _, _, _ = run(False)
    dp1, wg_a, wg_n, wg_ln = run(True)
    assert_same_bits(dp0, dp1, what + " dprompt with / without the weight-gradient outputs")
    # wg_a: head-merged relayout and bf16 rounding of dkp / dvp, no factor (dkp is w.r.t. the un-scaled K: prompt_ref.py)
    want_a = torch.stack([R.head_merge(dkp, n_p), R.head_merge(dvp, n_p)]).float().bfloat16()
    assert_same_bits(wg_a, want_a, what + " wg_a")
    yln = R.layernorm(o["prompt"], o["ln_w"], o["ln_b"], eps)
    R.assert_rounds_from_interval(wg_n, yln, (Cc * 2.0 ** -23 * yln.abs().amax(1, keepdim=True)).expand_as(yln), what + " wg_n")
    ref_dp, ref_ln = R.prompt_kv_bwd(dkp, dvp, o["prompt"], o["ln_w"], o["ln_b"], o["wqkv"], heads, eps)
    f32_dp, f32_ln = R.prompt_kv_bwd(dkp, dvp, o["prompt"], o["ln_w"], o["ln_b"], o["wqkv"], heads, eps, dtype=F32)
    failures = []
    for name, got, f32, ref in (("dprompt", dp1, f32_dp, ref_dp), ("wg_ln", wg_ln, f32_ln, ref_ln)):
        err32, err = R.rel_max_err(f32, ref), R.rel_max_err(got, ref)
        bar = 8 * err32 + 2.0 ** -22
        print(f"{what} {name}: err32 {err32:.3e}  kernel {err:.3e}  bar {bar:.3e}")
        if not err <= bar:
            failures.append(f"{name}: {err:.3e} > {bar:.3e}")
    assert not failures, (what, failures)


# =============================================================================================
# the batched Python path against the per-block path
# =============================================================================================
BLOCK_WINDOW, BLOCK_DIMS = (3, 3, 2), (6, 6, 4)
BLOCK_SPECS = [(16, 4, 8, 16), (48, 4, 16, 16), (96, 8, 16, 16)]  # (C, heads, Np, enc_token rows): the first has spare rows


def make_blocks(specs, seed):
    torch.manual_seed(seed)
    out = []
    for Cc, heads, n_p, rows in specs:
        blk = SwinTransformerBlock(Cc, BLOCK_WINDOW, EMBED, heads, 1, rows).to(DEV).train()
        for name, q in blk.named_parameters():                    # frozen body and content tables: prompt tuning
            q.requires_grad_("enc_token" in name or "weights_token" in name)
        with torch.no_grad():
            blk.pe.weights_token.mul_(4.0)                        # token scores large enough to matter in the softmax
        prm = torch.nn.Parameter(torch.randn((n_p, Cc), device=DEV) * 0.5)
        x = torch.randn((1,) + BLOCK_DIMS + (Cc,), device=DEV).to(BF16)
        gy = torch.randn((1,) + BLOCK_DIMS + (Cc,), device=DEV)
        out.append((blk, prm, x, gy))
    return out


def run_blocks(blocks, batched):
    leaves = []
    for blk, prm, _, _ in blocks:
        leaves += [prm, blk.pe.weights_token, blk.pe.enc_token[0]]
        blk.__dict__.pop("_pre", None)
    for q in leaves:
        q.grad = None
    parked = []
    if batched:
        Fn.prepare_prompted_blocks([(blk, prm) for blk, prm, _, _ in blocks])
        for blk, prm, _, _ in blocks:
            pre = blk.__dict__.get("_pre")
            parked.append(None if pre is None else (pre[1].detach().clone(),) + tuple(t.clone() for t in pre[2][1:]))
    ys = [blk(x, prm) for blk, prm, x, _ in blocks]
    sum((y.float() * gy).sum() for y, (_, _, _, gy) in zip(ys, blocks)).backward()
    torch.cuda.synchronize()
    return [y.detach().clone() for y in ys], [q.grad.detach().clone() for q in leaves], parked


@pytest.mark.parametrize("nblk", [2, 3])
def test_batched_prompt_path_equals_the_per_block_path(nblk):
    blocks = make_blocks(BLOCK_SPECS[:nblk], 40 + nblk)
    y_b, g_b, parked = run_blocks(blocks, True)
    y_s, g_s, _ = run_blocks(blocks, False)
    for i, (blk, prm, _, _) in enumerate(blocks):
        Cc, heads, n_p, rows = BLOCK_SPECS[i]
        what = f"block {i} of {nblk} (C={Cc}, heads={heads}, Np={n_p})"
        assert parked[i] is not None, what + ": an eligible block was left to the per-block path"
        ts, kp, vp, qa, ka = parked[i]
        # the parked operands against the per-block C calls on the same parameters
        w = Fn._block_weights(blk, torch.device(DEV))
        d = swin_ops.prompt_desc(Cc, heads, BLOCK_WINDOW, n_p)
        with torch.no_grad():
            ts1 = Fn.token_scores(blk.pe, n_p)
        assert_same_bits(ts, ts1, what + " ts")
        o = dict(dev=dict(prompt=prm.detach().float().contiguous(), ln_w=w.ln1_w, ln_b=w.ln1_b, wqkv=w.wqkv,
                          tabs=[w.t_h, w.t_w, w.t_d]))
        kp1, vp1, _ = kv_fwd_single(d, o, what, with_yln=False)
        assert_same_bits(kp.cpu(), kp1, what + " kp")
        assert_same_bits(vp.cpu(), vp1, what + " vp")
        qa1, ka1 = relbias_aug(d, o, ts1.contiguous(), what)
        assert_same_bits(qa.cpu(), qa1.done(what + " qa"), what + " qa")
        assert_same_bits(ka.cpu(), ka1.done(what + " ka"), what + " ka")
        # block outputs and the prompt / token-parameter gradients
        assert_same_bits(y_b[i], y_s[i], what + " y")
        for name, a, b in zip(("dprompt", "d weights_token", "d enc_token"), g_b[3 * i:3 * i + 3], g_s[3 * i:3 * i + 3]):
            assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0, (what, name)
            assert_same_bits(a, b, f"{what} {name}")
        assert not bool(bits(g_b[3 * i + 2][n_p:]).any()), what + ": enc_token rows beyond Np take no gradient"


def test_a_single_eligible_block_stays_on_the_per_block_path():
    blocks = make_blocks(BLOCK_SPECS[:2], 77)
    (b0, p0, x0, _), (b1, p1, _, _) = blocks
    Fn.prepare_prompted_blocks([(b0, p0)])
    assert "_pre" not in b0.__dict__
    b1.attn_norm.weight.requires_grad_(True)                      # a trainable body makes the second block ineligible
    Fn.prepare_prompted_blocks([(b0, p0), (b1, p1)])
    assert "_pre" not in b0.__dict__ and "_pre" not in b1.__dict__
    y = b0(x0, p0)                                                # and the per-block path still runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.float()).all())
