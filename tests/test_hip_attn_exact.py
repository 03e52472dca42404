"""Element-exact routing and tie tests of the window-attention kernels.

The C entries are called directly on operands built by tests/attn_ref.py: in every row a set W of 2^m keys holds the same
integer logit and every other key (masked keys at logit 0, padding keys, decoys of another region) sits >= 32 log2 units
below (asserted by ``Case.check``; 36 by construction at g = 18, 256 in the dropout and the g = 128 backward cases), so ``o`` is the mean of v over W -- a bf16 number -- and the stored output must be BIT-equal to it.  Preconditions
(a)-(d) are asserted on 100 % of the reference rows (``Case.check``) before any kernel output is looked at.

Measured against the float64 reference on an MI355X (worst over all cases; bars = 4 x, summation order may differ
between builds): see LSE_BAR / PART_BAR_EXACT / PART_BAR_G18 below and DESIGN.md 5.2.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd.geometry import build_tables_numpy, mask_words_numpy

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# |lse - float64| over the rows < Nq of every case: measured worst 3.464e-6 (tested-walk cases, lse = 184 ln 2 = 127.5, where
# one f32 ulp is 7.6e-6; 1.3e-6 in the ties at lse 62, 1.2e-7 in the routing rows at lse 44).  Bar = 4 x the worst.  An 8-way
# tie that lost or gained one key moves lse by ln(8/7) = 0.134: the bar must stay below half of it (asserted).
LSE_BAR = 1.4e-5
# f32 partials dkp_part / dtok_part / dka_part: max |got - ref| relative to max |ref| of the tensor, against float64.  Bars =
# 4 x the measured worst.  g = 128 cases: measured 0 everywhere -- every product and partial sum is a dyadic rational that
# f32 holds in any summation order -- so equality is asserted.  g = 18 case: see the figures beside each bar.  Every bar is
# asserted to stay below half the smallest change that moving one (query, key) pair makes (one_pair_change, per case).
PART_BAR_EXACT = {"dkp_part": 0.0, "dtok_part": 0.0, "dka_part": 0.0}
# g = 18 (bwd_tie_hd12_cut_g18), measured worst over the implementations: dkp_part 2.833e-10, dtok_part 1.533e-10, dka_part
# 1.489e-8 (one-pair changes 5.0e-4, 5.5e-4, 5.5e-4)
PART_BAR_G18 = {"dkp_part": 1.2e-9, "dtok_part": 6.2e-10, "dka_part": 6.0e-8}

GEOMS = {
    "g14": ((14, 14, 14), (7, 7, 7), (0, 0, 0)),
    "g14s": ((14, 14, 14), (7, 7, 7), (3, 3, 3)),
    "g21s": ((21, 21, 7), (7, 7, 7), (3, 3, 3)),
    "g16s": ((16, 16, 8), (8, 8, 4), (4, 4, 2)),
    "g8s": ((8, 8, 4), (4, 4, 2), (2, 2, 1)),
    "gsm": ((6, 6, 4), (3, 3, 2), (0, 0, 0)),
    "gsms": ((6, 6, 4), (3, 3, 2), (1, 1, 1)),
    "gpad": ((12, 12, 24), (7, 7, 7), (3, 3, 3)),           # padded to (14, 14, 28): region id 100
}
# name: (geometry | "syn", B, heads, head_dim, Np, mode, walk, g, fp8).  Work items B P heads: 32 (< 64), 64 (remap on),
# 108 (>= 64, not a multiple of 8).  head_dim 12 = DKS 1 + ones row, 24 = DKS 2 + ones row, 48 = DKS 3, no ones row.
CASES = {
    "route_hd12_cut": ("g14s", 1, 4, 12, 64, "route", "optimistic", 18, False),
    "route_hd12_cut_tested": ("g14s", 1, 4, 12, 64, "route", "tested", 18, False),
    "route_hd12_neg": ("g14", 1, 4, 12, 64, "route", "optimistic", 18, False),      # L = -40: a padding key at 0 would win
    "tie_hd12": ("g14", 1, 4, 12, 64, "tie", "optimistic", 18, False),
    "route_hd12_b3_np0": ("g21s", 3, 4, 12, 0, "route", "optimistic", 18, False),
    "route_hd24_remap": ("g14s", 2, 4, 24, 64, "route", "optimistic", 18, False),
    "tie_hd24": ("g14", 1, 4, 24, 64, "tie", "optimistic", 18, False),
    "route_hd48_cut": ("g14s", 1, 2, 48, 64, "route", "optimistic", 18, False),
    "tie_hd48_tested": ("g14", 1, 2, 48, 64, "tie", "tested", 18, False),
    "route_w884_remap": ("g16s", 2, 4, 12, 64, "route", "optimistic", 18, False),
    "tie_w442_cut": ("g8s", 1, 4, 12, 16, "tie", "optimistic", 18, False),
    "tie_small_cut": ("gsms", 1, 2, 4, 8, "tie", "optimistic", 18, False),
    "route_pad100": ("gpad", 1, 4, 12, 64, "route", "optimistic", 18, False),
    "route_syn": ("syn", 1, 4, 12, 64, "route", "optimistic", 18, False),
    "tie_syn": ("syn", 1, 4, 12, 64, "tie", "optimistic", 18, False),
    # the corner window of (14,14,14) at shift 3 with its 4x4x4 region kept and the seven others merged: the 279 rows of the
    # merged region have every surviving key at -40 and are carried by the 64 masked keys at logit 0 (a real table cannot
    # give this: there a row's masked keys are ALL other regions, 279 or more keys, whose mean is not a bf16 number)
    "allmasked_corner": ("syn64", 1, 4, 12, 64, "route", "optimistic", 18, False),
    "route_drop_cut": ("g14s", 1, 4, 12, 64, "route", "any", 128, False),
    "tie_drop": ("g14", 1, 4, 12, 64, "tie", "any", 128, False),
    "route_small_fp8": ("gsm", 1, 2, 4, 8, "route", "optimistic", 18, True),
    "route_hd12_fp8": ("g14", 1, 4, 12, 64, "route", "optimistic", 18, True),
}
# Backward cases: g = 128 and L >= 256, so that every loser AND every masked key (logit 0) underflows to exactly 0 in
# P = exp2(S - lse).  With the 2^-36 losers of the forward cases the f32 partials and the cancelling dv entries came out one
# f32 ulp (2^-24 at 0.5) off the exact rational on the MI355X: the bf16 MFMA aligns its 32 products to the largest addend and
# does not round the absorbed ones to nearest, so "bit-equal" holds only where nothing is absorbed inside the accumulator.
for _n, _geo, _h, _hd, _np, _mode in (("bwd_tie_hd12", "g14", 4, 12, 64, "tie"), ("bwd_route_hd12_cut", "g14s", 4, 12, 64, "route"),
                                      ("bwd_tie_hd12_cut", "g14s", 4, 12, 64, "tie"), ("bwd_tie_hd24", "g14", 4, 24, 64, "tie"),
                                      ("bwd_tie_hd48", "g14", 2, 48, 64, "tie"), ("bwd_tie_w442_cut", "g8s", 4, 12, 16, "tie"),
                                      ("bwd_tie_small_cut", "gsms", 2, 4, 8, "tie")):
    CASES[_n] = (_geo, 1, _h, _hd, _np, _mode, "any", 128, False)
# ... and one backward case on the forward operands (g = 18, ties at 90 ... 36 in a cut window): the losers and the masked
# keys keep P of 2^-36 and more, so the mask multiply of the backward kernels meets non-zero masked probabilities and
# decoys above the winner.  Nothing is bit-equal there; every output is held to the neighbour rule / the measured bars.
CASES["bwd_tie_hd12_cut_g18"] = ("g14s", 1, 4, 12, 64, "tie", "optimistic", 18, False)
FWD = [n for n in CASES if "drop" not in n and "fp8" not in n and "bwd" not in n]
BWD = [n for n in CASES if n.startswith("bwd_")]


@functools.lru_cache(maxsize=None)
def case(name):
    geom, B, heads, hd, Np, mode, walk, g, fp8 = CASES[name]
    carried = None
    if geom == "syn64":
        meta, (_, _, rid) = build_tables_numpy(*GEOMS["g14s"])
        win, P, Nq = (7, 7, 7), 1, meta["Nq"]
        rid = np.asarray(rid).reshape(meta["P"], -1)
        ids, cnt = np.unique(rid[0, :Nq], return_counts=True)     # window 0 holds the 4x4x4 region of the shifted grid
        carried = int(ids[cnt == 64][0])
        rid = np.where(rid[0] == carried, carried, carried + 1).astype(np.int32)[None]
        rid[0, Nq:] = 0
    elif geom == "syn":
        # borders inside 16-slot tiles (slots 5, 21, 40, 200, 339) and one uncut window
        win, P, Nq = (7, 7, 7), 3, 343
        rid = R.synthetic_rid(P, Nq, 352, [[5, 21, 200], [], [40, 339]])
    else:
        dims, win, shift = GEOMS[geom]
        meta, (_, _, rid) = build_tables_numpy(dims, win, shift)
        P, Nq = meta["P"], meta["Nq"]
        if not meta["has_mask"]:
            rid = None
    L0 = None
    if g == 128:                      # dropout: every loser underflows to exactly 0 (gap 256), a dropped winner leaves o = 0;
        L0 = 192 if rid is not None else 64                   # masked keys sit at logit 0: the winner must be 150 above them too
    if name.startswith("bwd_") and g == 128:
        L0 = 640                      # ties at 640, 512, 384, 256
    if name == "route_hd12_neg":
        L0 = -40
    if name == "route_hd12_fp8":      # the keys' offset L0 - 9 g must be an E4M3 number: 66 - 162 = -96
        L0 = 66
    c = R.build_case(name, rid, P, Nq, win, B, heads, hd, Np, mode=mode, g=g, L0=L0, walk=walk, fp8=fp8,
                     vbase=16 if fp8 else 32, carried=carried)
    return c.check()                  # (a)-(d) on every row, before any kernel runs


def make_desc(c, drop=False):
    d = L.SwinDesc()
    d.B, d.C, d.heads = c.B, c.C, c.heads
    d.vol_in = d.vol_out = c.P * c.Nq
    d.P, d.Nq, d.Nqp, d.Np, d.Npp, d.Nkp = c.P, c.Nq, c.Nqp, c.Np, c.Npp, c.Nkp
    d.aug, d.augp, d.has_mask = c.aug, c.augp, 1 if c.has_mask else 0
    for a in range(3):
        d.win[a] = c.win[a]
    d.q_scale, d.ln_eps = float(c.hd ** -0.5), 1e-6
    if drop:                          # attn_drop p = 0.5: thr 32768, scale exactly 2
        d.attn_drop_thr, d.attn_drop_scale, d.attn_seed = 32768, 2.0, 0x1234567
    return d


def gpu(t, dtype=BF16):
    return None if t is None else t.to(dtype).cuda().contiguous()


@functools.lru_cache(maxsize=None)
def operands(name):
    c = case(name)
    ops = dict(q=gpu(c.q), k=gpu(c.k), v=gpu(c.v), kp=gpu(c.kp), vp=gpu(c.vp), qa=gpu(c.qa), ka=gpu(c.ka),
               rid=torch.from_numpy(c.rid.reshape(-1).copy()).cuda(), words=None, cut=None)
    if c.has_mask:
        fwd, _, cut = mask_words_numpy(c.rid.reshape(-1), c.P, c.Nq, c.Nqp)
        ops["words"] = torch.from_numpy(fwd.view(np.int64)).cuda()
        ops["cut"] = torch.from_numpy(cut).cuda()
    return ops


def run_fwd(name, save, words=True, drop=False, fp8=False):
    c, t = case(name), operands(name)
    d = make_desc(c, drop)
    o = torch.full((c.BP, c.Nqp, c.C), float("nan"), dtype=BF16, device="cuda")
    lse = torch.full((c.BP, c.heads, c.Nqp), float("nan"), dtype=torch.float32, device="cuda") if save else None
    if fp8:
        L.call("mivp_win_attn_fwd_fp8", C.byref(d), L.ptr(t["q"]), L.ptr(t["k"]), L.ptr(t["v"]), L.ptr(t["kp"]), L.ptr(t["vp"]),
               L.ptr(t["qa"]), L.ptr(t["ka"]), L.ptr(t["rid"]), L.ptr(o), L.ptr(lse), L.stream())
    else:
        L.call("mivp_win_attn_fwd", C.byref(d), L.ptr(t["q"]), L.ptr(t["k"]), L.ptr(t["v"]), L.ptr(t["kp"]), L.ptr(t["vp"]),
               L.ptr(t["qa"]), L.ptr(t["ka"]), L.ptr(t["rid"]), L.ptr(o), L.ptr(lse),
               L.ptr(t["words"] if words else None), L.ptr(t["cut"] if words else None), L.stream())
    torch.cuda.synchronize()
    return o.cpu().to(R.F64), (None if lse is None else lse.cpu().to(R.F64))


@functools.lru_cache(maxsize=None)
def ref_fwd(name):
    o, lse, _ = case(name).forward()
    return o, lse


def assert_rows_equal(got, want, Nq, what):
    """Bit-equality of the rows < Nq with the reference rounded to bf16 (it IS a bf16 number there: condition (c))."""
    g, w = got[:, :Nq], R.r16(want[:, :Nq])
    bad = g != w
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}: " \
                                f"{float(g[bad][0])} != {float(w[bad][0])}"


def lse_step(c):
    """The smallest change of lse that one (query, key) pair moving into or out of a row's winner set makes, over the rows
    of the case: ln((w + 1) / w) for a gained key (ln(w / (w - 1)) for a lost one is larger)."""
    return float(torch.log((c.nwin + 1) / c.nwin).min())


@pytest.mark.parametrize("name", FWD)
def test_forward_exact(name):
    """o[n < Nq] is bit-equal to the mean of v over the winners: with lse saved (first-step maximum), with lse = NULL (zero
    reference point), and for shifted blocks with mask words + cut flags and with both NULL (class compare).  Every masked
    key of the other region group is a decoy with a raw logit >= 72 above the winner (asserted below on every cut row)."""
    c = case(name)
    want, lse_ref = ref_fwd(name)
    if c.has_mask and c.extra["carried"] is None:
        raw, S = c.raw_logits()[:, :, :c.Nq], c.logits()[:, :, :c.Nq]
        decoy = ((raw >= c.L[..., None] + 32) & (S == 0)).any(-1)
        cutw = torch.from_numpy(np.array([np.unique(c.rid[p, :c.Nq]).size > 1 for p in range(c.P)]))
        assert bool(decoy[cutw.repeat(c.B)].all()), "every row of a cut window must see a masked decoy above its winner"
    for words in ((True, False) if c.has_mask else (True,)):
        o, lse = run_fwd(name, save=True, words=words)
        assert_rows_equal(o, want, c.Nq, f"{name} lse saved, words={words}")
        err = float((lse - lse_ref)[:, :, :c.Nq].abs().max())
        print(f"MEASURE {name} words={words} lse_err {err:.3e} (lse max {float(lse_ref[:, :, :c.Nq].abs().max()):.2f})")
        assert LSE_BAR < 0.5 * lse_step(c)
        assert err <= LSE_BAR, err
        o0, _ = run_fwd(name, save=False, words=words)
        assert_rows_equal(o0, want, c.Nq, f"{name} lse NULL, words={words}")


@pytest.mark.parametrize("name", ["route_drop_cut", "tie_drop"])
def test_forward_dropout_exact(name):
    """attn_drop p = 0.5 (thr 32768, scale exactly 2) with the masks mivp_dropout_masks exports: a routing row is 2 v[sel]
    where the winner is kept and exactly 0 where it is dropped (the losers sit 256 below: they underflow), a tie row is the
    kept winners' sum times 2 / |W|."""
    c = case(name)
    d = make_desc(c, drop=True)
    keep = torch.empty((c.BP * c.heads, c.Nqp, c.Nkp), dtype=torch.uint8, device="cuda")
    L.call("mivp_dropout_masks", C.byref(d), L.ptr(keep), L.ptr(None), L.stream())
    torch.cuda.synchronize()
    keep = keep.cpu().reshape(c.BP, c.heads, c.Nqp, c.Nkp)
    frac = float(keep.double().mean())
    assert 0.45 < frac < 0.55, frac
    want, _, _ = c.forward(keep=keep, scale=2.0)
    assert R.near_bf16(want[:, :c.Nq])                       # (c) for the dropped-out means
    W = R.winners(c)
    kept = (W & (keep[:, :, :c.Nq] != 0)).sum(-1)
    assert bool((kept == 0).any()) and bool((kept == c.nwin).any())      # both a fully dropped and a fully kept row occur
    o, _ = run_fwd(name, save=True, drop=True)
    assert_rows_equal(o, want, c.Nq, name)
    gone = (kept == 0).permute(0, 2, 1)[..., None].expand(-1, -1, -1, c.hd).reshape(c.BP, c.Nq, c.C)
    assert bool((o[:, :c.Nq][gone] == 0).all())


@pytest.mark.parametrize("name", ["route_small_fp8", "route_hd12_fp8"])
def test_forward_fp8_exact(name):
    """E4M3 forward, routing case, operands restricted to E4M3 numbers (the padding bias is given as -448, where the kernel
    saturates it anyway).  The kernel applies no scale at all -- q, k', v and P = exp2(s - reference) with an integer
    reference are converted as they are, P is a power of two <= 2^8 on the winner and rounds to 0 elsewhere -- so the result
    is bit-equal."""
    c = case(name)
    want, lse_ref = ref_fwd(name)
    o, lse = run_fwd(name, save=True, fp8=True)
    assert_rows_equal(o, want, c.Nq, name)
    err = float((lse - lse_ref)[:, :, :c.Nq].abs().max())
    print(f"MEASURE {name} lse_err {err:.3e}")
    assert err <= LSE_BAR, err


def ulp16(x):
    """bf16 spacing at |x| (float64 tensor)."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 7)


def assert_neighbour(got, ref, floor, what):
    """Each bf16 output is the reference rounded to bf16 or its neighbour (entries under ``floor`` -- the absorbed keys'
    share -- compare absolutely)."""
    tol = torch.maximum(ulp16(ref), torch.zeros_like(ref) + floor)
    bad = (got - ref).abs() > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} off, worst {float(((got - ref).abs() / tol).max()):.2f} ulp"


def run_bwd(name, impl, o16, lse32, d_o):
    c, t = case(name), operands(name)
    d = make_desc(c)
    dev = "cuda"
    nan16 = lambda *s: torch.full(s, float("nan"), dtype=BF16, device=dev)
    nan32 = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    out = {}
    BPH = c.BP * c.heads
    if c.Np:
        out["dkp_part"], out["dvp_part"] = nan32(BPH, c.Npp, c.hd), nan32(BPH, c.Npp, c.hd)
        out["dtok_part"] = nan32(BPH, c.Npp)
    part = [L.ptr(out.get("dkp_part")), L.ptr(out.get("dvp_part")), L.ptr(out.get("dtok_part"))]
    common = [L.ptr(t["q"]), L.ptr(t["k"]), L.ptr(t["v"]), L.ptr(t["kp"]), L.ptr(t["vp"]), L.ptr(t["qa"]), L.ptr(t["ka"]),
              L.ptr(t["rid"])]
    if impl == "two_pass":
        out["delta"] = nan32(c.BP, c.heads, c.Nqp)
        out["dq"], out["dk"], out["dv"] = (nan16(c.BP, c.heads, c.Nqp, c.hd) for _ in range(3))
        out["dka_part"] = nan32(BPH, c.Nkp, 32)
        L.call("mivp_win_attn_bwd_dq", C.byref(d), *common, L.ptr(o16), L.ptr(d_o), L.ptr(lse32), L.ptr(out["delta"]),
               L.ptr(out["dq"]), L.stream())
        L.call("mivp_win_attn_bwd_dkv", C.byref(d), *common, L.ptr(d_o), L.ptr(lse32), L.ptr(out["delta"]), L.ptr(out["dk"]),
               L.ptr(out["dv"]), *part, L.ptr(out["dka_part"]), L.stream())
    elif impl == "fused":
        out["dq"], out["dk"], out["dv"] = (nan16(c.BP, c.heads, c.Nqp, c.hd) for _ in range(3))
        L.call("mivp_win_attn_bwd_fused", C.byref(d), *common, L.ptr(o16), L.ptr(d_o), L.ptr(lse32), L.ptr(out["dq"]),
               L.ptr(out["dk"]), L.ptr(out["dv"]), *part, L.stream())
    else:
        L.call("mivp_win_attn_bwd_prompt", C.byref(d), L.ptr(t["q"]), L.ptr(t["kp"]), L.ptr(t["vp"]), L.ptr(t["qa"]),
               L.ptr(t["ka"]), L.ptr(o16), L.ptr(d_o), L.ptr(lse32), *part, L.stream())
    torch.cuda.synchronize()
    return {k2: v2.cpu().to(R.F64).reshape(c.BP, c.heads, *v2.shape[1:]) if v2.shape[0] == BPH else v2.cpu().to(R.F64)
            for k2, v2 in out.items()}


def one_pair_change(c, ref, key):
    """The smallest change that moving ONE (query, key) pair makes in an f32 partial, relative to the tensor's largest
    entry (the unit of the bars): |dS[n, j]| for dtok_part, |dS[n, j]| max|q[n]| for dkp_part, |dS[n, j]| max|qa[n]| for
    dka_part, over the pairs whose dS is not absorbed (a winner whose dP equals delta contributes nothing either way)."""
    dS = ref["dS"][:, :, :c.Nq].abs()
    if key == "dka_part":
        chg = dS * c.qa[:c.Nq].abs().amax(-1)[None, None, :, None]
    else:
        dS = dS[..., c.Nqp:c.Nqp + c.Npp]
        chg = dS * c.q[:, :, :c.Nq].abs().amax(-1)[..., None] if key == "dkp_part" else dS
    return float(chg[dS > 2.0 ** -20].min()) / float(ref[key].abs().max())


@pytest.mark.parametrize("name", BWD)
def test_backward_exact(name):
    """Integer dO (+-1 in one channel per row and head), the reference's o (a bf16 number) and lse (rounded to f32) as saved
    tensors, for every implementation whose ``_supported`` says yes.  The g = 128 cases are exact throughout (every loser
    and masked key has P = 0 in f32, every product and partial sum is a dyadic rational that f32 holds in any order); the
    g = 18 case runs the forward operands -- non-zero masked probabilities, decoys above the winner -- under the neighbour
    rule and the measured bars."""
    c = case(name)
    exact = c.extra["g"] == 128
    d = make_desc(c)
    impls = ["two_pass"]
    if L.lib().mivp_win_attn_bwd_fused_supported(C.byref(d)):
        impls.append("fused")
    if c.Np and L.lib().mivp_win_attn_bwd_prompt_supported(C.byref(d)):
        impls.append("prompt")
    if c.hd <= 16:
        assert "fused" in impls, "head_dim <= 16 is the fused kernel's range"
    want_o, lse_ref = ref_fwd(name)
    o16 = R.r16(want_o)
    o16[:, c.Nq:] = 0
    dO = R.int_grad(c)
    ref = c.backward(dO)
    route = bool((c.nwin == 1).all())
    # what the losers can add: their share (b) of the row times the largest |dP - delta| and |k'| / |q|
    Pm = c.forward()[2][:, :, :c.Nq]
    lose = float((Pm * (~R.winners(c))).sum(-1).max())
    assert lose <= 2.0 ** -29
    K, V = c.keys()
    span = 2.0 * float(V.abs().max())
    floor_q = 1.05 * lose * span * float(K.abs().max()) * R.LN2
    floor_k = 1.05 * lose * span * float(c.q.abs().max()) * c.Nq
    # dv / dvp_part = sum_n P[n, j] dO[n]: the losers' share, and for g = 18 (P of a winner is 1 / |W| less 2^-31 or so,
    # so the sum no longer cancels exactly) one f32 rounding per added row of the largest column sum of |P dO|
    floor_v = 1.05 * lose * c.Nq
    if not exact:
        floor_v += c.Nq * 2.0 ** -23 * float(Pm.sum(2).max())
        assert floor_v < 0.5 / 8                                 # half of what one pair moves in dv: dO / |W| >= 1 / 8
    acc_q = acc_k = 0.0
    if not exact:
        # ... and the f32 accumulation of each dot product, elementwise: n 2^-24 sum |terms| (n adds, each rounding at most
        # half an ulp of a partial sum that the sum of magnitudes bounds) -- it matters where the winners' terms cancel
        dSa = ref["dS"].abs()
        acc_q = (c.Nkp * 2.0 ** -24 * R.LN2 * (dSa @ K.abs()))[:, :, :c.Nq]
        acc_k = (c.Nq * 2.0 ** -24 * (dSa[:, :, :c.Nq].transpose(-1, -2) @ c.q[:, :, :c.Nq].abs()))[:, :, :c.Nq]
    bars = PART_BAR_EXACT if exact else PART_BAR_G18
    o_dev, lse_dev, dO_dev = gpu(o16), gpu(lse_ref, torch.float32), gpu(dO)
    got, late = {}, []
    for impl in impls:
        g = got[impl] = run_bwd(name, impl, o_dev, lse_dev, dO_dev)
        tag = f"{name}/{impl}"
        if "delta" in g:                                         # exact: integers times bf16 means of small integers
            want = (dO.reshape(c.BP, c.Nqp, c.heads, c.hd) * o16.reshape(c.BP, c.Nqp, c.heads, c.hd)).sum(-1).permute(0, 2, 1)
            assert bool((g["delta"][:, :, :c.Nq] == want[:, :, :c.Nq]).all()), tag
        if "dv" in g:                                            # scatter-add of dO / |W| over the rows that chose the key
            dv_ref = ref["dv"][:, :, :c.Nq]
            gv = g["dv"][:, :, :c.Nq]
            if exact:
                big = dv_ref.abs() >= 2.0 ** -10
                assert R.near_bf16(torch.where(big, dv_ref, torch.zeros_like(dv_ref)))        # (c)
                assert bool((gv[big] == R.r16(dv_ref)[big]).all()), f"{tag} dv"
                assert bool((gv[~big].abs() <= floor_v).all()), f"{tag} dv of unselected keys"
            else:
                assert_neighbour(gv, dv_ref, floor_v, f"{tag} dv")
        if c.Np:
            dvp = ref["dvp_part"]
            if exact:
                big = dvp.abs() >= 2.0 ** -10
                grid = (dvp * 64).round() / 64
                assert bool(((grid - dvp).abs() <= 2.0 ** -20)[big].all())                    # (c): multiples of 1 / |W|
                assert bool((g["dvp_part"][big] == grid[big]).all()), f"{tag} dvp_part"
                assert bool((g["dvp_part"][~big].abs() <= floor_v).all()), f"{tag} dvp_part of unselected keys"
            else:
                assert bool(((g["dvp_part"] - dvp).abs() <= floor_v).all()), f"{tag} dvp_part"
        if route:
            # the winner's dS is exactly 0 (delta = dO . v[sel] = its dP): what is left is the losers' share
            for key, fl in (("dq", floor_q), ("dk", floor_k)):
                if key in g:
                    assert float(g[key][:, :, :c.Nq].abs().max()) <= fl, (tag, key, fl)
        else:
            if "dq" in g:
                for key, fl in (("dq", floor_q + acc_q), ("dk", floor_k + acc_k)):
                    try:                                         # (reported after the partials' figures have been printed)
                        assert_neighbour(g[key][:, :, :c.Nq], ref[key][:, :, :c.Nq], fl, f"{tag} {key}")
                    except AssertionError as e:
                        late.append(str(e))
            for key in ("dkp_part", "dtok_part", "dka_part"):
                if key in g:
                    scale = float(ref[key].abs().max())
                    # (g = 128: against the reference rounded to f32 -- float64 keeps the 2^-256 losers that f32 cannot hold)
                    want = ref[key].to(torch.float32).to(R.F64) if exact else ref[key]
                    err = float((g[key] - want).abs().max()) / scale
                    step = one_pair_change(c, ref, key)
                    print(f"MEASURE {tag} {key} rel_err {err:.3e} (scale {scale:.3g}, one-pair change {step:.3e}, bar {bars[key]:.3e})")
                    assert bars[key] < 0.5 * step, (tag, key, bars[key], step)
                    if err > bars[key]:
                        late.append((tag, key, err, bars[key]))
    assert not late, late
    # the implementations agree with each other: the same bits where the reference is met exactly, else twice the bar
    # (each is within one bar of the reference)
    for impl in impls[1:]:
        for key, val in got[impl].items():
            base = got["two_pass"][key]
            if key in ("dq", "dk") or (key == "dv" and not exact):
                fl = 2 * (floor_v if key == "dv" else max(floor_q, floor_k))
                tol = torch.maximum(2 * ulp16(base), torch.full_like(base, fl))
                assert bool(((val - base).abs() <= tol)[:, :, :c.Nq].all()), (impl, key)
            elif key == "dv":
                assert bool((val[:, :, :c.Nq] == base[:, :, :c.Nq]).all()), (impl, key)
            elif key == "dvp_part":
                assert float((val - base).abs().max()) <= (0.0 if exact else 2 * floor_v), (impl, key)
            else:
                scale = float(ref[key].abs().max())
                assert float((val - base).abs().max()) / scale <= 2 * bars[key], (impl, key)
