"""CPU proof that the routing / tie equalities of tests/attn_ref.py see single (query, key) mistakes of the window attention
that the block-level bars (rel-L2 2e-3, max-abs 6e-2: test_hip_swin_block.py, test_hip_swin_bwd.py) do not.  Everything runs
on the float64 reference: each test corrupts the operands the way a kernel with one wrong index would, on a realistic random
block input AND on the exact operands.  On the realistic input the corruption must stay under the old bars, measured on
t1 = tokens + o (unit-variance tokens: the residual the block adds before anything is compared); on the exact operands it
must break the bit-equality.  Where a corruption was too loud for the bars at this shape it was shrunk, never the bars."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402
from mivp_amd.geometry import build_tables_numpy, mask_words_numpy  # noqa: E402

REL_BAR, ABS_BAR = 2e-3, 6e-2
DIMS, WIN, SHIFT = (14, 14, 14), (7, 7, 7), (3, 3, 3)
B, HEADS, HD, NP = 1, 4, 12, 64


@pytest.fixture(scope="module")
def cases():
    meta, (_, _, rid) = build_tables_numpy(DIMS, WIN, SHIFT)
    P, Nq = meta["P"], meta["Nq"]
    real = R.random_case("real", rid, P, Nq, WIN, B, HEADS, HD, NP)
    exact = R.build_case("exact", rid, P, Nq, WIN, B, HEADS, HD, NP, mode="tie").check()
    neg = R.build_case("exact_neg", None, P, Nq, WIN, B, HEADS, HD, NP, mode="route", L0=-40).check()
    drop = R.build_case("exact_drop", rid, P, Nq, WIN, B, HEADS, HD, NP, mode="route", g=128, L0=192, walk="any").check()
    gen = torch.Generator().manual_seed(5)
    keep = (torch.rand((real.BP, HEADS, real.Nqp, real.Nkp), generator=gen) >= 0.5)
    tok = torch.randn((real.BP, real.Nqp, real.C), generator=gen, dtype=R.F64)
    return dict(real=real, exact=exact, drop=drop, neg=neg, keep=keep, tok=tok)


def _judge(cases, mutate, which="exact", keep=None, keep_mut=None):
    """``mutate(case)`` corrupts a deep copy in place.  Returns the figures of the realistic input."""
    real, ex, tok = cases["real"], cases[which], cases["tok"]
    scale = 1.0 if keep is None else 2.0
    kw = {} if keep is None else dict(keep=keep, scale=scale)
    kwm = {} if keep is None else dict(keep=keep_mut, scale=scale)
    good = real.forward(**kw)[0][:, :real.Nq]
    bad_c = copy.deepcopy(real)
    mutate(bad_c)
    bad = bad_c.forward(**kwm)[0][:, :real.Nq]
    t1 = tok[:, :real.Nq] + good
    rel = float((bad - good).norm() / t1.norm())
    mx = float((bad - good).abs().max())
    print(f"realistic input: rel-L2 {rel:.2e} (bar {REL_BAR:g}), max-abs {mx:.2e} (bar {ABS_BAR:g})")
    assert 0 < rel < REL_BAR and mx < ABS_BAR, "the corruption is louder than the old bars: shrink the corruption"
    want = R.r16(ex.forward(**kw)[0][:, :ex.Nq])
    bad_e = copy.deepcopy(ex)
    mutate(bad_e)
    got = R.r16(bad_e.forward(**kwm)[0][:, :ex.Nq])
    nbad = int((got != want).sum())
    print(f"exact operands: {nbad} elements differ")
    assert nbad > 0, "the exact comparison did not see the corruption"
    return rel, mx


def test_flipped_mask_bit(cases):
    """(i) one flipped mask_words bit: one (query, key) pair of one window survives / is masked wrongly."""
    def mutate(c):
        lv = c.live().clone()
        n = 40
        m = int(c.extra["sel"][0, 0, n]) if "sel" in c.extra else 41
        if m >= c.Nq:
            n, m = 41, int(c.extra["sel"][0, 0, 41])
        lv[0, n, m] = ~lv[0, n, m]
        c.extra["live"] = lv
    _judge(cases, mutate)


def test_keys_swapped_across_tiles(cases):
    """(ii) keys 15 and 16 (the last key of one 16-key tile, the first of the next) swapped: K' rows of one window and head
    (head dims) and of that head (bias columns); v stays."""
    def mutate(c):
        c.k[0, 0, [15, 16]] = c.k[0, 0, [16, 15]]
        c.ka[0, [15, 16]] = c.ka[0, [16, 15]]               # (the bias columns of a head are shared by its windows)
    _judge(cases, mutate)


def test_padding_key_without_bias(cases):
    """(iii) one padding key (slot Nq) given bias 0 in one head.  Such a key sits at logit 0 like a masked one: only rows
    whose winners are BELOW zero see it, hence the routing case at L = -40 (un-shifted block: nothing else at 0)."""
    def mutate(c):
        c.ka[0, c.Nq, :] = 0
    _judge(cases, mutate, which="neg")


def test_prompt_row_63_read_as_62(cases):
    """(iv) prompt row 63 replaced by row 62 (keys, values and bias columns), one head."""
    def mutate(c):
        c.kp[0, 63], c.vp[0, 63] = c.kp[0, 62].clone(), c.vp[0, 62].clone()
        c.ka[0, c.Nqp + 63] = c.ka[0, c.Nqp + 62].clone()
    _judge(cases, mutate)


def test_windows_exchanged(cases):
    """(v) two windows' v exchanged for one head -- shrunk to ONE key (whole windows move t1 by 3e-2: the wrong window is
    served for that key only)."""
    def mutate(c):
        j = int(c.extra["sel"][0, 1, 7]) if "sel" in c.extra else 100
        j = j if j < c.Nq else int(c.extra["sel"][0, 1, 8])
        a, b = c.v[0, 1, j].clone(), c.v[1, 1, j].clone()
        c.v[0, 1, j], c.v[1, 1, j] = b, a
    _judge(cases, mutate)


def test_dropped_dropout_bit(cases):
    """(vi) one dropout bit taken from the wrong (query, key) index: the keep bit of one winner flipped."""
    keep = cases["keep"]
    ex = cases["drop"]
    n = 10
    j = int(ex.extra["sel"][0, 0, n])
    keep_mut = keep.clone()
    keep_mut[0, 0, n, j] = ~keep_mut[0, 0, n, j]
    _judge(cases, lambda c: None, which="drop", keep=keep, keep_mut=keep_mut)


@pytest.mark.parametrize("geom", [((14, 14, 14), (7, 7, 7), (3, 3, 3)), ((12, 12, 24), (7, 7, 7), (3, 3, 3)), "syn"])
def test_mask_words_agree_with_class_compare(geom):
    """mask_words_numpy (the table the forward kernel reads) against the class compare of attn_ref, bit by bit, on real
    geometries (padded-volume region id 100 included) and on a synthetic table with borders inside 16-slot tiles."""
    if geom == "syn":
        P, Nq, Nqp = 3, 343, 352
        rid = R.synthetic_rid(P, Nq, Nqp, [[5, 21, 200], [], [40, 339]])
    else:
        meta, (_, _, rid) = build_tables_numpy(*geom)
        P, Nq, Nqp = meta["P"], meta["Nq"], meta["Nqp"]
    c = R.Case(name="m", B=1, P=P, heads=1, hd=4, Nq=Nq, Nqp=Nqp, Np=0, Npp=0, Nkp=R.round_up(Nqp, 32), aug=0, augp=4,
               win=(7, 7, 7), has_mask=True, q=None, k=None, v=None, kp=None, vp=None, qa=None, ka=None,
               rid=np.asarray(rid).reshape(P, Nqp))
    live = c.live()[:, :, :Nqp].numpy()
    fwd, bwd, cut = mask_words_numpy(np.asarray(rid).reshape(-1), P, Nq, Nqp)
    nt = Nqp // 16
    bits = ((fwd[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)      # [P, qt, kt, j, 16 g + r]
    got = bits.reshape(P, nt, nt, 4, 4, 16).transpose(0, 1, 5, 2, 4, 3).reshape(P, Nqp, Nqp)      # [P, (qt, r), (kt, g, j)]
    assert (got == live).all()
    bitsb = ((bwd[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)     # bit 16 g + r: query 4 g + j, key r
    gotb = bitsb.reshape(P, nt, nt, 4, 4, 16).transpose(0, 1, 4, 3, 2, 5).reshape(P, Nqp, Nqp)
    assert (gotb == live).all()
    assert (cut == np.array([np.unique(np.asarray(rid).reshape(P, Nqp)[p, :Nq]).size > 1 for p in range(P)])).all()
