"""The C = 48 gather + LayerNorm + QKV forward with several tile pairs per wave (k_swin_qkv_fwd<2, true>),
through mivp_swin_qkv_fwd with the cases, the reference (tests/tok_ref.py) and the located-parity bound of
tests/test_hip_tok_kernels.py.

A wave owns R = QKV_C48_PAIRS = 2 consecutive pairs of 16-token tiles and a workgroup 4 R = 8; the launcher takes this
kernel only when the token count alone fills the machine (one column split: at least 1024 workgroups of the generic grid,
T > 130 944), so the smallest pair counts that reach it are 4093 and up, and what a tile loop can get wrong is chosen by the
pair count's remainder, not by its size (Nqp = 32: a window is one pair, pairs = B * P):

  pairs % 8 == 0   4096   the grid ends exactly with a full workgroup
  pairs % 8 == 1   4097   one pair in the last workgroup: its first wave holds fewer pairs than R, the other three leave
  pairs % 8 == 3   4099   the last live wave is half full (pairs % R == 1)
  pairs % 8 == 5   4093   two full waves, a half-full one, a dead one

Every case has padded slots (source -2: zero rows), zero-padding tokens (source -1: LayerNorm's beta through the GEMM, in
the first, a middle and the last position) and a permuted gather order (tok_ref.make_tables), NaN in every x row that no
source names, NaN-filled outputs with a guard tail (every row of [0, T) written, nothing behind it).

Position independence: the 4093 windows of one volume, replicated at B = 3 and B = 5, give in every replica the bits of
B = 1.  4093 is odd, so a window that is the first pair of its wave in one replica is the second in the next, and replica
b starts in wave (4093 b / 2) % 4 of its workgroup."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tok_ref as T  # noqa: E402
from test_hip_prompt_path import DEV, Out, assert_same_bits  # noqa: E402
from test_hip_tok_kernels import BF16, Case, margin, qkv_fwd_arm, run_qkv_fwd, subset_rows  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import swin_ops

pytestmark = pytest.mark.gpu
R = 2                                                                     # QKV_C48_PAIRS (swin_fwd.hip)
CC, HEADS, NQP = 48, 4, 32
_cases = {}


def case(BP):
    if BP not in _cases:
        assert qkv_fwd_arm(CC, HEADS, NQP, BP) == "ch12"
        _cases[BP] = Case(CC, HEADS, NQP, BP)
    return _cases[BP]


@pytest.mark.parametrize("BP", [4096, 4097, 4099, 4093], ids=lambda bp: f"pairs{bp}_mod8_{bp % 8}")
def test_ragged_tail_and_grid_clamp(BP):
    pairs = BP * NQP // 32
    assert pairs == BP and pairs % (4 * R) == {4096: 0, 4097: 1, 4099: 3, 4093: 5}[BP]
    c = case(BP)
    d, o = c.d, c.o
    assert bool((c.src == -1).any()) and bool((c.src == -2).any())
    q, k, v = run_qkv_fwd(c, c.x_dev())                                   # Out.done: all of [0, T) written, the guard untouched
    what = f"qkv_fwd ch12 pairs={pairs} B={c.B} P={c.P}"
    T.check_qkv_structure(d, c.src, q, k, v, what)
    ref = T.qkv_fwd(d, o.x, c.src, o.ln1_w, o.ln1_b, o.Wq, o.Wk, o.Wv)
    rows = subset_rows(c.T)                                               # among them the first and the last 256 token rows
    pick = lambda t: t.permute(0, 2, 1, 3).reshape(c.T, d.C)[rows]
    m = {n: T.check_interval(pick(g), pick(getattr(ref, n)), pick(getattr(ref, "b" + n)), f"{what} {n} [token row][channel]")
         for n, g in zip("qkv", (q, k, v))}
    margin("qkv_fwd", f"ch12 pairs % 8 = {pairs % 8}", **m)


def test_position_independence():
    c = case(4093)
    assert c.B == 1 and c.P % R == 1
    x1 = c.x_dev()
    base = run_qkv_fwd(c, x1)
    hd = CC // HEADS
    for B in (3, 5):
        d = swin_ops._fill_desc(B, CC, HEADS, (NQP - 3, 1, 1), c.P, NQP - 3, NQP, c.vol, 0, False)
        assert qkv_fwd_arm(CC, HEADS, NQP, B * c.P) == "ch12" and (B * c.P) % (4 * R) != 0
        xB = x1.repeat(B, 1, 1).contiguous()
        outs = [Out((B * c.P, HEADS, NQP, hd), BF16) for _ in range(3)]
        L.call("mivp_swin_qkv_fwd", C.byref(d), L.ptr(xB), L.ptr(c.src_d), L.ptr(c.ln1[0]), L.ptr(c.ln1[1]),
               L.ptr(c.img["wqkv_f"].t), L.ptr(outs[0].t), L.ptr(outs[1].t), L.ptr(outs[2].t), L.stream())
        torch.cuda.synchronize()
        for name, out, one in zip("qkv", outs, base):
            got = out.done(f"qkv_fwd ch12 B={B} {name}")
            for b in range(B):
                assert_same_bits(got[b * c.P:(b + 1) * c.P], one, f"qkv_fwd ch12 {name}: replica {b} of B={B} against B=1")
