"""Direct parity tests of the input-side kernels against tests/input_prompt_ref.py (float64, CPU), each entry called through
``_lib.call`` on its own operands: mivp_patch_embed_dgrad, mivp_input_prompt_fwd, mivp_input_prompt_bwd.

Kinds of assertion (no bar is a measured figure):
  exact   dgrad on integer operands (dz and w in -2 .. 2: every partial sum is an integer below 2^24, exact in fp32 in any
          order): bit-equal to float64, the first wrong element named as (b, ci, h, w, d); every element written, nothing around
          the buffer touched.  The full-resolution prompt (lattice == roi, every weight 0 or 1): x + P in the bits forward, the
          fixed-order batch sum of input_prompt_ref.identity_bwd_f32 backward.
  E32     the interpolating prompt cases: E32 = max |float32 eager torch composition - float64| on the same operands
          (x + scale * F.interpolate(P, align_corners=True) and its autograd, on the CPU); every element within 8 E32.
  equal   two equal calls give equal bits.
  refusal the error code, every output untouched."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import input_prompt_ref as R  # noqa: E402
from test_hip_prompt_path import DEV, Out, assert_same_bits, dev  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import ops

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EINVAL = r"failed with code -1"
CANARY = 12345.0                                  # no sum of at most 48 products of values in -2 .. 2 reaches it


def embed_desc(B, Cin, dims, Cc, nblk):
    d = L.EmbedDesc()
    d.B, d.Cin, d.C, d.nblk = B, Cin, Cc, nblk
    for a in range(3):
        d.dims[a] = dims[a]
    return d


def ints(g, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


# (B, Cin, dims, C, nblk or None for the wrapper's, note)
DGRAD = [(1, 1, (2, 2, 2), 8, 1, "one_voxel"),
         (2, 3, (6, 10, 14), 48, None, "105_voxels_per_sample"),
         (3, 1, (16, 16, 16), 48, 2, "stride_walk_wraps"),
         (2, 2, (4, 6, 10), 16, None, "distinct_dims_canary")]


@pytest.mark.parametrize("B,Cin,dims,Cc,nblk,note", DGRAD, ids=[f"{c[5]}-B{c[0]}_Cin{c[1]}_{'x'.join(map(str, c[2]))}_C{c[3]}" for c in DGRAD])
def test_patch_embed_dgrad_exact(B, Cin, dims, Cc, nblk, note):
    n_out = B * math.prod(dims) // 8
    if nblk is None:
        nblk = ops._nblk(n_out * (Cc // 8), Cc // 8, cap=2048)
    if note == "stride_walk_wraps":
        assert n_out >= 3 * nblk * 256                                 # three rounds of the grid-stride walk
    if note == "105_voxels_per_sample":
        assert n_out // B == 105 and n_out % 256 != 0
    if note == "distinct_dims_canary":
        assert len(set(dims)) == 3
    g = torch.Generator().manual_seed(n_out + Cc)
    dz = ints(g, (B, dims[0] // 2, dims[1] // 2, dims[2] // 2, Cc))
    w = ints(g, (Cc, Cin, 2, 2, 2))
    ref = R.embed_dgrad(dz.numpy(), w.numpy())
    assert float(np.abs(ref).max()) <= 4 * Cc < 2 ** 24 and np.array_equal(ref, np.round(ref))
    n = B * Cin * math.prod(dims)
    guard = 64
    buf = torch.full((guard + n + guard,), CANARY, dtype=F32, device=DEV)   # a canary in front of, inside and behind dx
    dx = buf[guard:guard + n].view(B, Cin, *dims)
    d = embed_desc(B, Cin, dims, Cc, nblk)
    dz_d, w_d = dev(dz, BF16), dev(w)
    what = f"patch_embed_dgrad B={B} Cin={Cin} dims={dims} C={Cc} nblk={nblk}"
    L.call("mivp_patch_embed_dgrad", C.byref(d), L.ptr(dz_d), L.ptr(w_d), L.ptr(dx), L.stream())
    torch.cuda.synchronize()
    flat = buf.cpu()
    assert bool((flat[:guard] == CANARY).all()) and bool((flat[guard + n:] == CANARY).all()), what + ": wrote outside dx"
    got = flat[guard:guard + n].view(B, Cin, *dims).to(F64).numpy()
    at = R.first_bad(got == CANARY)
    assert at is None, f"{what}: {int((got == CANARY).sum())} elements were never written; first (b, ci, h, w, d) = {at}"
    at = R.first_bad(got != ref)
    assert at is None, (f"{what}: {int((got != ref).sum())} of {n} elements differ from float64; first (b, ci, h, w, d) = {at}: "
                        f"got {got[at]!r}, want {ref[at]!r}")
    # equal calls, equal bits (and a second call over a written buffer changes nothing: no accumulation into dx)
    L.call("mivp_patch_embed_dgrad", C.byref(d), L.ptr(dz_d), L.ptr(w_d), L.ptr(dx), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), flat), what + ": a second call changed the bits"


@pytest.mark.parametrize("dims,Cc,why", [((6, 10, 13), 48, "odd_dim"), ((6, 10, 14), 44, "C_not_multiple_of_8")])
def test_patch_embed_dgrad_refusals(dims, Cc, why):
    B, Cin = 1, 2
    g = torch.Generator().manual_seed(1)
    dz = dev(torch.randn((B, dims[0] // 2, dims[1] // 2, (dims[2] + 1) // 2, 48), generator=g), BF16)
    w = dev(torch.randn((48, Cin, 2, 2, 2), generator=g))
    dx = Out((B, Cin, dims[0], dims[1], dims[2] + 1))
    with pytest.raises(RuntimeError, match=EINVAL):
        L.call("mivp_patch_embed_dgrad", C.byref(embed_desc(B, Cin, dims, Cc, 3)), L.ptr(dz), L.ptr(w), L.ptr(dx.t), L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.flat).all()), "a refused call wrote to dx"


# =============================================================================================
# mivp_input_prompt_fwd / _bwd
# =============================================================================================
def prompt_fwd(x_d, p_d, s_d, B, Cin, roi, lattice, what):
    y = Out((B, Cin, *roi))
    L.call("mivp_input_prompt_fwd", L.ptr(x_d), L.ptr(p_d), L.ptr(s_d), B, Cin, roi[0], roi[1], roi[2], lattice[0], lattice[1],
           lattice[2], L.ptr(y.t), L.stream())
    torch.cuda.synchronize()
    return y.done(what + " forward")


def prompt_bwd(g_d, s_d, B, Cin, roi, lattice, what):
    dp = Out((Cin, *lattice))
    L.call("mivp_input_prompt_bwd", L.ptr(g_d), L.ptr(s_d), B, Cin, roi[0], roi[1], roi[2], lattice[0], lattice[1],
           lattice[2], L.ptr(dp.t), L.stream())
    torch.cuda.synchronize()
    return dp.done(what + " backward")


def operands(B, Cin, roi, lattice):
    g = torch.Generator().manual_seed(B + Cin + sum(roi) + 7 * sum(lattice))
    x = torch.randn((B, Cin, *roi), generator=g, dtype=F32)
    P = torch.randn((Cin, *lattice), generator=g, dtype=F32)
    gout = torch.randn((B, Cin, *roi), generator=g, dtype=F32)
    return x, P, gout


# (lattice, roi, Cin, B, path)
INTERP = [((2, 2, 2), (4, 6, 8), 1, 2, "group64_V4"),
          ((3, 4, 5), (8, 10, 12), 2, 3, "group64_V4"),
          ((1, 3, 2), (4, 6, 8), 2, 2, "one_node_axis"),
          ((3, 1, 1), (5, 4, 6), 1, 1, "two_one_node_axes_V2"),
          ((3, 3, 3), (4, 4, 5), 2, 2, "node_kernel_V1"),
          ((2, 2, 2), (16, 16, 16), 1, 2, "group256"),
          ((16, 16, 16), (32, 32, 32), 1, 1, "16cubed_nodes_in_LDS")]


@pytest.mark.parametrize("lattice,roi,Cin,B,path", INTERP,
                         ids=[f"{c[4]}-lat{'x'.join(map(str, c[0]))}_roi{'x'.join(map(str, c[1]))}_Cin{c[2]}_B{c[3]}" for c in INTERP])
def test_input_prompt_interpolating(lattice, roi, Cin, B, path):
    scale = 0.75
    x, P, gout = operands(B, Cin, roi, lattice)
    what = f"input_prompt lattice={lattice} roi={roi} Cin={Cin} B={B} ({path})"
    ref_y = R.prompt_fwd(x.numpy(), P.numpy(), scale)
    ref_dp = R.prompt_bwd(gout.numpy(), lattice, scale)
    # the float32 eager torch composition on the same operands
    P32 = P.clone().requires_grad_(True)
    y32 = x + scale * F.interpolate(P32[None], size=roi, mode="trilinear", align_corners=True)
    (y32 * gout).sum().backward()
    x_d, p_d, g_d = dev(x), dev(P), dev(gout)
    s_d = torch.tensor([scale], dtype=F32, device=DEV)
    y = prompt_fwd(x_d, p_d, s_d, B, Cin, roi, lattice, what)
    dp = prompt_bwd(g_d, s_d, B, Cin, roi, lattice, what)
    R.check_err32(y.numpy(), ref_y, y32.detach().numpy(), what + " forward", "bchwd")
    R.check_err32(dp.numpy(), ref_dp, P32.grad.numpy(), what + " backward", "cijk")
    assert_same_bits(prompt_fwd(x_d, p_d, s_d, B, Cin, roi, lattice, what), y, what + ": two equal forward calls")
    assert_same_bits(prompt_bwd(g_d, s_d, B, Cin, roi, lattice, what), dp, what + ": two equal backward calls")
    if 1 in lattice:                                                   # constant along a one-node axis: same bits along it
        zero = prompt_fwd(torch.zeros_like(x_d), p_d, s_d, B, Cin, roi, lattice, what + " (x = 0)")
        for a in range(3):
            if lattice[a] == 1:
                first = zero.index_select(2 + a, torch.tensor([0]))
                assert torch.equal(zero, first.expand_as(zero)), f"{what}: not constant along axis {a}"


# (roi, Cin, B, note)
IDENT = [((4, 6, 8), 2, 3, "lattice_in_LDS"), ((16, 20, 28), 1, 2, "lattice_in_global_memory"), ((3, 5, 7), 1, 4, "odd_dims_V1")]


@pytest.mark.parametrize("roi,Cin,B,note", IDENT, ids=[f"{c[3]}-roi{'x'.join(map(str, c[0]))}_Cin{c[1]}_B{c[2]}" for c in IDENT])
def test_input_prompt_full_resolution_is_exact(roi, Cin, B, note):
    if note == "lattice_in_global_memory":
        assert Cin * math.prod(roi) * 4 > 32 * 1024                    # beyond the LDS staging bound
    x, P, gout = operands(B, Cin, roi, roi)
    what = f"input_prompt lattice == roi = {roi} Cin={Cin} B={B} ({note})"
    x_d, p_d, g_d = dev(x), dev(P), dev(gout)
    one = torch.ones(1, dtype=F32, device=DEV)
    half = torch.full((1,), 0.5, dtype=F32, device=DEV)
    y = prompt_fwd(x_d, p_d, one, B, Cin, roi, roi, what)
    assert_same_bits(y, x + P[None], what + ": forward against x + P")
    dp = prompt_bwd(g_d, one, B, Cin, roi, roi, what)
    assert_same_bits(dp, torch.from_numpy(R.identity_bwd_f32(gout.numpy(), 1.0)), what + ": backward against the ordered batch sum")
    dp = prompt_bwd(g_d, half, B, Cin, roi, roi, what + " scale 0.5")
    assert_same_bits(dp, torch.from_numpy(R.identity_bwd_f32(gout.numpy(), 0.5)), what + ": backward, scale 0.5")
    assert_same_bits(prompt_bwd(g_d, half, B, Cin, roi, roi, what), dp, what + ": two equal backward calls")


@pytest.mark.parametrize("roi,lattice,why", [((4, 6, 8), (5, 2, 2), "more_nodes_than_voxels"), ((4, 6, 8), (0, 2, 2), "no_node"),
                                             ((4000, 90, 8), (2, 2, 2), "axes_sum_beyond_the_tables")])
def test_input_prompt_refusals(roi, lattice, why):
    x = torch.zeros(64, dtype=F32, device=DEV)
    one = torch.ones(1, dtype=F32, device=DEV)
    y, dp = Out((64,)), Out((64,))
    with pytest.raises(RuntimeError, match=EINVAL):
        L.call("mivp_input_prompt_fwd", L.ptr(x), L.ptr(x), L.ptr(one), 1, 1, roi[0], roi[1], roi[2], lattice[0], lattice[1],
               lattice[2], L.ptr(y.t), L.stream())
    with pytest.raises(RuntimeError, match=EINVAL):
        L.call("mivp_input_prompt_bwd", L.ptr(x), L.ptr(one), 1, 1, roi[0], roi[1], roi[2], lattice[0], lattice[1], lattice[2],
               L.ptr(dp.t), L.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.flat).all()) and bool(torch.isnan(dp.flat).all()), "a refused call wrote to its output"
