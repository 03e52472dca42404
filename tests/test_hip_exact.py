"""Exact-integer parity of the convolution and GEMM kernels (through the wrappers of mivp_amd.ops) against float64
torch on the CPU: bit-equal at every element, no tolerance (method and conditions: tests/exact_ref.py, DESIGN.md
"Exact-integer parity").  Inputs are seeded sparse draws of small integers (dyadic multiples where a kernel has 1/4 and
3/4 weights); every case asserts conditions (a) and (b) on 100 % of its float64 reference before it looks at the kernel.
The one assertion that is not an equality is the 4-ulp bar on the BatchNorm affine (three fp32 roundings after exact
sums).  Not covered here, with their own tests elsewhere: LeakyReLU prologues (0.01 is not dyadic), align_corners=True
(weights are not dyadic), LayerNorm / softmax / attention (transcendental).  The low-resolution head (uphead) folds
measured statistics only at the level of functional.uphead; its kernels are exact below that level, where the test
chooses scale, shift, mean and rstd: tests/test_hip_uphead.py."""
import contextlib
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16

X_VALS = (-2, -1, 1, 2)
W_VALS = (-1, 1)
BIAS_VALS = tuple(range(-3, 4))
RES_VALS = tuple(range(-2, 3))
SCALE_VALS = (1, 2, -1, 0.5)
SHIFT_VALS = tuple(range(-3, 4))


def _ops():
    import mivp_amd  # noqa: F401
    from mivp_amd import ops
    return ops


def _lib():
    from mivp_amd import _lib as L
    return L


def cl(t, dtype=BF16):
    """float64 [B, C, H, W, D] -> channels-last device tensor (the cast is exact: operands are bf16 numbers)."""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)


def cl64(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def dev(t, dtype=torch.float32):
    return None if t is None else t.contiguous().to(DEV, dtype)


@contextlib.contextmanager
def im2col_only(ops):
    saved = ops.halo_brick
    ops.halo_brick = lambda *a: 0
    try:
        yield
    finally:
        ops.halo_brick = saved


def _densities(limit, terms, second_moment):
    """The density ladder of exact_ref from the first rung at which 5.5 sigma of a sum of ``terms`` products with the
    given second moment stays under ``limit`` (a starting point only: conditions (a) and (b) decide)."""
    want = (limit / 5.5) ** 2 / max(terms * second_moment, 1e-9)
    lad = [d for d in E.DENSITIES if d <= want]
    return tuple(lad) if lad else (E.DENSITIES[-1],)


class Case(dict):
    __getattr__ = dict.__getitem__


def conv_case(seed, B, cin, cout, dims, bias=True, residual=False, affine=False, stored_bf16=True):
    """A seeded integer conv case whose float64 reference meets (a) and (b)."""
    def make(dens):
        g = E.gen(seed)
        x = E.draw(g, (B, cin, *dims), X_VALS, 0.5)
        w = E.draw(g, (cout, cin, 3, 3, 3), W_VALS, dens)
        b = E.draw(g, (cout,), BIAS_VALS) if bias else None
        r = E.draw(g, (B, cout, *dims), RES_VALS) if residual else None
        sc = E.draw(g, (cin,), SCALE_VALS) if affine else None
        sh = E.draw(g, (cin,), SHIFT_VALS) if affine else None
        ref, bound = E.conv3d_ref(x, w, b, sc, sh, r)
        return ref, bound, stored_bf16, Case(x=x, w=w, b=b, r=r, sc=sc, sh=sh, ref=ref, bound=bound)
    # bf16 stores: integers up to 256, half-integers (scale 0.5) up to 128; f32 stores: condition (a) alone
    limit = (120.0 if affine else 250.0) if stored_bf16 else 1e6
    c = E.first_exact(make, _densities(limit, 27 * cin, 6.0 if affine else 1.25))
    E.assert_exact_inputs(c.ref, c.bound, stored_bf16, "conv")
    E.assert_bf16_operands(c.x, c.w, c.r, E.affine_input(c.x, c.sc, c.sh))
    return c


def run_conv(ops, c, cout, out_f32=False, force_halo=False, wp=None):
    wp = ops.pack_conv_weight(c.w.float().to(DEV)) if wp is None else wp
    y = ops.conv3d(cl(c.x), wp, dev(c.b), cout, dev(c.sc), dev(c.sh), False, None if c.r is None else cl(c.r), out_f32,
                   force_halo=force_halo)
    return y, wp


# ---------------------------------------------------------------------------------------------
# im2col conv
# ---------------------------------------------------------------------------------------------
IM2COL_DIMS = [(1, 1, 1), (1, 2, 40), (3, 3, 3), (5, 6, 7)]
IM2COL_FEATURES = [dict(bias=True, residual=False, affine=False, f32=False),
                   dict(bias=True, residual=True, affine=True, f32=False),
                   dict(bias=True, residual=False, affine=True, f32=True),
                   dict(bias=False, residual=True, affine=False, f32=True)]


@pytest.mark.parametrize("cout", [2, 16, 36, 48, 96])          # conv_ntn 1 / 1 / 3 / 3 / 6
@pytest.mark.parametrize("cin", [8, 24, 48, 144])
def test_im2col_conv(cin, cout):
    """Every (cin, cout) runs B in {1, 3} x four volumes x (bf16 | f32 output, bias, residual, affine prologue)."""
    ops = _ops()
    n = 0
    with im2col_only(ops):
        for B in (1, 3):
            for dims in IM2COL_DIMS:
                for k, f in enumerate(IM2COL_FEATURES):
                    c = conv_case(1000 * cin + 10 * cout + k + B, B, cin, cout, dims, f["bias"], f["residual"], f["affine"],
                                  not f["f32"])
                    y, _ = run_conv(ops, c, cout, f["f32"])
                    assert y.dtype == (torch.float32 if f["f32"] else BF16)
                    E.assert_equal_located(y, cl64(c.ref), "bhwdc", f"im2col {cin}->{cout} B={B} dims={dims} {f}")
                    n += 1
    assert n == 32


@pytest.mark.parametrize("cout", [32, 64])                     # conv_ntn 2 and 4 (the list above has 1, 3 and 6)
def test_im2col_conv_two_and_four_channel_tiles(cout):
    ops = _ops()
    with im2col_only(ops):
        for B, dims in ((1, (1, 2, 40)), (3, (5, 6, 7))):
            for k, f in enumerate(IM2COL_FEATURES):
                c = conv_case(77 + cout + k, B, 24, cout, dims, f["bias"], f["residual"], f["affine"], not f["f32"])
                y, _ = run_conv(ops, c, cout, f["f32"])
                E.assert_equal_located(y, cl64(c.ref), "bhwdc", f"im2col 24->{cout} B={B} dims={dims} {f}")


def test_im2col_conv_split_k_and_unsplit():
    """144 -> 48 at B = 1, (3, 3, 3): 27 voxels = one 256-voxel tile x one channel block (three 16-channel tiles, NTN 3)
    = 1 workgroup < 256, so K is split: Kp = 3904 -> 122 k-steps; slices = min(512, 122 // 8 = 15) = 15, 9 k-steps per
    slice -> ceil(122 / 9) = 14 slices of f32 partials.  The same channels at B = 6, (11, 25, 40) = 66000 voxels are 258
    tiles >= 256 workgroups: the unsplit kernel."""
    ops, L = _ops(), _lib()
    cin, cout = 144, 48
    with im2col_only(ops):
        d = ops.conv_desc(1, (3, 3, 3), cin, cout, False, False, True, False)
        assert L.lib().mivp_conv3d_fwd_ws(ctypes.byref(d)) == 14 * 27 * cout * 4
        for k, f in enumerate(IM2COL_FEATURES):
            c = conv_case(500 + k, 1, cin, cout, (3, 3, 3), f["bias"], f["residual"], f["affine"], not f["f32"])
            y, _ = run_conv(ops, c, cout, f["f32"])
            E.assert_equal_located(y, cl64(c.ref), "bhwdc", f"split-K {f}")
        big = (11, 25, 40)
        d = ops.conv_desc(6, big, cin, cout, False, False, True, False)
        assert (6 * 11 * 25 * 40 + 255) // 256 >= 256 and L.lib().mivp_conv3d_fwd_ws(ctypes.byref(d)) == 0
        c = conv_case(510, 6, cin, cout, big, True, True, False, True)
        y, _ = run_conv(ops, c, cout, False)
        E.assert_equal_located(y, cl64(c.ref), "bhwdc", "unsplit, 258 voxel tiles")


# ---------------------------------------------------------------------------------------------
# halo-brick conv
# ---------------------------------------------------------------------------------------------
BRICK_CODES = (8, 4, 6, 66, 36)
HALO_PAIRS = [(16, 16), (32, 36), (48, 144), (144, 48), (16, 48)]


def residue_shapes(brick):
    """One axis at a time {1, b-1, b, b+1, 2b+1} of its own brick edge around one brick, plus b+1 on every axis."""
    shapes = []
    for ax in range(3):
        for v in (1, brick[ax] - 1, brick[ax], brick[ax] + 1, 2 * brick[ax] + 1):
            s = list(brick)
            s[ax] = v
            if tuple(s) not in shapes:
                shapes.append(tuple(s))
    shapes.append(tuple(b + 1 for b in brick))
    return shapes


def run_halo(ops, c, cout, code):
    y, wp = run_conv(ops, c, cout, False, force_halo=code)
    assert getattr(wp, "_mivp_halo", None) is not None, "the halo-brick kernel did not run"
    return y


@pytest.mark.parametrize("code", BRICK_CODES)
def test_halo_brick_residues(code):
    """Every residue shape of this brick, plain (LDS-DMA staging; bias, residual when cin == cout) and with the fused
    affine prologue (register staging); channel pairs and batch sizes rotate over the shapes."""
    ops = _ops()
    brick = ops._HALO_BRICKS[code][:3]
    shapes = residue_shapes(brick)
    assert len(shapes) == 14
    for i, dims in enumerate(shapes):
        cin, cout = HALO_PAIRS[i % len(HALO_PAIRS)]
        B = (1, 3)[i % 2]
        for affine in (False, True):
            c = conv_case(31 * code + 2 * i + affine, B, cin, cout, dims, True, cin == cout and not affine, affine, True)
            y = run_halo(ops, c, cout, code)
            E.assert_equal_located(y, cl64(c.ref), "bhwdc",
                                   f"halo brick {code} {cin}->{cout} B={B} dims={dims} affine={affine}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cin,cout", HALO_PAIRS)
def test_halo_brick_channels_all_geometries(cin, cout, B):
    """(7, 9, 19) is ragged for every brick (7 = 4+3 = 6+1 = 2*3+1, 9 = 8+1 = 2*4+1 = 6+3, 19 = 16+3 = 2*8+3): the five
    geometries against the reference, hence bit-equal to each other."""
    ops = _ops()
    dims = (7, 9, 19)
    for affine in (False, True):
        c = conv_case(900 + cin + cout + B + affine, B, cin, cout, dims, True, cin == cout, affine, True)
        ref = cl64(c.ref)
        outs = []
        for code in BRICK_CODES:
            y = run_halo(ops, c, cout, code)
            E.assert_equal_located(y, ref, "bhwdc", f"halo brick {code} {cin}->{cout} B={B} affine={affine}")
            outs.append(y)
        for y in outs[1:]:
            assert torch.equal(y, outs[0])


# ---------------------------------------------------------------------------------------------
# data-gradient packs through both conv kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout", [2, 5, 8, 24])
def test_dgrad_packs_through_both_kernels(cout):
    """dx of y = conv3d(x, w) as the same conv of dy with flipped / transposed weights: pack_conv_weight_dgrad (dy padded
    to 8 channels) through the im2col kernel and pack_conv_weight_dgrad16 (dy padded to 16) through the halo kernel,
    against autograd of F.conv3d.  Cout = 24 has no 16-channel pack and 24 input channels are outside the halo kernel's
    window: the halo request must fall to the im2col kernel and stay exact."""
    ops, L = _ops(), _lib()
    for cin, B, dims in ((16, 2, (5, 6, 19)), (48, 1, (3, 7, 9))):
        def make(dens):
            g = E.gen(40 + cout + cin)
            w = E.draw(g, (cout, cin, 3, 3, 3), W_VALS, dens)
            dy = E.draw(g, (B, cout, *dims), X_VALS, 0.5)
            xz = torch.zeros(B, cin, *dims, dtype=torch.float64)
            (dx, _, _), (bx, _, _) = E.conv3d_grads_ref(xz, w, dy)
            return dx, bx, True, Case(w=w, dy=dy, dx=dx, bound=bx)
        c = E.first_exact(make, _densities(250.0, 27 * cout, 1.25))
        E.assert_exact_inputs(c.dx, c.bound, True, "dgrad")
        E.assert_bf16_operands(c.w, c.dy)
        ref = cl64(c.dx)
        wd, cpad = ops.pack_conv_weight_dgrad(c.w.float().to(DEV))
        assert cpad == (cout + 7) // 8 * 8
        dyp = torch.zeros(B, *dims, cpad, dtype=BF16, device=DEV)
        dyp[..., :cout] = cl(c.dy)
        with im2col_only(ops):
            dx = ops.conv3d(dyp, wd, None, cin)
        E.assert_equal_located(dx, ref, "bhwdc", f"dgrad pack, im2col, cout={cout} cin={cin}")
        w16 = ops.pack_conv_weight_dgrad16(c.w.float().to(DEV))
        if cpad >= 16:
            assert w16 is None
            d = ops.conv_desc(B, dims, cpad, cin, False, False, False, False)
            assert (L.lib().mivp_conv3d_halo_supported(ctypes.byref(d)) == 1) == (cpad % 16 == 0)
            dx = ops.conv3d(dyp, wd, None, cin, force_halo=8)
            assert (getattr(wd, "_mivp_halo", None) is not None) == (cpad % 16 == 0)
            E.assert_equal_located(dx, ref, "bhwdc", f"dgrad pack, halo request, cout={cout} cin={cin}")
            continue
        dy16 = torch.zeros(B, *dims, 16, dtype=BF16, device=DEV)
        dy16[..., :cout] = cl(c.dy)
        for code in BRICK_CODES:
            dx = ops.conv3d(dy16, w16, None, cin, force_halo=code)
            assert getattr(w16, "_mivp_halo", None) is not None
            E.assert_equal_located(dx, ref, "bhwdc", f"dgrad16 pack, halo brick {code}, cout={cout} cin={cin}")


# ---------------------------------------------------------------------------------------------
# gemm_tn
# ---------------------------------------------------------------------------------------------
TN_T = [1, 31, 128, 129, 4097]
TN_MN = [8, 24, 64, 72, 130 * 4]


def _misaligned(t):
    """The same bf16 matrix at a device address 8 bytes past a 16-byte boundary (the 16-byte-piece kernel is illegal)."""
    flat = torch.zeros(t.numel() + 4, dtype=BF16, device=DEV)
    flat[4:] = t.reshape(-1).to(DEV, BF16)
    out = flat[4:].view(t.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 8
    return out


def _tn_splits(ops, L, T, M, N):
    d = L.GemmTnDesc(T, M, N, ops.operand_rows(M), ops.operand_rows(N), 1.0, 0, 0)
    return L.lib().mivp_gemm_tn_ws(ctypes.byref(d)) // (M * N * 4)


@pytest.mark.parametrize("T", TN_T)
def test_gemm_tn_rows(T):
    """All M x N of the list; per pair one of: plain; row stride != M with alpha 0.5 accumulated onto an integer matrix;
    row stride M + 4 (8-byte pieces); column offset mis-aligned by 4 elements (8-byte pieces), alpha 0.5."""
    ops, L = _ops(), _lib()
    if T == 4097:
        assert _tn_splits(ops, L, T, 64, 64) == 33            # > 32 splits: the reduce tree's strided slices
        assert _tn_splits(ops, L, T, 520, 520) == 7           # 33 chunks in splits of 5: a short last split
    if T == 129:
        assert _tn_splits(ops, L, T, 8, 8) == 2               # straddles the 128-token chunk: second split holds 1 token
    n = 0
    for i, M in enumerate(TN_MN):
        for j, N in enumerate(TN_MN):
            variant = (i + 2 * j + T) % 4
            lda = (M, M + 8, M + 4, M + 8)[variant]
            ldb = (N, N + 16, N, N)[variant]
            alpha, acc = ((1.0, False), (0.5, True), (1.0, False), (0.5, False))[variant]
            g = E.gen(T * 1000 + M + N)
            a = E.draw(g, (T, lda), X_VALS, 0.5)
            b = E.draw(g, (T, ldb), X_VALS, 0.5)
            out0 = E.draw(g, (M, N), BIAS_VALS) if acc else None
            ref, bound = E.matmul_tn_ref(a[:, :M], b[:, :N])
            ref, bound = alpha * ref, alpha * bound
            if acc:
                ref, bound = ref + out0, bound + out0.abs()
            E.assert_exact_inputs(ref, bound, False, "gemm_tn rows")
            ad = _misaligned(a) if variant == 3 else a.to(DEV, BF16)
            bd = b.to(DEV, BF16)
            out = ops.gemm_tn(ad, ops.operand_rows(lda), bd, ops.operand_rows(ldb), T, M, N,
                              out=None if out0 is None else out0.to(DEV, torch.float32), alpha=alpha, accumulate=acc)
            E.assert_equal_located(out, ref, "mn", f"gemm_tn rows T={T} M={M} N={N} variant={variant}")
            n += 1
    assert n == 25


@pytest.mark.parametrize("win,rows", [(1, 1), (1, 31), (2, 64), (3, 43), (17, 241)])     # T = 1, 31, 128, 129, 4097
def test_gemm_tn_head_split(win, rows):
    """The attention layout [T/rows][C/hd][rows][hd] as the A operand (and once as the B operand) against plain rows."""
    ops = _ops()
    T = win * rows
    assert T in TN_T
    for k, (heads, hd) in enumerate([(2, 4), (2, 12), (4, 16), (3, 24), (5, 104)]):       # C = 8, 24, 64, 72, 520
        Cc = heads * hd
        N = TN_MN[(k + 1) % len(TN_MN)]
        alpha = (1.0, 0.5)[k % 2]
        g = E.gen(T + Cc)
        a = E.draw(g, (win, heads, rows, hd), X_VALS, 0.5)
        b = E.draw(g, (T, N), X_VALS, 0.5)
        a_rows = a.permute(0, 2, 1, 3).reshape(T, Cc)
        ref, bound = E.matmul_tn_ref(a_rows, b)
        E.assert_exact_inputs(alpha * ref, alpha * bound, False, "gemm_tn heads")
        ad, bd = a.to(DEV, BF16), b.to(DEV, BF16)
        out = ops.gemm_tn(ad, ops.operand_heads(rows, hd), bd, ops.operand_rows(N), T, Cc, N, alpha=alpha)
        E.assert_equal_located(out, alpha * ref, "mn", f"gemm_tn head-split A T={T} C={Cc} N={N}")
        out = ops.gemm_tn(bd, ops.operand_rows(N), ad, ops.operand_heads(rows, hd), T, N, Cc, alpha=alpha)
        E.assert_equal_located(out, alpha * ref.t(), "mn", f"gemm_tn head-split B T={T} C={Cc} N={N}")


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 3, 5), (6, 5, 7)])
def test_gemm_tn_conv_taps(B, dims):
    """dW of a 3x3x3 'same' convolution in nn.Conv3d's layout against autograd of F.conv3d (Cin = 4: 8-byte pieces)."""
    ops = _ops()
    vox = B * dims[0] * dims[1] * dims[2]
    for cin, cout in ((8, 16), (4, 72), (24, 8), (48, 24)):
        g = E.gen(vox + cin)
        x = E.draw(g, (B, cin, *dims), X_VALS, 0.5)
        dy = E.draw(g, (B, cout, *dims), X_VALS, 0.5)
        wz = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64)
        (_, dw, _), (_, bw, _) = E.conv3d_grads_ref(x, wz, dy)
        E.assert_exact_inputs(dw, bw, False, "gemm_tn taps")
        out = ops.gemm_tn(cl(dy), ops.operand_rows(cout), cl(x), ops.operand_conv_taps(dims, cin, cin), vox, cout, 27 * cin,
                          perm_cin=cin)
        E.assert_equal_located(out.view(cout, cin, 3, 3, 3), dw, "oiabc", f"gemm_tn taps B={B} dims={dims} {cin}->{cout}")


# ---------------------------------------------------------------------------------------------
# conv weight-gradient wrappers
# ---------------------------------------------------------------------------------------------
def wgrad_case(seed, B, cin, cout, dims, affine):
    g = E.gen(seed)
    x = E.draw(g, (B, cin, *dims), X_VALS, 0.5)
    dy = E.draw(g, (B, cout, *dims), X_VALS, 0.5)
    sc = E.draw(g, (cin,), SCALE_VALS) if affine else None
    sh = E.draw(g, (cin,), SHIFT_VALS) if affine else None
    xin = E.affine_input(x, sc, sh)
    wz = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64)
    (_, dw, db), (_, bw, bb) = E.conv3d_grads_ref(xin, wz, dy)
    E.assert_exact_inputs((dw, db), (bw, bb), False, "wgrad")
    E.assert_bf16_operands(x, dy, xin)
    return Case(x=x, dy=dy, sc=sc, sh=sh, xin=xin, dw=dw, db=db)


def _pad_channels(t_cl, n):
    out = torch.zeros(*t_cl.shape[:-1], n, dtype=t_cl.dtype, device=t_cl.device)
    out[..., :t_cl.shape[-1]] = t_cl
    return out


@pytest.mark.parametrize("cout", [2, 5])
def test_conv3d_wgrad_small(cout):
    """Affine prologue, no LeakyReLU; (9, 13, 20) is 2340 voxels = two voxel ranges (two partial blocks)."""
    ops = _ops()
    for cin, B, dims in ((8, 1, (1, 1, 1)), (48, 2, (5, 6, 7)), (8, 1, (9, 13, 20)), (24, 3, (1, 2, 40))):
        c = wgrad_case(60 + cout + cin, B, cin, cout, dims, True)
        dw, db = ops.conv3d_wgrad_small(cl(c.x), dev(c.sc), dev(c.sh), False, _pad_channels(cl(c.dy), 8), cout)
        E.assert_equal_located(dw, c.dw, "oiabc", f"wgrad_small dW cin={cin} cout={cout} dims={dims}")
        E.assert_equal_located(db, c.db, "o", f"wgrad_small db cin={cin} cout={cout} dims={dims}")


@pytest.mark.parametrize("cout", [2, 5, 8])
def test_conv3d_wgrad_rows(cout):
    """(G, S) of the rows formulation are the weight gradient of the raw x and of a ones channel; dW and db of the
    (affine -> conv) head follow through head_grads_from_gs with power-of-two scales and integer shifts."""
    ops = _ops()
    for cin, B, dims in ((8, 1, (1, 1, 1)), (48, 2, (4, 5, 7)), (8, 2, (2, 3, 33)), (56, 1, (3, 2, 65))):
        assert ops.conv3d_wgrad_rows_supported(cin, cout, dims[2])
        c = wgrad_case(70 + cout + cin, B, cin, cout, dims, True)
        ones = torch.ones(B, 1, *dims, dtype=torch.float64)
        wz = torch.zeros(cout, cin + 1, 3, 3, 3, dtype=torch.float64)
        (_, gs, _), (_, bgs, _) = E.conv3d_grads_ref(torch.cat([c.x, ones], 1), wz, c.dy)
        E.assert_exact_inputs(gs, bgs, False, "wgrad_rows")
        G, S = ops.conv3d_wgrad_rows(cl(c.x), _pad_channels(cl(c.dy), 8), cout)
        E.assert_equal_located(G, gs[:, :cin].reshape(cout, cin, 27).permute(0, 2, 1), "otc", f"wgrad_rows G cin={cin} dims={dims}")
        E.assert_equal_located(S, gs[:, cin].reshape(cout, 27), "ot", f"wgrad_rows S cin={cin} dims={dims}")
        mr = torch.cat([torch.zeros(cin), torch.ones(cin)]).to(DEV)
        dW, db, _, _ = ops.head_grads_from_gs(G, S, torch.zeros(cout, cin, 3, 3, 3, device=DEV), dev(c.sc), dev(c.sh), mr)
        E.assert_equal_located(dW, c.dw, "oiabc", f"wgrad_rows dW cin={cin} dims={dims}")
        E.assert_equal_located(db, c.db, "o", f"wgrad_rows db cin={cin} dims={dims}")
    assert not ops.conv3d_wgrad_rows_supported(64, cout, 8) and not ops.conv3d_wgrad_rows_supported(12, cout, 8)
    with pytest.raises(RuntimeError):                          # outside the window: refused, no other path is taken
        ops.conv3d_wgrad_rows(torch.zeros(1, 2, 2, 8, 64, dtype=BF16, device=DEV),
                              torch.zeros(1, 2, 2, 8, 8, dtype=BF16, device=DEV), cout)


@pytest.mark.parametrize("cin,cin_p,cout,ld", [(48, 48, 5, 8), (6, 8, 16, 16), (24, 24, 48, 48), (16, 16, 2, 8), (4, 4, 8, 8)])
def test_conv3d_wgrad(cin, cin_p, cout, ld):
    """Both operand arrangements of conv3d_wgrad (few output channels: x rows against the dy taps; otherwise dy rows against
    the x taps), x channel padding included."""
    ops = _ops()
    for B, dims in ((2, (2, 3, 5)), (1, (6, 5, 7)), (2, (1, 1, 1))):
        c = wgrad_case(80 + cin + cout + B, B, cin, cout, dims, False)
        dw, db = ops.conv3d_wgrad(_pad_channels(cl(c.x), cin_p), _pad_channels(cl(c.dy), ld), cout, cin)
        E.assert_equal_located(dw, c.dw, "oiabc", f"conv3d_wgrad dW {cin}->{cout} dims={dims}")
        E.assert_equal_located(db, c.db, "o", f"conv3d_wgrad db {cin}->{cout} dims={dims}")


# ---------------------------------------------------------------------------------------------
# transposed conv k2s2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [(2, 2, 2), (2, 2, 1)])
@pytest.mark.parametrize("cin,cout", [(16, 8), (96, 48)])
def test_conv_transpose_k2s2(cin, cout, stride):
    ops = _ops()
    for B, dims in ((1, (1, 1, 1)), (2, (2, 3, 5)), (3, (3, 3, 6))):
        hi = tuple(n * s for n, s in zip(dims, stride))

        def make(dens):
            g = E.gen(90 + cin + B)
            x = E.draw(g, (B, cin, *dims), X_VALS, 0.5)
            w = E.draw(g, (cin, cout, *stride), W_VALS, dens)
            dy = E.draw(g, (B, cout, *hi), X_VALS, 0.5)
            refs, bounds = E.conv_transpose_ref(x, w, stride, dy)
            return refs, bounds, (True, True, False), Case(x=x, w=w, dy=dy, refs=refs, bounds=bounds)
        c = E.first_exact(make)
        E.assert_exact_inputs(c.refs, c.bounds, (True, True, False), "convt")
        E.assert_bf16_operands(c.x, c.w, c.dy)
        w1, w2 = ops.pack_convt_weight(c.w.float().to(DEV))
        what = f"convt {cin}->{cout} stride={stride} B={B} dims={dims}"
        E.assert_equal_located(ops.convt_forward(cl(c.x), w1, stride, cout), cl64(c.refs[0]), "bhwdc", what + " forward")
        E.assert_equal_located(ops.convt_dgrad(cl(c.dy), w2, stride, cin), cl64(c.refs[1]), "bhwdc", what + " dgrad")
        E.assert_equal_located(ops.convt_wgrad(cl(c.x), cl(c.dy), stride), c.refs[2], "ioabc", what + " wgrad")


# ---------------------------------------------------------------------------------------------
# pointwise conv
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vox", [1, 255, 257, 1000])
@pytest.mark.parametrize("C", [8, 48])
def test_pointwise_conv(C, n_vox):
    """1x1x1 conv to <= 4 channels and its backward; 5 output channels are outside the kernels' window and refused."""
    ops = _ops()
    for cout in (1, 2, 5):
        g = E.gen(n_vox + C + cout)
        x = E.draw(g, (n_vox, C), X_VALS, 0.5)
        w = E.draw(g, (cout, C), W_VALS, 0.5)
        b = E.draw(g, (cout,), BIAS_VALS)
        dy = E.draw(g, (n_vox, cout), X_VALS, 0.75)
        xd = x.view(1, n_vox, 1, 1, C).to(DEV, BF16)
        dyd = dy.view(1, n_vox, 1, 1, cout).to(DEV, torch.float32)
        if cout > 4:
            with pytest.raises(RuntimeError):
                ops.pointwise_conv(xd, dev(w), dev(b))
            with pytest.raises(RuntimeError):
                ops.pointwise_conv_backward(xd, dev(w), dyd)
            continue
        y, by = x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()
        dx, bdx = dy @ w, dy.abs() @ w.abs()
        dw, bdw = E.matmul_tn_ref(dy, x)
        db, bdb = dy.sum(0), dy.abs().sum(0)
        E.assert_exact_inputs((y, dx, dw, db), (by, bdx, bdw, bdb), (False, True, False, False), "pointwise")
        E.assert_bf16_operands(x, dy)
        what = f"pointwise C={C} n_vox={n_vox} cout={cout}"
        E.assert_equal_located(ops.pointwise_conv(xd, dev(w), dev(b)).view(n_vox, cout), y, "vo", what + " forward")
        gx, gw, gb = ops.pointwise_conv_backward(xd, dev(w), dyd)
        E.assert_equal_located(gx.view(n_vox, C), dx, "vc", what + " dx")
        E.assert_equal_located(gw, dw, "oc", what + " dW")
        E.assert_equal_located(gb, db, "o", what + " db")


# ---------------------------------------------------------------------------------------------
# head conv
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,dims", [(48, 2, (5, 6, 17)), (8, 2, (4, 5, 7)), (32, 1, (1, 1, 1)), (16, 2, (9, 4, 33)),
                                           (56, 2, (3, 3, 3))])
def test_head_conv(cin, cout, dims):
    """The fold is exact for power-of-two scales and integer shifts: scale * w is +-2^k (a bf16 number, so the lo half
    of the hi | lo pair is zero) and the ones-channel entry sum_c shift[c] * w[co][c][tap] is an integer of at most
    3 * cin <= 168 < 256 (a bf16 number).  The per-voxel tap partials are parked as fp16 (11 significant bits), so
    condition (a) is tightened for this kernel to sum |a||b| < 2**10: every partial is then a multiple of 1/2 below 1024,
    an fp16 number, and the f32 logits are exact."""
    ops = _ops()
    assert ops.head_conv_supported(cin, cout)
    B = 2

    def make(dens):
        g = E.gen(cin + cout + dims[2])
        x = E.draw(g, (B, cin, *dims), X_VALS, 0.5)
        w = E.draw(g, (cout, cin, 3, 3, 3), W_VALS, dens)
        b = E.draw(g, (cout,), BIAS_VALS)
        sc = E.draw(g, (cin,), SCALE_VALS)
        sh = E.draw(g, (cin,), SHIFT_VALS)
        ref, bound = E.conv3d_ref(x, w, b, sc, sh)
        return ref, bound * 2.0 ** 14, False, Case(x=x, w=w, b=b, sc=sc, sh=sh, ref=ref, bound=bound)
    c = E.first_exact(make)
    E.assert_exact_inputs(c.ref, c.bound * 2.0 ** 14, False, "head_conv (fp16 partials: 2**10)")
    fold = torch.einsum("c,ocxyz->oxyz", c.sh.abs(), c.w.abs())
    assert float(fold.max()) <= 256
    E.assert_bf16_operands(c.x, c.w * c.sc.view(1, -1, 1, 1, 1), torch.einsum("c,ocxyz->oxyz", c.sh, c.w))
    y = ops.head_conv(cl(c.x), dev(c.w), dev(c.b), dev(c.sc), dev(c.sh))
    assert y.dtype == torch.float32
    E.assert_equal_located(y, cl64(c.ref), "bhwdc", f"head_conv {cin}->{cout} dims={dims}")


def test_head_conv_refuses_three_classes():
    ops = _ops()
    assert not ops.head_conv_supported(48, 3) and not ops.head_conv_supported(64, 2)
    with pytest.raises(RuntimeError):
        ops.head_conv(torch.zeros(1, 2, 2, 2, 48, dtype=BF16, device=DEV), torch.zeros(3, 48, 3, 3, 3, device=DEV),
                      torch.zeros(3, device=DEV), torch.ones(48, device=DEV), torch.zeros(48, device=DEV))


# ---------------------------------------------------------------------------------------------
# upsample + concat
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,idims,sdims,cx,cs", [
    ((2, 2, 2), (1, 1, 1), (2, 2, 2), 16, 8),
    ((2, 2, 1), (1, 1, 3), (2, 2, 3), 16, 8),
    ((2, 2, 2), (1, 1, 3), (2, 2, 6), 48, 0),               # cs = 0: plain upsample
    ((2, 2, 2), (3, 4, 2), (5, 7, 4), 16, 8),               # skip smaller than 2x: crop
    ((2, 2, 1), (3, 4, 2), (6, 8, 2), 16, 0),
    ((2, 2, 2), (3, 4, 2), (6, 8, 4), 96, 48),
    ((2, 2, 2), (2, 3, 24), (4, 5, 47), 16, 8),             # crop, long rows
    ((2, 2, 1), (2, 3, 24), (4, 6, 24), 384, 192),          # 1152 pieces per source row
])
def test_upcat(scale, idims, sdims, cx, cs):
    """x = 64 * {-1, 1} (density 0.5): the align_corners=False weights are products of 1/4, 3/4 and 1, so every upsampled
    value is an integer of at most 64.  dy = 64 * {-1, 1} at density 0.1 on the upsampled channels keeps dx (up to 64
    weighted terms, weights summing to 8) an integer below 256 -- condition (b) checks it."""
    ops = _ops()
    B = 2
    g = E.gen(cx + cs + idims[2] + sdims[2])
    x = 64 * E.draw(g, (B, cx, *idims), W_VALS, 0.5)
    skip = 64 * E.draw(g, (B, cs, *sdims), W_VALS, 0.5) if cs else None
    dy = torch.cat([64 * E.draw(g, (B, cx, *sdims), W_VALS, 0.1), E.draw(g, (B, cs, *sdims), X_VALS, 0.5)], 1)
    (y, dx, dskip), (by, bdx, bdskip) = E.upcat_ref(x, skip, scale, sdims, dy)
    E.assert_exact_inputs((y, dx), (by, bdx), True, "upcat")
    E.assert_bf16_operands(x, skip, dy)
    what = f"upcat scale={scale} idims={idims} sdims={sdims} cx={cx} cs={cs}"
    xd, sd = cl(x), (None if skip is None else cl(skip))
    got = ops.upcat(xd, sd, scale, odims=sdims)
    E.assert_equal_located(got, cl64(y), "bhwdc", what + " forward")
    gx, gskip = ops.upcat_backward(cl(dy), idims, scale, cx, cs)
    E.assert_equal_located(gx, cl64(dx), "bhwdc", what + " dx")
    if cs:
        E.assert_exact_inputs(dskip, bdskip, True, "upcat dskip")
        E.assert_equal_located(gskip, cl64(dskip), "bhwdc", what + " dskip")
    else:
        assert gskip is None
    full = tuple(sdims) == tuple(i * s for i, s in zip(idims, scale))
    if not cs and not full:
        return                                                 # without a skip tensor the statistics kernels take the uncropped size
    # partial sums of the never-materialised tensor: the rows of `part` add up to the integer sums exactly
    s1, s2 = y.sum((0, 2, 3, 4)), (y * y).sum((0, 2, 3, 4))
    E.assert_exact_inputs((s1, s2), (y.abs().sum((0, 2, 3, 4)), s2), False, "upcat_stats")
    part, nblk, n_vox = ops.upcat_stats(xd, sd, scale)
    assert n_vox == B * sdims[0] * sdims[1] * sdims[2] and tuple(part.shape) == (nblk, 2 * (cx + cs))
    E.assert_equal_located(part.double().sum(0), torch.cat([s1, s2]), "c", what + " stats")
    sc, sh = E.draw(g, (cx + cs,), SCALE_VALS), E.draw(g, (cx + cs,), SHIFT_VALS)
    ya = E.affine_input(y, sc, sh)
    E.assert_exact_inputs(ya, E.affine_input(y.abs(), sc.abs(), sh.abs()), True, "upcat_affine")
    got = ops.upcat_affine(xd, sd, scale, dev(sc), dev(sh), False)
    E.assert_equal_located(got, cl64(ya), "bhwdc", what + " affine")


# ---------------------------------------------------------------------------------------------
# BatchNorm partial sums
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,B,dims", [(8, 2, (3, 3, 2)), (48, 2, (6, 6, 6)), (144, 2, (4, 5, 6)), (16, 3, (9, 13, 21))])
def test_bn_partial_sums_and_affine(C, B, dims):
    """Sum x and sum x^2 over the partial rows equal the integer sums exactly.  After exact sums the affine has at most three
    fp32 roundings (the cast of the double rstd, w * rstd, b - mean * scale): scale, shift, mean_rstd and the running
    statistics within 4 fp32 ulp of the float64 value rounded to fp32.  x is drawn from {-2, -1, 1, 2, 3} (positive mean),
    the weight is positive and the bias negative, so b - mean * scale adds two numbers of one sign: no cancellation that
    would turn an ulp of a term into many ulp of the result."""
    ops = _ops()
    g = E.gen(C + dims[0])
    x = E.draw(g, (B, C, *dims), (-2, -1, 1, 2, 3), 0.75)
    w = E.draw(g, (C,), (1, 2, 3))
    b = E.draw(g, (C,), (-3, -2, -1))
    rm0, rv0 = E.draw(g, (C,), (0, 1, 2)), E.draw(g, (C,), (1, 2))
    n = float(B * dims[0] * dims[1] * dims[2])
    s1, s2 = x.sum((0, 2, 3, 4)), (x * x).sum((0, 2, 3, 4))
    E.assert_exact_inputs((s1, s2), (x.abs().sum((0, 2, 3, 4)), s2), False, "bn sums")
    E.assert_bf16_operands(x)
    assert float(s1.min()) > 0
    xd = cl(x)
    part, nblk, n_vox = ops.bn_partial_sums(xd)
    assert n_vox == n and tuple(part.shape) == (nblk, 2 * C)
    E.assert_equal_located(part.double().sum(0), torch.cat([s1, s2]), "c", f"bn partial sums C={C} dims={dims}")
    eps = float(torch.tensor(1e-5, dtype=torch.float32))       # the values the kernel receives as f32 arguments
    mom = float(torch.tensor(0.1, dtype=torch.float32))
    rm, rv = dev(rm0), dev(rv0)
    scale, shift, mr = ops.bn_batch_stats(xd, dev(w), dev(b), 1e-5, rm, rv, 0.1)
    mean = s1 / n
    var = s2 / n - mean * mean
    rstd = 1.0 / torch.sqrt(var + eps)
    want = {"scale": (scale, w * rstd), "shift": (shift, b - mean * (w * rstd)), "mean": (mr[:C], mean), "rstd": (mr[C:], rstd),
            "running_mean": (rm, (1.0 - mom) * rm0 + mom * mean),
            "running_var": (rv, (1.0 - mom) * rv0 + mom * var * n / (n - 1.0))}
    for name, (got, ref) in want.items():
        ulp = E.ulp_distance(got, ref)
        print(f"bn {name} C={C} dims={dims}: max {float(ulp.max()):.2f} ulp")
        assert float(ulp.max()) <= 4.0, (name, float(ulp.max()), int(ulp.argmax()))


@pytest.mark.parametrize("C,B,dims", [(8, 2, (3, 3, 2)), (48, 2, (6, 6, 6)), (144, 2, (4, 5, 6)), (16, 3, (9, 13, 21))])
def test_bn_backward_statistics(C, B, dims):
    """dbeta = sum dy and dgamma = sum dy * (x - mean) * rstd with an integer mean and a power-of-two rstd handed in:
    every term is dyadic, the sums are exact."""
    ops = _ops()
    g = E.gen(2 * C + dims[1])
    x = E.draw(g, (B, C, *dims), X_VALS, 0.75)
    dy = E.draw(g, (B, C, *dims), X_VALS, 0.5)
    mean, rstd = E.draw(g, (C,), (-1, 0, 1)), E.draw(g, (C,), (0.5, 1, 2))
    xh = (x - mean.view(1, -1, 1, 1, 1)) * rstd.view(1, -1, 1, 1, 1)
    dbeta, dgamma = dy.sum((0, 2, 3, 4)), (dy * xh).sum((0, 2, 3, 4))
    bounds = (dy.abs().sum((0, 2, 3, 4)), (dy.abs() * (x.abs() + mean.abs().view(1, -1, 1, 1, 1)) * rstd.view(1, -1, 1, 1, 1)).sum((0, 2, 3, 4)))
    E.assert_exact_inputs((dbeta, dgamma), bounds, False, "bn backward sums")
    E.assert_bf16_operands(x, dy)
    mr = torch.cat([mean, rstd]).to(DEV, torch.float32)
    _, got_dgamma, got_dbeta = ops.bn_backward(cl(x), cl(dy), dev(rstd), dev(-mean * rstd), mr, False)
    E.assert_equal_located(got_dbeta, dbeta, "c", f"bn_backward dbeta C={C} dims={dims}")
    E.assert_equal_located(got_dgamma, dgamma, "c", f"bn_backward dgamma C={C} dims={dims}")
