"""Direct located parity tests of the four Swin token kernels and of mivp_pack_block_weights against tests/tok_ref.py
(float64, CPU).  Each entry is called through ``_lib.call`` on its own operands, with synthetic descriptors and tables.

Kinds of assertion (the list of tests/test_hip_prompt_path.py; derivations in the header of tests/tok_ref.py; no bar is measured):
  exact     q / k / v rows of slots >= Nq are +0 bits; rows with source -1 carry identical bits; slots that gather the same x row
            give bit-identical q / k / v rows wherever they sit; y / dx voxels nobody names stay NaN and every named voxel is
            written; dyw is dy in window order (zero rows where cropped); optional outputs absent or present change no bit of the
            mandatory ones where one kernel serves both calls; the weight images bit-equal tok_ref.block_images
  interval  q, k, v:  C u sum |a||W| (a = bf16 LayerNorm output) + sum D |W| (ln interval), times the scale, + u |ref| for the
                      closing multiplication
            t1:       (C + 3) u ((sum |o||Wp| + |bp|) keep scale + |shortcut|)
            y:        (C + 2) u (sum |a||Wm| + |t1| + |bm|) + sum D |Wm|, from the GPU's OWN stored t1 (a neighbour rounding
                      of one t1 element moves the whole LayerNorm row; test_prompt_kv_fwd treats yln the same way)
            dn_out:   C u sum |dyw||Wm|  (proj_mlp_bwd),  3C u sum |g||Wqkv|  (qkv_bwd, g = bf16(dq q_scale) | dk | dv)
            dO:       C u sum |a||Wp| with a = the GPU's own stored d_pj (weight-gradient mode with dropout), its dt1 (no
                      dropout), or 2 dt1 under the mask at p = 0.5 (the scale 2 is exact, so the masked operand is known)
  err32     dt1, d_pj (through mlp_norm backward) and dx (through attn_norm backward)
  refusal   C = 384 with Nqp = 16: MIVP_EUNSUPPORTED from all four entries, every output untouched

dx of mivp_swin_qkv_bwd is a plain store through tok_src: voxels no source names are not written (kernel headers: "zero-pad /
padding-slot tokens have no voxel to write"; autograd gives them no gradient), and where the synthetic table lets two slots
gather one voxel either slot's row is a correct result -- the tables of real blocks name every voxel once.

The arm each case selects is restated from the launchers (swin_fwd.hip / swin_bwd.hip / swin_tok_wide.hip) in ``*_arm`` below,
asserted on the case's shape and part of the test id."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tok_ref as T  # noqa: E402
from test_hip_prompt_path import DEV, Out, assert_same_bits, bits, dev  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import swin_ops

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NAN = float("nan")
WIDE_C = (48, 96, 192, 384)


# =============================================================================================
# the launchers' dispatch, restated
# =============================================================================================
def wide_supported(Cc, heads, Nqp):                                       # mivp_tok_wide_supported
    return Cc in (96, 192, 384) and (Cc // heads) % 4 == 0 and Nqp % 32 == 0


def rows_supported(Cc, heads, Nqp):                                       # mivp_tok_rows_supported
    return Cc == 48 or wide_supported(Cc, heads, Nqp)


def qkv_fwd_arm(Cc, heads, Nqp, BP):                                      # mivp_swin_qkv_fwd, mivp_tok_wide_qkv_fwd
    if wide_supported(Cc, heads, Nqp):
        return "ws" if Cc in (96, 192) and Nqp >= 64 else "wide"
    gx = (BP * Nqp + 127) // 128
    nsplit = max(1, min((4096 + 4 * gx - 1) // (4 * gx), ((3 * Cc + 15) // 16) // 3))
    if Cc == 48 and heads == 4 and nsplit == 1 and Nqp % 32 == 0:
        return "ch12"
    ks = (Cc + 31) // 32
    return f"ks{ks}" + ("_nsplit1" if nsplit == 1 else "") if ks in (1, 2, 3, 4, 6) else "unsupported"


def tok16_arm(Cc):
    ct = (Cc + 15) // 16
    return f"tok16_ct{ct}" if ct in (1, 2, 3, 4, 6, 8, 12) else "unsupported"


def proj_fwd_arm(Cc, heads, Nqp):                                         # mivp_swin_proj_mlp_fwd
    return f"rows_c{Cc}" if rows_supported(Cc, heads, Nqp) else tok16_arm(Cc)


def proj_bwd_arm(Cc, heads, Nqp, wgrad):                                  # mivp_swin_proj_mlp_bwd: rows only without dn_out / dyw / d_pj
    return f"rows_c{Cc}" if rows_supported(Cc, heads, Nqp) and not wgrad else tok16_arm(Cc)


def qkv_bwd_arm(Cc, heads, Nqp):                                          # mivp_swin_qkv_bwd
    return f"wide_c{Cc}" if wide_supported(Cc, heads, Nqp) else tok16_arm(Cc)


# =============================================================================================
# cases
# =============================================================================================
class Case:
    """Descriptor, tables, operands (float64 on the CPU = exactly the device values) and device copies of one shape."""

    def __init__(self, Cc, heads, Nqp, BP, p=0.0, seed=0, dup=True):
        self.B, self.P = (2, BP // 2) if BP % 2 == 0 else (1, BP)
        Nq = Nqp - 3
        self.vol = self.P * Nq + 19
        d = swin_ops._fill_desc(self.B, Cc, heads, (Nq, 1, 1), self.P, Nq, Nqp, self.vol, 0, False)
        if p:
            swin_ops.set_dropout(d, (0.0, p, 11, 0xC0FFEE + seed))
        self.d, self.p = d, p
        self.scale = float(d.proj_drop_scale) if p else 1.0
        self.src, self.dst = T.make_tables(self.P, Nq, self.vol, 1000 + seed + Cc + Nqp, dup=dup)
        o = self.o = T.block_operands(d, 2000 + seed + Cc + Nqp)
        if self.B == 2:                                                   # the same x row in both batches, at one slot
            o.x[1, self.src[0, 1]] = o.x[0, self.src[0, 1]]
        self.T = BP * Nqp
        self.src_d, self.dst_d = self.src.to(torch.int32).to(DEV), self.dst.to(torch.int32).to(DEV)
        self.ln1 = (dev(o.ln1_w), dev(o.ln1_b))
        self.ln2 = (dev(o.ln2_w), dev(o.ln2_b))
        self.bp, self.bm = dev(o.bp), dev(o.bm)
        self.img = pack_images(Cc, o, 1 if Cc in WIDE_C else 0)

    def x_dev(self):
        """x with NaN in every voxel row no source names (the contract: never read)."""
        x = self.o.x.clone()
        unread = torch.ones(self.vol, dtype=torch.bool)
        unread[self.src[self.src >= 0]] = False
        assert bool(unread.any())
        x[:, unread] = NAN
        return dev(x, BF16)

    def keep(self):
        """The proj-dropout keep mask the kernels derive, [B*P][Nqp][C] float64 in {0, 1} (None without dropout)."""
        if not self.p:
            return None
        m = torch.empty((self.T, self.d.C), dtype=torch.uint8, device=DEV)
        L.call("mivp_dropout_masks", C.byref(self.d), None, L.ptr(m), L.stream())
        m = m.cpu().to(F64).view(self.B * self.P, self.d.Nqp, self.d.C)
        assert 0.2 < float(m.mean()) < 0.9
        return m


def image_sizes(Cc, with_natural):
    ct, ks = (Cc + 15) // 16, (Cc + 31) // 32
    img, two = ct * ks * 512, 2 if with_natural else 1
    return dict(wqkv_rm=3 * Cc * Cc, wqkv_f=((3 * Cc + 15) // 16) * ks * 512, wproj_f=img, wmlp_f=two * img,
                wqkv_t=ct * ((3 * 16 * ct + 31) // 32) * 512, wmlp_t=img, wproj_t=two * img)


NAMES = ("wqkv_rm", "wqkv_f", "wproj_f", "wmlp_f", "wqkv_t", "wmlp_t", "wproj_t")


def pack_images(Cc, o, with_natural, skip=None):
    """mivp_pack_block_weights into guarded NaN buffers -> {name: Out}; ``skip`` names the output passed as NULL."""
    masters = [dev(w) for w in (o.Wq, o.Wk, o.Wv, o.Wp, o.Wm)]
    outs = {k: Out((n,), BF16) for k, n in image_sizes(Cc, with_natural).items() if k != skip}
    wq, wk, wv, wp, wm = (L.ptr(m) for m in masters)
    a, b, c, e, f, g, h = (L.ptr(outs[k].t) if k in outs else None for k in NAMES)
    L.call("mivp_pack_block_weights", Cc, wq, wk, wv, wp, wm, with_natural, a, b, c, e, f, g, h, L.stream())
    torch.cuda.synchronize()
    return outs


def margin(entry, arm, **ratios):
    print(f"[margin] {entry} {arm}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def subset_rows(Tn):
    """All rows of a small case; of a large one the first and last 256, both sides of every 128-row boundary, every 97th."""
    if Tn <= 8192:
        return torch.arange(Tn)
    r = torch.arange(Tn)
    return r[(r < 256) | (r >= Tn - 256) | (r % 128 == 0) | (r % 128 == 127) | (r % 97 == 0)]


# =============================================================================================
# mivp_swin_qkv_fwd
# =============================================================================================
QKV_FWD = [(8, 2, 16, 5), (40, 2, 16, 5), (64, 4, 16, 4), (96, 4, 16, 5), (128, 8, 48, 3), (192, 4, 48, 3),
           (48, 4, 16, 5), (48, 4, 32, 4096), (48, 4, 352, 373), (48, 3, 32, 4096), (48, 12, 32, 4096),
           (96, 4, 64, 3), (192, 4, 64, 3), (96, 4, 96, 3), (96, 4, 32, 3), (192, 8, 32, 3), (384, 16, 32, 3)]
QKV_FWD_ARMS = ["ks1_nsplit1", "ks2", "ks2", "ks3", "ks4", "ks6", "ks2", "ch12", "ch12", "ks2_nsplit1", "ks2_nsplit1", "ws", "ws", "ws",
                "wide", "wide", "wide"]


def run_qkv_fwd(c, x_d):
    d = c.d
    hd = d.C // d.heads
    outs = [Out((c.B * c.P, d.heads, d.Nqp, hd), BF16) for _ in range(3)]
    L.call("mivp_swin_qkv_fwd", C.byref(d), L.ptr(x_d), L.ptr(c.src_d), L.ptr(c.ln1[0]), L.ptr(c.ln1[1]),
           L.ptr(c.img["wqkv_f"].t), L.ptr(outs[0].t), L.ptr(outs[1].t), L.ptr(outs[2].t), L.stream())
    torch.cuda.synchronize()
    return [o.done(f"qkv_fwd {n}") for o, n in zip(outs, "qkv")]


@pytest.mark.parametrize("shape,arm", list(zip(QKV_FWD, QKV_FWD_ARMS)),
                         ids=[f"{a}-C{s[0]}_h{s[1]}_Nqp{s[2]}_BP{s[3]}" for s, a in zip(QKV_FWD, QKV_FWD_ARMS)])
def test_qkv_fwd(shape, arm):
    Cc, heads, Nqp, BP = shape
    assert qkv_fwd_arm(Cc, heads, Nqp, BP) == arm
    if arm in ("ws", "wide") and (Nqp, BP) in ((96, 3), (32, 3)) and Cc == 96:
        assert (BP * Nqp) % 64 != 0                                       # WideGeom<6>::ROWS = 64: a partial last workgroup
    if shape == (48, 4, 352, 373):
        assert (BP * Nqp) % 128 == 96 and (BP * Nqp + 127) // 128 >= 1024  # ch12 with a partial last workgroup
    c = Case(Cc, heads, Nqp, BP)
    d, o = c.d, c.o
    q, k, v = run_qkv_fwd(c, c.x_dev())
    what = f"qkv_fwd {arm} C={Cc} heads={heads} Nqp={Nqp} B={c.B} P={c.P}"
    T.check_qkv_structure(d, c.src, q, k, v, what)
    # slots that gather the same x row: slot 1 of window 0 and the slot before the last of the last window; both batches
    srcs = c.src.repeat(c.B, 1)
    twins = [(0, 1), (c.P - 1, d.Nq - 2)] + ([(c.P, 1), (2 * c.P - 1, d.Nq - 2)] if c.B == 2 else [])
    assert len({int(srcs[a, s]) for a, s in twins}) == 1
    for name, t in zip("qkv", (q, k, v)):
        for a, s in twins[1:]:
            assert_same_bits(t[a, :, s], t[0, :, 1], f"{what} {name}: window {a} slot {s} gathers the x row of window 0 slot 1")
    ref = T.qkv_fwd(d, o.x, c.src, o.ln1_w, o.ln1_b, o.Wq, o.Wk, o.Wv)
    rows = subset_rows(c.T)
    pick = lambda t: t.permute(0, 2, 1, 3).reshape(c.T, d.C)[rows]        # [token rows][head-major channels]
    m = {n: T.check_interval(pick(g), pick(getattr(ref, n)), pick(getattr(ref, "b" + n)), f"{what} {n} [token row][channel]")
         for n, g in zip("qkv", (q, k, v))}
    margin("qkv_fwd", arm, **m)


# =============================================================================================
# mivp_swin_proj_mlp_fwd
# =============================================================================================
TOK16 = [(8, 2, 16, 5), (32, 2, 16, 5), (40, 2, 16, 5), (64, 4, 16, 4), (96, 4, 16, 5), (128, 8, 48, 3), (192, 4, 48, 3)]
ROWS32 = [(48, 4, 32, 3), (96, 4, 32, 3), (192, 8, 32, 3), (384, 16, 32, 3)]
ROWS48 = [(48, 4, 16, 5), (48, 4, 48, 5), (48, 4, 80, 5)]
PROJ_FWD = [(s, 0.0) for s in TOK16 + ROWS32 + ROWS48] + [(s, p) for s in ((40, 2, 16, 5), (48, 4, 16, 5), (96, 4, 32, 3))
                                                          for p in (0.5, 0.3)]


def proj_id(s, p, arm):
    return f"{arm}-C{s[0]}_h{s[1]}_Nqp{s[2]}_BP{s[3]}" + (f"_p{p}" if p else "")


def run_proj_fwd(c, x_d, o_d, with_t1):
    d = c.d
    t1 = Out((c.B * c.P, d.Nqp, d.C), BF16) if with_t1 else None
    y = Out((c.B, c.vol, d.C), BF16)
    L.call("mivp_swin_proj_mlp_fwd", C.byref(d), L.ptr(o_d), L.ptr(x_d), L.ptr(c.src_d), L.ptr(c.dst_d),
           L.ptr(c.img["wproj_f"].t), L.ptr(c.bp), L.ptr(c.ln2[0]), L.ptr(c.ln2[1]), L.ptr(c.img["wmlp_f"].t), L.ptr(c.bm),
           L.ptr(t1.t) if with_t1 else None, L.ptr(y.t), L.stream())
    torch.cuda.synchronize()
    flat = y.flat.cpu()
    assert bool(torch.isnan(flat[y.n:]).all()), "proj_mlp_fwd wrote behind y"
    return (t1.done("proj_mlp_fwd t1") if with_t1 else None), flat[:y.n].view(c.B, c.vol, d.C)


@pytest.mark.parametrize("shape,p", PROJ_FWD, ids=[proj_id(s, p, proj_fwd_arm(*s[:3])) for s, p in PROJ_FWD])
def test_proj_mlp_fwd(shape, p):
    Cc, heads, Nqp, BP = shape
    arm = proj_fwd_arm(Cc, heads, Nqp)
    assert arm == (f"rows_c{Cc}" if shape in ROWS32 + ROWS48 else f"tok16_ct{(Cc + 15) // 16}")
    if shape in ROWS48:
        assert Nqp % 32 != 0 and BP % 2 == 1 and (BP * Nqp) % 32 != 0     # granules across windows and across the end of T
    c = Case(Cc, heads, Nqp, BP, p)
    d, o = c.d, c.o
    x_d, o_d = c.x_dev(), dev(o.o, BF16)
    keep = c.keep()
    what = f"proj_mlp_fwd {arm} C={Cc} Nqp={Nqp} B={c.B} P={c.P} p={p}"
    t1, y = run_proj_fwd(c, x_d, o_d, True)
    ref = T.proj_mlp_fwd(d, o.o, o.x, c.src, c.dst, o.Wp, o.bp, o.ln2_w, o.ln2_b, o.Wm, o.bm, keep, c.scale, t1_stored=t1)
    m1 = T.check_interval(t1, ref.t1, ref.b_t1, what + " t1 [window][slot][channel]")
    named = ~torch.isnan(ref.y)
    assert bool(named.any()) and not bool(named.all())
    assert torch.equal(torch.isnan(y), ~named), what + ": y voxels no destination names stay NaN, every named one is written"
    m2 = T.check_interval(y, ref.y, ref.b_y, what + " y [batch][voxel][channel]")
    margin("proj_mlp_fwd", arm + (f" p={p}" if p else ""), t1=m1, y=m2)
    _, y2 = run_proj_fwd(c, x_d, o_d, False)                              # t1 = NULL: the same kernel, the same bits
    T.check_bits_equal(torch.nan_to_num(y2), torch.nan_to_num(y), what + " y without t1")
    assert torch.equal(torch.isnan(y2), torch.isnan(y))


# =============================================================================================
# mivp_swin_proj_mlp_bwd
# =============================================================================================
PROJ_BWD = ([(s, 0.0, w) for s in TOK16 + ROWS32 + ROWS48 for w in (False, True)]
            + [(s, p, True) for s in ((40, 2, 16, 5), (48, 4, 16, 5), (96, 4, 32, 3)) for p in (0.5, 0.3)]
            + [(s, 0.5, False) for s in ((40, 2, 16, 5), (48, 4, 16, 5), (96, 4, 32, 3))])


def run_proj_bwd(c, dy_d, t1_d, wgrad):
    d = c.d
    shape = (c.B * c.P, d.Nqp, d.C)
    names = ["dO", "dt1"] + (["dn_out", "dyw"] + (["d_pj"] if c.p else []) if wgrad else [])
    outs = {n: Out(shape, BF16) for n in names}
    ptr = lambda n: L.ptr(outs[n].t) if n in outs else None
    L.call("mivp_swin_proj_mlp_bwd", C.byref(d), L.ptr(dy_d), L.ptr(c.dst_d), L.ptr(t1_d), L.ptr(c.ln2[0]), L.ptr(c.ln2[1]),
           L.ptr(c.img["wmlp_t"].t), L.ptr(c.img["wproj_t"].t), ptr("dO"), ptr("dt1"), ptr("dn_out"), ptr("dyw"), ptr("d_pj"),
           L.stream())
    torch.cuda.synchronize()
    return {n: o.done(f"proj_mlp_bwd {n}") for n, o in outs.items()}


@pytest.mark.parametrize("shape,p,wgrad", PROJ_BWD,
                         ids=[proj_id(s, p, proj_bwd_arm(*s[:3], w)) + ("_wgrad" if w else "_data") for s, p, w in PROJ_BWD])
def test_proj_mlp_bwd(shape, p, wgrad):
    Cc, heads, Nqp, BP = shape
    arm = proj_bwd_arm(Cc, heads, Nqp, wgrad)
    want_arm = f"rows_c{Cc}" if shape in ROWS32 + ROWS48 and not wgrad else f"tok16_ct{(Cc + 15) // 16}"
    assert arm == ("unsupported" if (Cc, wgrad) == (384, True) else want_arm)
    c = Case(Cc, heads, Nqp, BP, p)
    d, o = c.d, c.o
    if arm == "unsupported":
        # FOUND by this test: weight-gradient mode leaves the row-image kernel, and the 16-token kernels stop at 12 channel
        # tiles, so C = 384 has no weight-gradient arm at any Nqp.  The contract for that is the refusal: MIVP_EUNSUPPORTED,
        # nothing launched, every output untouched.
        outs = [Out((BP, Nqp, Cc), BF16) for _ in range(4)]
        with pytest.raises(RuntimeError, match=r"failed with code -2"):
            L.call("mivp_swin_proj_mlp_bwd", C.byref(d), L.ptr(dev(o.dy, BF16)), L.ptr(c.dst_d), L.ptr(dev(o.t1, BF16)),
                   L.ptr(c.ln2[0]), L.ptr(c.ln2[1]), L.ptr(c.img["wmlp_t"].t), L.ptr(c.img["wproj_t"].t),
                   L.ptr(outs[0].t), L.ptr(outs[1].t), L.ptr(outs[2].t), L.ptr(outs[3].t), None, L.stream())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t.flat).all()) for t in outs)
        return
    dy = o.dy.clone()
    unnamed = torch.ones(c.vol, dtype=torch.bool)
    unnamed[c.dst[c.dst >= 0]] = False
    dy[:, unnamed] = NAN                                                  # dy of voxels no destination names is never read
    dy_d, t1_d = dev(dy, BF16), dev(o.t1, BF16)
    keep = c.keep()
    what = f"proj_mlp_bwd {arm} C={Cc} Nqp={Nqp} B={c.B} P={c.P} p={p} {'wgrad' if wgrad else 'data'}"
    got = run_proj_bwd(c, dy_d, t1_d, wgrad)
    if "d_pj" in got:
        operand = got["d_pj"]
    elif p:                                                               # p = 0.5: the masked operand is 2 dt1, exactly
        assert c.scale == 2.0
        operand = (got["dt1"].to(F64) * keep * 2.0)
    else:
        operand = got["dt1"]
    args = (d, torch.nan_to_num(dy), c.dst, o.t1, o.ln2_w, o.Wm, o.Wp, keep, c.scale)
    ref = T.proj_mlp_bwd(*args, operand_stored=operand)
    r32 = T.proj_mlp_bwd(*args, dt=F32, rnd=T.bf16_f32)
    m = {"dO": T.check_interval(got["dO"], ref.dO, ref.b_dO, what + " dO [window][slot][channel]")}
    m["dt1"], _ = T.check_err32(got["dt1"], ref.dt1, r32.dt1, what + " dt1 [window][slot][channel]")
    if wgrad:
        m["dn_out"] = T.check_interval(got["dn_out"], ref.dn_out, ref.b_dn, what + " dn_out [window][slot][channel]")
        T.check_bits_equal(got["dyw"], T.stored(ref.dyw), what + " dyw: dy in window order, zero rows where cropped")
        if p:
            m["d_pj"], _ = T.check_err32(got["d_pj"], ref.d_pj, r32.d_pj, what + " d_pj [window][slot][channel]")
            assert not bool(bits(got["d_pj"])[keep == 0].any()), what + ": dropped elements of d_pj are +0"
        if not rows_supported(Cc, heads, Nqp):                            # one kernel serves both modes: the same bits
            data = run_proj_bwd(c, dy_d, t1_d, False)
            assert_same_bits(data["dO"], got["dO"], what + " dO without the optional outputs")
            assert_same_bits(data["dt1"], got["dt1"], what + " dt1 without the optional outputs")
        # (rows arm: the data-gradient call runs another kernel; its own case above is checked by interval / err32)
    margin("proj_mlp_bwd", arm + (f" p={p}" if p else ""), **m)


# =============================================================================================
# mivp_swin_qkv_bwd
# =============================================================================================
QKV_BWD = TOK16 + ROWS48 + [(96, 4, 32, 3), (192, 8, 32, 3), (384, 16, 32, 3), (96, 4, 64, 3)]


def run_qkv_bwd(c, ins, with_dn):
    d = c.d
    dx = Out((c.B, c.vol, d.C), BF16)
    dn = Out((c.B * c.P, d.Nqp, d.C), BF16) if with_dn else None
    L.call("mivp_swin_qkv_bwd", C.byref(d), L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(ins[2]), L.ptr(ins[3]), L.ptr(c.src_d),
           L.ptr(c.ln1[0]), L.ptr(c.ln1[1]), L.ptr(c.img["wqkv_t"].t), L.ptr(ins[4]), L.ptr(dx.t),
           L.ptr(dn.t) if with_dn else None, L.stream())
    torch.cuda.synchronize()
    flat = dx.flat.cpu()
    assert bool(torch.isnan(flat[dx.n:]).all()), "qkv_bwd wrote behind dx"
    return flat[:dx.n].view(c.B, c.vol, d.C), (dn.done("qkv_bwd dn_out") if with_dn else None)


@pytest.mark.parametrize("shape", QKV_BWD, ids=[f"{qkv_bwd_arm(*s[:3])}-C{s[0]}_h{s[1]}_Nqp{s[2]}_BP{s[3]}" for s in QKV_BWD])
def test_qkv_bwd(shape):
    Cc, heads, Nqp, BP = shape
    arm = qkv_bwd_arm(Cc, heads, Nqp)
    assert arm == (f"wide_c{Cc}" if shape in QKV_BWD[-4:] else f"tok16_ct{(Cc + 15) // 16}")
    c = Case(Cc, heads, Nqp, BP)
    d, o = c.d, c.o
    ins = [dev(o.dq, BF16), dev(o.dk, BF16), dev(o.dv, BF16), c.x_dev(), dev(o.dt1, BF16)]
    what = f"qkv_bwd {arm} C={Cc} heads={heads} Nqp={Nqp} B={c.B} P={c.P}"
    dx, dn = run_qkv_bwd(c, ins, True)
    args = (d, o.dq, o.dk, o.dv, o.x, c.src, o.ln1_w, o.Wq, o.Wk, o.Wv, o.dt1)
    ref, r32 = T.qkv_bwd(*args), T.qkv_bwd(*args, dt=F32, rnd=T.bf16_f32)
    m = {"dn_out": T.check_interval(dn, ref.dn_out, ref.b_dn, what + " dn_out [window][slot][channel]")}
    named = ~torch.isnan(ref.dx)
    assert bool(named.any()) and not bool(named.all())
    assert torch.equal(torch.isnan(dx), ~named), what + ": dx voxels no source names stay untouched, every named one is written"
    # the voxel two slots gather: either slot's row is right; everything else against the one row it has
    twin = int(c.src[0, 1])
    once64, once32 = ref.dx.clone(), r32.dx.clone()
    once64[:, twin], once32[:, twin] = NAN, NAN
    m["dx"], err32 = T.check_err32(dx, once64, once32, what + " dx [batch][voxel][channel]")
    bar = (8 * err32 + 2.0 ** -22) * float(torch.nan_to_num(once64).abs().max())
    for b in range(c.B):
        cands = [ref.dx_rows[b * c.P + pw, s] for pw, s in ((0, 1), (c.P - 1, d.Nq - 2))]
        fits = []
        for cand in cands:
            try:
                T.check_interval(dx[b, twin], cand, torch.full_like(cand, bar), what)
                fits.append(True)
            except T.Located:
                fits.append(False)
        assert any(fits), f"{what}: dx[{b}][{twin}] is the row of neither slot that gathers that voxel"
    margin("qkv_bwd", arm, **m)
    dx2, _ = run_qkv_bwd(c, ins, False)                                   # dn_out = NULL: the same kernel
    same = torch.ones(c.vol, dtype=torch.bool)
    same[twin] = False
    T.check_bits_equal(torch.nan_to_num(dx2[:, same]), torch.nan_to_num(dx[:, same]), what + " dx without dn_out")


# =============================================================================================
# refusal
# =============================================================================================
def test_c384_with_nqp16_is_refused_by_all_four_entries():
    Cc, heads, Nqp, BP = 384, 16, 16, 3
    assert not rows_supported(Cc, heads, Nqp) and tok16_arm(Cc) == "unsupported"
    assert qkv_fwd_arm(Cc, heads, Nqp, BP) == "unsupported" and qkv_bwd_arm(Cc, heads, Nqp) == "unsupported"
    c = Case(Cc, heads, Nqp, BP)
    d, o = c.d, c.o
    rows, hm, vox = (BP, Nqp, Cc), (BP, heads, Nqp, Cc // heads), (c.B, c.vol, Cc)
    x_d, o_d, t1_d, dy_d = c.x_dev(), dev(o.o, BF16), dev(o.t1, BF16), dev(o.dy, BF16)
    g = [dev(t, BF16) for t in (o.dq, o.dk, o.dv, o.dt1)]
    im = {k: L.ptr(v.t) for k, v in c.img.items()}
    z = [Out(hm, BF16) for _ in range(3)] + [Out(rows, BF16), Out(vox, BF16)] + [Out(rows, BF16) for _ in range(5)] \
        + [Out(vox, BF16), Out(rows, BF16)]
    zp = [L.ptr(t.t) for t in z]
    refused = pytest.raises(RuntimeError, match=r"failed with code -2")     # MIVP_EUNSUPPORTED
    with refused:
        L.call("mivp_swin_qkv_fwd", C.byref(d), L.ptr(x_d), L.ptr(c.src_d), L.ptr(c.ln1[0]), L.ptr(c.ln1[1]), im["wqkv_f"],
               zp[0], zp[1], zp[2], L.stream())
    with refused:
        L.call("mivp_swin_proj_mlp_fwd", C.byref(d), L.ptr(o_d), L.ptr(x_d), L.ptr(c.src_d), L.ptr(c.dst_d), im["wproj_f"],
               L.ptr(c.bp), L.ptr(c.ln2[0]), L.ptr(c.ln2[1]), im["wmlp_f"], L.ptr(c.bm), zp[3], zp[4], L.stream())
    with refused:
        L.call("mivp_swin_proj_mlp_bwd", C.byref(d), L.ptr(dy_d), L.ptr(c.dst_d), L.ptr(t1_d), L.ptr(c.ln2[0]), L.ptr(c.ln2[1]),
               im["wmlp_t"], im["wproj_t"], zp[5], zp[6], zp[7], zp[8], zp[9], L.stream())
    with refused:
        L.call("mivp_swin_qkv_bwd", C.byref(d), L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]), L.ptr(x_d), L.ptr(c.src_d),
               L.ptr(c.ln1[0]), L.ptr(c.ln1[1]), im["wqkv_t"], L.ptr(g[3]), zp[10], zp[11], L.stream())
    torch.cuda.synchronize()
    for i, t in enumerate(z):
        assert bool(torch.isnan(t.flat).all()), f"a refused call wrote to its output {i}"


# =============================================================================================
# mivp_pack_block_weights
# =============================================================================================
@pytest.mark.parametrize("with_natural", [0, 1])
@pytest.mark.parametrize("Cc", [8, 40, 48, 96, 128, 384])
def test_pack_block_weights(Cc, with_natural):
    g = torch.Generator().manual_seed(Cc)
    o = T.SimpleNamespace(**{n: torch.randn((Cc, Cc), generator=g, dtype=F32) for n in ("Wq", "Wk", "Wv", "Wp", "Wm")})   # f32 masters
    want = T.block_images(Cc, o.Wq, o.Wk, o.Wv, o.Wp, o.Wm, with_natural)
    ks, ct = (Cc + 31) // 32, (Cc + 15) // 16
    b = lambda t: t.to(BF16).to(DEV)
    wqkv = torch.cat([b(o.Wq), b(o.Wk), b(o.Wv)], 0)
    frag = lambda W, p=False, k=0: swin_ops.pack_weight_frags(W.contiguous(), paired=p, k_steps=k).reshape(-1)
    single = dict(wqkv_rm=wqkv.reshape(-1), wqkv_f=frag(wqkv), wproj_f=frag(b(o.Wp)), wmlp_f=frag(b(o.Wm), True),
                  wqkv_t=frag(wqkv.t(), k=(3 * 16 * ct + 31) // 32), wmlp_t=frag(b(o.Wm).t()), wproj_t=frag(b(o.Wp).t(), True))
    if with_natural:
        single["wmlp_f"] = torch.cat([single["wmlp_f"], frag(b(o.Wm))])
        single["wproj_t"] = torch.cat([single["wproj_t"], frag(b(o.Wp).t())])
    for skip in (None,) + NAMES:                                          # every output, then each pointer NULL in turn
        outs = pack_images(Cc, o, with_natural, skip)
        assert set(outs) == set(NAMES) - {skip}
        for k, buf in outs.items():
            what = f"pack_block_weights C={Cc} natural={with_natural} without {skip}: {k}"
            got = buf.done(what)                                          # guard tail untouched, also behind the natural image
            T.check_bits_equal(got, want[k], what + " against tok_ref.block_images")
            if skip is None:
                T.check_bits_equal(got, single[k].cpu(), what + " against mivp_pack_weight_frags")
