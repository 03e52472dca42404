"""Direct parity tests of the loss, optimizer and metric-count kernels against tests/loss_optim_ref.py (float64, CPU).

Entries under test, each called through ``_lib.call`` on its own operands: mivp_dice_focal / mivp_dice_focal_grad /
mivp_dice_focal_ws (csrc/loss.hip), mivp_adamw_multi / mivp_adamw_multi_dev / mivp_ema_multi / mivp_store_floats
(csrc/proto.hip), mivp_seg_counts (csrc/metrics.hip); and the wrappers train.dice_focal_loss, losses.dice_loss,
optim.FusedAdamW, optim.ema_update_ where a case is about the wrapper.

Bars (tests/loss_optim_ref.py derives them; tests/test_loss_optim_host.py shows on the CPU that f32 torch meets them and that
plausible kernel bugs do not):
  loss value     2e-5 max(1, |want|) against float64
  loss gradient  rel-L2 < 1e-4, and per element LOSS_MARGIN x E32 x max |g64| with E32 the error of the reference's own
                 formulas run in f32 on the same case (each case prints E32, the kernel's error and their ratio)
  AdamW, EMA     per element within the propagated rounding bound, after every step, on p, exp_avg and exp_avg_sq
  counts, store  integer- / bit-exact

Every output and workspace buffer sits between guard words that must come back untouched; outputs start as the guard
pattern (a NaN), so an element that was never written is seen as well.  NaN logits are out of contract for
mivp_seg_counts (an arg-max over NaN has no defined winner) and are not tested."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_optim_ref as R  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import optim, train
from mivp_amd.losses import dice_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
GUARD = 64                                                        # floats: 256 bytes, keeps the payload 16-byte aligned
PATTERN = 0x7FC0BEEF                                              # a quiet NaN with a payload no arithmetic produces
GAPS = (3, 64, 1, 5, 17)                                          # floats between the tensors of an arena: odd addresses too
K_LOSS = 3 * 8 + 1                                                # floats per partial row of the loss workspace


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not torch.equal(bits(a), bits(b)):
        bad = torch.nonzero(bits(a) != bits(b))
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} elements differ in their bits; first at {first}: "
                             f"{float(a.cpu()[first])!r} != {float(b.cpu()[first])!r}")


class Arena:
    """f32 tensors carved out of one allocation, a guard before the first, gaps between them and a guard after the last,
    all filled with PATTERN.  ``init[i] is None`` leaves tensor i as PATTERN (an output that has to be written)."""

    def __init__(self, shapes, init=None):
        self.shapes = [tuple(s) for s in shapes]
        self.off, pos = [], GUARD
        for i, s in enumerate(self.shapes):
            self.off.append(pos)
            pos += int(math.prod(s)) + (GAPS[i % len(GAPS)] if i + 1 < len(self.shapes) else 0)
        self.total = pos + GUARD
        self.flat = torch.empty(self.total, dtype=F32, device=DEV)
        self.flat.view(torch.int32).fill_(PATTERN)
        self.t = [self.flat[o:o + int(math.prod(s))].view(s) for o, s in zip(self.off, self.shapes)]
        payload = torch.zeros(self.total, dtype=torch.bool)
        for o, s in zip(self.off, self.shapes):
            payload[o:o + int(math.prod(s))] = True
        self.payload = payload
        if init is not None:
            for t, v in zip(self.t, init):
                if v is not None:
                    t.copy_(v)

    def done(self, what, written=True):
        """Guards and gaps untouched (and, with ``written``, no payload element left as PATTERN): the tensors on the CPU."""
        flat = self.flat.cpu()
        raw = flat.view(torch.int32)
        bad = torch.nonzero((raw != PATTERN) & ~self.payload)
        assert bad.numel() == 0, (f"{what}: {bad.shape[0]} guard words were overwritten, first at float offset {int(bad[0])} "
                                  f"(tensors start at {self.off[:8]}...)")
        if written:
            left = torch.nonzero((raw == PATTERN) & self.payload)
            assert left.numel() == 0, f"{what}: {left.shape[0]} output elements were never written, first at offset {int(left[0])}"
        return [flat[o:o + int(math.prod(s))].view(s) for o, s in zip(self.off, self.shapes)]


def one(shape, init=None):
    return Arena([shape], None if init is None else [init])


# =============================================================================================
# Dice + focal loss
# =============================================================================================
def bpb_of(vol):
    return max(1, min(256, (vol + 1023) // 1024))


def loss_call(zd, yd, inc_bg, gamma, form="fused", gscale=None):
    """(loss, dz) on the CPU.  fused: mivp_dice_focal with dlogits; split: the value call without dlogits, then
    mivp_dice_focal_grad on the same workspace with ``gscale`` (None: a NULL pointer)."""
    B, vol, Cc = zd.shape
    n_ws = int(L.lib().mivp_dice_focal_ws(B, vol))
    assert n_ws == B * (bpb_of(vol) + 1) * K_LOSS
    ws, loss, dz = one((n_ws,)), one((1,)), one((B, vol, Cc))
    gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    if form == "fused":
        assert gscale is None
        L.call("mivp_dice_focal", L.ptr(zd), L.ptr(yd), B, vol, Cc, inc_bg, gamma, L.ptr(ws.t[0]), L.ptr(loss.t[0]),
               L.ptr(dz.t[0]), L.stream())
    else:
        L.call("mivp_dice_focal", L.ptr(zd), L.ptr(yd), B, vol, Cc, inc_bg, gamma, L.ptr(ws.t[0]), L.ptr(loss.t[0]), None,
               L.stream())
        L.call("mivp_dice_focal_grad", L.ptr(zd), L.ptr(yd), B, vol, Cc, inc_bg, gamma, L.ptr(ws.t[0]), L.ptr(gs),
               L.ptr(dz.t[0]), L.stream())
    torch.cuda.synchronize()
    ws.done("loss workspace", written=False)
    return loss.done("loss value")[0], dz.done("dlogits")[0]


class LossRef:
    def __init__(self, z, y, inc_bg, gamma):
        self.l64, self.g64 = R.dice_focal_ref64(z, y, inc_bg, gamma)
        _, g32 = R.dice_focal_ref64(z, y, inc_bg, gamma, dtype=F32)
        self.e32, self.scale = R.loss_yardstick(g32, self.g64)
        self.bar_abs, self.bar_norm = R.loss_grad_bar(g32, self.g64)


def loss_failures(got_loss, got_dz, ref, what, k=1.0):
    """Print the case's figures, then return the list of bars it misses (k: the incoming gradient)."""
    out = []
    want = float(ref.l64)
    if not abs(float(got_loss) - want) <= R.LOSS_VALUE_BAR * max(1.0, abs(want)):
        out.append(f"{what}: loss {float(got_loss)!r}, float64 {want!r}")
    if k == 0.0:
        if bool(got_dz.double().abs().max() > 0):
            out.append(f"{what}: gscale 0 must give zeros")
        return out
    g64 = k * ref.g64
    err = float((got_dz.double() - g64).abs().max()) / (abs(k) * ref.scale)
    print(f"[loss-ratio] {what}: E32 {ref.e32:.3e} kernel {err:.3e} ratio {err / ref.e32:.3f} bar {ref.bar_norm:.3e}")
    if not ref.bar_norm <= 1e-4:
        out.append(f"{what}: the per-element bar {ref.bar_norm:.3e} is looser than 1e-4")
    l2 = R.rel_l2(got_dz, g64)
    if not l2 < R.LOSS_L2_BAR:
        out.append(f"{what}: gradient rel-L2 {l2:.3e}")
    try:
        R.assert_within_located(got_dz, g64, abs(k) * ref.bar_abs, "bvc", what)
    except AssertionError as e:
        out.append(str(e))
    return out


def run_loss_case(z, y, inc_bg, gamma, what, form="fused"):
    ref = LossRef(z, y, inc_bg, gamma)
    zd, yd = z.to(DEV), y.to(DEV)
    loss, dz = loss_call(zd, yd, inc_bg, gamma, form, None if form == "fused" else 1.0)
    return loss_failures(loss, dz, ref, what)


@pytest.mark.parametrize("C", R.LOSS_CLASSES)
@pytest.mark.parametrize("dims", R.SCALAR_VOLS + R.VEC_VOLS, ids=lambda d: "x".join(str(v) for v in d))
def test_loss_every_instantiation(dims, C):
    """Scalar (vol % 4 != 0) and vectorised kernels for every C in 2..8, with and without background, focal and Dice alone.
    B = 3 puts the sample boundaries of the scalar gradient pass at odd offsets; vol = 4 with B = 5: every quad a sample."""
    vol = dims[0] * dims[1] * dims[2]
    B = 5 if vol == 4 else 3
    assert (vol % 4 != 0) == (dims in R.SCALAR_VOLS) and bpb_of(vol) <= 2
    z, y = R.loss_inputs(B, vol, C, 1000 * C + vol)
    fails = []
    for inc_bg, gamma in R.LOSS_MODES:
        fails += run_loss_case(z, y, inc_bg, gamma, f"vol {vol} B {B} C {C} bg {inc_bg} gamma {gamma}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("vol,bpb", [(2052, 3), (2053, 3), (66 * 64 * 64, 256)])
def test_loss_partial_rows(vol, bpb, C):
    """Several partial rows per sample in the statistics pass; at 270 336 voxels the 256 cap makes its loop stride."""
    assert bpb_of(vol) == bpb and (vol + 1023) // 1024 >= bpb
    z, y = R.loss_inputs(2, vol, C, vol + C)
    fails = run_loss_case(z, y, 1, 4.0, f"vol {vol} ({bpb} partial rows) C {C}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dims", [(101, 101, 103), (164, 160, 160)], ids=["scalar", "vec"])
def test_loss_gradient_grid_cap(dims):
    """The smallest shapes whose gradient pass needs more than its 8192 workgroups: 8209 (scalar), 8200 (vectorised)."""
    vol = dims[0] * dims[1] * dims[2]
    work = 2 * vol if vol % 4 else 2 * vol // 4
    assert (work + 255) // 256 > 8192 and ((vol % 4 != 0) == (dims[0] == 101))
    z, y = R.loss_inputs(2, vol, 2, 99)
    fails = run_loss_case(z, y, 1, 4.0, f"grid cap {dims}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("vol", [315, 336])
@pytest.mark.parametrize("kind,C,gamma", [("sample_bg", 2, 4.0), ("absent", 5, 4.0), ("saturated", 3, 4.0), ("plain", 4, 0.0),
                                          ("saturated", 2, -1.0)])
def test_loss_awkward_data(kind, C, gamma, vol):
    """A sample that is background everywhere (T = 0 and I = 0 for the foreground class), a class that occurs nowhere,
    logits at +-30 where softmax and sigmoid saturate, and gamma = 0 (the focal branch with every weight 1)."""
    z, y = R.loss_inputs(3, vol, C, 77 + vol, kind)
    fails = []
    for inc_bg in (1, 0):
        fails += run_loss_case(z, y, inc_bg, gamma, f"{kind} vol {vol} C {C} bg {inc_bg} gamma {gamma}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("vol", [315, 336])
@pytest.mark.parametrize("gamma", [4.0, -1.0])
def test_loss_entry_forms(vol, gamma):
    B, Cc, inc_bg = 3, 3, 0
    z, y = R.loss_inputs(B, vol, Cc, 55 + vol)
    ref = LossRef(z, y, inc_bg, gamma)
    zd, yd = z.to(DEV), y.to(DEV)
    what = f"vol {vol} gamma {gamma}"
    l_f, g_f = loss_call(zd, yd, inc_bg, gamma, "fused")          # value + gradient in one call: gscale == nullptr
    l_s, g_s = loss_call(zd, yd, inc_bg, gamma, "split", 1.0)
    l_n, g_n = loss_call(zd, yd, inc_bg, gamma, "split", None)
    l_2, g_2 = loss_call(zd, yd, inc_bg, gamma, "fused")
    fails = loss_failures(l_f, g_f, ref, what + " fused")
    assert_same_bits(g_s, g_f, what + ": gradient, split with gscale 1 against fused")
    assert_same_bits(g_n, g_f, what + ": gradient, split with a NULL gscale against fused")
    assert_same_bits(g_2, g_f, what + ": gradient of a second identical call")
    for other in (l_s, l_n, l_2):
        assert_same_bits(other.reshape(1), l_f.reshape(1), what + ": loss value")
    for k in (0.0, -2.5):
        l_k, g_k = loss_call(zd, yd, inc_bg, gamma, "split", k)
        fails += loss_failures(l_k, g_k, ref, what + f" gscale {k}", k)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dims", [(5, 7, 9), (6, 7, 8)], ids=["odd", "vec"])
def test_loss_wrappers(dims):
    """train.dice_focal_loss and losses.dice_loss on the channels-first VIEW of channels-last storage, and dice_loss on a
    contiguous channels-first tensor (copied to channels-last, never an eager path), with an incoming gradient."""
    B, Cc = 3, 4
    vol = dims[0] * dims[1] * dims[2]
    z, y = R.loss_inputs(B, vol, Cc, 66 + vol)
    yd = y.view(B, 1, *dims).to(DEV)
    fails = []
    for inc_bg in (True, False):
        ref = LossRef(z, y, int(inc_bg), 4.0)
        base = z.view(B, *dims, Cc).to(DEV).requires_grad_(True)
        got = train.dice_focal_loss(base.permute(0, 4, 1, 2, 3), yd, inc_bg, 4.0)
        (got * 2.5).backward()
        torch.cuda.synchronize()
        fails += loss_failures(got.detach().cpu(), base.grad.cpu().view(B, vol, Cc), ref, f"dice_focal_loss {dims} bg {inc_bg}", 2.5)
        ref = LossRef(z, y, int(inc_bg), -1.0)
        base = z.view(B, *dims, Cc).to(DEV).requires_grad_(True)
        got = dice_loss(base.permute(0, 4, 1, 2, 3), yd, inc_bg)
        (got * 0.7).backward()
        plain = z.view(B, *dims, Cc).permute(0, 4, 1, 2, 3).contiguous().to(DEV).requires_grad_(True)
        got2 = dice_loss(plain, yd, inc_bg)
        got2.backward()
        torch.cuda.synchronize()
        fails += loss_failures(got.detach().cpu(), base.grad.cpu().view(B, vol, Cc), ref, f"dice_loss view {dims} bg {inc_bg}", 0.7)
        grad2 = plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(B, vol, Cc)
        fails += loss_failures(got2.detach().cpu(), grad2, ref, f"dice_loss channels-first {dims} bg {inc_bg}")
        assert float(got2.detach()) == float(got.detach())
    assert not fails, "\n".join(fails)


# =============================================================================================
# AdamW
# =============================================================================================
def chunk_tables(sizes):
    """(chunks [n_chunks, 2] int32: tensor id, 1024-element piece; begin [n + 1]: first chunk of each tensor)."""
    rows, begin = [], [0]
    for t, n in enumerate(sizes):
        k = (n + 1023) // 1024
        rows += [(t, j) for j in range(k)]
        begin.append(begin[-1] + k)
    return np.asarray(rows, np.int32).reshape(-1, 2), begin


class AdamArena:
    """p, m, v of every tensor of a case in ONE arena (p0, m0, v0, p1, ...): a write past a tensor's end lands in a gap or
    in a neighbour, and both are compared."""

    def __init__(self, case):
        shapes, init = [], []
        for s, p in zip(case["shapes"], case["p0"]):
            shapes += [s, s, s]
            init += [p, torch.zeros(s), torch.zeros(s)]
        self.case = case
        self.arena = Arena(shapes, init)
        self.p, self.m, self.v = self.arena.t[0::3], self.arena.t[1::3], self.arena.t[2::3]

    def check(self, ref_states, what):
        got = self.arena.done(what)
        for i, st in enumerate(ref_states):
            p, m, v = got[3 * i], got[3 * i + 1], got[3 * i + 2]
            w = f"{what} tensor {i} {self.case['shapes'][i]} group {self.case['group_of'][i]}"
            if st is None:                                        # no gradient: nothing of it may move
                assert_same_bits(p, self.case["p0"][i], w + " p (no gradient)")
                assert not bool(bits(m).any()) and not bool(bits(v).any()), w
                continue
            for name, g, val, bound in (("p", p, st.p, st.ep), ("exp_avg", m, st.m, st.em), ("exp_avg_sq", v, st.v, st.ev)):
                R.assert_within_located(g.reshape(-1), val.reshape(-1), bound.reshape(-1), "i", f"{w} {name}")
        return got


def fused_adamw(aa, capturable):
    case = aa.case
    params = [torch.nn.Parameter(p) for p in aa.p]
    assert all(q.data_ptr() == p.data_ptr() for q, p in zip(params, aa.p))
    used = sorted(set(case["group_of"]))
    opt = optim.FusedAdamW([dict(params=[q for q, gi in zip(params, case["group_of"]) if gi == k], **R.ADAM_GROUPS[k])
                            for k in used], capturable=capturable)
    assert used == list(range(len(used)))
    for i, q in enumerate(params):                                # the state lives in the arena, not in fresh allocations
        opt.state[q] = {"step": torch.tensor(0.0), "exp_avg": aa.m[i], "exp_avg_sq": aa.v[i]}
    return opt, params


def test_adamw_groups_steps_and_states():
    """Eight groups (one without weight decay, group 7 in use), the tensor ladder, an all-zero gradient, a tensor without
    gradient in the middle, three steps: p, exp_avg and exp_avg_sq after every step; plain and capturable forms bit-equal."""
    assert int(L.lib().mivp_sizeof_opt(0)) == 40
    case = R.adam_case()
    assert max(case["group_of"]) == 7 and any(g["weight_decay"] == 0.0 for g in R.ADAM_GROUPS)
    assert float(case["grads"][0][R.ADAM_ZERO_GRAD].abs().max()) == 0.0 and case["grads"][0][R.ADAM_NO_GRAD] is None
    ref = R.adam_reference(case)
    results = {}
    for capturable in (False, True):
        aa = AdamArena(case)
        opt, params = fused_adamw(aa, capturable)
        for step, row in enumerate(case["grads"]):
            for q, gr in zip(params, row):
                q.grad = None if gr is None else gr.to(DEV)
            opt.step()
            torch.cuda.synchronize()
            results[capturable, step] = aa.check(ref[step], f"{'capturable' if capturable else 'plain'} step {step + 1}")
    for step in range(len(case["grads"])):
        for i, (a, b) in enumerate(zip(results[False, step], results[True, step])):
            assert_same_bits(a, b, f"plain against capturable, step {step + 1}, arena tensor {i}")


def test_adamw_more_tensors_than_one_launch_holds():
    """400 tensors: the second launch of adamw_launch and its grad_base offset.  The entry is called directly with a host
    gradient-pointer array of exactly n entries and a chunk_begin of n + 1, then through FusedAdamW from the same start."""
    assert int(L.lib().mivp_sizeof_opt(0)) == 40
    case = R.adam_many_case()
    n = len(case["shapes"])
    sizes = [int(math.prod(s)) for s in case["shapes"]]
    assert n == 400 and sizes[383] == 1025 and sizes[384] == 3073 and sizes[399] == 257 and max(case["group_of"]) == 7
    ref = R.adam_reference(case)
    chunks, begin = chunk_tables(sizes)
    assert len(begin) == n + 1 and begin[-1] == chunks.shape[0]

    direct = AdamArena(case)
    rows = np.zeros((n, 5), np.int64)
    for i in range(n):
        rows[i] = (direct.p[i].data_ptr(), direct.m[i].data_ptr(), direct.v[i].data_ptr(), sizes[i], case["group_of"][i])
    tensors_dev = torch.from_numpy(rows).to(DEV)
    chunks_dev = torch.from_numpy(chunks).to(DEV)
    begin_arr = (C.c_int32 * (n + 1))(*begin)
    got_direct = []
    for step, row in enumerate(case["grads"]):
        grads = [g.to(DEV) for g in row]                          # alive until the synchronize below
        gptr = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
        hyper = np.ascontiguousarray(np.stack([R.adam_hyper_row(step=step + 1, **grp) for grp in R.ADAM_GROUPS]))
        L.call("mivp_adamw_multi", L.ptr(tensors_dev), gptr, n, begin_arr, hyper.ctypes.data_as(C.POINTER(C.c_float)),
               len(R.ADAM_GROUPS), L.ptr(chunks_dev), L.stream())
        torch.cuda.synchronize()
        got_direct.append(direct.check(ref[step], f"direct entry, step {step + 1}"))

    for capturable in (False, True):
        aa = AdamArena(case)
        opt, params = fused_adamw(aa, capturable)
        for step, row in enumerate(case["grads"]):
            for q, gr in zip(params, row):
                q.grad = gr.to(DEV)
            opt.step()
            torch.cuda.synchronize()
            got = aa.check(ref[step], f"FusedAdamW(capturable={capturable}), step {step + 1}")
            for i, (a, b) in enumerate(zip(got, got_direct[step])):
                assert_same_bits(a, b, f"FusedAdamW(capturable={capturable}) against the direct call, step {step + 1}, arena tensor {i}")


# =============================================================================================
# EMA, store_floats
# =============================================================================================
@pytest.mark.parametrize("tau", R.EMA_TAUS)
def test_ema_ladder(tau):
    teachers, students = R.ema_case()
    n = len(teachers)
    ta = Arena([t.shape for t in teachers], teachers)
    sa = Arena([s.shape for s in students], students)
    sizes = [t.numel() for t in teachers]
    rows = np.asarray([(ta.t[i].data_ptr(), sa.t[i].data_ptr(), sizes[i]) for i in range(n)], np.int64)
    chunks, _ = chunk_tables(sizes)
    rows_dev, chunks_dev = torch.from_numpy(rows).to(DEV), torch.from_numpy(chunks).to(DEV)
    L.call("mivp_ema_multi", L.ptr(rows_dev), L.ptr(chunks_dev), chunks.shape[0], tau, L.stream())
    torch.cuda.synchronize()
    got = ta.done(f"EMA teachers tau={tau}")
    for i, s in enumerate(sa.done(f"EMA students tau={tau}")):
        assert_same_bits(s, students[i], f"tau={tau}: student {i} was modified")
    for i, g in enumerate(got):
        what = f"EMA tau={tau} tensor {i} {tuple(teachers[i].shape)}"
        val, bound = R.ema_ref64(teachers[i], students[i], tau)
        R.assert_within_located(g.reshape(-1), val.reshape(-1), bound.reshape(-1), "i", what)
        if tau == 1.0:
            assert_same_bits(g, teachers[i], what + ": tau = 1 keeps the teacher")
        if tau == 0.0:
            assert_same_bits(g, students[i], what + ": tau = 0 copies the student")
    # the wrapper builds the same tables: same bits
    tw = Arena([t.shape for t in teachers], teachers)
    optim.ema_update_(tw.t, sa.t, tau, optim.EmaPlan())
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(tw.done(f"ema_update_ tau={tau}"), got)):
        assert_same_bits(a, b, f"ema_update_ against the direct call, tau={tau}, tensor {i}")


@pytest.mark.parametrize("n", [1, 63, 64])
def test_store_floats(n):
    g = R.gen(n)
    host = torch.randn(64, generator=g, dtype=F32).numpy().copy()
    host[0], host[n - 1] = np.float32(-0.0) if n > 1 else np.float32(1e-40), np.float32(1e-40)
    dst = one((64,))
    L.call("mivp_store_floats", L.ptr(dst.t[0]), host.ctypes.data_as(C.POINTER(C.c_float)), n, L.stream())
    torch.cuda.synchronize()
    got = dst.done(f"store_floats n={n}", written=False)[0]
    assert_same_bits(got[:n], torch.from_numpy(host[:n]), f"store_floats n={n}")
    assert bool((bits(got[n:]) == PATTERN).all()), f"store_floats n={n} wrote beyond n"


# =============================================================================================
# per-class counts
# =============================================================================================
GUARD64 = 0x5EEDFACE5EEDFACE


class CountTable:
    """The full-size int64 [16][3] table, zeroed, with guard words behind it."""

    def __init__(self):
        self.flat = torch.zeros(48 + 16, dtype=torch.int64, device=DEV)
        self.flat[48:] = GUARD64

    def add(self, z, y, Cc, clast):
        B, _, vol = z.shape
        zd = (z.permute(0, 2, 1).contiguous() if clast else z.contiguous()).to(DEV)
        yd = y.contiguous().to(DEV)
        L.call("mivp_seg_counts", L.ptr(zd), L.ptr(yd), B * vol, Cc, clast, vol, L.ptr(self.flat), L.stream())
        torch.cuda.synchronize()

    def check(self, want, Cc, what):
        flat = self.flat.cpu()
        assert bool((flat[48:] == GUARD64).all()), what + ": wrote behind the table"
        R.assert_equal_located(flat[:3 * Cc].view(Cc, 3), want.to(F64), "ck", what + " [class][inter, pred, target]")
        assert not bool(flat[3 * Cc:48].any()), what + f": the {48 - 3 * Cc} cells of unused classes must stay zero"


@pytest.mark.parametrize("clast", [0, 1])
@pytest.mark.parametrize("Cc", [1, 2, 5, 16])
def test_seg_counts(Cc, clast):
    """B = 3 at an odd volume, logits from five values (frequent ties, voxels with all channels equal), labels outside the
    class range and non-integer labels; two calls into one table accumulate."""
    B, vol = 3, 5 * 7 * 9
    z, y = R.seg_case(B, vol, Cc, 40 + Cc)
    if Cc > 1:
        assert bool(((z == z.amax(1, keepdim=True)).sum(1) > 1).any()) and bool((z == z[:, :1]).all(1).any())
    assert bool((y < 0).any()) and bool((y >= Cc).any()) and bool((y != y.round()).any())
    want = R.seg_counts_ref(z, y, Cc)
    assert int(want[:, 1].sum()) == B * vol and int(want[:, 2].sum()) < B * vol
    tab = CountTable()
    tab.add(z, y, Cc, clast)
    tab.check(want, Cc, f"seg_counts C={Cc} channels_last={clast}")
    z2, y2 = R.seg_case(B, vol, Cc, 50 + Cc)
    tab.add(z2, y2, Cc, clast)
    tab.check(want + R.seg_counts_ref(z2, y2, Cc), Cc, f"seg_counts C={Cc} channels_last={clast}, second call")


@pytest.mark.parametrize("clast", [0, 1])
def test_seg_counts_beyond_the_grid_cap(clast):
    """2049 x 256 + 3 voxels need 2050 workgroups, the launch has 2048: the grid-stride loop runs."""
    B, Cc = 3, 5
    nvox = 2049 * 256 + 3
    assert nvox % B == 0 and (nvox + 255) // 256 > 2048
    z, y = R.seg_case(B, nvox // B, Cc, 60)
    tab = CountTable()
    tab.add(z, y, Cc, clast)
    tab.check(R.seg_counts_ref(z, y, Cc), Cc, f"seg_counts nvox={nvox} channels_last={clast}")
