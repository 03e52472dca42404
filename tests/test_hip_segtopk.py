"""Direct tests of the top-k cross-entropy kernels (csrc/segtopk.hip) against tests/segtopk_ref.py (float64, CPU), and of
the wrappers above them.

mivp_seg_topk / mivp_seg_topk_grad / mivp_seg_topk_ws are called through ``_lib.call`` on their own operands between guard
words.  The keys and the record are read out of the workspace (layout: include/mivp.h):
  exact select   k == max(1, floor(top_k N)); tau bit-equal to sort(keys of the valid voxels, descending)[k - 1]; N, n_gt,
                 n_eq equal to the counts over the keys: integers, no tolerance
  keys           |key - u64| <= band / 2 at every valid voxel, band = KEY_MARGIN x E_u (tests/segtopk_ref.py); with the
                 decidable condition that tests/test_segtopk_host.py checks on these very cases, the kernel's selection is
                 then the reference's, and n_gt / n_eq are compared with the reference's too
  value          2e-5 max(1, |want|) against float64
  gradient       rel-L2 < 1e-4 and per element LOSS_MARGIN x E32 x max |g64|; invalid voxels +0 in every bit
Every case prints its key and gradient ratios ([segtopk-key] / [segtopk-grad])."""
import copy
import math
import os
import sys
from functools import lru_cache

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segloss_ref as R  # noqa: E402
import segtopk_ref as T  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import losses, train

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
GUARD = 64                                                        # floats: 256 bytes, keeps the payload 16-byte aligned
PATTERN = 0x7FC0BEEF                                              # a quiet NaN with a payload no arithmetic produces
RECORD_WORDS, KEYS_OFFSET = 16, 5136                              # MIVP_SEG_TOPK_RECORD_WORDS, MIVP_SEG_TOPK_KEYS_OFFSET
INVALID_KEY = -1                                                  # 0xFFFFFFFF as an int32


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not torch.equal(bits(a), bits(b)):
        bad = torch.nonzero(bits(a) != bits(b))
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} elements differ in their bits; first at "
                             f"{tuple(int(i) for i in bad[0])}")


class Guarded:
    """One f32 tensor between two guards; ``fill``: the int32 pattern it starts with (an output to be written)."""

    def __init__(self, shape, init=None, fill=PATTERN):
        self.n = int(math.prod(shape))
        self.flat = torch.empty(self.n + 2 * GUARD, dtype=F32, device=DEV)
        self.flat.view(torch.int32).fill_(PATTERN)
        self.t = self.flat[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.t.copy_(init)
        elif fill != PATTERN:
            self.t.view(torch.int32).fill_(fill)

    def done(self, what, written=True):
        raw = self.flat.cpu().view(torch.int32)
        guards = torch.cat([raw[:GUARD], raw[GUARD + self.n:]])
        bad = torch.nonzero(guards != PATTERN)
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} guard words were overwritten, first at guard offset {int(bad[0])}"
        if written:
            left = torch.nonzero(raw[GUARD:GUARD + self.n] == PATTERN)
            assert left.numel() == 0, f"{what}: {left.shape[0]} elements were never written, first at offset {int(left[0])}"
        return self.t.cpu().clone()


def record_offset(B, vol):
    return (int(L.lib().mivp_seg_loss_ws(B, vol)) + 3) // 4 * 4


def topk_call(zd, yd, o, form="fused", gscale=None, ws_fill=PATTERN):
    """(loss, dz, record dict, keys int32 [B, vol]) on the CPU.  fused: mivp_seg_topk with dlogits; split: the value call
    without dlogits, then mivp_seg_topk_grad on the same workspace with ``gscale`` (None: a NULL pointer)."""
    B, vol, Cc = zd.shape
    n_ws = int(L.lib().mivp_seg_topk_ws(B, vol))
    off = record_offset(B, vol)
    assert n_ws == off + KEYS_OFFSET + (B * vol + 3) // 4 * 4
    ws, loss, dz = Guarded((n_ws,), fill=ws_fill), Guarded((1,)), Guarded((B, vol, Cc))
    wd = None if o["class_weights"] is None else Guarded((Cc,), torch.tensor(o["class_weights"], dtype=F32))
    wp = None if wd is None else wd.t
    gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    bg, bt, ig = int(o["include_background"]), int(o["batch"]), o["ignore_index"]
    ign, has = (0, 0) if ig is None else (ig, 1)
    al, be, gam, lr, lv, tk = o["alpha"], o["beta"], o["focal_gamma"], o["lambda_region"], o["lambda_voxel"], o["top_k"]
    if form == "fused":
        assert gscale is None
        L.call("mivp_seg_topk", L.ptr(zd), L.ptr(yd), B, vol, Cc, bg, bt, al, be, gam, L.ptr(wp), ign, has, lr, lv, tk,
               L.ptr(ws.t), L.ptr(loss.t), L.ptr(dz.t), L.stream())
    else:
        L.call("mivp_seg_topk", L.ptr(zd), L.ptr(yd), B, vol, Cc, bg, bt, al, be, gam, L.ptr(wp), ign, has, lr, lv, tk,
               L.ptr(ws.t), L.ptr(loss.t), None, L.stream())
        L.call("mivp_seg_topk_grad", L.ptr(zd), L.ptr(yd), B, vol, Cc, bg, bt, al, be, gam, L.ptr(wp), ign, has, lr, lv, tk,
               L.ptr(ws.t), L.ptr(gs), L.ptr(dz.t), L.stream())
    torch.cuda.synchronize()
    raw = ws.done("workspace", written=False).view(torch.int32)
    if wd is not None:
        wd.done("class weights")
    rec = raw[off:off + RECORD_WORDS]
    record = dict(N=int(rec[0]), k=int(rec[1]), tau_bits=int(rec[2]), tau=float(rec[2:3].view(F32)[0]), n_gt=int(rec[3]),
                  n_eq=int(rec[4]), rho=float(rec[5:6].view(F32)[0]), voxel=float(rec[6:7].view(F32)[0]))
    keys = raw[off + KEYS_OFFSET:off + KEYS_OFFSET + B * vol].view(B, vol).clone()
    return loss.done("loss value")[0], dz.done("dlogits"), record, keys


def select_failures(record, keys, z, y, o, what):
    """The exact-select checks on the keys themselves, then the keys against the reference."""
    out = []
    C = z.shape[-1]
    valid = R.valid_mask(y, C, o["ignore_index"])
    if not torch.equal(keys == INVALID_KEY, ~valid):
        out.append(f"{what}: the sentinel does not mark exactly the invalid voxels")
        return out
    kv = keys[valid]
    if bool((kv < 0).any()):
        out.append(f"{what}: a valid key has its sign bit set")
        return out
    N = int(valid.sum())
    k = max(1, math.floor(o["top_k"] * N))
    if (record["N"], record["k"]) != (N, k):
        out.append(f"{what}: record N {record['N']} k {record['k']}, want {N} {k}")
    if N == 0:
        if (record["n_gt"], record["n_eq"], record["voxel"]) != (0, 0, 0.0):
            out.append(f"{what}: an empty selection must leave n_gt = n_eq = 0 and voxel = 0: {record}")
        return out
    tau = int(torch.sort(kv, descending=True).values[k - 1])
    n_gt, n_eq = int((kv > tau).sum()), int((kv == tau).sum())
    if (record["tau_bits"], record["n_gt"], record["n_eq"]) != (tau, n_gt, n_eq):
        out.append(f"{what}: record tau {record['tau_bits']:#x} n_gt {record['n_gt']} n_eq {record['n_eq']}, the keys give "
                   f"{tau:#x} {n_gt} {n_eq}")
    want_rho = float(torch.tensor((k - n_gt) / n_eq, dtype=F64).to(F32))
    if record["rho"] != want_rho:
        out.append(f"{what}: rho {record['rho']!r}, want {want_rho!r}")
    # the keys against the reference
    e, u64, _ = T.e_u(z, y, o)
    err = float((kv.view(F32).to(F64) - u64[valid]).abs().max())
    print(f"[segtopk-key] {what}: E_u {e:.3e} kernel {err:.3e} ratio {err / e:.3f} (allowed {T.KEY_MARGIN / 2:g})")
    if not err <= T.KEY_MARGIN * e / 2:
        out.append(f"{what}: a key is {err:.3e} from u64, band / 2 = {T.KEY_MARGIN * e / 2:.3e}")
    sel = T.Select(u64, valid, o["top_k"])
    if (sel.n_gt, sel.n_eq) != (n_gt, n_eq):
        out.append(f"{what}: the reference selects n_gt {sel.n_gt} n_eq {sel.n_eq}, the keys {n_gt} {n_eq}")
    return out


def failures(got_loss, got_dz, ref, what, k=1.0):
    out = []
    want = float(ref.l64)
    if not abs(float(got_loss) - want) <= T.LOSS_VALUE_BAR * max(1.0, abs(want)):
        out.append(f"{what}: loss {float(got_loss)!r}, float64 {want!r}")
    if ref.zero:
        if not torch.equal(bits(got_dz), torch.zeros_like(bits(got_dz))):
            out.append(f"{what}: a zero gradient must be +0 in every bit, {int((bits(got_dz) != 0).sum())} elements are not")
        return out
    if k == 0.0:
        if not bool(got_dz.double().abs().max() == 0):
            out.append(f"{what}: gscale 0 must give zeros")
        return out
    g64 = k * ref.g64
    err = float((got_dz.double() - g64).abs().max()) / (abs(k) * ref.scale)
    print(f"[segtopk-grad] {what}: E32 {ref.e32:.3e} kernel {err:.3e} ratio {err / ref.e32:.3f} bar {ref.bar_norm:.3e}")
    l2 = T.rel_l2(got_dz, g64)
    if not l2 < T.LOSS_L2_BAR:
        out.append(f"{what}: gradient rel-L2 {l2:.3e}")
    try:
        T.assert_within_located(got_dz, g64, abs(k) * ref.bar_abs, "bvc", what)
    except AssertionError as e:
        out.append(str(e))
    return out


def run_case(z, y, o, what, form="fused"):
    ref = T.TopkRef(z, y, o)
    loss, dz, record, keys = topk_call(z.to(DEV), y.to(DEV), o, form, None if form == "fused" else 1.0)
    out = select_failures(record, keys, z, y, o, what) + failures(loss, dz, ref, what)
    invalid = ~R.valid_mask(y, z.shape[-1], o["ignore_index"])
    if bool(invalid.any()) and not torch.equal(bits(dz[invalid]), torch.zeros_like(bits(dz[invalid]))):
        out.append(f"{what}: an invalid voxel's gradient is not +0 in every bit")
    if ref.sel.N == 0 and o["lambda_region"] == 0.0 and float(loss) != 0.0:
        out.append(f"{what}: nothing valid and no region term: the loss must be 0, got {float(loss)!r}")
    return out


# =============================================================================================
# the kernels
# =============================================================================================
SELECT_NAMES = sorted({c[0] for c in T.select_cases()}, key=[c[0] for c in T.select_cases()].index)


@pytest.mark.parametrize("name", SELECT_NAMES, ids=[n.replace(" ", "_").replace(",", "") for n in SELECT_NAMES])
def test_exact_select(name):
    """Shapes on both paths (scalar / 16-byte loads, one and several partial rows, several workgroups flushing), every C, and
    the operands that decide the radix levels and the tie rule; every fraction of the case."""
    fails = []
    for i, (nm, z, y, o) in enumerate(c for c in T.select_cases() if c[0] == name):
        fails += run_case(z, y, o, f"{nm} {T.opts_name(o)}", "fused" if i % 2 == 0 else "split")
    assert not fails, "\n".join(fails)


def test_value_and_gradient_over_the_full_product_of_the_options():
    fails = []
    for name, z, y, o in T.product_cases():
        fails += run_case(z, y, o, name)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("vol", T.FORMS_VOLS)
def test_entry_forms(vol):
    """Fused against the value call followed by mivp_seg_topk_grad (gscale 1, NULL, 0, -2.5), a repeated call, and a
    workspace that starts as garbage (all ones in every bit, and a large count in every word): equal bits throughout, so
    the call zeroes its own histograms and record."""
    z, y, o = T.forms_case(vol)
    ref = T.TopkRef(z, y, o)
    zd, yd = z.to(DEV), y.to(DEV)
    what = f"vol {vol}"
    l_f, g_f, r_f, k_f = topk_call(zd, yd, o, "fused")
    fails = failures(l_f, g_f, ref, what + " fused") + select_failures(r_f, k_f, z, y, o, what)
    runs = {"split gscale 1": topk_call(zd, yd, o, "split", 1.0), "split NULL gscale": topk_call(zd, yd, o, "split", None),
            "second call": topk_call(zd, yd, o, "fused"), "workspace of ones": topk_call(zd, yd, o, "fused", ws_fill=-1),
            "workspace of counts": topk_call(zd, yd, o, "split", 1.0, ws_fill=0x01234567),
            "workspace of zeros": topk_call(zd, yd, o, "fused", ws_fill=0)}
    for name, (l_o, g_o, r_o, k_o) in runs.items():
        assert_same_bits(g_o, g_f, f"{what}: gradient, {name}")
        assert_same_bits(l_o.reshape(1), l_f.reshape(1), f"{what}: loss value, {name}")
        assert r_o == r_f and torch.equal(k_o, k_f), f"{what}: record or keys, {name}"
    invalid = ~R.valid_mask(y, 3, 255)
    for k in (0.0, -2.5):
        l_k, g_k, _, _ = topk_call(zd, yd, o, "split", k)
        assert_same_bits(l_k.reshape(1), l_f.reshape(1), what + f": loss value, gscale {k}")
        fails += failures(l_k, g_k, ref, what + f" gscale {k}", k)
        assert torch.equal(bits(g_k[invalid]), torch.zeros_like(bits(g_k[invalid]))), f"gscale {k}: -0 at an invalid voxel"
    assert not fails, "\n".join(fails)


# =============================================================================================
# the wrappers
# =============================================================================================
def wrapper_run(z, y, spec, dims, module=None, scale=1.0):
    B, vol, Cc = z.shape
    base = z.view(B, *dims, Cc).to(DEV).requires_grad_(True)
    yd = y.view(B, 1, *dims).to(DEV)
    got = module(base.permute(0, 4, 1, 2, 3), yd) if module is not None else losses.seg_loss(base.permute(0, 4, 1, 2, 3), yd, spec)
    (got * scale).backward()
    torch.cuda.synchronize()
    return got, base.grad.cpu().view(B, vol, Cc)


def test_top_k_none_is_the_spec_without_the_argument():
    z, y, o = R.wrapper_case((6, 7, 8))
    a_l, a_g = wrapper_run(z, y, losses.SegLossSpec(**o), (6, 7, 8))
    b_l, b_g = wrapper_run(z, y, losses.SegLossSpec(top_k=None, **o), (6, 7, 8))
    assert type(a_l.grad_fn).__name__ == type(b_l.grad_fn).__name__ and "SegLossFn" in type(b_l.grad_fn).__name__
    assert torch.equal(a_l.detach(), b_l.detach()) and torch.equal(a_g, b_g)


def test_top_k_one_without_weights_is_the_existing_loss():
    for dims in ((5, 7, 9), (6, 7, 8)):
        z, y, o = R.wrapper_case(dims)
        o = dict(o, class_weights=None)
        ref = R.SegRef(z, y, o)
        got, grad = wrapper_run(z, y, losses.SegLossSpec(top_k=1.0, **o), dims)
        assert "SegTopkFn" in type(got.grad_fn).__name__
        assert abs(float(got) - float(ref.l64)) <= R.LOSS_VALUE_BAR * max(1.0, abs(float(ref.l64)))
        assert R.rel_l2(grad, ref.g64) < R.LOSS_L2_BAR
        R.assert_within_located(grad, ref.g64, ref.bar_abs, "bvc", f"top_k 1 {dims}")


@pytest.mark.parametrize("dims", [(5, 7, 9), (6, 7, 8)], ids=["5x7x9", "6x7x8"])
def test_wrappers_and_top_k_stats(dims):
    """seg_loss / SegLoss on the channels-first view of channels-last storage (the kernels) with an incoming gradient, on a
    contiguous channels-first tensor (the torch composition), and ``top_k_stats`` against the record of both."""
    vol = math.prod(dims)
    z, y, o = T.forms_case(vol)
    ref = T.TopkRef(z, y, o)
    spec = losses.SegLossSpec(**o)
    got, grad = wrapper_run(z, y, spec, dims, scale=2.5)
    fails = failures(got.detach().cpu(), grad, ref, f"seg_loss view {dims}", 2.5)
    mod = losses.SegLoss(spec).to(DEV)
    got2, grad2 = wrapper_run(z, y, spec, dims, module=mod)
    fails += failures(got2.detach().cpu(), grad2, ref, f"SegLoss view {dims}")
    assert float(got2.detach()) == float(got.detach())
    st = mod.top_k_stats()
    _, _, record, _ = topk_call(z.to(DEV), y.to(DEV), o)
    assert st == {k: record[k] for k in ("N", "k", "tau", "n_gt", "n_eq")} and st["N"] == ref.sel.N and st["k"] == ref.sel.k
    assert (st["n_gt"], st["n_eq"]) == (ref.sel.n_gt, ref.sel.n_eq)
    B, Cc = z.shape[0], z.shape[2]
    plain = z.view(B, *dims, Cc).permute(0, 4, 1, 2, 3).contiguous().to(DEV).requires_grad_(True)
    got3 = mod(plain, y.view(B, 1, *dims).to(DEV))
    assert "SegTopkFn" not in type(got3.grad_fn).__name__                      # the composition, not the kernels
    (got3 * 0.7).backward()
    torch.cuda.synchronize()
    grad3 = plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(B, vol, Cc)
    fails += failures(got3.detach().cpu(), grad3, ref, f"SegLoss channels-first {dims}", 0.7)
    st3 = mod.top_k_stats()
    assert (st3["N"], st3["k"], st3["n_gt"], st3["n_eq"]) == (st["N"], st["k"], st["n_gt"], st["n_eq"])
    assert not fails, "\n".join(fails)


def test_recorded_value_and_backward_replay_on_new_batch_content():
    """torch.cuda.graph around value + backward; each replay on another batch content (another N, k and tau) gives the bits
    of the eager call on that content, and ``top_k_stats`` reads that replay's record."""
    o, batches = T.graph_cases()
    dims = T.GRAPH_DIMS
    B, vol, Cc = batches[0][0].shape
    mod = losses.SegLoss(losses.SegLossSpec(**o)).to(DEV)
    eager = []
    for z, y in batches:
        l, g = wrapper_run(z, y, mod.spec, dims, module=mod)
        eager.append((l.detach().clone(), g, mod.top_k_stats()))
    assert eager[0][2]["N"] != eager[1][2]["N"] and eager[0][2]["tau"] != eager[1][2]["tau"]
    base = torch.zeros((B, *dims, Cc), device=DEV, requires_grad=True)
    yd = torch.zeros((B, 1, *dims), device=DEV)
    base.data.copy_(batches[0][0].view(B, *dims, Cc))
    yd.copy_(batches[0][1].view(B, 1, *dims))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mod(base.permute(0, 4, 1, 2, 3), yd).backward()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    base.grad = None
    with torch.cuda.graph(graph):
        loss = mod(base.permute(0, 4, 1, 2, 3), yd)
        loss.backward()
    for i in (1, 0, 1):
        base.data.copy_(batches[i][0].view(B, *dims, Cc))
        yd.copy_(batches[i][1].view(B, 1, *dims))
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(loss.detach().reshape(1), eager[i][0].reshape(1), f"replay on content {i}: loss")
        assert_same_bits(base.grad.cpu().view(B, vol, Cc), eager[i][1], f"replay on content {i}: gradient")
        assert mod.top_k_stats() == eager[i][2]
        ref = T.TopkRef(*batches[i], o)
        assert not failures(loss.detach().cpu(), base.grad.cpu().view(B, vol, Cc), ref, f"replay {i}")


@lru_cache(maxsize=None)
def _step_runs():
    """Three eager steps and (two eager warm-up steps + one replay) of the smallest configuration tests/test_hip_graph.py
    uses, with ``conf.seg_loss = SegLoss(top_k=0.1, ignore_index=255)``."""
    from mivp_amd.swin_unetr import SwinUnetR
    conf, size, batch = train.make_conf("tiny")
    torch.manual_seed(5)
    start = SwinUnetR(conf).to(DEV).train()
    x, y = train.synthetic_batch(conf, batch, size, DEV)
    y_ig = y.clone()
    y_ig[:, :, : size // 4] = 255.0
    mod = losses.SegLoss(top_k=0.1, ignore_index=255).to(DEV)
    conf_seg = copy.copy(conf)
    conf_seg.seg_loss = mod
    m = copy.deepcopy(start)
    opt = train.build_optimizer(m, conf_seg)
    l_e = [float(train.train_step(m, opt, conf_seg, x, y_ig)) for _ in range(3)]
    torch.cuda.synchronize()
    stats_e = mod.top_k_stats()
    mg = copy.deepcopy(start)
    og = train.build_optimizer(mg, conf_seg, capturable=True)
    step = train.graphed_train_step(mg, og, conf_seg, x, y_ig, warmup=2)
    l_g = [float(step())]
    torch.cuda.synchronize()
    logits = copy.deepcopy(start)(x)["downstream"].detach()
    n_cls = conf.output_channels_downstream
    zc = logits.permute(0, 2, 3, 4, 1).reshape(batch, -1, n_cls).float().cpu()
    return l_e, m, l_g, mg, stats_e, mod.top_k_stats(), (zc, y_ig.reshape(batch, -1).cpu())


def test_train_step_and_graphed_step_with_a_top_k_seg_loss():
    l_e, m_e, l_g, m_g, stats_e, stats_g, (z, y) = _step_runs()
    print(f"[segtopk step] eager {l_e}, replayed {l_g}, stats {stats_g}")
    assert all(math.isfinite(v) for v in l_e) and l_g == l_e[2:]
    sd_e, sd_g = dict(m_e.state_dict()), dict(m_g.state_dict())
    assert [k for k in sd_e if not torch.equal(sd_e[k], sd_g[k])] == []
    assert stats_g == stats_e and stats_e["k"] == max(1, math.floor(0.1 * stats_e["N"]))
    assert stats_e["N"] == int(R.valid_mask(y, z.shape[-1], 255).sum())
    want, _, _ = T.topk_loss(z, y, T.opts(0.1, ignore_index=255))
    assert abs(l_e[0] - float(want)) <= T.LOSS_VALUE_BAR * max(1.0, abs(float(want))), (l_e[0], float(want))
