"""Direct parity tests of the Tversky + weighted cross-entropy loss kernels (csrc/segloss.hip) against
tests/segloss_ref.py (float64, CPU), and of the wrappers above them.

mivp_seg_loss / mivp_seg_loss_grad / mivp_seg_loss_ws are called through ``_lib.call`` on their own operands: every output
and the workspace of exactly ``mivp_seg_loss_ws`` floats sit between guard words that must come back untouched, and the
outputs start as the guard pattern (a NaN), so an element that was never written is seen as well.

Bars (tests/test_segloss_host.py shows on the CPU that f32 torch meets them on these very cases and that plausible kernel
bugs do not):
  value      2e-5 max(1, |want|) against float64
  gradient   rel-L2 < 1e-4, and per element LOSS_MARGIN x E32 x max |g64| with E32 the error of the reference's own formulas
             run in f32 on the same case (each case prints E32, the kernel's error and their ratio)
  a case whose reference gradient is zero everywhere (everything ignored, or only zero-weight classes under the voxel term
  alone) owes bit-exact zeros and a finite value."""
import copy
import math
import os
import sys
from functools import lru_cache

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segloss_ref as R  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import losses, train

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
GUARD = 64                                                        # floats: 256 bytes, keeps the payload 16-byte aligned
PATTERN = 0x7FC0BEEF                                              # a quiet NaN with a payload no arithmetic produces
K_SEG = 3 * 8 + 2                                                 # floats per row of the workspace
ids_dims = lambda d: "x".join(str(v) for v in d)  # noqa: E731


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not torch.equal(bits(a), bits(b)):
        bad = torch.nonzero(bits(a) != bits(b))
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} elements differ in their bits; first at {first}: "
                             f"{float(a.cpu()[first])!r} != {float(b.cpu()[first])!r}")


class Guarded:
    """One f32 tensor between two guards, all filled with PATTERN; ``init`` None leaves it so (an output to be written)."""

    def __init__(self, shape, init=None):
        self.n = int(math.prod(shape))
        self.flat = torch.empty(self.n + 2 * GUARD, dtype=F32, device=DEV)
        self.flat.view(torch.int32).fill_(PATTERN)
        self.t = self.flat[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def done(self, what, written=True):
        raw = self.flat.cpu().view(torch.int32)
        guards = torch.cat([raw[:GUARD], raw[GUARD + self.n:]])
        bad = torch.nonzero(guards != PATTERN)
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} guard words were overwritten, first at guard offset {int(bad[0])}"
        if written:
            left = torch.nonzero(raw[GUARD:GUARD + self.n] == PATTERN)
            assert left.numel() == 0, f"{what}: {left.shape[0]} elements were never written, first at offset {int(left[0])}"
        return self.t.cpu().clone()


def bpb_of(vol):
    return max(1, min(256, (vol + 1023) // 1024))


def seg_call(zd, yd, o, form="fused", gscale=None):
    """(loss, dz) on the CPU.  fused: mivp_seg_loss with dlogits; split: the value call without dlogits, then
    mivp_seg_loss_grad on the same workspace with ``gscale`` (None: a NULL pointer)."""
    B, vol, Cc = zd.shape
    n_ws = int(L.lib().mivp_seg_loss_ws(B, vol))
    assert n_ws == (B * (bpb_of(vol) + 1) + 1) * K_SEG
    ws, loss, dz = Guarded((n_ws,)), Guarded((1,)), Guarded((B, vol, Cc))
    wd = None if o["class_weights"] is None else Guarded((Cc,), torch.tensor(o["class_weights"], dtype=F32))
    wp = None if wd is None else wd.t
    gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
    bg, bt, ig = int(o["include_background"]), int(o["batch"]), o["ignore_index"]
    ign, has = (0, 0) if ig is None else (ig, 1)
    if form == "fused":
        assert gscale is None
        L.call("mivp_seg_loss", L.ptr(zd), L.ptr(yd), B, vol, Cc, bg, bt, o["alpha"], o["beta"], o["focal_gamma"], L.ptr(wp), ign,
               has, o["lambda_region"], o["lambda_voxel"], L.ptr(ws.t), L.ptr(loss.t), L.ptr(dz.t), L.stream())
    else:
        L.call("mivp_seg_loss", L.ptr(zd), L.ptr(yd), B, vol, Cc, bg, bt, o["alpha"], o["beta"], o["focal_gamma"], L.ptr(wp), ign,
               has, o["lambda_region"], o["lambda_voxel"], L.ptr(ws.t), L.ptr(loss.t), None, L.stream())
        L.call("mivp_seg_loss_grad", L.ptr(zd), L.ptr(yd), B, vol, Cc, bg, bt, o["alpha"], o["beta"], o["focal_gamma"], L.ptr(wp),
               ign, has, o["lambda_region"], o["lambda_voxel"], L.ptr(ws.t), L.ptr(gs), L.ptr(dz.t), L.stream())
    torch.cuda.synchronize()
    ws.done("workspace", written=False)
    if wd is not None:
        wd.done("class weights")
    return loss.done("loss value")[0], dz.done("dlogits")


def failures(got_loss, got_dz, ref, what, k=1.0):
    """Print the case's figures, then return the list of bars it misses (k: the incoming gradient)."""
    out = []
    want = float(ref.l64)
    if not abs(float(got_loss) - want) <= R.LOSS_VALUE_BAR * max(1.0, abs(want)):
        out.append(f"{what}: loss {float(got_loss)!r}, float64 {want!r}")
    if ref.zero:
        if not torch.equal(bits(got_dz), torch.zeros_like(bits(got_dz))):
            out.append(f"{what}: a zero gradient must be +0 in every bit, {int((bits(got_dz) != 0).sum())} elements are not")
        if not (math.isfinite(float(got_loss)) and (want != 0.0 or float(got_loss) == 0.0)):
            out.append(f"{what}: loss {float(got_loss)!r} where every term is exactly zero")
        return out
    if k == 0.0:
        if not bool(got_dz.double().abs().max() == 0):
            out.append(f"{what}: gscale 0 must give zeros")
        return out
    g64 = k * ref.g64
    err = float((got_dz.double() - g64).abs().max()) / (abs(k) * ref.scale)
    print(f"[segloss-ratio] {what}: E32 {ref.e32:.3e} kernel {err:.3e} ratio {err / ref.e32:.3f} bar {ref.bar_norm:.3e}")
    l2 = R.rel_l2(got_dz, g64)
    if not l2 < R.LOSS_L2_BAR:
        out.append(f"{what}: gradient rel-L2 {l2:.3e}")
    try:
        R.assert_within_located(got_dz, g64, abs(k) * ref.bar_abs, "bvc", what)
    except AssertionError as e:
        out.append(str(e))
    return out


def run_case(z, y, o, what, form="fused"):
    ref = R.SegRef(z, y, o)
    loss, dz = seg_call(z.to(DEV), y.to(DEV), o, form, None if form == "fused" else 1.0)
    invalid = ~R.valid_mask(y, z.shape[-1], o["ignore_index"])
    out = failures(loss, dz, ref, what)
    if bool(invalid.any()) and not torch.equal(bits(dz[invalid]), torch.zeros_like(bits(dz[invalid]))):
        out.append(f"{what}: an invalid voxel's gradient is not +0 in every bit")
    return out


# =============================================================================================
# the kernels
# =============================================================================================
@pytest.mark.parametrize("C", R.CLASSES)
@pytest.mark.parametrize("dims", R.SCALAR_VOLS + R.VEC_VOLS, ids=ids_dims)
def test_every_instantiation(dims, C):
    """Scalar (vol % 4 != 0) and vectorised kernels for every C in 2..8 under six option sets that hold every option value.
    B = 3 puts the sample boundaries of the scalar gradient pass at odd offsets; vol = 4 with B = 5: every quad a sample."""
    vol = dims[0] * dims[1] * dims[2]
    assert (vol % 4 != 0) == (dims in R.SCALAR_VOLS) and bpb_of(vol) <= 2
    fails = []
    for o in R.ladder_options(C):
        z, y = R.ladder_case(dims, C, o)
        fails += run_case(z, y, o, f"vol {vol} B {z.shape[0]} C {C} {R.opts_name(o)}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("ignore", R.IGNORES)
@pytest.mark.parametrize("dims", R.PRODUCT_DIMS, ids=ids_dims)
@pytest.mark.parametrize("C", R.PRODUCT_CLASSES)
def test_full_product_of_the_options(C, dims, ignore):
    z, y = R.ladder_case(dims, C, R.opts(ignore_index=ignore))
    fails = []
    for o in R.product_options(C, ignore):
        fails += run_case(z, y, o, f"{ids_dims(dims)} C {C} {R.opts_name(o)}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("C", R.PRODUCT_CLASSES)
@pytest.mark.parametrize("vol,bpb", R.PARTIAL_ROW_VOLS)
def test_partial_rows(vol, bpb, C):
    assert bpb_of(vol) == bpb
    fails = []
    for o in (R.opts(), R.big_options(C)):
        z, y = R.seg_inputs(2, vol, C, vol + C, "plain" if o["ignore_index"] is None else "ignored", o["ignore_index"])
        fails += run_case(z, y, o, f"vol {vol} ({bpb} partial rows) C {C} {R.opts_name(o)}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("which", ["cap", "grid"])
def test_large_cases(which):
    """270 336 voxels: the 256-row cap makes the statistics loop stride.  (101, 101, 103) at B = 2: the scalar gradient pass
    needs 8209 workgroups and has 8192."""
    vol = R.CAP_VOL if which == "cap" else math.prod(R.GRID_CAP_DIMS)
    if which == "cap":
        assert (vol + 1023) // 1024 > 256 and vol % 4 == 0
    else:
        assert (2 * vol + 255) // 256 > 8192 and vol % 4 != 0
    o = R.big_options()
    z, y = R.seg_inputs(2, vol, 2, vol + 2, "ignored", o["ignore_index"])
    fails = run_case(z, y, o, f"{which} vol {vol}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("vol", R.SPECIAL_VOLS)
@pytest.mark.parametrize("i", range(len(R.special_cases())), ids=[c[0].replace(" ", "_").replace(",", "") for c in R.special_cases()])
def test_special_operands(i, vol):
    name, C, kind, o = R.special_cases()[i]
    z, y = R.special_inputs(i, vol)
    fails = run_case(z, y, o, f"{name} vol {vol} {R.opts_name(o)}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("vol", R.FORMS_VOLS)
def test_entry_forms(vol):
    """mivp_seg_loss with dlogits against the value call followed by mivp_seg_loss_grad (gscale 1, NULL, 0, -2.5), and a
    repeated call: fixed-order reductions, equal bits."""
    z, y, o = R.forms_case(vol)
    ref = R.SegRef(z, y, o)
    zd, yd = z.to(DEV), y.to(DEV)
    what = f"vol {vol}"
    l_f, g_f = seg_call(zd, yd, o, "fused")
    l_s, g_s = seg_call(zd, yd, o, "split", 1.0)
    l_n, g_n = seg_call(zd, yd, o, "split", None)
    l_2, g_2 = seg_call(zd, yd, o, "fused")
    fails = failures(l_f, g_f, ref, what + " fused")
    assert_same_bits(g_s, g_f, what + ": gradient, split with gscale 1 against fused")
    assert_same_bits(g_n, g_f, what + ": gradient, split with a NULL gscale against fused")
    assert_same_bits(g_2, g_f, what + ": gradient of a second identical call")
    for other in (l_s, l_n, l_2):
        assert_same_bits(other.reshape(1), l_f.reshape(1), what + ": loss value")
    for k in (0.0, -2.5):
        l_k, g_k = seg_call(zd, yd, o, "split", k)
        assert_same_bits(l_k.reshape(1), l_f.reshape(1), what + f": loss value, gscale {k}")
        fails += failures(l_k, g_k, ref, what + f" gscale {k}", k)
        invalid = ~R.valid_mask(y, 3, 255)
        assert torch.equal(bits(g_k[invalid]), torch.zeros_like(bits(g_k[invalid]))), f"gscale {k}: -0 at an invalid voxel"
    assert not fails, "\n".join(fails)


# =============================================================================================
# the wrappers
# =============================================================================================
@pytest.mark.parametrize("dims", R.WRAPPER_DIMS, ids=ids_dims)
def test_wrappers(dims):
    """losses.seg_loss / SegLoss on the channels-first VIEW of channels-last storage (the kernels) and on a contiguous
    channels-first tensor (the plain-torch composition), with an incoming gradient."""
    z, y, o = R.wrapper_case(dims)
    B, vol, Cc = z.shape
    ref = R.SegRef(z, y, o)
    spec = losses.SegLossSpec(**o)
    yd = y.view(B, 1, *dims).to(DEV)
    fails = []
    base = z.view(B, *dims, Cc).to(DEV).requires_grad_(True)
    got = losses.seg_loss(base.permute(0, 4, 1, 2, 3), yd, spec)
    (got * 2.5).backward()
    torch.cuda.synchronize()
    fails += failures(got.detach().cpu(), base.grad.cpu().view(B, vol, Cc), ref, f"seg_loss view {dims}", 2.5)
    mod = losses.SegLoss(spec).to(DEV)
    assert mod.class_weights.is_cuda
    base2 = z.view(B, *dims, Cc).to(DEV).requires_grad_(True)
    got2 = mod(base2.permute(0, 4, 1, 2, 3), yd.view(B, *dims).long())        # an integer [B, H, W, D] target
    got2.backward()
    torch.cuda.synchronize()
    fails += failures(got2.detach().cpu(), base2.grad.cpu().view(B, vol, Cc), ref, f"SegLoss view {dims}")
    assert float(got2.detach()) == float(got.detach())
    plain = z.view(B, *dims, Cc).permute(0, 4, 1, 2, 3).contiguous().to(DEV).requires_grad_(True)
    got3 = mod(plain, yd)
    assert got3.grad_fn is not None and "SegLossFn" not in type(got3.grad_fn).__name__            # the composition, not the kernels
    (got3 * 0.7).backward()
    torch.cuda.synchronize()
    grad3 = plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(B, vol, Cc)
    fails += failures(got3.detach().cpu(), grad3, ref, f"SegLoss channels-first {dims}", 0.7)
    assert not fails, "\n".join(fails)


@lru_cache(maxsize=None)
def _step_runs(workload):
    """Three eager steps and (two eager warm-up steps + one replay) of the smallest configuration tests/test_hip_graph.py
    uses, with ``conf.seg_loss`` set; and three eager steps of the same model without the attribute, twice: once on a
    configuration that never had it, once on one where it was set and removed."""
    from mivp_amd.swin_unetr import SwinUnetR
    conf, size, batch = train.make_conf("tiny" if workload == "tiny" else "sup_all")
    if workload != "tiny":
        size, batch = 32, 2
    torch.manual_seed(5)
    start = SwinUnetR(conf).to(DEV).train()
    x, y = train.synthetic_batch(conf, batch, size, DEV)
    n_cls = conf.output_channels_downstream if workload == "tiny" else conf.output_channels_pretrain
    y_ig = y.clone()
    y_ig[:, :, : size // 4] = 255.0                               # a slab outside the scan
    mod = losses.SegLoss(alpha=0.3, beta=0.7, focal_gamma=2.0, class_weights=R.WEIGHTS8[:n_cls], ignore_index=255).to(DEV)
    out = {}

    def eager(cf, target, steps=3):
        m = copy.deepcopy(start)
        opt = train.build_optimizer(m, cf)
        ls = [float(train.train_step(m, opt, cf, x, target)) for _ in range(steps)]
        torch.cuda.synchronize()
        return ls, m, opt

    conf_seg = copy.copy(conf)
    conf_seg.seg_loss = mod
    out["eager"] = eager(conf_seg, y_ig)
    m = copy.deepcopy(start)
    opt = train.build_optimizer(m, conf_seg, capturable=True)
    step = train.graphed_train_step(m, opt, conf_seg, x, y_ig, warmup=2)
    ls = [float(step())]
    torch.cuda.synchronize()
    out["graph"] = (ls, m, opt)
    out["plain"] = eager(conf, y)
    conf_back = copy.copy(conf_seg)
    del conf_back.seg_loss
    out["plain_again"] = eager(conf_back, y)
    # the first loss of the eager run, again from the model's output through the float64 reference
    key = "downstream" if workload == "tiny" else "seg_pred"
    logits = copy.deepcopy(start)(x)[key].detach()
    zc = logits.permute(0, 2, 3, 4, 1).reshape(batch, -1, n_cls).float().cpu()
    out["first"] = (zc, y_ig.reshape(batch, -1).cpu(), R.opts(0.3, 0.7, False, True, 2.0, R.WEIGHTS8[:n_cls], 255))
    return out


@pytest.mark.parametrize("workload", ["tiny", "sup_all_small"])
def test_train_step_and_graphed_step_with_a_seg_loss(workload):
    """Graph against eager the way tests/test_hip_graph.py compares the default loss: equal loss values and equal bits in
    every parameter, buffer and optimizer state after three steps; and the first loss is the reference's on the model's
    own logits."""
    runs = _step_runs(workload)
    (l_e, m_e, o_e), (l_g, m_g, o_g) = runs["eager"], runs["graph"]
    print(f"[segloss step {workload}] eager {l_e}, replayed {l_g}")
    assert l_g == l_e[2:]
    sd_e, sd_g = dict(m_e.state_dict()), dict(m_g.state_dict())
    assert [k for k in sd_e if not torch.equal(sd_e[k], sd_g[k])] == []
    sa, sb = o_e.state_dict()["state"], o_g.state_dict()["state"]
    assert all(torch.equal(sa[k]["exp_avg"], sb[k]["exp_avg"]) and torch.equal(sa[k]["exp_avg_sq"], sb[k]["exp_avg_sq"])
               and float(sa[k]["step"]) == float(sb[k]["step"]) == 3 for k in sa)
    z, y, o = runs["first"]
    want, _ = R.seg_loss_ref64(z, y, o)
    assert abs(l_e[0] - float(want)) <= R.LOSS_VALUE_BAR * max(1.0, abs(float(want))), (l_e[0], float(want))
    assert l_e[0] != runs["plain"][0][0]                          # the objective did change


@pytest.mark.parametrize("workload", ["tiny", "sup_all_small"])
def test_without_the_attribute_the_step_is_the_default_path(workload):
    """The same calls on identical inputs, on a configuration that never had ``seg_loss`` and on one it was removed from:
    equal loss values and equal parameter bits; and the default objective itself, called directly on the model's output."""
    runs = _step_runs(workload)
    (l_a, m_a, _), (l_b, m_b, _) = runs["plain"], runs["plain_again"]
    assert l_a == l_b
    sd_a, sd_b = dict(m_a.state_dict()), dict(m_b.state_dict())
    assert [k for k in sd_a if not torch.equal(sd_a[k], sd_b[k])] == []
    from mivp_amd.swin_unetr import SwinUnetR
    conf, size, batch = train.make_conf("tiny" if workload == "tiny" else "sup_all")
    if workload != "tiny":
        size, batch = 32, 2
    torch.manual_seed(5)
    model = SwinUnetR(conf).to(DEV).train()
    x, y = train.synthetic_batch(conf, batch, size, DEV)
    out = model(x)
    want = train.dice_focal_loss(out["downstream"], y, conf.include_background, 4.0) if workload == "tiny" \
        else losses.dice_loss(out["seg_pred"], y, conf.include_background)
    got = train.step_loss(out, conf, y)
    assert_same_bits(got.detach().reshape(1), want.detach().reshape(1), "step_loss without seg_loss")
    assert float(got) == l_a[0]
