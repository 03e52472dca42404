"""GPU tests of the multi-label (overlapping label groups) kernels (csrc/multilabel.hip) and of the layers above them
(mivp_amd/multilabel.py), against tests/multilabel_ref.py (float64 / numpy, CPU).

Shapes: (5, 6, 7) with B = 2 -- 210 voxels, no multiple of 4: the scalar path, one workgroup per sample and a sample
boundary -- at R = 1, 3, 8; (8, 12, 12) with B = 2 -- 1152 voxels: the 16-byte path and two partial rows per sample -- at
R = 3.

Loss bars (the siblings', tests/segloss_ref.py): value 2e-5 max(1, |want|) against float64; gradient rel-L2 < 1e-4 and per
element LOSS_MARGIN x E32 x max |g64| with E32 the error of the reference's own formulas run in f32 on the same case (each
case prints E32, the kernel's error and their ratio as ``[multilabel-ratio]``); invalid voxels owe bit-exact zeros; every
output and the workspace sit between guard words.  Decode, bits and counts are bit-equal to the numpy restatement; the
probabilities stay within 8 x the error of float32 ``torch.sigmoid`` on the same values."""
import copy
import math
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multilabel_ref as R  # noqa: E402
from mivp_amd import _lib as L
from mivp_amd import multilabel as M
from mivp_amd import train

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
GUARD = 64                                                        # floats: 256 bytes, keeps the payload 16-byte aligned
PATTERN = 0x7FC0BEEF                                              # a quiet NaN with a payload no arithmetic produces
SHAPES = (((5, 6, 7), 1), ((5, 6, 7), 3), ((5, 6, 7), 8), ((8, 12, 12), 3))
N_CASES = len(R.loss_cases(3))
ids_shape = lambda s: "x".join(str(v) for v in s[0]) + f"-R{s[1]}"  # noqa: E731


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


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


def _dev_vec(v):
    return None if v is None else torch.tensor(v, dtype=F32, device=DEV)


def ml_call(zd, yd, groups, o, form="fused", gscale=None):
    """(loss, dz) on the CPU.  fused: mivp_multilabel_loss with dlogits; split: the value call without dlogits, then
    mivp_multilabel_loss_grad on the same workspace with ``gscale`` (None: a NULL pointer)."""
    B, vol, Rg = zd.shape
    member = torch.from_numpy(R.member_np(groups)).to(DEV)
    n_ws = int(L.lib().mivp_multilabel_loss_ws(B, vol))
    assert n_ws == (B * (max(1, min(256, (vol + 1023) // 1024)) + 1) + 1) * 26
    z, y = Guarded(zd.shape, zd), Guarded(yd.shape, yd)
    ws, loss, dz = Guarded((n_ws,)), Guarded((1,)), Guarded(zd.shape)
    gw, pw = _dev_vec(o["group_weights"]), _dev_vec(o["pos_weight"])
    bt, ig = int(o["batch"]), o["ignore_index"]
    ign, has = (0, 0) if ig is None else (ig, 1)
    mp, gp, pp = L.ptr(member), L.ptr(gw), L.ptr(pw)
    if form == "fused":
        assert gscale is None
        L.call("mivp_multilabel_loss", L.ptr(z.t), L.ptr(y.t), B, vol, Rg, mp, bt, o["alpha"], o["beta"], o["focal_gamma"], gp, pp,
               ign, has, o["lambda_region"], o["lambda_voxel"], L.ptr(ws.t), L.ptr(loss.t), L.ptr(dz.t), L.stream())
    else:
        gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device=DEV)
        L.call("mivp_multilabel_loss", L.ptr(z.t), L.ptr(y.t), B, vol, Rg, mp, bt, o["alpha"], o["beta"], o["focal_gamma"], gp, pp,
               ign, has, o["lambda_region"], o["lambda_voxel"], L.ptr(ws.t), L.ptr(loss.t), None, L.stream())
        L.call("mivp_multilabel_loss_grad", L.ptr(z.t), L.ptr(y.t), B, vol, Rg, mp, bt, o["alpha"], o["beta"], o["focal_gamma"],
               gp, pp, ign, has, o["lambda_region"], o["lambda_voxel"], L.ptr(ws.t), L.ptr(gs), L.ptr(dz.t), L.stream())
    torch.cuda.synchronize()
    ws.done("workspace", written=False)
    assert torch.equal(bits(z.done("logits")), bits(zd)) and torch.equal(bits(y.done("target", written=False)), bits(yd))
    return loss.done("loss")[0], dz.done("dlogits")


@lru_cache(maxsize=None)
def case(shape_i, i):
    dims, Rg = SHAPES[shape_i]
    name, kind, o = R.loss_cases(Rg)[i]
    vol = dims[0] * dims[1] * dims[2]
    groups = R.GROUPS[Rg]
    z, y = R.inputs(2, vol, groups, 1000 * shape_i + i, kind, o["ignore_index"])
    return name, groups, o, z, y, R.MlRef(z, y, groups, o)


def failures(got_loss, got_dz, ref, what, k=1.0):
    out = []
    want = float(ref.l64)
    if not abs(float(got_loss) - want) <= R.LOSS_VALUE_BAR * max(1.0, abs(want)):
        out.append(f"{what}: loss {float(got_loss)!r}, float64 reference {want!r}")
    inv = bits(got_dz)[~ref.valid]
    if not bool((inv == 0).all()):
        out.append(f"{what}: {int((inv != 0).sum())} gradient words of invalid voxels are not +0")
    assert not ref.zero
    g64 = k * ref.g64
    err = float((got_dz.double() - g64).abs().max()) / (abs(k) * ref.scale)
    print(f"[multilabel-ratio] {what}: E32 {ref.e32:.3e} kernel {err:.3e} ratio {err / ref.e32:.3f} bar {ref.bar_norm:.3e}")
    l2 = R.rel_l2(got_dz, g64)
    if not l2 < R.LOSS_L2_BAR:
        out.append(f"{what}: gradient rel-L2 {l2:.3e}")
    try:
        R.assert_within_located(got_dz, g64, abs(k) * ref.bar_abs, "bvr", what)
    except AssertionError as e:
        out.append(str(e))
    return out


# ============================================================================================= 1. the loss entries
@pytest.mark.parametrize("i", range(N_CASES))
@pytest.mark.parametrize("shape_i", range(len(SHAPES)), ids=[ids_shape(s) for s in SHAPES])
def test_loss_cases(shape_i, i):
    name, groups, o, z, y, ref = case(shape_i, i)
    loss, dz = ml_call(z, y, groups, o)
    fails = failures(loss, dz, ref, f"{ids_shape(SHAPES[shape_i])} {name}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape_i", [1, 3], ids=[ids_shape(SHAPES[1]), ids_shape(SHAPES[3])])
def test_split_form_with_an_upstream_gradient_and_equal_calls(shape_i):
    name, groups, o, z, y, ref = case(shape_i, 3)                  # gamma 2 with both weight tables
    l0, d0 = ml_call(z, y, groups, o)
    l1, d1 = ml_call(z, y, groups, o)
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(bits(d0), bits(d1))       # equal calls, equal bits
    ls, ds = ml_call(z, y, groups, o, "split", None)
    assert torch.equal(bits(ls), bits(l0)) and torch.equal(bits(ds), bits(d0))       # NULL gscale is 1
    lk, dk = ml_call(z, y, groups, o, "split", 0.37)
    fails = failures(lk, dk, ref, f"{ids_shape(SHAPES[shape_i])} {name}, upstream 0.37", float(np.float32(0.37)))
    assert not fails, "\n".join(fails)
    assert torch.equal(bits(lk), bits(l0))


def test_entries_refuse_bad_arguments():
    name, groups, o, z, y, _ = case(1, 0)
    zd, yd = z.to(DEV), y.to(DEV)
    member = torch.from_numpy(R.member_np(groups)).to(DEV)
    ws = torch.empty(int(L.lib().mivp_multilabel_loss_ws(2, 210)), dtype=F32, device=DEV)
    out = torch.empty(1, dtype=F32, device=DEV)

    def call(Rg=3, mem=member, alpha=0.5, gamma=0.0, lr=1.0, lv=1.0):
        L.call("mivp_multilabel_loss", L.ptr(zd), L.ptr(yd), 2, 210, Rg, L.ptr(mem), 0, alpha, 0.5, gamma, None, None, 0, 0,
               lr, lv, L.ptr(ws), L.ptr(out), None, L.stream())
    call()
    for kw in (dict(Rg=0), dict(Rg=9), dict(mem=None), dict(alpha=-1.0), dict(gamma=0.5), dict(lr=0.0, lv=0.0)):
        with pytest.raises(RuntimeError, match="contract violated"):
            call(**kw)
    with pytest.raises(RuntimeError, match="contract violated"):
        L.call("mivp_multilabel_decode", L.ptr(zd), 1, 210, 3, 1, L.ptr(out), L.ptr(member), None, None, None, L.stream())
    with pytest.raises(RuntimeError, match="contract violated"):                    # a float bits map
        L.call("mivp_group_counts", L.ptr(yd), 3, 0, L.ptr(yd), 3, 420, 3, L.ptr(member), 0, 0, L.ptr(ws), L.stream())
    torch.cuda.synchronize()


# ============================================================================================= 2. the public loss
@pytest.mark.parametrize("shape_i", [1, 3], ids=[ids_shape(SHAPES[1]), ids_shape(SHAPES[3])])
def test_wrappers(shape_i):
    """``multilabel_loss`` on the model's layout (a channels-first view of channels-last storage) and ``MultiLabelLoss`` on
    contiguous channels-first logits with integer labels: both take the kernels and meet the bars under an upstream 0.37."""
    dims, Rg = SHAPES[shape_i]
    name, groups, o, z, y, ref = case(shape_i, 4)                  # ignore label, bad labels, gamma 1, pos_weight
    g = M.LabelGroups(groups)
    spec = M.MultiLabelSpec(**o)
    store = z.reshape(2, *dims, Rg).to(DEV).requires_grad_(True)
    got = M.multilabel_loss(store.permute(0, 4, 1, 2, 3), y.reshape(2, 1, *dims).to(DEV), g, spec)
    assert "MultiLabelFn" in type(got.grad_fn).__name__
    (got * 0.37).backward()
    torch.cuda.synchronize()
    k = float(np.float32(0.37))
    fails = failures(got.detach().cpu(), store.grad.cpu().reshape(2, -1, Rg), ref, f"multilabel_loss {dims}", k)
    name2, _, o2, z2, y2, ref2 = case(shape_i, 3)
    mod = M.MultiLabelLoss(g, M.MultiLabelSpec(**o2)).to(DEV)
    assert mod.group_weights.is_cuda and mod.pos_weight.is_cuda
    plain = z2.reshape(2, *dims, Rg).permute(0, 4, 1, 2, 3).contiguous().to(DEV).requires_grad_(True)
    got2 = mod(plain, y2.reshape(2, *dims).to(torch.int64).to(DEV))
    (got2 * 0.37).backward()
    torch.cuda.synchronize()
    fails += failures(got2.detach().cpu(), plain.grad.cpu().permute(0, 2, 3, 4, 1).reshape(2, -1, Rg), ref2,
                      f"MultiLabelLoss {dims}", k)
    assert not fails, "\n".join(fails)


def test_recorded_value_and_gradient_replay_on_new_content():
    """Value + gradient recorded once in a ``torch.cuda.graph``; the replay on new logits and labels -- a group goes absent
    -- equals the eager call in the bits."""
    shape_i = 3
    dims, Rg = SHAPES[shape_i]
    name, groups, o, z, y, _ = case(shape_i, 3)
    _, _, _, z_new, y_new, _ = case(shape_i, 7)                    # the absent-group draw
    assert not bool((y_new == 3.0).any()) and bool((y == 3.0).any())
    mod = M.MultiLabelLoss(M.LabelGroups(groups), M.MultiLabelSpec(**o)).to(DEV)

    def eager(zc, yc):
        zz = zc.reshape(2, *dims, Rg).to(DEV).requires_grad_(True)
        loss = mod(zz.permute(0, 4, 1, 2, 3), yc.reshape(2, 1, *dims).to(DEV))
        (g,) = torch.autograd.grad(loss, zz)
        torch.cuda.synchronize()
        return loss.detach().cpu().reshape(1), g.cpu()

    want_old, want_new = eager(z, y), eager(z_new, y_new)
    zs = z.reshape(2, *dims, Rg).to(DEV).requires_grad_(True)
    ys = y.reshape(2, 1, *dims).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(mod(zs.permute(0, 4, 1, 2, 3), ys), zs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = mod(zs.permute(0, 4, 1, 2, 3), ys)
        (grad_s,) = torch.autograd.grad(loss_s, zs)
    for zc, yc, want in ((z, y, want_old), (z_new, y_new, want_new), (z, y, want_old)):
        with torch.no_grad():
            zs.copy_(zc.reshape(2, *dims, Rg))
            ys.copy_(yc.reshape(2, 1, *dims))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(loss_s.detach().reshape(1)), bits(want[0]))
        assert torch.equal(bits(grad_s), bits(want[1]))


# ============================================================================================= 3. decode
def _decode_case(dims, seed):
    """logits [2, 3, dims] f32 on the CPU; some equal the logit of 0.3, 0 or the logit of 0.7 exactly."""
    g = R.gen(seed)
    z = 2.0 * torch.randn((2, 3) + dims, generator=g, dtype=F32)
    tau = torch.from_numpy(R.logit_thresholds_np((0.3, 0.5, 0.7), 3))
    pick = torch.randint(0, 3, z.shape, generator=g)
    hit = torch.rand(z.shape, generator=g) < 0.15
    return torch.where(hit, tau[pick], z)


@pytest.mark.parametrize("layout", ["planes", "channels_last"])
@pytest.mark.parametrize("qs", [0.5, (0.3, 0.5, 0.7)], ids=["q0.5", "q-per-group"])
@pytest.mark.parametrize("dims", [(5, 6, 7), (8, 12, 12)], ids=["5x6x7", "8x12x12"])
def test_decode(dims, qs, layout):
    z = _decode_case(dims, 31 + dims[0])
    groups = M.LabelGroups(R.BRATS)
    zd = z.to(DEV)
    if layout == "channels_last":
        zd = zd.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    out = M.decode_groups(zd, groups, qs, return_bits=True, return_probs=True)
    only = M.decode_groups(zd, groups, qs)
    torch.cuda.synchronize()
    assert set(only) == {"labels"} and torch.equal(only["labels"], out["labels"])
    assert out["labels"].shape == (2, 1) + dims and out["bits"].dtype == torch.uint8 and out["probs"].shape == (2, 3) + dims
    tau = R.logit_thresholds_np(qs, 3)
    n_equal = 0
    for b in range(2):
        want_l, want_b = R.decode_np(z[b].numpy(), R.BRATS, (1, 2, 3), qs)
        assert np.array_equal(out["labels"][b, 0].cpu().numpy(), want_l)
        assert np.array_equal(out["bits"][b, 0].cpu().numpy(), want_b)
        for r in range(3):
            eq = z[b, r].numpy() == tau[r]
            n_equal += int(eq.sum())
            assert not (want_b[eq] >> r & 1).any()                 # a logit equal to its threshold gives bit 0
    assert n_equal > 10
    p64 = torch.sigmoid(z.double())
    e_torch = float((torch.sigmoid(zd.contiguous()).cpu().double() - p64).abs().max())
    e_kernel = float((out["probs"].cpu().double() - p64).abs().max())
    print(f"[multilabel-probs] {dims} {layout}: torch f32 sigmoid {e_torch:.3e}, kernel {e_kernel:.3e}")
    assert e_torch > 0 and e_kernel <= 8 * e_torch


# ============================================================================================= 4. counts
def _count_case(dims, seed):
    g = R.gen(seed)
    vals = torch.tensor([0, 1, 2, 3, 4, 200], dtype=torch.uint8)
    pred = vals[torch.randint(0, len(vals), (2,) + dims, generator=g)]
    tgt = vals[torch.randint(0, len(vals), (2,) + dims, generator=g)]
    tgt[torch.rand(tgt.shape, generator=g) < 0.2] = 255
    bitsmap = torch.randint(0, 8, (2,) + dims, generator=g).to(torch.uint8)
    return pred, tgt, bitsmap


@pytest.mark.parametrize("ignore", [None, 255, 2])
@pytest.mark.parametrize("dims", [(5, 6, 7), (8, 12, 12)], ids=["5x6x7", "8x12x12"])
def test_group_counts(dims, ignore):
    pred, tgt, bitsmap = _count_case(dims, 5 + dims[1])
    groups = M.LabelGroups(R.BRATS)
    want_l = R.counts_np(pred.numpy(), tgt.numpy(), R.BRATS, ignore)
    want_b = R.counts_np(bitsmap.numpy(), tgt.numpy(), R.BRATS, ignore, pred_bits=True)
    assert want_l[:, 0].min() > 0 and (want_l != want_b).any()
    tgt_f = tgt.float()
    tgt_f[0, 0, 0, :3] = torch.tensor([0.5, float("nan"), 1e9])    # no labels: invalid in either dtype's reading
    want_lf = R.counts_np(pred.numpy(), tgt_f.numpy(), R.BRATS, ignore)
    for p, t, kw, want in ((pred, tgt, {}, want_l), (pred.float(), tgt, {}, want_l), (pred, tgt_f, {}, want_lf),
                           (pred.float(), tgt_f, {}, want_lf), (pred.to(torch.int64), tgt.to(torch.int32), {}, want_l),
                           (bitsmap, tgt, {"pred_bits": True}, want_b),
                           (bitsmap, tgt_f, {"pred_bits": True}, R.counts_np(bitsmap.numpy(), tgt_f.numpy(), R.BRATS, ignore, True))):
        got = M.group_counts(p.to(DEV), t.to(DEV), groups, ignore, **kw)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (p.dtype, t.dtype, kw)
    pooled = M.group_counts(pred.to(DEV), tgt.to(DEV), groups, ignore)
    again = M.group_counts(bitsmap.to(DEV), tgt.to(DEV), groups, ignore, out=pooled, pred_bits=True)
    assert again is pooled and np.array_equal(pooled.cpu().numpy(), want_l + want_b)
    s = M.group_scores(pooled)
    c = (want_l + want_b).astype(np.float64)
    assert np.array_equal(s["dice"], 2 * c[:, 0] / (c[:, 1] + c[:, 2]))
    with pytest.raises(ValueError):
        M.group_counts(bitsmap.float().to(DEV), tgt.to(DEV), groups, pred_bits=True)
    with pytest.raises(ValueError):
        M.group_counts(pred.to(DEV), tgt.to(DEV), groups, out=torch.zeros((3, 3), dtype=torch.int32, device=DEV))


# ============================================================================================= 5. the predictor
class StandIn(torch.nn.Module):
    """A deterministic per-window model with three output channels: element-wise functions of the first input channel,
    returned like the HIP model's output -- a channels-first view of channels-last fp32 storage."""

    K = ((1.7, 0.3), (-2.3, 0.9), (3.1, -1.4))

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1), requires_grad=False)

    def forward(self, x):
        x0 = x[:, 0]
        ch = [torch.tanh(x0 * k + b) + 0.25 * torch.sin(x0 * (3.0 + c)) for c, (k, b) in enumerate(self.K)]
        return {"downstream": torch.stack(ch, dim=-1).permute(0, 4, 1, 2, 3)}


def test_predictor_groups():
    from mivp_amd.inference import SlidingWindowPredictor, evaluate_volume_groups
    image = roi = (16, 16, 16)
    torch.manual_seed(4)
    x = torch.rand((1, 1) + image, device=DEV) * 6 - 3             # wide enough for every channel to cross its threshold
    seg = torch.randint(0, 4, (1, 1) + image, device=DEV).float()
    seg[0, 0, :2] = 255.0
    groups = M.LabelGroups(R.BRATS)
    model = StandIn().to(DEV)
    p = SlidingWindowPredictor(model, image, 1, 3, roi, overlap=0.5, sub_batch=2)
    qs = (0.3, 0.5, 0.7)
    logits = p.predict(x, return_logits=True)["logits"].clone()
    want = M.decode_groups(logits, groups, qs, return_bits=True, return_probs=True)
    got = p.predict_groups(x, groups, qs, return_bits=True, return_probs=True)
    torch.cuda.synchronize()
    assert set(got) == {"labels", "bits", "probs"}
    for k in got:
        assert torch.equal(got[k], want[k]), k
    assert len(torch.unique(got["labels"])) > 2
    counts = p.evaluate_groups(x, seg, groups, qs, ignore_index=255)
    want_c = M.group_counts(want["bits"], seg, groups, 255, pred_bits=True)
    assert torch.equal(counts, want_c) and int(counts[:, 0].min()) > 0
    assert np.array_equal(counts.cpu().numpy(), R.counts_np(want["bits"].cpu().numpy(), seg.cpu().numpy(), R.BRATS, 255, True))
    pooled = p.evaluate_groups(x, seg, groups, qs, ignore_index=255, out=counts.clone())
    assert torch.equal(pooled, 2 * want_c)
    one = evaluate_volume_groups(model, x, seg, roi, groups, qs, 255, sub_batch=2)
    assert torch.equal(one, want_c)
    # an ordinary label map scored by groups
    lab = p.predict(x)["labels"]
    assert np.array_equal(M.group_counts(lab, seg, groups).cpu().numpy(),
                          R.counts_np(lab.cpu().numpy(), seg.cpu().numpy(), R.BRATS))
    two = M.LabelGroups([(1,), (2,)])
    for call in (lambda: p.predict_groups(x, two), lambda: p.evaluate_groups(x, seg, two)):
        with pytest.raises(ValueError, match="num_classes=3.*2 groups"):
            call()
    with pytest.raises(ValueError):
        p.predict_groups(x, groups, 1.5)


# ============================================================================================= 6. training
def test_train_step_with_a_multilabel_loss():
    """One ``train_step`` of the smallest downstream configuration the step tests use (``tiny``) with three output channels
    and ``conf.seg_loss = MultiLabelLoss(BraTS groups)``: a finite loss, the float64 reference's on the model's own logits,
    and a finite gradient in every trainable parameter."""
    from mivp_amd.swin_unetr import SwinUnetR
    conf, size, batch = train.make_conf("tiny")
    conf.output_channels_downstream = 3
    torch.manual_seed(5)
    model = SwinUnetR(conf).to(DEV).train()
    x, _ = train.synthetic_batch(conf, batch, size, DEV)
    y = torch.randint(0, 4, (batch, 1, size, size, size), generator=R.gen(9)).float().to(DEV)
    y[:, :, : size // 4] = 255.0
    conf.seg_loss = M.MultiLabelLoss(M.LabelGroups(R.BRATS), alpha=0.3, beta=0.7, focal_gamma=2.0, ignore_index=255).to(DEV)
    logits = copy.deepcopy(model)(x)["downstream"].detach()
    assert logits.shape[1] == 3
    opt = train.build_optimizer(model, conf)
    loss = float(train.train_step(model, opt, conf, x, y))
    torch.cuda.synchronize()
    zc = logits.permute(0, 2, 3, 4, 1).reshape(batch, -1, 3).float().cpu()
    want, _ = R.multilabel_ref64(zc, y.reshape(batch, -1).cpu(), R.BRATS, R.opts(0.3, 0.7, False, 2.0, None, None, 255))
    assert math.isfinite(loss) and abs(loss - float(want)) <= R.LOSS_VALUE_BAR * max(1.0, abs(float(want))), (loss, float(want))
    missing = [k for k, q in model.named_parameters() if q.requires_grad and (q.grad is None or not bool(torch.isfinite(q.grad).all()))]
    assert missing == []
    assert any(float(q.grad.abs().max()) > 0 for q in model.parameters() if q.requires_grad)
