"""GPU tests of whole-volume sliding-window prediction (mivp_amd.inference.SlidingWindowPredictor, csrc/stitch.hip):
the window gather against torch slicing, the blend + finalize against a float64 restatement of the weighted average,
sub-batch invariance, the no-overlap identity, the HIP model against the oracle, the Dice / IoU counts, graph replay
against eager runs and the argument checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


class StandIn(torch.nn.Module):
    """A deterministic per-window model: element-wise functions of the first input channel (no reduction, so a window's
    logits do not depend on the batch it runs in), returned like the HIP model's output -- a channels-first view of
    channels-last fp32 storage."""

    K = ((1.7, 0.3), (-2.3, 0.9), (3.1, -1.4), (0.6, 0.1))

    def __init__(self, ncls=3, contiguous_out=False):
        super().__init__()
        self.ncls, self.contiguous_out = ncls, contiguous_out
        self.anchor = torch.nn.Parameter(torch.zeros(1), requires_grad=False)

    def forward(self, x):
        x0 = x[:, 0]
        ch = [torch.tanh(x0 * k + b) + 0.25 * torch.sin(x0 * (3.0 + c)) for c, (k, b) in enumerate(self.K[:self.ncls])]
        out = torch.stack(ch, dim=-1).permute(0, 4, 1, 2, 3)
        return {"downstream": out.contiguous() if self.contiguous_out else out}


def _padded_windows(x, roi, overlap):
    """All windows of x [1, Cin, H, W, D] by torch slicing of the zero-padded volume, [N, Cin, roi], and the origins."""
    from mivp_amd.inference import window_origins, window_padding
    pad, pdims = window_padding(x.shape[2:], roi)
    xp = torch.zeros((1, x.shape[1]) + tuple(pdims), dtype=x.dtype, device=x.device)
    n = x.shape[2:]
    xp[:, :, pad[0]:pad[0] + n[0], pad[1]:pad[1] + n[1], pad[2]:pad[2] + n[2]] = x
    o = window_origins(n, roi, overlap)
    w = torch.stack([xp[0, :, a:a + roi[0], b:b + roi[1], c:c + roi[2]] for a, b, c in o.tolist()])
    return w, o, pad, pdims


def _stitch64(win_logits, x_shape, roi, overlap, mode, sigma_scale=0.125):
    """float64 weighted average of per-window logits [N, C, roi] -> [C, H, W, D]."""
    from mivp_amd.inference import importance_tables, window_origins, window_padding
    n = tuple(x_shape[2:])
    pad, pdims = window_padding(n, roi)
    o = window_origins(n, roi, overlap)
    tabs, floor = importance_tables(roi, mode, sigma_scale)
    wmap = torch.from_numpy(np.maximum(tabs[0][:, None, None] * tabs[1][None, :, None] * tabs[2][None, None, :], floor))
    lg = win_logits.detach().double().cpu()
    acc = torch.zeros((lg.shape[1],) + tuple(pdims), dtype=torch.float64)
    ws = torch.zeros(tuple(pdims), dtype=torch.float64)
    for i, (a, b, c) in enumerate(o.tolist()):
        acc[:, a:a + roi[0], b:b + roi[1], c:c + roi[2]] += wmap * lg[i]
        ws[a:a + roi[0], b:b + roi[1], c:c + roi[2]] += wmap
    res = acc / ws
    return res[:, pad[0]:pad[0] + n[0], pad[1]:pad[1] + n[1], pad[2]:pad[2] + n[2]]


def _rel(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


def _labels_where_decided(labels, ref, margin=1e-5):
    top2 = ref.topk(2, dim=0).values
    decided = (top2[0] - top2[1]) > margin
    want = ref.argmax(0)
    got = labels.reshape(want.shape).long().cpu()
    return bool((got[decided] == want[decided]).all()), float(decided.double().mean())


def _counts_cpu(labels, seg, ncls):
    p, t = labels.reshape(-1).long().cpu(), seg.reshape(-1).long().cpu()
    return torch.tensor([[int(((p == c) & (t == c)).sum()), int((p == c).sum()), int((t == c).sum())] for c in range(ncls)],
                        dtype=torch.int64)


def _miou_dice(counts):
    c = counts.double()
    inter, psum, tsum = c[:, 0], c[:, 1], c[:, 2]
    return float((inter / (psum + tsum - inter + 1e-6)).mean()), float((2 * inter / (psum + tsum + 1e-6)).mean())


# -------------------------------------------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("cin,image,roi,sub_batch", [
    (1, (10, 13, 7), (16, 8, 12), 4),      # H and D shorter than the roi (both faces), scalar rows (D % 4 != 0)
    (4, (9, 6, 8), (12, 8, 12), 3),        # every axis padded; 16-byte path with misaligned rows (pad 2 along D)
    (4, (20, 12, 16), (16, 8, 8), 5),      # no padding, aligned 16-byte rows
    (1, (21, 11, 9), (8, 8, 4), 7),
])
def test_gather_equals_torch_slicing_bitwise(cin, image, roi, sub_batch):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    torch.manual_seed(0)
    x = torch.randn((1, cin) + image, device=DEV)
    p = SlidingWindowPredictor(StandIn().to(DEV), image, cin, 3, roi, overlap=0.5, sub_batch=sub_batch)
    want, o, _, _ = _padded_windows(x, roi, 0.5)
    n = o.shape[0]
    assert n % sub_batch != 0 or n < sub_batch                                       # a tail sub-batch
    for s in range(p.n_sub):
        p.sub_idx.fill_(s)
        p.xb.fill_(float("nan"))
        p._gather(x)
        torch.cuda.synchronize()
        k = min(sub_batch, n - s * sub_batch)
        assert torch.equal(p.xb[:k], want[s * sub_batch:s * sub_batch + k]), s
        assert torch.equal(p.xb[k:], torch.zeros_like(p.xb[k:]))


# -------------------------------------------------------------------------------------------------- 2. blend + finalize
@pytest.mark.parametrize("mode", ["gaussian", "constant"])
@pytest.mark.parametrize("image,roi,overlap,sub_batch,contig", [
    ((40, 36, 28), (16, 16, 12), 0.5, 5, False),
    ((13, 30, 11), (16, 10, 4), 0.25, 4, True),            # H padded, channels-first logits
    ((24, 20, 18), (8, 8, 8), 0.75, 10, False),
])
def test_blend_finalize_match_float64_average(mode, image, roi, overlap, sub_batch, contig):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    torch.manual_seed(1)
    model = StandIn(contiguous_out=contig).to(DEV)
    x = torch.rand((1, 1) + image, device=DEV) * 2 - 1
    p = SlidingWindowPredictor(model, image, 1, 3, roi, overlap=overlap, mode=mode, sub_batch=sub_batch)
    out = p.predict(x, return_logits=True)
    torch.cuda.synchronize()
    assert out["labels"].shape == (1, 1) + image and out["labels"].dtype == torch.uint8
    assert out["logits"].shape == (1, 3) + image and out["logits"].dtype == torch.float32
    wins, _, _, _ = _padded_windows(x, roi, overlap)
    ref = _stitch64(model(wins)["downstream"], x.shape, roi, overlap, mode)
    rel = _rel(out["logits"][0], ref)
    assert rel <= 1e-6, rel
    ok, frac = _labels_where_decided(out["labels"], ref)
    assert ok and frac > 0.99


# -------------------------------------------------------------------------------------------------- 3. sub-batch invariance
@pytest.mark.parametrize("mode", ["gaussian", "constant"])
def test_result_is_bitwise_independent_of_the_sub_batch(mode):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    torch.manual_seed(2)
    image, roi = (30, 26, 21), (12, 12, 8)
    x = torch.rand((1, 1) + image, device=DEV)
    model = StandIn().to(DEV)
    runs = []
    n = None
    for sb in (1, 3, None):
        if sb is None:
            sb = n
        p = SlidingWindowPredictor(model, image, 1, 3, roi, overlap=0.5, mode=mode, sub_batch=sb)
        n = p.n_windows
        runs.append(p.predict(x, return_logits=True))
    torch.cuda.synchronize()
    assert n > 3 and n % 3 != 0
    for r in runs[1:]:
        assert torch.equal(r["logits"], runs[0]["logits"])
        assert torch.equal(r["labels"], runs[0]["labels"])


# -------------------------------------------------------------------------------------------------- 4. no overlap
def test_no_overlap_puts_every_window_back_in_place():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    torch.manual_seed(3)
    image, roi = (24, 16, 12), (8, 8, 4)
    x = torch.rand((1, 1) + image, device=DEV)
    model = StandIn().to(DEV)
    p = SlidingWindowPredictor(model, image, 1, 3, roi, overlap=0.0, mode="constant", sub_batch=5)
    out = p.predict(x, return_logits=True)
    want = torch.empty((3,) + image, device=DEV)
    for a, b, c in p.origins.tolist():
        w = x[:, :, a:a + roi[0], b:b + roi[1], c:c + roi[2]].contiguous()
        want[:, a:a + roi[0], b:b + roi[1], c:c + roi[2]] = model(w)["downstream"][0]
    torch.cuda.synchronize()
    assert p.n_windows == 3 * 2 * 3
    assert torch.equal(out["logits"][0], want)
    assert torch.equal(out["labels"][0, 0].long(), want.argmax(0))


# -------------------------------------------------------------------------------------------------- 5. HIP model vs oracle
def _tiny_model(seed=4):
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    from test_hip_configs import round_weights
    conf, _, _ = train.make_conf("tiny")
    torch.manual_seed(seed)
    model = SwinUnetR(conf)
    sd = round_weights({k: v.clone() for k, v in model.state_dict().items()})
    sd["extra_heads.downstream.1.bias"] = torch.tensor([0.3, -0.3])              # a margin, so that arg-max ties do not decide
    model.load_state_dict(sd)
    return conf, sd, model.to(DEV).eval()


def test_hip_model_whole_volume_against_oracle():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    from oracle.unetr_ref import OracleSwinUnetR
    conf, sd, model = _tiny_model()
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 1, 56, 48, 40, generator=g)
    seg = torch.randint(0, 2, (1, 1, 56, 48, 40), generator=g).float()
    roi = (32, 32, 32)
    p = SlidingWindowPredictor(model, x.shape[2:], 1, 2, roi, overlap=0.5, mode="gaussian", sub_batch=10)
    labels = p.predict(x.to(DEV))["labels"]
    iou, dice = p.evaluate(x.to(DEV), seg.to(DEV))
    wins, _, _, _ = _padded_windows(x, roi, 0.5)
    assert wins.shape[0] == 3 * 2 * 2
    want, _ = OracleSwinUnetR(conf, sd, emulate_bf16=True)(wins, training=False)
    ref = _stitch64(want["downstream"], x.shape, roi, 0.5, "gaussian")
    ref_labels = ref.argmax(0)
    same = labels[0, 0].long().cpu() == ref_labels
    agree = float(same.double().mean())
    # the bf16 model differs from the oracle by ~1e-3 in a logit, and this random-init head puts ~0.2 % of the voxels
    # within that of a tie (measured agreement 0.9982): the 0.999 bar holds where the oracle's top-2 margin exceeds 0.05
    top2 = ref.topk(2, dim=0).values
    decided = (top2[0] - top2[1]) > 0.05
    agree_decided = float(same[decided].double().mean())
    w_iou, w_dice = _miou_dice(_counts_cpu(ref_labels, seg, 2))
    print(f"[predict] label agreement {agree:.5f} (margin > 0.05: {agree_decided:.6f} of {float(decided.double().mean()):.4f}); "
          f"IoU {iou:.5f} / oracle {w_iou:.5f}; Dice {dice:.5f} / oracle {w_dice:.5f}")
    assert agree >= 0.995
    assert agree_decided >= 0.999 and float(decided.double().mean()) > 0.8
    assert abs(iou - w_iou) < 2e-3 and abs(dice - w_dice) < 2e-3


# -------------------------------------------------------------------------------------------------- 6. counts
@pytest.mark.parametrize("ncls", [2, 3])
def test_evaluate_counts_equal_cpu_counts_of_the_labels(ncls):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    torch.manual_seed(6)
    image, roi = (33, 20, 14), (16, 8, 8)
    x = torch.rand((1, 1) + image, device=DEV) * 2 - 1
    seg = torch.randint(0, ncls, (1, 1) + image, device=DEV).float()
    p = SlidingWindowPredictor(StandIn(ncls).to(DEV), image, 1, ncls, roi, overlap=0.5, sub_batch=4)
    labels = p.predict(x)["labels"]
    iou, dice = p.evaluate(x, seg)
    want = _counts_cpu(labels, seg, ncls)
    assert torch.equal(p.counts.cpu(), want)
    w_iou, w_dice = _miou_dice(want)
    assert iou == w_iou and dice == w_dice
    iou2, dice2 = p.evaluate(x, seg)                                      # the table is reset per volume
    assert (iou2, dice2) == (iou, dice) and torch.equal(p.counts.cpu(), want)


# -------------------------------------------------------------------------------------------------- 7. graph vs eager
def test_graph_equals_eager_tiny_with_tail():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    _, _, model = _tiny_model()
    g = torch.Generator().manual_seed(7)
    x = torch.rand(1, 1, 56, 48, 40, generator=g).to(DEV)
    x2 = torch.rand(1, 1, 56, 48, 40, generator=g).to(DEV)
    kw = dict(overlap=0.5, mode="gaussian", sub_batch=5)
    e = SlidingWindowPredictor(model, x.shape[2:], 1, 2, (32, 32, 32), **kw)
    gp = SlidingWindowPredictor(model, x.shape[2:], 1, 2, (32, 32, 32), graph=True, **kw)
    assert e.n_windows % 5 != 0
    for v in (x, x2):                                                     # the recorded graph serves a second volume
        a = e.predict(v, return_logits=True)
        b = gp.predict(v, return_logits=True)
        torch.cuda.synchronize()
        assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["labels"], b["labels"])


def test_graph_equals_eager_cfg1_real_size():
    import mivp_amd  # noqa: F401
    from mivp_amd import train
    from mivp_amd.inference import SlidingWindowPredictor
    from mivp_amd.swin_unetr import SwinUnetR
    conf, _, _ = train.make_conf("cfg1")
    torch.manual_seed(8)
    model = SwinUnetR(conf).to(DEV).eval()
    x = torch.rand(1, 1, 160, 144, 120, generator=torch.Generator().manual_seed(9)).to(DEV)
    kw = dict(overlap=0.5, mode="gaussian", sub_batch=4)
    a = SlidingWindowPredictor(model, x.shape[2:], 1, 2, (96, 96, 96), **kw).predict(x, return_logits=True)
    b = SlidingWindowPredictor(model, x.shape[2:], 1, 2, (96, 96, 96), graph=True, **kw).predict(x, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["labels"], b["labels"])
    assert torch.isfinite(a["logits"]).all()


# -------------------------------------------------------------------------------------------------- 8. validation
def test_predictor_refuses_bad_arguments():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor, predict_volume
    conf, _, model = _tiny_model()
    image, roi = (40, 36, 32), (32, 32, 32)
    p = SlidingWindowPredictor(model, image, 1, 2, roi, sub_batch=2)
    with pytest.raises(RuntimeError, match="GPU"):
        p.predict(torch.rand((1, 1) + image))                                          # CPU tensor
    with pytest.raises(RuntimeError, match="GPU"):
        predict_volume(model, torch.rand((1, 1) + image), roi, 2)
    with pytest.raises(ValueError):
        p.predict(torch.rand((2, 1) + image, device=DEV))                              # batch > 1
    with pytest.raises(ValueError):
        p.predict(torch.rand((1, 1, 40, 36, 30), device=DEV))                          # not the size it was built for
    with pytest.raises(ValueError):
        SlidingWindowPredictor(model, image, 2, 2, roi)                                # Cin != model
    with pytest.raises(ValueError):
        SlidingWindowPredictor(model, image, 1, 3, roi)                                # classes != model
    for ov in (-0.25, 1.0):
        with pytest.raises(ValueError):
            SlidingWindowPredictor(model, image, 1, 2, roi, overlap=ov)
    with pytest.raises(ValueError):
        SlidingWindowPredictor(model, image, 1, 2, (24, 32, 32))                       # not a multiple of 16
    with pytest.raises(ValueError):
        SlidingWindowPredictor(model, image, 1, 2, (32, 32, 30))                       # not a multiple of 4 along D
    with pytest.raises(ValueError):
        p.evaluate(torch.rand((1, 1) + image, device=DEV), torch.zeros((1, 2) + image, device=DEV))
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            SlidingWindowPredictor(model, image, 1, 2, roi, graph=True).predict(torch.rand((1, 1) + image, device=DEV))
    finally:
        model.eval()
