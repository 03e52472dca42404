"""GPU tests of mirror test-time augmentation and the probability maps of whole-volume prediction
(mivp_amd.inference.SlidingWindowPredictor(mirror_axes=...), csrc/stitch.hip ABI 18): the flip-aware gather against
torch.flip of torch slicing, blend + finalize against a float64 restatement per window and flip code, sub-batch and graph
invariance, the HIP model, identities that need no oracle, the softmax / confidence / entropy maps and the paths that
run under augmentation with no further arguments."""
import math

import numpy as np
import pytest
import torch

from test_hip_predict import StandIn, _counts_cpu, _labels_where_decided, _miou_dice, _padded_windows, _rel, _tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


class RampStandIn(torch.nn.Module):
    """A per-window model that is NOT flip-equivariant: element-wise functions of the first input channel multiplied by a
    fixed, asymmetric per-position ramp of the roi's shape (so a flip that is not undone, or undone along the wrong axis,
    changes the result), with no reduction over the batch.  Returned like the HIP model's output: a channels-first view of
    channels-last fp32 storage (or contiguous)."""

    def __init__(self, ncls=3, contiguous_out=False):
        super().__init__()
        self.ncls, self.contiguous_out = ncls, contiguous_out
        self.anchor = torch.nn.Parameter(torch.zeros(1), requires_grad=False)

    @staticmethod
    def ramp(r, device):
        i, j, k = [torch.arange(n, dtype=torch.float32, device=device) for n in r]
        return ((1.0 + 0.5 * i / r[0])[:, None, None] * (1.0 - 0.3 * (j / r[1]) ** 2)[None, :, None]
                * (0.75 + 0.5 * torch.sqrt(k / r[2]))[None, None, :])

    def forward(self, x):
        x0 = x[:, 0]
        ramp = self.ramp(x0.shape[1:], x0.device)
        ch = [(torch.tanh(x0 * k + b) + 0.25 * torch.sin(x0 * (3.0 + c))) * ramp + 0.05 * c * (ramp - 1.0)
              for c, (k, b) in enumerate(StandIn.K[:self.ncls])]
        out = torch.stack(ch, dim=-1).permute(0, 4, 1, 2, 3)
        return {"downstream": out.contiguous() if self.contiguous_out else out}


def _flip_dims(code, first):
    """torch.flip dims of a flip code for a tensor whose roi axes start at ``first``."""
    return [first + a for a in range(3) if (code >> a) & 1]


def _flip(t, code, first):
    d = _flip_dims(code, first)
    return torch.flip(t, d) if d else t


def _codes(axes):
    mask = sum(1 << a for a in axes)
    return [m for m in range(8) if m & ~mask == 0]


def _entry_inputs(x, roi, overlap, codes):
    """The model inputs of every work-list entry, window-major and flip-minor, by torch slicing and torch.flip:
    [N * F, Cin, roi]."""
    wins, o, _, _ = _padded_windows(x, roi, overlap)
    ent = torch.stack([_flip(wins, m, 2) for m in codes], dim=1)               # [N, F, Cin, roi]
    return ent.reshape((-1,) + tuple(wins.shape[1:])), o


def _restate64(entry_logits, image, roi, overlap, mode, codes, sigma_scale=0.125):
    """float64 restatement of the augmented blend: entry w * F + j holds the model's logits [C, roi] of window w under
    codes[j]; they are flipped back, weighted by the UNFLIPPED importance map, summed and divided.  -> [C, H, W, D]."""
    from mivp_amd.inference import importance_tables, window_origins, window_padding
    n = tuple(image)
    pad, pdims = window_padding(n, roi)
    o = window_origins(n, roi, overlap)
    tabs, floor = importance_tables(roi, mode, sigma_scale)
    wmap = torch.from_numpy(np.maximum(tabs[0][:, None, None] * tabs[1][None, :, None] * tabs[2][None, None, :], floor))
    lg = entry_logits.detach().double().cpu()
    f = len(codes)
    assert lg.shape[0] == o.shape[0] * f
    acc = torch.zeros((lg.shape[1],) + tuple(pdims), dtype=torch.float64)
    ws = torch.zeros(tuple(pdims), dtype=torch.float64)
    for w, (a, b, c) in enumerate(o.tolist()):
        for j, m in enumerate(codes):
            acc[:, a:a + roi[0], b:b + roi[1], c:c + roi[2]] += wmap * _flip(lg[w * f + j], m, 1)
            ws[a:a + roi[0], b:b + roi[1], c:c + roi[2]] += wmap
    res = acc / ws
    return res[:, pad[0]:pad[0] + n[0], pad[1]:pad[1] + n[1], pad[2]:pad[2] + n[2]]


def _predictor(model, image, cin, ncls, roi, **kw):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    return SlidingWindowPredictor(model, image, cin, ncls, roi, **kw)


# -------------------------------------------------------------------------------------------------- 1. gather
@pytest.mark.parametrize("cin,image,roi,sub_batch", [
    (1, (10, 13, 7), (16, 8, 12), 5),      # H and D shorter than the roi (both faces), scalar rows (D % 4 != 0)
    (4, (9, 6, 8), (12, 8, 12), 3),        # every axis padded; 16-byte path with misaligned rows (pad 2 along D)
    (4, (20, 12, 16), (16, 8, 8), 5),      # no padding, aligned 16-byte rows, mirrored quads reversed in registers
    (1, (21, 11, 9), (8, 8, 5), 7),        # an odd roi edge along D
])
def test_gather_equals_flipped_torch_slicing_bitwise(cin, image, roi, sub_batch):
    torch.manual_seed(0)
    x = torch.randn((1, cin) + image, device=DEV)
    p = _predictor(StandIn().to(DEV), image, cin, 3, roi, overlap=0.5, sub_batch=sub_batch, mirror_axes=(0, 1, 2))
    assert p.flip_codes == (0, 1, 2, 3, 4, 5, 6, 7) and p.n_flips == 8 and p.n_entries == 8 * p.n_windows
    want, _ = _entry_inputs(x, roi, 0.5, list(p.flip_codes))
    n = p.n_entries
    assert n % sub_batch != 0                                                        # a tail sub-batch
    assert p.n_sub == math.ceil(n / sub_batch)
    for s in range(p.n_sub):
        p.sub_idx.fill_(s)
        p.xb.fill_(float("nan"))
        p._gather(x)
        torch.cuda.synchronize()
        k = min(sub_batch, n - s * sub_batch)
        assert torch.equal(p.xb[:k], want[s * sub_batch:s * sub_batch + k]), s
        assert torch.equal(p.xb[k:], torch.zeros_like(p.xb[k:]))                     # invalid slots are zero


# -------------------------------------------------------------------------------------------------- 2. blend + finalize
BLEND_CASES = [
    ((40, 36, 28), (16, 16, 12), 0.5, 5, False, (0, 1, 2)),
    ((13, 30, 11), (16, 10, 5), 0.25, 4, True, (2,)),       # H padded, an odd roi edge, channels-first logits
    ((24, 20, 18), (8, 8, 8), 0.75, 10, False, (0, 1)),
    ((20, 18, 15), (8, 6, 7), 0.5, 6, True, (0, 1, 2)),     # 8 x 8 contributions per inner voxel, odd roi edge
]


def _blend_case_reference(model, x, roi, overlap, mode, axes):
    codes = _codes(axes)
    ent, _ = _entry_inputs(x, roi, overlap, codes)
    return _restate64(model(ent)["downstream"], x.shape[2:], roi, overlap, mode, codes)


@pytest.mark.parametrize("mode", ["gaussian", "constant"])
@pytest.mark.parametrize("image,roi,overlap,sub_batch,contig,axes", BLEND_CASES)
def test_blend_finalize_match_float64_restatement(mode, image, roi, overlap, sub_batch, contig, axes):
    torch.manual_seed(1)
    model = RampStandIn(contiguous_out=contig).to(DEV)
    x = torch.rand((1, 1) + image, device=DEV) * 2 - 1
    p = _predictor(model, image, 1, 3, roi, overlap=overlap, mode=mode, sub_batch=sub_batch, mirror_axes=axes)
    assert p.n_flips == 2 ** len(axes) and list(p.flip_codes) == _codes(axes)
    out = p.predict(x, return_logits=True)
    torch.cuda.synchronize()
    assert out["labels"].shape == (1, 1) + image and out["labels"].dtype == torch.uint8
    assert out["logits"].shape == (1, 3) + image and out["logits"].dtype == torch.float32
    ref = _blend_case_reference(model, x, roi, overlap, mode, axes)
    rel = _rel(out["logits"][0], ref)
    ok, frac = _labels_where_decided(out["labels"], ref)
    print(f"[tta blend] {mode} {image} {roi} ov {overlap} axes {axes}: rel-L2 {rel:.3e}, decided {frac:.5f}")
    assert rel <= 1e-6, rel
    assert ok and frac > 0.99
    # the augmentation is not a no-op for this model: the plain prediction differs
    plain = _predictor(model, image, 1, 3, roi, overlap=overlap, mode=mode, sub_batch=sub_batch).predict(x, return_logits=True)
    assert _rel(plain["logits"][0], ref) > 1e-3


# -------------------------------------------------------------------------------------------------- 3. invariance
@pytest.mark.parametrize("mode", ["gaussian", "constant"])
def test_result_is_bitwise_independent_of_the_sub_batch(mode):
    torch.manual_seed(2)
    image, roi = (30, 26, 21), (12, 12, 8)
    x = torch.rand((1, 1) + image, device=DEV)
    model = RampStandIn().to(DEV)
    runs, n, f = [], None, 8
    for sb in (1, 3, f, None):
        p = _predictor(model, image, 1, 3, roi, overlap=0.5, mode=mode, sub_batch=sb if sb else n,
                       mirror_axes=(0, 1, 2))
        n = p.n_entries
        assert p.n_flips == f and n == p.n_windows * f
        runs.append(p.predict(x, return_logits=True))
    torch.cuda.synchronize()
    assert n > 3 and n % 3 != 0
    for r in runs[1:]:
        assert torch.equal(r["logits"], runs[0]["logits"])
        assert torch.equal(r["labels"], runs[0]["labels"])


def test_graph_equals_eager_stand_in_with_tail():
    torch.manual_seed(3)
    image, roi = (30, 26, 21), (12, 12, 8)
    model = RampStandIn().to(DEV).eval()
    kw = dict(overlap=0.5, mode="gaussian", sub_batch=6, mirror_axes=(0, 2))
    e = _predictor(model, image, 1, 3, roi, **kw)
    g = _predictor(model, image, 1, 3, roi, graph=True, **kw)
    assert e.n_entries % 6 != 0 and g.n_sub == math.ceil(e.n_entries / 6)
    for seed in (0, 1):                                                   # the recorded graph serves a second volume
        x = torch.rand((1, 1) + image, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
        a = e.predict(x, return_logits=True)
        b = g.predict(x, return_logits=True)
        torch.cuda.synchronize()
        assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["labels"], b["labels"])


# -------------------------------------------------------------------------------------------------- 4. HIP model
def _entry_logits(p, x):
    """The model's own eager logits of every work-list entry, computed in the predictor's sub-batch composition."""
    vol = x.float().contiguous()
    outs = []
    for s in range(p.n_sub):
        p.sub_idx.fill_(s)
        p._gather(vol)
        outs.append(p.model(p.xb)["downstream"].float().clone())
    return torch.cat(outs)[:p.n_entries]


def test_hip_model_graph_equals_eager_and_matches_restatement():
    """Tiny HIP model in eval(), mirror_axes=(0, 1, 2).  The float64 restatement is fed the model's own eager per-entry
    logits, so what is compared is the stitching arithmetic alone.  The bar is twice the relative L2 the plain
    (no-augmentation) path shows against its own restatement on the same model and volume.

    Measured on one MI355X: plain 4.78e-08, augmented 4.17e-08, bar 9.57e-08.  (With a plain sequential fp32 sum of the
    8 x longer list the augmented figure was 2.54e-07; the blend's compensated sums are what holds the bar.)"""
    _, _, model = _tiny_model()
    image, roi = (56, 48, 40), (32, 32, 32)
    x = torch.rand((1, 1) + image, generator=torch.Generator().manual_seed(7)).to(DEV)
    kw = dict(overlap=0.5, mode="gaussian", sub_batch=5)
    plain = _predictor(model, image, 1, 2, roi, **kw)
    base = _rel(plain.predict(x, return_logits=True)["logits"][0],
                _restate64(_entry_logits(plain, x), image, roi, 0.5, "gaussian", [0]))
    e = _predictor(model, image, 1, 2, roi, mirror_axes=(0, 1, 2), **kw)
    g = _predictor(model, image, 1, 2, roi, mirror_axes=(0, 1, 2), graph=True, **kw)
    assert e.n_entries == 8 * plain.n_windows and e.n_entries % 5 != 0
    a = e.predict(x, return_logits=True)
    b = g.predict(x, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["labels"], b["labels"])
    rel = _rel(a["logits"][0], _restate64(_entry_logits(e, x), image, roi, 0.5, "gaussian", list(e.flip_codes)))
    print(f"[tta hip model] rel-L2 vs restatement: no-TTA {base:.3e}, TTA {rel:.3e} (bar {2 * base:.3e})")
    assert torch.isfinite(a["logits"]).all()
    assert rel <= 2 * base, (rel, base)


# -------------------------------------------------------------------------------------------------- 5. identities
@pytest.mark.parametrize("axes", [(2,), (0, 1), (0, 1, 2)])
def test_pointwise_model_at_overlap_zero_returns_the_plain_logits(axes):
    """A flip-equivariant (pointwise) model, constant weights, an image that is a multiple of the roi at overlap 0: every
    voxel averages F identical values v, and the augmented logits equal the plain ones bitwise.  The blend's compensated
    sum holds fl(k v) after k additions (the compensation word is the exact error of the last addition, and v minus it is
    exact but for significands within F units of the top of a binade), F v is a power of two times v and so exact, and
    the weight sum is F.  (A plain fp32 sum would not do for F = 8: a significand congruent to 2 mod 8 rounds down three
    times between 4 v and 8 v and ends one unit low.)"""
    torch.manual_seed(4)
    image, roi = (24, 16, 12), (8, 8, 4)
    x = torch.rand((1, 1) + image, device=DEV)
    model = StandIn().to(DEV)
    kw = dict(overlap=0.0, mode="constant", sub_batch=5)
    plain = _predictor(model, image, 1, 3, roi, **kw).predict(x, return_logits=True)
    p = _predictor(model, image, 1, 3, roi, mirror_axes=axes, **kw)
    out = p.predict(x, return_logits=True)
    torch.cuda.synchronize()
    assert p.n_flips == 2 ** len(axes)
    assert torch.equal(out["logits"], plain["logits"]) and torch.equal(out["labels"], plain["labels"])


@pytest.mark.parametrize("cin,image,roi,sub_batch", [(1, (30, 26, 21), (12, 12, 8), 4), (4, (9, 6, 8), (12, 8, 12), 3),
                                                     (1, (21, 11, 9), (8, 8, 5), 7)])
def test_flip_aware_kernels_without_flips_equal_the_plain_entry_points(cin, image, roi, sub_batch):
    torch.manual_seed(5)
    x = torch.rand((1, cin) + image, device=DEV) * 2 - 1
    model = RampStandIn().to(DEV)
    old = _predictor(model, image, cin, 3, roi, overlap=0.5, sub_batch=sub_batch)
    new = _predictor(model, image, cin, 3, roi, overlap=0.5, sub_batch=sub_batch, mirror_axes=())
    assert old.flip_codes == new.flip_codes == (0,) and new.n_entries == new.n_windows and not old._tta_kernels
    new._tta_kernels = True                                                # the ABI 18 gather / blend with code 0 everywhere
    for s in range(old.n_sub):
        for p in (old, new):
            p.sub_idx.fill_(s)
            p.xb.fill_(float("nan"))
            p._gather(x)
        assert torch.equal(old.xb, new.xb)
    a = old.predict(x, return_logits=True)
    b = new.predict(x, return_logits=True, return_probs=True, return_confidence=True, return_entropy=True)
    torch.cuda.synchronize()
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["labels"], b["labels"])


# -------------------------------------------------------------------------------------------------- 6. maps
def _maps64(logits):
    lg = logits.double().cpu()[0]                                          # [C, H, W, D]
    pr = torch.softmax(lg, dim=0)
    c = lg.shape[0]
    ent = -(pr * torch.log(pr.clamp_min(1e-300))).sum(0) / math.log(c) if c > 1 else torch.zeros_like(pr[0])
    return pr, pr.max(0).values, ent


@pytest.mark.parametrize("ncls,axes,scale", [(3, (0, 1, 2), 1.0), (2, (), 1.0), (4, (1,), 6.0), (1, (2,), 1.0)])
def test_probability_maps_match_float64_softmax(ncls, axes, scale):
    torch.manual_seed(6)
    image, roi = (26, 20, 14), (12, 8, 8)
    x = (torch.rand((1, 1) + image, device=DEV) * 2 - 1) * scale
    model = RampStandIn(ncls).to(DEV)
    p = _predictor(model, image, 1, ncls, roi, overlap=0.5, sub_batch=4, mirror_axes=axes)
    plain = p.predict(x, return_logits=True)
    out = p.predict(x, return_logits=True, return_probs=True, return_confidence=True, return_entropy=True)
    torch.cuda.synchronize()
    assert set(out) == {"labels", "logits", "probs", "confidence", "entropy"}
    assert out["probs"].shape == (1, ncls) + image and out["probs"].dtype == torch.float32
    assert out["confidence"].shape == out["entropy"].shape == (1, 1) + image
    assert torch.equal(out["labels"], plain["labels"]) and torch.equal(out["logits"], plain["logits"])
    pr, conf, ent = _maps64(out["logits"])
    e_p = float((out["probs"][0].double().cpu() - pr).abs().max())
    e_c = float((out["confidence"][0, 0].double().cpu() - conf).abs().max())
    e_e = float((out["entropy"][0, 0].double().cpu() - ent).abs().max())
    e_s = float((out["probs"][0].double().sum(0) - 1).abs().max())
    print(f"[tta maps] C {ncls} axes {axes}: max abs err probs {e_p:.2e} confidence {e_c:.2e} entropy {e_e:.2e}; "
          f"|sum p - 1| {e_s:.2e}")
    assert e_p <= 1e-5 and e_c <= 1e-5 and e_e <= 1e-5 and e_s <= 1e-5
    for k in ("probs", "confidence", "entropy"):
        assert float(out[k].min()) >= 0.0 and float(out[k].max()) <= 1.0
    if ncls == 1:
        assert torch.equal(out["entropy"], torch.zeros_like(out["entropy"]))
        assert torch.equal(out["probs"], torch.ones_like(out["probs"]))
    # any subset of the maps, with and without the logits: the same values, the same labels
    names = ("probs", "confidence", "entropy")
    for bits in range(1, 7):
        sel = {n: bool(bits >> i & 1) for i, n in enumerate(names)}
        sub = p.predict(x, return_logits=bool(bits & 1), **{"return_" + n: on for n, on in sel.items()})
        assert set(sub) == {"labels"} | {n for n, on in sel.items() if on} | ({"logits"} if bits & 1 else set())
        assert torch.equal(sub["labels"], plain["labels"])
        for n, on in sel.items():
            if on:
                assert torch.equal(sub[n], out[n]), n


# -------------------------------------------------------------------------------------------------- 7. pass-through
def test_evaluate_counts_under_tta_equal_cpu_counts_of_the_tta_labels():
    torch.manual_seed(7)
    image, roi, ncls = (33, 20, 14), (16, 8, 8), 3
    x = torch.rand((1, 1) + image, device=DEV) * 2 - 1
    seg = torch.randint(0, ncls, (1, 1) + image, device=DEV).float()
    p = _predictor(RampStandIn(ncls).to(DEV), image, 1, ncls, roi, overlap=0.5, sub_batch=4, mirror_axes=(0, 1, 2))
    labels = p.predict(x)["labels"]
    iou, dice = p.evaluate(x, seg)
    want = _counts_cpu(labels, seg, ncls)
    assert torch.equal(p.counts.cpu(), want)
    assert (iou, dice) == _miou_dice(want)
    surf = p.evaluate_surface(x, seg)
    assert surf["iou"] == iou and surf["dice"] == dice


def test_scan_paths_and_postprocess_under_tta():
    import mivp_amd
    from mivp_amd import components, scan
    torch.manual_seed(8)
    shape, roi, ncls = (40, 36, 20), (16, 16, 8), 2
    geom = scan.ScanGeometry.from_affine(shape, np.diag([-0.8, -0.8, 2.5, 1.0]))
    raw = torch.randint(-900, 900, (1,) + shape, dtype=torch.int16, device=DEV)
    seg = torch.randint(0, ncls, shape, dtype=torch.int16, device=DEV)
    model = RampStandIn(ncls).to(DEV).eval()
    kw = dict(overlap=0.5, sub_batch=6, mirror_axes=(0, 2))
    p = _predictor(model, geom.size, 1, ncls, roi, **kw)
    g = _predictor(model, geom.size, 1, ncls, roi, graph=True, **kw)
    x = scan.prepare_scan(raw, geom)
    steps = p.predict(x, return_logits=True)
    a = p.predict_scan(raw, geom)
    assert torch.equal(a["labels_oriented"], steps["labels"])
    assert torch.equal(a["labels"], scan.restore_labels(steps["labels"], geom))
    b = g.predict_scan(raw, geom)
    assert torch.equal(b["labels"], a["labels"])
    c = p.predict_scan(raw, geom, restore="logits")
    assert torch.equal(c["labels"], scan.restore_labels_from_logits(steps["logits"], geom))
    post = {"largest": True}
    d = p.predict(x, postprocess=post, return_logits=True, return_confidence=True)
    assert torch.equal(d["labels"][0, 0], components.postprocess_labels(steps["labels"][0, 0], ncls, **post))
    assert torch.equal(d["logits"], steps["logits"])                       # the maps describe the blend before it
    assert torch.equal(d["confidence"], p.predict(x, return_confidence=True)["confidence"])
    assert not torch.equal(d["labels"], steps["labels"])
    got = p.evaluate_scan(raw, seg, geom)
    assert got == p.evaluate(x, scan.prepare_labels(seg, geom))
    one = mivp_amd.predict_volume(model, x, roi, ncls, overlap=0.5, sub_batch=6, mirror_axes=(0, 2), return_entropy=True)
    assert torch.equal(one["labels"], steps["labels"]) and one["entropy"].shape == (1, 1) + tuple(geom.size)
    assert mivp_amd.evaluate_volume(model, x, scan.prepare_labels(seg, geom), roi, ncls, overlap=0.5, sub_batch=6,
                                    mirror_axes=(0, 2)) == got


# -------------------------------------------------------------------------------------------------- 8. validation
def test_predictor_refuses_bad_mirror_axes():
    from mivp_amd.inference import predict_volume
    model = StandIn().to(DEV)
    for bad in ((3,), (-1,), (0, 0), (2, 1, 2), (0, 1, 2, 0)):
        with pytest.raises(ValueError, match="mirror_axes"):
            _predictor(model, (16, 16, 16), 1, 3, (8, 8, 8), mirror_axes=bad)
        with pytest.raises(ValueError, match="mirror_axes"):
            predict_volume(model, torch.rand(1, 1, 16, 16, 16, device=DEV), (8, 8, 8), 3, mirror_axes=bad)
