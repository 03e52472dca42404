"""GPU tests of window skipping in whole-volume prediction (SlidingWindowPredictor(skip=WindowSkip(...)),
csrc/window_skip.hip): the occupancy counts and the compacted work list against numpy (tests/window_skip_ref.py), bit
equality with the unfiltered predictor wherever every covering window is kept, the fill elsewhere, a float64 restatement
of the average over the kept windows, sub-batch and graph invariance, the metrics and the refusals."""
import numpy as np
import pytest
import torch

from window_skip_ref import compact, covered, occupancy, padded_foreground

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGE, ROI = (30, 26, 21), (12, 12, 8)                           # 4 x 4 x 5 = 80 windows at overlap 0.5
PADDED = ((13, 30, 11), (16, 10, 4))                             # H shorter than the roi
ALIGNED = ((20, 12, 16), (16, 8, 8))                             # D % 4 == 0: the 16-byte rows
SLABS = (((40, 36, 12), (32, 32, 8)), ((40, 36, 13), (32, 32, 8)))   # 8 large windows: two slabs of rows per window
THR = 0.0025


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


def _blob(image, cin=1, channel=0, box=None, seed=0, lo=(0, 0, 0)):
    """fp32 [1, cin, image] numpy volume: zero (air) outside a box at ``lo``, values in (0.1, 1] inside it."""
    rng = np.random.default_rng(seed)
    box = box or tuple(max(2, n // 3) for n in image)
    v = np.zeros((1, cin) + tuple(image), dtype=np.float32)
    sl = tuple(slice(a, a + b) for a, b in zip(lo, box))
    v[(0, channel) + sl] = 0.1 + 0.9 * rng.random(tuple(min(a + b, n) - a for a, b, n in zip(lo, box, image)),
                                                  dtype=np.float32)
    return v


def _predictor(image=IMAGE, roi=ROI, cin=1, skip=None, **kw):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    kw.setdefault("sub_batch", 7)
    return SlidingWindowPredictor(StandIn().to(DEV).eval(), image, cin, 3, roi, overlap=0.5, skip=skip, **kw)


def _fill_row(k, ncls=3):
    row = torch.full((ncls,), -k.fill_logit, dtype=torch.float32)
    row[k.fill_class] = k.fill_logit
    return row


def _crop(a, p):
    """[pdims] numpy array -> the image region."""
    return a[tuple(slice(q, q + n) for q, n in zip(p.pad, p.image_size))]


# -------------------------------------------------------------------------------------------------- 1. occupancy
@pytest.mark.parametrize("image,roi", [(IMAGE, ROI), PADDED, ALIGNED, SLABS[0], SLABS[1]])
@pytest.mark.parametrize("cin,channel", [(1, 0), (4, 2)])
def test_occupancy_equals_numpy(image, roi, cin, channel):
    from mivp_amd.inference import WindowSkip
    v = _blob(image, cin, channel)
    v[0, channel, 0, 1, 0:2] = np.float32(THR)                   # exactly the threshold: not foreground
    v[0, channel, 1, 0, 1] = np.nan                              # not foreground
    v[0, (channel + 1) % cin] += 0.0 if cin == 1 else 1.0        # another channel is all foreground: must not be read
    p = _predictor(image, roi, cin, WindowSkip(channel=channel))
    x = torch.from_numpy(v).to(DEV)
    p._reset()
    p._select(x[0].contiguous())
    want = occupancy(p.origins, roi, padded_foreground(image, roi, vol=v[0], channel=channel, threshold=THR))
    assert p.occupancy.dtype == torch.int32 and p.occupancy.cpu().numpy().tolist() == want.tolist()
    assert 0 < int((want > 0).sum()) < want.shape[0]
    # the mask source: the threshold is ignored
    mask = (np.random.default_rng(5).random(image) > 0.9).astype(np.uint8) * 3
    mask[image[0] // 2:] = 0
    mask[:, image[1] // 2:] = 0
    mask[:, :, image[2] // 4:] = 0                               # the windows further along hold nothing
    p.set_region(torch.from_numpy(mask).to(DEV))
    p._select(x[0].contiguous())
    want = occupancy(p.origins, roi, padded_foreground(image, roi, mask=mask))
    assert p.occupancy.cpu().numpy().tolist() == want.tolist()
    assert 0 < int((want > 0).sum()) < want.shape[0]
    p.set_region(None)
    p._select(x[0].contiguous())
    want = occupancy(p.origins, roi, padded_foreground(image, roi, vol=v[0], channel=channel, threshold=THR))
    assert p.occupancy.cpu().numpy().tolist() == want.tolist()


# -------------------------------------------------------------------------------------------------- 2. compaction
@pytest.mark.parametrize("mirror_axes", [(), (0, 2)])
@pytest.mark.parametrize("min_voxels", [1, 50])
def test_compacted_table_equals_numpy(mirror_axes, min_voxels):
    from mivp_amd.inference import WindowSkip, tta_table
    v = _blob(IMAGE)
    p = _predictor(skip=WindowSkip(min_voxels=min_voxels), mirror_axes=mirror_axes, sub_batch=3)
    x = torch.from_numpy(v).to(DEV)
    full = tta_table(p.origins, p.sub_batch, p.flip_codes)
    out = p.predict(x)
    counts = occupancy(p.origins, ROI, padded_foreground(IMAGE, ROI, vol=v[0]))
    want, meta = compact(full, counts, p.n_flips, min_voxels)
    assert p.table_full.cpu().numpy().tolist() == full.tolist()   # the full list is never written
    assert p.table.cpu().numpy().tolist() == want.tolist()
    assert p.meta.cpu().numpy().tolist() == meta.tolist()
    assert p.n_kept == int(meta[0]) and 0 < p.n_kept < p.n_windows
    assert p.n_kept * p.n_flips % p.sub_batch != 0                # a tail sub-batch
    assert p.n_sub_run == -(-p.n_kept * p.n_flips // p.sub_batch) < p.n_sub
    assert out["labels"].shape == (1, 1) + IMAGE


# -------------------------------------------------------------------------------------------------- 3. all windows kept
@pytest.mark.parametrize("mirror_axes", [(), (0, 2)])
def test_all_windows_kept_is_the_unfiltered_prediction_bitwise(mirror_axes):
    from mivp_amd.inference import WindowSkip
    x = torch.rand((1, 1) + IMAGE, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    ref = _predictor(mirror_axes=mirror_axes).predict(x, return_logits=True)
    p = _predictor(skip=WindowSkip(threshold=-1.0), mirror_axes=mirror_axes)
    got = p.predict(x, return_logits=True)
    assert p.n_kept == p.n_windows and p.n_sub_run == p.n_sub
    assert torch.equal(got["logits"], ref["logits"]) and torch.equal(got["labels"], ref["labels"])


# -------------------------------------------------------------------------------------------------- 4. foreground exactness
@pytest.mark.parametrize("far_corner", [False, True])
@pytest.mark.parametrize("mirror_axes", [(), (1,)])
def test_foreground_is_bitwise_unfiltered_and_uncovered_is_fill(mirror_axes, far_corner):
    from mivp_amd.inference import WindowSkip
    k = WindowSkip(min_voxels=1, fill_class=1, fill_logit=7.5)
    v = _blob(IMAGE)
    if far_corner:                                               # two small blobs: one sub-batch spans the whole volume
        v = _blob(IMAGE, box=(5, 5, 3)) + _blob(IMAGE, box=(4, 4, 3), lo=(26, 22, 18), seed=1)
    x = torch.from_numpy(v).to(DEV)
    ref = _predictor(mirror_axes=mirror_axes).predict(x, return_logits=True)
    p = _predictor(skip=k, mirror_axes=mirror_axes)
    got = p.predict(x, return_logits=True)
    fgp = padded_foreground(IMAGE, ROI, vol=v[0])
    counts = occupancy(p.origins, ROI, fgp)
    fg = torch.from_numpy(_crop(fgp, p))
    unc = torch.from_numpy(~_crop(covered(p.origins, ROI, p.pdims, counts >= 1), p))
    assert int(fg.sum()) > 0 and int(unc.sum()) > 0 and not bool((fg & unc).any())
    t = p.table.cpu().numpy()
    boxes = []
    for i in range(p.n_sub_run):
        e = t[i * p.sub_batch:(i + 1) * p.sub_batch]
        e = e[(e[:, 3] & 1) != 0, :3]
        boxes.append(int(np.prod([e[:, a].max() - e[:, a].min() + ROI[a] for a in range(3)])))
    # with the far corner a compacted sub-batch's union box outgrows the launch grid: the blend walks it with a stride
    assert (max(boxes) > int(np.prod(p.ubox))) == far_corner
    gl, rl = got["logits"][0].cpu(), ref["logits"][0].cpu()
    assert torch.equal(gl[:, fg], rl[:, fg])
    assert torch.equal(got["labels"][0, 0].cpu()[fg], ref["labels"][0, 0].cpu()[fg])
    assert torch.equal(gl[:, unc], _fill_row(k)[:, None].expand(3, int(unc.sum())))
    assert bool((got["labels"][0, 0].cpu()[unc] == k.fill_class).all())


# -------------------------------------------------------------------------------------------------- 5. everything else
def _stitch64_kept(model, x, p, keep, k, mode):
    """float64 weighted average over the kept windows only, fill elsewhere -> [C, H, W, D]."""
    from mivp_amd.inference import importance_tables
    roi, pdims, pad, n = p.roi, p.pdims, p.pad, p.image_size
    xp = torch.zeros((1, x.shape[1]) + tuple(pdims), dtype=x.dtype, device=x.device)
    xp[:, :, pad[0]:pad[0] + n[0], pad[1]:pad[1] + n[1], pad[2]:pad[2] + n[2]] = x
    tabs, floor = importance_tables(roi, mode, 0.125)
    wmap = torch.from_numpy(np.maximum(tabs[0][:, None, None] * tabs[1][None, :, None] * tabs[2][None, None, :], floor))
    acc = torch.zeros((3,) + tuple(pdims), dtype=torch.float64)
    ws = torch.zeros(tuple(pdims), dtype=torch.float64)
    for (a, b, c), on in zip(p.origins.tolist(), keep):
        if not on:
            continue
        w = xp[:, :, a:a + roi[0], b:b + roi[1], c:c + roi[2]].contiguous()
        lg = model(w)["downstream"][0].double().cpu()
        acc[:, a:a + roi[0], b:b + roi[1], c:c + roi[2]] += wmap * lg
        ws[a:a + roi[0], b:b + roi[1], c:c + roi[2]] += wmap
    empty = ws == 0
    acc[:, empty] = _fill_row(k).double()[:, None]
    ws[empty] = 1.0
    res = acc / ws
    return res[:, pad[0]:pad[0] + n[0], pad[1]:pad[1] + n[1], pad[2]:pad[2] + n[2]]


@pytest.mark.parametrize("mode", ["gaussian", "constant"])
@pytest.mark.parametrize("min_voxels", [1, 50])
@pytest.mark.parametrize("image,roi", [(IMAGE, ROI), PADDED])
def test_logits_match_float64_average_over_kept_windows(image, roi, min_voxels, mode):
    from mivp_amd.inference import WindowSkip
    k = WindowSkip(min_voxels=min_voxels)
    v = _blob(image, box=tuple(max(3, n // 2) for n in image))
    x = torch.from_numpy(v).to(DEV)
    p = _predictor(image, roi, skip=k, mode=mode, sub_batch=4)
    got = p.predict(x, return_logits=True)
    counts = occupancy(p.origins, roi, padded_foreground(image, roi, vol=v[0]))
    keep = counts >= min_voxels
    assert p.n_kept == int(keep.sum()) and 0 < p.n_kept < p.n_windows
    ref = _stitch64_kept(p.model, x, p, keep, k, mode)
    a, b = got["logits"][0].double().cpu().reshape(-1), ref.reshape(-1)
    rel = float((a - b).norm() / b.norm())
    assert rel <= 1e-6, rel
    top2 = ref.topk(2, dim=0).values
    decided = (top2[0] - top2[1]) > 1e-5
    assert bool((got["labels"][0, 0].long().cpu()[decided] == ref.argmax(0)[decided]).all())
    assert float(decided.double().mean()) > 0.99


# -------------------------------------------------------------------------------------------------- 6. invariance
@pytest.mark.parametrize("mirror_axes", [(), (0, 2)])
def test_result_is_bitwise_independent_of_the_sub_batch(mirror_axes):
    from mivp_amd.inference import WindowSkip
    x = torch.from_numpy(_blob(IMAGE, box=(14, 11, 9))).to(DEV)
    runs, n, kept = [], None, set()
    for sb in (1, 3, None):
        p = _predictor(skip=WindowSkip(), mirror_axes=mirror_axes, sub_batch=n if sb is None else sb)
        n = p.n_windows
        runs.append(p.predict(x, return_logits=True))
        kept.add(p.n_kept)
    assert len(kept) == 1 and 0 < kept.pop() < n
    for r in runs[1:]:
        assert torch.equal(r["logits"], runs[0]["logits"]) and torch.equal(r["labels"], runs[0]["labels"])


def test_graph_equals_eager_over_volumes_with_different_kept_sets():
    from mivp_amd.inference import WindowSkip
    k = WindowSkip()
    vols = [_blob(IMAGE, box=(10, 9, 7)), _blob(IMAGE, box=(10, 9, 7), lo=(17, 12, 10))]
    eager, graph = _predictor(skip=k, sub_batch=3), _predictor(skip=k, sub_batch=3, graph=True)
    kept, recorded = [], []
    for v in vols:
        x = torch.from_numpy(v).to(DEV)
        e, g = eager.predict(x, return_logits=True), graph.predict(x, return_logits=True)
        assert torch.equal(g["logits"], e["logits"]) and torch.equal(g["labels"], e["labels"])
        assert torch.equal(graph.table, eager.table) and graph.n_kept == eager.n_kept
        assert graph.n_sub_run == eager.n_sub_run < graph.n_sub
        kept.append(graph.table.cpu().numpy().tolist())
        recorded.append(graph.graph)
    assert kept[0] != kept[1]
    assert recorded[0] is not None and recorded[1] is recorded[0]  # recorded once, replayed for both volumes


def test_all_air_volume_runs_no_sub_batch_and_is_all_fill():
    from mivp_amd.inference import WindowSkip
    k = WindowSkip(fill_class=2, fill_logit=10.0)
    for graph in (False, True):
        p = _predictor(skip=k, graph=graph)
        out = p.predict(torch.zeros((1, 1) + IMAGE, device=DEV), return_logits=True, return_probs=True,
                        return_confidence=True, return_entropy=True)
        assert p.n_kept == 0 and p.n_sub_run == 0
        assert int(p.occupancy.abs().sum()) == 0 and not bool(p.table.any())
        assert bool((out["labels"] == 2).all())
        want = _fill_row(k).to(DEV)[None, :, None, None, None].expand_as(out["logits"])
        assert torch.equal(out["logits"], want)
        for name in ("probs", "confidence", "entropy"):
            assert bool(torch.isfinite(out[name]).all()), name
        assert float(out["confidence"].min()) > 0.99 and float(out["entropy"].max()) < 0.01
        assert torch.equal(out["probs"].argmax(1, keepdim=True), out["labels"].long())


# -------------------------------------------------------------------------------------------------- 7. evaluation, post-processing
def test_evaluate_counts_and_postprocess():
    from mivp_amd.inference import WindowSkip
    v = _blob(IMAGE, box=(14, 11, 9))
    x = torch.from_numpy(v).to(DEV)
    seg = torch.from_numpy((v[:, :1] > 0.5).astype(np.float32)).to(DEV)
    p = _predictor(skip=WindowSkip())
    iou, dice = p.evaluate(x, seg)
    labels = p.predict(x)["labels"]
    pl, tl = labels.reshape(-1).long().cpu(), seg.reshape(-1).long().cpu()
    want = torch.tensor([[int(((pl == c) & (tl == c)).sum()), int((pl == c).sum()), int((tl == c).sum())]
                         for c in range(3)], dtype=torch.int64)
    assert torch.equal(p.counts.cpu(), want)
    c = want.double()
    assert iou == pytest.approx(float((c[:, 0] / (c[:, 1] + c[:, 2] - c[:, 0] + 1e-6)).mean()), abs=1e-12)
    assert dice == pytest.approx(float((2 * c[:, 0] / (c[:, 1] + c[:, 2] + 1e-6)).mean()), abs=1e-12)
    assert 0 < p.n_kept < p.n_windows
    post = p.predict(x, postprocess={"largest": True})["labels"]
    assert post.shape == labels.shape and post.dtype == torch.uint8
    assert int(post.max()) < 3


# -------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    import mivp_amd
    from mivp_amd.inference import WindowSkip, predict_volume
    plain = _predictor()
    with pytest.raises(ValueError):
        plain.set_region(torch.zeros(IMAGE, dtype=torch.uint8, device=DEV))
    p = _predictor(skip=WindowSkip())
    for bad in (torch.zeros((4, 4, 4), dtype=torch.uint8, device=DEV), torch.zeros(IMAGE, dtype=torch.float32, device=DEV),
                torch.zeros(IMAGE, dtype=torch.bool, device=DEV), torch.zeros((1,) + IMAGE, dtype=torch.uint8, device=DEV),
                torch.zeros(IMAGE, dtype=torch.uint8), np.zeros(IMAGE, dtype=np.uint8)):
        with pytest.raises(ValueError):
            p.set_region(bad)
    p.set_region(torch.ones(IMAGE, dtype=torch.uint8, device=DEV))
    p.set_region(None)
    for bad in (dict(channel=-1), dict(min_voxels=0), dict(fill_class=-1), dict(fill_logit=0.0),
                dict(fill_logit=float("inf")), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            WindowSkip(**bad)
    with pytest.raises(ValueError):
        _predictor(skip=WindowSkip(channel=1))                   # a 1-channel volume
    with pytest.raises(ValueError):
        _predictor(skip=WindowSkip(fill_class=3))                # 3 classes
    with pytest.raises(ValueError):
        _predictor(skip=0.0025)
    # the one-shot helper passes skip through
    x = torch.from_numpy(_blob(IMAGE)).to(DEV)
    k = WindowSkip(fill_class=1)
    out = predict_volume(StandIn().to(DEV), x, ROI, 3, sub_batch=7, skip=k)
    assert torch.equal(out["labels"], _predictor(skip=k).predict(x)["labels"])
    assert mivp_amd.WindowSkip is WindowSkip
