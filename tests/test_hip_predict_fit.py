"""GPU tests of fitting the prediction windows to the foreground bounding box (SlidingWindowPredictor(fit=WindowFit(...)),
inference.foreground_box, csrc/window_fit.hip): the box and the fitted work list against numpy (tests/window_fit_ref.py),
bit equality with the predictor without ``fit`` when the box is the whole volume, a float64 restatement of the average over
the fitted windows with the fill elsewhere, sub-batch and graph invariance, the metrics and the refusals."""
import numpy as np
import pytest
import torch

from components_ref import postprocess as postprocess_ref
from window_fit_ref import box_of, covered, fitted_origins, fitted_table, foreground

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGE, ROI = (30, 26, 21), (12, 12, 8)                           # 4 x 4 x 5 = 80 windows at overlap 0.5
PADDED = ((13, 30, 11), (16, 10, 4))                             # H shorter than the roi
ALIGNED = ((20, 12, 16), (16, 8, 8))                             # D % 4 == 0: the 16-byte rows
SHAPES = [(IMAGE, ROI), PADDED, ALIGNED]
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


def _vol(image, cin=1, channel=0, lo=None, size=None, pts=(), nan=False, noise=False, seed=0):
    """fp32 [1, cin, image] numpy volume whose channel ``channel`` is foreground (values in [0.1, 1]) exactly in the box
    of ``size`` at ``lo`` and at the voxels ``pts``.  ``noise``: the air holds values in [0, 0.002), below the threshold.
    ``nan``: two NaN corners and a voxel exactly at the threshold (none of them foreground).  Any other channel is all
    foreground: it must not be read."""
    rng = np.random.default_rng(seed)
    v = np.zeros((1, cin) + tuple(image), dtype=np.float32)
    if noise:
        v[0, channel] = 0.002 * rng.random(tuple(image), dtype=np.float32)
    if lo is not None:
        sl = (0, channel) + tuple(slice(a, a + b) for a, b in zip(lo, size))
        v[sl] = 0.1 + 0.9 * rng.random(v[sl].shape, dtype=np.float32)
    for pt in pts:
        v[(0, channel) + tuple(pt)] = 0.7
    if nan:
        v[0, channel, 0, 0, 0] = np.nan
        v[0, channel, -1, -1, -1] = np.nan
        v[0, channel, 0, -1, 0] = np.float32(THR)
    if cin > 1:
        v[0, (channel + 1) % cin] = 1.0
    return v


def _cases(image, cin=1, channel=0, noise=False):
    """name -> (volume, region mask or None, margin): the box placements."""
    n = tuple(image)
    q, h, far = [a // 4 for a in n], [a // 2 for a in n], [a - 1 for a in n]
    mask = np.zeros(n, dtype=np.uint8)
    mask[q[0]:q[0] + h[0], q[1]:q[1] + 2, far[2]] = 5            # thin in W, on the far D face
    mk = lambda **kw: _vol(image, cin, channel, noise=noise, **kw)   # noqa: E731
    return {
        "interior": (mk(lo=q, size=h), None, (0, 0, 0)),
        "thin": (mk(lo=q, size=(h[0], 2, h[2])), None, (0, 0, 0)),                 # thinner than the roi: widened
        "corner": (mk(lo=[a - 3 for a in n], size=(3, 3, 3)), None, (0, 0, 0)),    # widened and clamped
        "single": (mk(pts=[(h[0], far[1], 0)]), None, (0, 0, 0)),
        "faces": (mk(pts=[(0, 0, 0), far]), None, (0, 0, 0)),                      # touches all six faces: the full tiling
        "empty": (mk(), None, (0, 0, 0)),
        "margin": (mk(lo=(1, q[1], n[2] - 3), size=(3, 4, 2)), None, (4, 1, 5)),   # past the low H and the high D edge
        "nan": (mk(lo=q, size=h, nan=True), None, (0, 0, 0)),
        "mask": (mk(lo=(0, 0, 0), size=n), mask, (1, 1, 1)),                       # the volume is all foreground
    }


def _box(v, channel, mask):
    return box_of(foreground(mask=mask) if mask is not None else foreground(v[0], channel, THR))


def _predictor(image=IMAGE, roi=ROI, cin=1, fit=None, **kw):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    kw.setdefault("sub_batch", 7)
    return SlidingWindowPredictor(StandIn().to(DEV).eval(), image, cin, 3, roi, overlap=0.5, fit=fit, **kw)


def _fill_row(k, ncls=3):
    row = torch.full((ncls,), -k.fill_logit, dtype=torch.float32)
    row[k.fill_class] = k.fill_logit
    return row


def _crop(a, p):
    """[pdims] numpy array -> the image region."""
    return a[tuple(slice(q, q + n) for q, n in zip(p.pad, p.image_size))]


# -------------------------------------------------------------------------------------------------- 1. the box
@pytest.mark.parametrize("image,roi", SHAPES)
@pytest.mark.parametrize("cin,channel", [(1, 0), (4, 2)])
def test_foreground_box_equals_numpy(image, roi, cin, channel):
    from mivp_amd.inference import foreground_box
    seen = set()
    for name, (v, mask, _) in _cases(image, cin, channel).items():
        want = _box(v, channel, mask)
        x = torch.from_numpy(v).to(DEV)
        src = torch.from_numpy(mask).to(DEV) if mask is not None else x
        got = foreground_box(src, channel, THR)
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (6,)
        assert got.cpu().tolist() == want.tolist(), name
        if mask is None:                                         # the [C, H, W, D] form, into a given tensor
            out = torch.full((6,), 77, dtype=torch.int32, device=DEV)
            assert foreground_box(x[0], channel, THR, out=out) is out
            assert out.cpu().tolist() == want.tolist(), name
        seen.add(tuple(want.tolist()))
    assert tuple(list(image) + [-1, -1, -1]) in seen             # the empty encoding
    assert tuple([0, 0, 0] + [n - 1 for n in image]) in seen     # the whole volume
    assert len(seen) >= 7


# -------------------------------------------------------------------------------------------------- 2. the work list
@pytest.mark.parametrize("image,roi", SHAPES)
@pytest.mark.parametrize("mirror_axes,cin,channel", [((), 1, 0), ((0, 2), 4, 2)])
def test_fitted_table_and_meta_equal_numpy(image, roi, mirror_axes, cin, channel):
    from mivp_amd.inference import WindowFit, tta_table
    kept = {}
    for name, (v, mask, margin) in _cases(image, cin, channel).items():
        p = _predictor(image, roi, cin, WindowFit(channel=channel, margin=margin), mirror_axes=mirror_axes)
        if mask is not None:
            p.set_region(torch.from_numpy(mask).to(DEV))
        out = p.predict(torch.from_numpy(v).to(DEV))
        box = _box(v, channel, mask)
        o = fitted_origins(box, image, roi, 0.5, margin)
        table, meta = fitted_table(o, p.table.shape[0], p.flip_codes)
        assert p.box.cpu().tolist() == box.tolist(), name
        assert p.table.cpu().numpy().tolist() == table.tolist(), name
        assert p.meta.cpu().tolist() == meta.tolist(), name
        fo = p.fit_origins.cpu().numpy()
        assert fo[:o.shape[0]].tolist() == o.tolist() and not fo[o.shape[0]:].any(), name
        assert p.n_kept == o.shape[0] <= p.n_windows, name
        assert p.n_sub_run == -(-o.shape[0] * p.n_flips // p.sub_batch) <= p.n_sub, name
        full = tta_table(p.origins, p.sub_batch, p.flip_codes)
        assert p.table_full.cpu().numpy().tolist() == full.tolist()               # the full list is never written
        if name == "faces":
            assert table.tolist() == full.tolist()
        assert out["labels"].shape == (1, 1) + tuple(image)
        kept[name] = p.n_kept
    assert kept["empty"] == 0 and kept["single"] == 1 and kept["corner"] == 1
    assert kept["faces"] == p.n_windows and kept["interior"] < p.n_windows


# -------------------------------------------------------------------------------------------------- 3. the whole volume
@pytest.mark.parametrize("image,roi", SHAPES)
@pytest.mark.parametrize("mirror_axes", [(), (0, 2)])
def test_whole_volume_box_is_the_unfitted_prediction_bitwise(image, roi, mirror_axes):
    from mivp_amd.inference import WindowFit
    rand = torch.rand((1, 1) + tuple(image), device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    faces = torch.from_numpy(_cases(image, noise=True)["faces"][0]).to(DEV)
    ref_p = _predictor(image, roi, mirror_axes=mirror_axes)
    for x, k in ((rand, WindowFit(threshold=-1.0)), (faces, WindowFit()), (faces, WindowFit(margin=(2, 0, 40)))):
        ref = ref_p.predict(x, return_logits=True)
        p = _predictor(image, roi, fit=k, mirror_axes=mirror_axes)
        got = p.predict(x, return_logits=True)
        assert p.box.cpu().tolist() == [0, 0, 0] + [n - 1 for n in image]
        assert p.n_kept == p.n_windows and p.n_sub_run == p.n_sub
        assert torch.equal(p.table, p.table_full)
        assert torch.equal(got["logits"], ref["logits"]) and torch.equal(got["labels"], ref["labels"])


# -------------------------------------------------------------------------------------------------- 4. float64 average
def _stitch64_fitted(model, x, p, origins, k, mode):
    """float64 weighted average over the fitted windows, fill elsewhere -> [C, H, W, D]."""
    from mivp_amd.inference import importance_tables
    roi, pdims, pad, n = p.roi, p.pdims, p.pad, p.image_size
    xp = torch.zeros((1, x.shape[1]) + tuple(pdims), dtype=x.dtype, device=x.device)
    xp[:, :, pad[0]:pad[0] + n[0], pad[1]:pad[1] + n[1], pad[2]:pad[2] + n[2]] = x
    tabs, floor = importance_tables(roi, mode, 0.125)
    wmap = torch.from_numpy(np.maximum(tabs[0][:, None, None] * tabs[1][None, :, None] * tabs[2][None, None, :], floor))
    acc = torch.zeros((3,) + tuple(pdims), dtype=torch.float64)
    ws = torch.zeros(tuple(pdims), dtype=torch.float64)
    for a, b, c in origins.tolist():
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
@pytest.mark.parametrize("place", ["interior", "thin", "corner", "margin"])
@pytest.mark.parametrize("image,roi", [(IMAGE, ROI), PADDED])
def test_logits_match_float64_average_over_fitted_windows(image, roi, place, mode):
    """The bound is the one of test_hip_predict_skip.py::test_logits_match_float64_average_over_kept_windows (relative
    L2 error <= 1e-6, labels equal where the float64 margin exceeds 1e-5), here also over the covered voxels alone."""
    from mivp_amd.inference import WindowFit
    v, _, margin = _cases(image, noise=True)[place]
    k = WindowFit(margin=margin, fill_class=1, fill_logit=7.5)
    x = torch.from_numpy(v).to(DEV)
    p = _predictor(image, roi, fit=k, mode=mode, sub_batch=4)
    got = p.predict(x, return_logits=True)
    o = fitted_origins(_box(v, 0, None), image, roi, 0.5, margin)
    assert p.n_kept == o.shape[0] and 0 < p.n_kept < p.n_windows
    ref = _stitch64_fitted(p.model, x, p, o, k, mode)
    unc = torch.from_numpy(~_crop(covered(o, roi, p.pdims), p))
    assert 0 < int(unc.sum()) < unc.numel()
    gl = got["logits"][0].cpu()
    assert torch.equal(gl[:, unc], _fill_row(k)[:, None].expand(3, int(unc.sum())))        # exactly the fill row
    assert bool((got["labels"][0, 0].cpu()[unc] == k.fill_class).all())
    a, b = gl.double().reshape(-1), ref.reshape(-1)
    rel = float((a - b).norm() / b.norm())
    ac, bc = gl.double()[:, ~unc].reshape(-1), ref[:, ~unc].reshape(-1)
    rel_cov = float((ac - bc).norm() / bc.norm())
    print(f"{place} {mode} {image}: rel {rel:.3e}, covered only {rel_cov:.3e}")
    assert rel <= 1e-6, rel
    assert rel_cov <= 1e-6, rel_cov
    top2 = ref.topk(2, dim=0).values
    decided = (top2[0] - top2[1]) > 1e-5
    assert bool((got["labels"][0, 0].long().cpu()[decided] == ref.argmax(0)[decided]).all())
    assert float(decided.double().mean()) > 0.99


# -------------------------------------------------------------------------------------------------- 5. invariance
@pytest.mark.parametrize("mirror_axes", [(), (0, 2)])
def test_result_is_bitwise_independent_of_the_sub_batch(mirror_axes):
    from mivp_amd.inference import WindowFit
    x = torch.from_numpy(_cases(IMAGE, noise=True)["interior"][0]).to(DEV)
    runs, kept = [], set()
    for sb in (1, 7, 64):
        p = _predictor(fit=WindowFit(), mirror_axes=mirror_axes, sub_batch=sb)
        runs.append(p.predict(x, return_logits=True))
        kept.add(p.n_kept)
        assert p.n_sub_run == -(-p.n_kept * p.n_flips // sb)
    assert len(kept) == 1 and 1 < kept.pop() < p.n_windows
    for r in runs[1:]:
        assert torch.equal(r["logits"], runs[0]["logits"]) and torch.equal(r["labels"], runs[0]["labels"])


def test_graph_equals_eager_over_volumes_with_different_boxes():
    from mivp_amd.inference import WindowFit
    k = WindowFit(fill_class=2)
    cases = _cases(IMAGE, noise=True)
    eager, graph = _predictor(fit=k, sub_batch=3), _predictor(fit=k, sub_batch=3, graph=True)
    subs, tables, recorded = [], [], []
    for name in ("interior", "single", "faces"):
        x = torch.from_numpy(cases[name][0]).to(DEV)
        e, g = eager.predict(x, return_logits=True), graph.predict(x, return_logits=True)
        assert torch.equal(g["logits"], e["logits"]) and torch.equal(g["labels"], e["labels"]), name
        assert torch.equal(graph.table, eager.table) and torch.equal(graph.box, eager.box)
        assert graph.n_kept == eager.n_kept and graph.n_sub_run == eager.n_sub_run <= graph.n_sub
        subs.append(graph.n_sub_run)
        tables.append(graph.table.cpu().numpy().tolist())
        recorded.append(graph.graph)
    assert len(set(subs)) == 3 and subs[1] == 1 and subs[2] == graph.n_sub
    assert tables[0] != tables[1] != tables[2]
    assert recorded[0] is not None and recorded[1] is recorded[0] and recorded[2] is recorded[0]   # recorded once


def test_all_air_volume_runs_no_sub_batch_and_is_all_fill():
    from mivp_amd.inference import WindowFit
    k = WindowFit(fill_class=2, fill_logit=10.0)
    for graph in (False, True):
        p = _predictor(fit=k, graph=graph)
        out = p.predict(torch.zeros((1, 1) + IMAGE, device=DEV), return_logits=True, return_probs=True,
                        return_confidence=True, return_entropy=True)
        assert p.n_kept == 0 and p.n_sub_run == 0
        assert p.box.cpu().tolist() == list(IMAGE) + [-1, -1, -1]
        assert p.meta.cpu().tolist() == [0, 0] and not bool(p.table.any()) and not bool(p.fit_origins.any())
        assert bool((out["labels"] == 2).all())
        want = _fill_row(k).to(DEV)[None, :, None, None, None].expand_as(out["logits"])
        assert torch.equal(out["logits"], want)
        for name in ("probs", "confidence", "entropy"):
            assert bool(torch.isfinite(out[name]).all()), name
        assert float(out["confidence"].min()) > 0.99 and float(out["entropy"].max()) < 0.01
        assert torch.equal(out["probs"].argmax(1, keepdim=True), out["labels"].long())


# -------------------------------------------------------------------------------------------------- 6. evaluation, post-processing
def _counts(pl, tl):
    return torch.tensor([[int(((pl == c) & (tl == c)).sum()), int((pl == c).sum()), int((tl == c).sum())]
                         for c in range(3)], dtype=torch.int64)


def test_evaluate_counts_and_postprocess_agree_with_numpy():
    from mivp_amd.inference import WindowFit
    v = _cases(IMAGE, noise=True)["interior"][0]
    x = torch.from_numpy(v).to(DEV)
    seg = torch.from_numpy((v[:, :1] > 0.5).astype(np.float32)).to(DEV)
    p = _predictor(fit=WindowFit())
    iou, dice = p.evaluate(x, seg)
    assert 0 < p.n_kept < p.n_windows
    labels = p.predict(x)["labels"]
    tl = seg.reshape(-1).long().cpu()
    want = _counts(labels.reshape(-1).long().cpu(), tl)
    assert torch.equal(p.counts.cpu(), want)
    c = want.double()
    assert iou == pytest.approx(float((c[:, 0] / (c[:, 1] + c[:, 2] - c[:, 0] + 1e-6)).mean()), abs=1e-12)
    assert dice == pytest.approx(float((2 * c[:, 0] / (c[:, 1] + c[:, 2] + 1e-6)).mean()), abs=1e-12)
    # post-processing works on the fitted labels: the numpy restatement of tests/components_ref.py on them
    post = p.predict(x, postprocess={"largest": True})["labels"]
    ref = postprocess_ref(labels[0, 0].cpu().numpy(), 3, largest=True)
    assert post.dtype == torch.uint8 and post[0, 0].cpu().numpy().tolist() == ref.tolist()
    assert (ref != labels[0, 0].cpu().numpy()).any()             # it removed something
    p.evaluate(x, seg, postprocess={"largest": True})
    assert torch.equal(p.counts.cpu(), _counts(torch.from_numpy(ref.reshape(-1)).long(), tl))


# -------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_and_one_shot_helper():
    import mivp_amd
    from mivp_amd.inference import WindowFit, WindowSkip, foreground_box, predict_volume
    with pytest.raises(ValueError):
        _predictor().set_region(torch.zeros(IMAGE, dtype=torch.uint8, device=DEV))          # neither fit nor skip
    with pytest.raises(ValueError, match="fit and skip cannot be combined"):
        _predictor(fit=WindowFit(), skip=WindowSkip())
    p = _predictor(fit=WindowFit())
    for bad in (torch.zeros((4, 4, 4), dtype=torch.uint8, device=DEV), torch.zeros(IMAGE, dtype=torch.float32, device=DEV),
                torch.zeros(IMAGE, dtype=torch.bool, device=DEV), torch.zeros((1,) + IMAGE, dtype=torch.uint8, device=DEV),
                torch.zeros(IMAGE, dtype=torch.uint8), np.zeros(IMAGE, dtype=np.uint8),
                torch.zeros(IMAGE[:2] + (2 * IMAGE[2],), dtype=torch.uint8, device=DEV)[:, :, ::2]):
        with pytest.raises(ValueError):
            p.set_region(bad)
    p.set_region(torch.ones(IMAGE, dtype=torch.uint8, device=DEV))
    p.set_region(None)
    with pytest.raises(ValueError):
        _predictor(fit=WindowFit(channel=1))                     # a 1-channel volume
    with pytest.raises(ValueError):
        _predictor(fit=WindowFit(fill_class=3))                  # 3 classes
    with pytest.raises(ValueError):
        _predictor(fit=0.0025)
    vol = torch.zeros((1, 2) + IMAGE, device=DEV)
    for bad, kw in ((vol.double(), {}), (vol[0, 0], {}), (vol.expand(2, 2, *IMAGE), {}), (vol, dict(channel=2)),
                    (vol, dict(channel=-1)), (vol, dict(threshold=float("nan"))), (vol[:, :, :, :, ::2], {}),
                    (torch.zeros(IMAGE, dtype=torch.int32, device=DEV), {}),
                    (vol, dict(out=torch.zeros(6, dtype=torch.int64, device=DEV))),
                    (vol, dict(out=torch.zeros(5, dtype=torch.int32, device=DEV))),
                    (vol, dict(out=torch.zeros(6, dtype=torch.int32)))):
        with pytest.raises(ValueError):
            foreground_box(bad, **kw)
    # the one-shot helper passes fit through
    x = torch.from_numpy(_cases(IMAGE)["interior"][0]).to(DEV)
    k = WindowFit(fill_class=1, margin=2)
    out = predict_volume(StandIn().to(DEV), x, ROI, 3, sub_batch=7, fit=k)
    assert torch.equal(out["labels"], _predictor(fit=k).predict(x)["labels"])
    assert mivp_amd.WindowFit is WindowFit and mivp_amd.foreground_box is foreground_box
