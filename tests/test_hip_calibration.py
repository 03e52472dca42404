"""GPU tests of the calibration tables (mivp_amd.calibration, csrc/calibration.hip) and of the lesion scores / FROC of
mivp_amd.regions against the numpy restatement tests/calibration_ref.py, with the conventions of test_hip_regions.py:
integer tables bit for bit, derived float64 values at rtol 1e-12, no voxel and no case excluded."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 1), (3, 5, 7), (9, 8, 4), (33, 17, 9), (64, 64, 40)]
FIELDS = ["spread", "saturated", "uniform", "onehot", "edges"]
# every shape x field at (2, 10) (+ the bin-edge field at its own n_bins = 64); the other pairs on two shapes each
OTHER = [(1, 1), (3, 15), (5, 64), (16, 1024), (2, 1024)]
OTHER_SHAPES = [(3, 5, 7), (64, 64, 40)]


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def case(field, shape, ncls, tdtype="uint8", seed=0):
    """(probs float32 [C, H, W, D], target) of one test case, numpy, made once and left unchanged."""
    rng = np.random.default_rng([FIELDS.index(field), ncls, seed, *shape])
    nvox = int(np.prod(shape))
    full = (ncls,) + shape
    if field in ("spread", "saturated"):
        # base logits of deviation 4; x 8 their differences pass the 103 where a float32 exp underflows to zero
        z = torch.from_numpy((4.0 * rng.standard_normal(full)).astype(np.float32)) * (0.5 if field == "spread" else 8.0)
        p = torch.softmax(z, 0).numpy()
        if field == "saturated" and nvox >= 1000:
            assert (p == 1.0).any() and (ncls == 1 or (p == 0.0).any())
    elif field == "uniform":
        p = np.full(full, np.float32(1.0) / np.float32(ncls), dtype=np.float32)
    elif field == "onehot":
        p = (rng.integers(0, ncls, shape)[None] == np.arange(ncls).reshape((-1, 1, 1, 1))).astype(np.float32)
    else:                                                    # exactly on the bin edges k / 64
        k = rng.integers(0, 65, shape)
        p = np.zeros(full, dtype=np.float32)
        p[0] = k / np.float32(64)
        if ncls > 1:
            p[1] = (64 - k) / np.float32(64)
    t = rng.integers(0, max(ncls - 1, 1), shape)            # the last class is absent from the reference
    if nvox >= 8:
        t[rng.random(shape) < 0.05] = 255
        for plane, value in ((0, np.nan), (ncls - 1, -0.1), (ncls // 2, 1.5)):
            p[plane][rng.random(shape) < 0.01] = value
    p.setflags(write=False)
    t = t.astype(tdtype)
    t.setflags(write=False)
    return p, t


@functools.lru_cache(maxsize=None)
def reference(field, shape, ncls, n_bins, tdtype="uint8", seed=0):
    p, t = case(field, shape, ncls, tdtype, seed)
    return CR.calibration(p, t, ncls, n_bins)


def _same(got, want, what=""):
    for k in CR.INT_FIELDS:
        assert np.asarray(got[k]).dtype == np.int64 or isinstance(got[k], int), k
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in CR.DERIVED:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=f"{what} {k}")


def _run(field, shape, ncls, n_bins, tdtype="uint8", **kw):
    from mivp_amd.calibration import calibration_tables
    p, t = case(field, shape, ncls, tdtype)
    return calibration_tables(_gpu(p), _gpu(t), ncls, n_bins, **kw)


# ------------------------------------------------------------------------------------------- 1. the tables
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_equal_reference(shape, field):
    import mivp_amd  # noqa: F401
    tdtype = "int64" if (SHAPES.index(shape) + FIELDS.index(field)) % 2 else "uint8"
    rep = _run(field, shape, 2, 10, tdtype)
    want = reference(field, shape, 2, 10, tdtype)
    _same(rep.cpu(), want, f"{field} {shape}")
    if int(np.prod(shape)) >= 1000:
        assert want["n_ignored"] > 0 and want["n_invalid"] > 0 and want["n_pos"][1] == 0
        assert np.isnan(want["roc_auc"][1]) and np.isnan(want["average_precision"][1])
    if field == "edges":
        _same(_run(field, shape, 2, 64, tdtype).cpu(), reference(field, shape, 2, 64, tdtype), f"{field} {shape} 64")


@pytest.mark.parametrize("field", ["spread", "saturated", "uniform"])
@pytest.mark.parametrize("shape", OTHER_SHAPES)
@pytest.mark.parametrize("ncls,n_bins", OTHER)
def test_other_class_and_bin_counts(ncls, n_bins, shape, field):
    """(16, 1024) has more cells than a workgroup keeps in LDS and adds in global memory; (2, 1024) fills the LDS table."""
    import mivp_amd  # noqa: F401
    tdtype = "int64" if field == "saturated" else "uint8"
    _same(_run(field, shape, ncls, n_bins, tdtype).cpu(), reference(field, shape, ncls, n_bins, tdtype),
          f"{field} {shape} {ncls} {n_bins}")


def test_layouts_dtypes_and_combine_path():
    import mivp_amd  # noqa: F401
    from mivp_amd.calibration import FLAG_COMBINE, calibration_tables
    shape = (33, 17, 9)
    p, t = case("saturated", shape, 3)
    want = reference("saturated", shape, 3, 15)
    gp = _gpu(p)
    for tt in (_gpu(t), _gpu(t, torch.int32), _gpu(t, torch.int64), _gpu(t, torch.float32), _gpu(t).reshape((1, 1) + shape)):
        _same(calibration_tables(gp, tt, 3, 15).cpu(), want, str(tt.dtype))
    _same(calibration_tables(gp[None], _gpu(t), 3, 15).cpu(), want, "5-d probs")
    _same(calibration_tables(gp, _gpu(t), 3, 15, flags=FLAG_COMBINE).cpu(), want, "combine")
    big = case("saturated", (64, 64, 40), 2)
    _same(calibration_tables(_gpu(big[0]), _gpu(big[1]), 2, 10, flags=FLAG_COMBINE).cpu(),
          reference("saturated", (64, 64, 40), 2, 10), "combine, vector loads")
    wide = case("saturated", (64, 64, 40), 16, "int64")
    _same(calibration_tables(_gpu(wide[0]), _gpu(wide[1]), 16, 1024, flags=FLAG_COMBINE).cpu(),
          reference("saturated", (64, 64, 40), 16, 1024, "int64"), "combine, global cells")
    off = torch.zeros(p.size + 1, dtype=torch.float32, device=DEV)[1:].view(p.shape)       # 4-byte aligned only
    off.copy_(gp)
    _same(calibration_tables(off, _gpu(t), 3, 15).cpu(), want, "unaligned")


def test_two_runs_are_bitwise_equal():
    import mivp_amd  # noqa: F401
    for field, ncls, n_bins in (("spread", 2, 10), ("saturated", 16, 1024)):
        a, b = _run(field, (64, 64, 40), ncls, n_bins), _run(field, (64, 64, 40), ncls, n_bins)
        assert torch.equal(a.tables, b.tables)
        ca, cb = a.cpu(), b.cpu()
        for k in CR.DERIVED:
            assert np.array_equal(ca[k], cb[k], equal_nan=True), k


def test_out_accumulates_like_the_concatenation():
    import mivp_amd  # noqa: F401
    from mivp_amd.calibration import CalibrationReport, calibration_tables
    (p1, t1), (p2, t2) = case("spread", (9, 8, 4), 3), case("saturated", (33, 8, 4), 3, seed=1)
    rep = calibration_tables(_gpu(p1), _gpu(t1), 3, 15)
    again = calibration_tables(_gpu(p2), _gpu(t2), 3, 15, out=rep)
    assert again is rep
    _same(rep.cpu(), CR.calibration(np.concatenate([p1, p2], 1), np.concatenate([t1, t2], 0), 3, 15))
    with pytest.raises(ValueError, match="out was made for"):
        calibration_tables(_gpu(p1), _gpu(t1), 3, 15, out=CalibrationReport(3, 10, DEV))


def test_graph_replay_adds_the_tables_again():
    import mivp_amd  # noqa: F401
    from mivp_amd.calibration import CalibrationReport, calibration_tables
    shape = (64, 64, 40)
    p, t = case("saturated", shape, 2)
    gp, gt = _gpu(p), _gpu(t)
    out = CalibrationReport(2, 10, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calibration_tables(gp, gt, 2, 10, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calibration_tables(gp, gt, 2, 10, out=out)
    out.zero_()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    got, want = out.cpu(), reference("saturated", shape, 2, 10)
    for k in CR.INT_FIELDS:
        assert np.array_equal(got[k], 2 * np.asarray(want[k])), k


# ------------------------------------------------------------------------------------------- 2. lesion scores and FROC
scipy_ndimage = pytest.importorskip("scipy.ndimage")
import regions_ref as R  # noqa: E402
from test_hip_regions import DERIVED_LESION, INT_LESION, StandIn, _same_report, lesion_map  # noqa: E402

FROC_FLOAT = ("sensitivity", "precision", "average_precision")


def _image(rng, shape):
    """A smooth confidence-like float32 image on a grid of 1 / 32: lesion scores differ, and some tie."""
    f = scipy_ndimage.gaussian_filter(rng.standard_normal(shape), 3.0, mode="nearest")
    f = (f - f.min()) / (f.max() - f.min())
    return (np.floor(f * 16 + 16) / 32).astype(np.float32)


def _same_scores(got, want):
    for k in INT_LESION:
        assert np.array_equal(got[k], want[k]), k
    for k in DERIVED_LESION:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    for k in ("score", "best_score"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["pred_regions"]["vmax"], want["pred_regions"]["vmax"])
    gf, wf = got["froc"], want["froc"]
    assert np.array_equal(gf["n_thresholds"], wf["n_thresholds"]) and np.array_equal(gf["fp"], wf["fp"])
    assert gf["thresholds"].dtype == np.float32 and np.array_equal(gf["thresholds"], wf["thresholds"], equal_nan=True)
    for k in FROC_FLOAT:
        np.testing.assert_allclose(gf[k], wf[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    np.testing.assert_allclose(got["froc_score"], want["froc_score"], rtol=1e-12, atol=0, equal_nan=True)


@pytest.mark.parametrize("min_size", [0, 5])
@pytest.mark.parametrize("thr", [0.0, 0.3])
@pytest.mark.parametrize("ncls", [2, 3])
@pytest.mark.parametrize("shape", [(37, 29, 23), (64, 64, 64)])
def test_lesion_scores_and_froc_equal_reference(shape, ncls, thr, min_size):
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics, lesion_score_metrics
    rng = np.random.default_rng(abs(hash((shape, ncls))) % 2 ** 32)
    t = lesion_map(rng, shape, 0.1, ncls)
    p = np.roll(t, (2, 1, 1), (0, 1, 2))
    p[rng.random(shape) < 0.0003] = 1                      # a few small false alarms, below min_size = 5
    img = _image(rng, shape)
    gp, gt = _gpu(p), _gpu(t)
    legacy = lesion_metrics(gp, gt, ncls, iou_threshold=thr, min_size=min_size)
    none = lesion_score_metrics(gp, gt, ncls, None, iou_threshold=thr, min_size=min_size)
    assert none.score is None and torch.equal(none.counts, legacy.counts) and torch.equal(none.matched, legacy.matched)
    assert legacy.score is None and legacy.best_score is None
    got = legacy.cpu()
    _same_report(got, R.lesion_metrics(p, t, ncls, iou_threshold=thr, min_size=min_size))
    assert set(got) == set(INT_LESION) | set(DERIVED_LESION) | {"pred_regions", "target_regions"}     # today's report
    with pytest.raises(RuntimeError, match="without pred_image"):
        legacy.froc()
    rep = lesion_score_metrics(gp, gt, ncls, _gpu(img), iou_threshold=thr, min_size=min_size)
    want = CR.lesion_scores(p, t, img, ncls, iou_threshold=thr, min_size=min_size)
    assert want["froc"]["n_thresholds"].max() > 1 and (thr > 0 or np.isfinite(want["best_score"]).any())
    _same_scores(rep.cpu(), want)
    again = lesion_score_metrics(gp, gt, ncls, _gpu(img), iou_threshold=thr, min_size=min_size).cpu()
    assert np.array_equal(again["best_score"], rep.cpu()["best_score"])


@pytest.mark.parametrize("empty", ["pred", "target"])
def test_froc_without_predictions_or_reference(empty):
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics, lesion_score_metrics
    rng = np.random.default_rng(3)
    shape = (37, 29, 23)
    full, none = lesion_map(rng, shape, 0.1, 3), np.zeros(shape, dtype=np.uint8)
    p, t = (none, full) if empty == "pred" else (full, none)
    img = _image(rng, shape)
    got = lesion_score_metrics(_gpu(p), _gpu(t), 3, _gpu(img)).cpu()
    want = CR.lesion_scores(p, t, img, 3)
    _same_scores(got, want)
    if empty == "pred":
        assert got["froc"]["thresholds"].shape == (3, 0) and np.all(got["best_score"] == -np.inf)
        assert got["froc_score"][1:].tolist() == [0.0, 0.0] and got["froc"]["average_precision"][1:].tolist() == [0.0, 0.0]
    else:
        assert np.isnan(got["froc_score"]).all() and got["best_score"].size == 0


def test_pred_image_must_be_float32():
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics, lesion_score_metrics
    x = torch.zeros((8, 9, 10), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="float32"):
        lesion_score_metrics(x, x, 2, torch.zeros((8, 9, 10), dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError, match="spatial shape"):
        lesion_score_metrics(x, x, 2, torch.zeros((8, 9, 11), dtype=torch.float32, device=DEV))


# ------------------------------------------------------------------------------------------- 3. the predictor
def test_predictor_calibration_and_lesion_scores():
    import mivp_amd  # noqa: F401
    from mivp_amd.calibration import calibration_tables
    from mivp_amd.inference import SlidingWindowPredictor, evaluate_volume_calibration
    from mivp_amd.regions import lesion_metrics, lesion_score_metrics
    ncls, image, roi = 3, (40, 28, 20), (16, 16, 8)
    rng = np.random.default_rng(31)
    field = scipy_ndimage.gaussian_filter(rng.standard_normal(image), 2.0)
    x = _gpu((field / field.std()).astype(np.float32)).reshape((1, 1) + image)
    seg = _gpu(lesion_map(rng, image, 0.3, ncls)).reshape((1, 1) + image)
    model = StandIn(ncls).to(DEV).eval()
    kw = dict(iou_threshold=0.1, min_size=3, connectivity=18)
    results = []
    for graph in (False, True):
        e = SlidingWindowPredictor(model, image, 1, ncls, roi, overlap=0.5, sub_batch=3, graph=graph)
        pred = e.predict(x, return_probs=True, return_confidence=True)
        want = calibration_tables(pred["probs"], seg, ncls, 15)
        got = e.evaluate_calibration(x, seg)
        assert torch.equal(got.tables, want.tables) and int(got.n[0]) == int(np.prod(image))
        _same(got.cpu(), CR.calibration(pred["probs"][0].cpu().numpy(), seg[0, 0].cpu().numpy(), ncls, 15))
        pooled = e.evaluate_calibration(x, seg, n_bins=10, out=e.evaluate_calibration(x, seg, n_bins=10))
        assert torch.equal(pooled.tables, 2 * calibration_tables(pred["probs"], seg, ncls, 10).tables)
        one = evaluate_volume_calibration(model, x, seg, roi, ncls, sub_batch=3, graph=graph)
        assert torch.equal(one.tables, want.tables)
        lw = lesion_score_metrics(pred["labels"], seg, ncls, pred["confidence"], **kw).cpu()
        lg = e.evaluate_lesions(x, seg, with_scores=True, **kw).cpu()
        assert lw["pred_regions"]["n"] > 1 and lg["froc"]["n_thresholds"].max() > 1
        for k in INT_LESION + DERIVED_LESION + ("score", "best_score", "froc_score"):
            assert np.array_equal(lg[k], lw[k], equal_nan=True), k
        for k in lw["froc"]:
            assert np.array_equal(lg["froc"][k], lw["froc"][k], equal_nan=True), k
        assert "score" not in e.evaluate_lesions(x, seg, **kw).cpu()
        results.append((got.tables.clone(), lg))
    assert torch.equal(results[0][0], results[1][0])                   # graph and eager: bitwise equal
    for k in ("score", "best_score", "froc_score"):
        assert np.array_equal(results[0][1][k], results[1][1][k], equal_nan=True), k
