"""GPU tests of the region statistics and lesion-wise metrics (mivp_amd.regions, csrc/regions.hip) against the numpy /
scipy restatement tests/regions_ref.py: integer fields bit for bit, derived float64 values at rtol 1e-12, float-image sums
within the bound of any float64 summation order, thresholds, min_size, repeatability, graph capture, the capacity flags
and the predictor's surface."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
scipy_ndimage = pytest.importorskip("scipy.ndimage")
import regions_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONN = (6, 18, 26)
SHAPES = [(1, 1, 1), (1, 17, 33), (37, 29, 23), (64, 64, 64), (160, 144, 120)]
MAX_REGIONS, MAX_PAIRS = 4096, 16384
INT_REGION = ("cls", "size", "first", "bbox", "coord_sum", "extent")
DERIVED_REGION = ("volume_mm3", "centroid", "centroid_mm")
INT_LESION = ("counts", "size", "valid", "overlap", "touching", "best_pred", "best_overlap", "detected", "matched", "pairs")
DERIVED_LESION = ("sensitivity", "precision", "f1", "lesion_dice", "best_iou", "dice_t")
U = 2.0 ** -53


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def lesion_map(rng, shape, density, ncls, sigma=2.0):
    """A lesion-like class map: smoothed noise above its (1 - density) quantile, the class from a second, smoother field
    (regions are neither single voxels nor one blob)."""
    if shape == (1, 1, 1):
        return np.ones(shape, dtype=np.uint8)
    f = scipy_ndimage.gaussian_filter(rng.standard_normal(shape), sigma, mode="nearest")
    g = scipy_ndimage.gaussian_filter(rng.standard_normal(shape), 2 * sigma, mode="nearest")
    fg = f > np.quantile(f, 1 - density)
    cls = 1 + (np.digitize(g, np.quantile(g, np.linspace(0, 1, ncls)[1:-1])) if ncls > 2 else 0)
    return (fg * cls).astype(np.uint8)


def _same_regions(got, want, image_float=False):
    assert got["n"] == want["n"] < MAX_REGIONS
    for k in INT_REGION:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in DERIVED_REGION:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    if "vsum" not in want:
        assert "vsum" not in got
        return
    assert got["vmin"].dtype == want["vmin"].dtype
    assert np.array_equal(got["vmin"], want["vmin"]) and np.array_equal(got["vmax"], want["vmax"])
    if not image_float:
        for k in ("vsum", "vsqsum"):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
        for k in ("vmean", "vstd"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    else:
        m = want["size"].astype(np.float64)
        assert got["vsum"].dtype == np.float64
        assert np.all(np.abs(got["vsum"] - want["vsum"]) <= m * U * want["_abs_sum"])
        assert np.all(np.abs(got["vsqsum"] - want["vsqsum"]) <= m * U * want["_sq_sum"])


def _same_report(got, want):
    assert len(want["pairs"]) < MAX_PAIRS
    _same_regions(got["pred_regions"], want["pred_regions"])
    _same_regions(got["target_regions"], want["target_regions"])
    for k in INT_LESION:
        assert np.array_equal(got[k], want[k]), k
    for k in DERIVED_LESION:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


# ------------------------------------------------------------------------------------------- 1. region_stats
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("density", [0.05, 0.3, 0.5])
@pytest.mark.parametrize("shape", SHAPES)
def test_region_stats_equal_reference(shape, density, conn):
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import region_stats
    rng = np.random.default_rng(abs(hash((shape, density, conn))) % 2 ** 32)
    x = lesion_map(rng, shape, density, 3)
    img = rng.integers(-1024, 3072, shape).astype(np.int16)
    sp = (0.8, 0.75, 2.5)
    tab = region_stats(_gpu(x), 3, image=_gpu(img), spacing=sp, connectivity=conn)
    want = R.region_stats(x, 3, img, sp, conn)
    _same_regions(tab.cpu(), want)
    assert np.array_equal(tab.labels.cpu().numpy(), want["labels"])
    assert int(tab.overflow) == 0


@pytest.mark.parametrize("shape", [(37, 29, 23), (96, 80, 72)])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64, torch.float32, torch.bool])
def test_region_stats_label_dtypes_and_classes(dtype, shape):
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import region_stats
    rng = np.random.default_rng(5)
    ncls = 2 if dtype == torch.bool else 4
    x = lesion_map(rng, shape, 0.3, ncls)
    t = _gpu(x, dtype).reshape((1, 1) + shape)
    _same_regions(region_stats(t, ncls, connectivity=18).cpu(), R.region_stats(x, ncls, connectivity=18))
    if ncls == 4:
        got = region_stats(t, ncls, classes=[3, 1]).cpu()
        _same_regions(got, R.region_stats(x, ncls, classes=[3, 1]))
        assert set(got["cls"].tolist()) <= {1, 3}
        if dtype == torch.float32:                         # values of no class are nobody's region
            y = x.astype(np.float32)
            y[x == 2] = 1.5
            y[0, 0, 0] = 7.0
            _same_regions(region_stats(_gpu(y), ncls).cpu(), R.region_stats(y, ncls))


@pytest.mark.parametrize("idtype", [np.int16, np.uint8, np.int32, np.float32])
def test_region_stats_image_dtypes(idtype):
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import region_stats
    rng = np.random.default_rng(6)
    shape = (64, 64, 64)
    x = lesion_map(rng, shape, 0.3, 3)
    if idtype == np.float32:
        img = (rng.standard_normal(shape) * 300 + 40).astype(np.float32)
    elif idtype == np.uint8:
        img = rng.integers(0, 256, shape).astype(np.uint8)
    elif idtype == np.int32:
        img = rng.integers(-2 ** 20, 2 ** 20, shape).astype(np.int32)
    else:
        img = rng.integers(-1024, 3072, shape).astype(np.int16)
    tab = region_stats(_gpu(x), 3, image=_gpu(img))
    want = R.region_stats(x, 3, img)
    got = tab.cpu()
    _same_regions(got, want, image_float=idtype == np.float32)
    if idtype == np.float32:
        # the sum's bound divided by the size, plus the rounding of the two divisions
        assert np.all(np.abs(got["vmean"] - want["vmean"]) <= U * want["_abs_sum"] + 2 * U * np.abs(want["vmean"]))


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("shape,density", [((160, 144, 120), 0.5), ((160, 144, 120), 0.05), ((37, 29, 23), 0.3)])
def test_region_stats_float_image_sums_and_deviation(shape, density, conn):
    """Float32 images where many workgroups add to the same region (the largest shape at density 0.5 has regions of
    10^5 voxels and more).  Bounds, with u = 2^-53, m = size, A = sum|x|, Q = sum x^2 (float64, from the restatement):
    |dsum| <= m u A and |dsq| <= m u Q (any summation order); dmean <= u A + 2 u |mean| (two rounded divisions);
    dvar <= u Q + 2 |mean| dmean + dmean^2 + 4 u (Q / m + mean^2) (the products, the subtraction and the division each
    round once); and |dstd| <= sqrt(dvar) because |sqrt a - sqrt b| <= sqrt|a - b|, plus one rounding of the root."""
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import region_stats
    rng = np.random.default_rng(abs(hash((shape, density, conn, 2))) % 2 ** 32)
    x = lesion_map(rng, shape, density, 3)
    img = (rng.standard_normal(shape) * 300 + 40).astype(np.float32)
    got = region_stats(_gpu(x), 3, image=_gpu(img), connectivity=conn).cpu()
    want = R.region_stats(x, 3, img, connectivity=conn)
    _same_regions(got, want, image_float=True)
    m, A, Q, mean = want["size"].astype(np.float64), want["_abs_sum"], want["_sq_sum"], np.abs(want["vmean"])
    dmean = U * A + 2 * U * mean
    assert np.all(np.abs(got["vmean"] - want["vmean"]) <= dmean)
    dvar = U * Q + 2 * mean * dmean + dmean * dmean + 4 * U * (Q / m + mean * mean)
    assert np.all(np.abs(got["vstd"] - want["vstd"]) <= np.sqrt(dvar) + U * want["vstd"])


def test_image_must_share_shape_dtype_and_device():
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import region_stats
    x = torch.zeros((8, 9, 10), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="spatial shape"):
        region_stats(x, 2, image=torch.zeros((8, 9, 11), dtype=torch.int16, device=DEV))
    with pytest.raises(ValueError, match="int16, uint8, int32 or float32"):
        region_stats(x, 2, image=torch.zeros((8, 9, 10), dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        region_stats(x, 2, image=torch.zeros((8, 9, 10), dtype=torch.int16))
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="is on"):
            region_stats(x, 2, image=torch.zeros((8, 9, 10), dtype=torch.int16, device="cuda:1"))


# ------------------------------------------------------------------------------------------- 2. lesion_metrics
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("density", [0.05, 0.3, 0.5])
@pytest.mark.parametrize("shape", SHAPES)
def test_lesion_metrics_equal_reference(shape, density, conn):
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics
    rng = np.random.default_rng(abs(hash((shape, density, conn, 1))) % 2 ** 32)
    p, t = lesion_map(rng, shape, density, 3), lesion_map(rng, shape, density, 3)
    rep = lesion_metrics(_gpu(p), _gpu(t), 3, spacing=(1.0, 1.0, 3.0), connectivity=conn)
    _same_report(rep.cpu(), R.lesion_metrics(p, t, 3, (1.0, 1.0, 3.0), conn))


@pytest.mark.parametrize("min_size", [0, 20])
@pytest.mark.parametrize("thr", [0.0, 0.1, 0.5])
def test_lesion_metrics_threshold_and_min_size(thr, min_size):
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics
    rng = np.random.default_rng(17)
    shape = (64, 64, 64)
    t = lesion_map(rng, shape, 0.1, 3)
    p = np.roll(t, (2, 1, 1), (0, 1, 2))                   # a shifted copy: every IoU is well between 0 and 1
    p[rng.random(shape) < 0.002] = 1                       # + speckle: small false alarms on both sides of min_size
    t = t.copy()
    t[rng.random(shape) < 0.002] = 2
    rep = lesion_metrics(_gpu(p, torch.int32), _gpu(t, torch.float32), 3, iou_threshold=thr, min_size=min_size)
    want = R.lesion_metrics(p, t, 3, iou_threshold=thr, min_size=min_size)
    _same_report(rep.cpu(), want)
    if min_size:
        sizes_p, sizes_t = want["pred_regions"]["size"], want["target_regions"]["size"]
        assert (sizes_p < min_size).any() and (sizes_t < min_size).any()            # it bites on both sides
        assert want["counts"][:, 0].sum() == (sizes_t >= min_size).sum()
        assert want["counts"][:, 1].sum() == (sizes_p >= min_size).sum()


def test_iou_of_exactly_one_half_and_ties():
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics
    t = np.zeros((4, 4, 40), dtype=np.uint8)
    p = np.zeros_like(t)
    t[0, 0, 0:6] = 1
    p[0, 0, 2:8] = 1                                       # 4 of 6 and 4 of 6 voxels: IoU = 4 / 8
    t[2, 2, 0:10] = 1
    p[2, 2, 0:2] = 1
    p[2, 2, 4:6] = 1                                       # a tie for best_pred
    for thr, det in ((0.5, [1, 0]), (0.0, [1, 1]), (0.51, [0, 0])):
        got = lesion_metrics(_gpu(p), _gpu(t), 2, iou_threshold=thr).cpu()
        _same_report(got, R.lesion_metrics(p, t, 2, iou_threshold=thr))
        assert got["detected"].tolist() == det and got["best_pred"].tolist() == [1, 2]
        assert got["best_iou"][0] == 0.5


def test_repeatability():
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics, region_stats
    rng = np.random.default_rng(23)
    shape = (96, 80, 64)
    p, t = _gpu(lesion_map(rng, shape, 0.3, 3)), _gpu(lesion_map(rng, shape, 0.3, 3))
    img = _gpu(rng.standard_normal(shape).astype(np.float32))
    a, b = lesion_metrics(p, t, 3).cpu(), lesion_metrics(p, t, 3).cpu()
    for k in INT_LESION + DERIVED_LESION:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    ra, rb = region_stats(p, 3, image=img).cpu(), region_stats(p, 3, image=img).cpu()
    for k in ra:
        if k not in ("vsum", "vsqsum", "vmean", "vstd"):     # the float-image sums: the one order-dependent pair
            assert np.array_equal(ra[k], rb[k]), k


def test_graph_capture():
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics, region_stats
    rng = np.random.default_rng(29)
    shape = (96, 80, 64)
    maps = [lesion_map(rng, shape, 0.2, 3) for _ in range(4)]
    imgs = [rng.integers(-1024, 3072, shape).astype(np.int16) for _ in range(2)]
    sp, st, si = _gpu(maps[0]), _gpu(maps[1]), _gpu(imgs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        region_stats(sp, 3, image=si)
        lesion_metrics(sp, st, 3, iou_threshold=0.1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tab = region_stats(sp, 3, image=si)
        rep = lesion_metrics(sp, st, 3, iou_threshold=0.1)
    for p, t, i in ((maps[2], maps[3], imgs[1]), (maps[0], maps[1], imgs[0])):
        sp.copy_(_gpu(p)); st.copy_(_gpu(t)); si.copy_(_gpu(i))
        g.replay()
        torch.cuda.synchronize()
        _same_regions(tab.cpu(), R.region_stats(p, 3, i))
        _same_report(rep.cpu(), R.lesion_metrics(p, t, 3, iou_threshold=0.1))
        eager = lesion_metrics(_gpu(p), _gpu(t), 3, iou_threshold=0.1).cpu()
        got = rep.cpu()
        for k in INT_LESION + DERIVED_LESION:
            assert np.array_equal(got[k], eager[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------- 3. capacity
def _checkerboard(shape):
    h, w, d = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return ((h + w + d) % 2).astype(np.uint8)


def test_region_overflow_is_flagged():
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics, region_stats
    x = _gpu(_checkerboard((48, 40, 32)))
    tab = region_stats(x, 2, connectivity=6, max_regions=64)
    assert int(tab.overflow) == 1 and int(tab.n) == 48 * 40 * 32 // 2
    with pytest.raises(RuntimeError, match=r"30720 components, capacity 64"):
        tab.cpu()
    assert np.array_equal(tab.size.cpu().numpy(), np.ones(64, dtype=np.int64))      # the listed ones are still right
    rep = lesion_metrics(x, x, 2, connectivity=6, max_regions=64)
    with pytest.raises(RuntimeError, match="capacity 64"):
        rep.cpu()
    ok = region_stats(x, 2, connectivity=26, max_regions=64)                       # 26-connected: one region, it fits
    assert ok.cpu()["n"] == 1 and int(ok.overflow) == 0


def test_pair_overflow_is_flagged():
    import mivp_amd  # noqa: F401
    from mivp_amd.regions import lesion_metrics
    x = _checkerboard((24, 20, 16))
    n = x.sum()
    assert 64 < n < MAX_REGIONS
    rep = lesion_metrics(_gpu(x), _gpu(x), 2, connectivity=6, max_pairs=64)
    assert int(rep.pair_overflow) == 1
    with pytest.raises(RuntimeError, match="more than 64 distinct"):
        rep.cpu()
    fits = lesion_metrics(_gpu(x), _gpu(x), 2, connectivity=6, max_pairs=int(n)).cpu()      # exactly at the capacity
    assert len(fits["pairs"]) == n and fits["counts"][1].tolist() == [n, n, n, n]


# ------------------------------------------------------------------------------------------- 4. the predictor
class StandIn(torch.nn.Module):
    """Element-wise functions of the first input channel (as in tests/test_hip_predict.py)."""

    K = ((1.7, 0.3), (-2.3, 0.9), (3.1, -1.4), (0.6, 0.1))

    def __init__(self, ncls=3):
        super().__init__()
        self.ncls = ncls
        self.anchor = torch.nn.Parameter(torch.zeros(1), requires_grad=False)

    def forward(self, x):
        x0 = x[:, 0]
        ch = [torch.tanh(x0 * k + b) + 0.25 * torch.sin(x0 * (3.0 + c)) for c, (k, b) in enumerate(self.K[:self.ncls])]
        return {"downstream": torch.stack(ch, dim=-1).permute(0, 4, 1, 2, 3)}


@pytest.mark.parametrize("graph", [False, True])
def test_predictor_lesions_and_regions(graph):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor, evaluate_volume_lesions
    from mivp_amd.regions import lesion_metrics
    ncls, image, roi = 3, (40, 28, 20), (16, 16, 8)
    rng = np.random.default_rng(31)
    field = scipy_ndimage.gaussian_filter(rng.standard_normal(image), 2.0)
    x = _gpu((field / field.std()).astype(np.float32)).reshape((1, 1) + image)
    seg = _gpu(lesion_map(rng, image, 0.3, ncls)).reshape((1, 1) + image)
    model = StandIn(ncls).to(DEV).eval()
    e = SlidingWindowPredictor(model, image, 1, ncls, roi, overlap=0.5, sub_batch=3, graph=graph)
    before = e.predict(x, return_confidence=True)
    assert set(before) == {"labels", "confidence"}                     # existing outputs are unchanged
    post = dict(largest=False, min_size=5)
    kw = dict(spacing=(0.8, 0.8, 2.5), iou_threshold=0.1, min_size=3, connectivity=18)
    for pp in (None, post):
        labels = e.predict(x, postprocess=pp)["labels"]
        want = lesion_metrics(labels, seg, ncls, **kw).cpu()
        assert want["pred_regions"]["n"] > 1
        got = e.evaluate_lesions(x, seg, postprocess=pp, **kw).cpu()
        for k in INT_LESION + DERIVED_LESION:
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        _same_report(got, R.lesion_metrics(labels[0, 0].cpu().numpy(), seg[0, 0].cpu().numpy(), ncls, **kw))
    one = evaluate_volume_lesions(model, x, seg, roi, ncls, sub_batch=3, graph=graph, postprocess=post, **kw).cpu()
    assert np.array_equal(one["counts"], got["counts"])
    out = e.predict_regions(x, return_confidence=True, spacing=(0.8, 0.8, 2.5))
    assert torch.equal(out["labels"], before["labels"]) and torch.equal(out["confidence"], before["confidence"])
    lab, conf = out["labels"][0, 0].cpu().numpy(), out["confidence"][0, 0].cpu().numpy()
    want = R.region_stats(lab, ncls, conf, (0.8, 0.8, 2.5))
    got = out["regions"].cpu()
    _same_regions(got, want, image_float=True)
    # the mean confidence per region: the sum's bound divided by the size, plus the rounding of the two divisions
    assert np.all(np.abs(got["vmean"] - want["vmean"]) <= U * want["_abs_sum"] + 2 * U * np.abs(want["vmean"]))
    assert "regions" in e.predict_regions(x) and e.predict_regions(x)["regions"].vsum is None
    with pytest.raises(ValueError, match="unknown"):
        e.evaluate_lesions(x, seg, bogus=1)
    with pytest.raises(ValueError, match="unknown"):
        e.predict_regions(x, bogus=1)
