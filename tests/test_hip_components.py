"""GPU tests of connected-component labelling and post-processing (mivp_amd.components, csrc/components.hip):
label_components against scipy.ndimage.label bit for bit (random masks, adversarial structures, multi-value maps),
postprocess_labels against the numpy / scipy restatement, run-to-run equality, graph capture, the predictor's
``postprocess`` keyword and the argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
scipy_ndimage = pytest.importorskip("scipy.ndimage")
import components_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONN = (6, 18, 26)


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _label(x, conn):
    from mivp_amd.components import label_components
    lab, n = label_components(x, conn)
    return lab.cpu().numpy(), n


def _check_mask(m, conn, dtype=torch.uint8):
    want, wn = scipy_ndimage.label(m, R.structure(conn))
    got, n = _label(_gpu(m.astype(np.uint8), dtype), conn)
    assert n == wn
    assert got.dtype == np.int32 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------- 1. random masks vs scipy
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("density", [0.05, 0.3, 0.5, 0.9])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 17, 33), (37, 29, 23), (64, 64, 64), (160, 144, 120)])
def test_label_random_masks_equal_scipy(shape, density, conn):
    import mivp_amd  # noqa: F401
    rng = np.random.default_rng(hash((shape, density, conn)) % 2 ** 32)
    _check_mask(rng.random(shape) < density, conn)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64, torch.float32, torch.bool])
@pytest.mark.parametrize("conn", CONN)
def test_label_input_dtypes(dtype, conn):
    import mivp_amd  # noqa: F401
    rng = np.random.default_rng(3)
    m = rng.random((37, 29, 23)) < 0.3
    _check_mask(m, conn, dtype)
    x = _gpu(m.astype(np.uint8), dtype).reshape(1, 1, 37, 29, 23)            # [1, 1, H, W, D] keeps its shape
    from mivp_amd.components import label_components
    lab, _ = label_components(x, conn)
    assert lab.shape == x.shape and lab.dtype == torch.int32


# ------------------------------------------------------------------------------------------- 2. adversarial structures
def serpentine(n):
    """A one-voxel-wide path through the whole n^3 cube (n even): a snake over rows w = 0, 2, ... in every even H plane,
    the planes joined through one voxel of the odd plane between them, at alternating ends."""
    plane = np.zeros((n, n), dtype=bool)
    plane[0::2, :] = True
    for i, w in enumerate(range(1, n - 1, 2)):
        plane[w, n - 1 if i % 2 == 0 else 0] = True
    end = (n - 2, n - 1 if (n // 2 - 1) % 2 == 0 else 0)
    a = np.zeros((n, n, n), dtype=bool)
    a[0::2] = plane
    for i, h in enumerate(range(1, n - 1, 2)):
        a[h][end if i % 2 == 0 else (0, 0)] = True
    return a


@pytest.mark.parametrize("conn", CONN)
def test_serpentine_is_one_component(conn):
    import mivp_amd  # noqa: F401
    m = serpentine(96)
    got, n = _label(_gpu(m.astype(np.uint8)), conn)
    assert n == 1
    assert np.array_equal(got, m.astype(np.int32))
    _check_mask(m, conn)


@pytest.mark.parametrize("conn", CONN)
def test_checkerboard(conn):
    import mivp_amd  # noqa: F401
    shape = (64, 48, 40)
    g = np.indices(shape).sum(0) % 2 == 0
    got, n = _label(_gpu(g.astype(np.uint8)), conn)
    assert n == (g.size // 2 if conn == 6 else 1)
    _check_mask(g, conn)


def test_all_foreground_and_empty():
    import mivp_amd  # noqa: F401
    for conn in CONN:
        got, n = _label(torch.ones((256, 256, 160), dtype=torch.uint8, device=DEV), conn)
        assert n == 1 and (got == 1).all()
        got, n = _label(torch.zeros((37, 29, 23), dtype=torch.float32, device=DEV), conn)
        assert n == 0 and not got.any()


@pytest.mark.parametrize("conn", CONN)
def test_lines_and_planes_across_tiles(conn):
    import mivp_amd  # noqa: F401
    shape = (37, 29, 41)
    for axis in range(3):
        line = np.zeros(shape, dtype=bool)
        idx = [slice(None) if a == axis else s // 2 + 1 for a, s in enumerate(shape)]
        line[tuple(idx)] = True
        _check_mask(line, conn)
        planes = np.zeros(shape, dtype=bool)
        for k in (0, 7, 8, 15, 16, shape[axis] - 1):
            sl = [slice(None)] * 3
            sl[axis] = k
            planes[tuple(sl)] = True
        _check_mask(planes, conn)


@pytest.mark.parametrize("conn", CONN)
def test_comb_joined_at_the_end(conn):
    import mivp_amd  # noqa: F401
    H, W, D = 24, 20, 36
    comb = np.zeros((H, W, D), dtype=bool)
    comb[:H - 1, 0::2, 0::2] = True                       # teeth along H, first voxels early in raster order
    comb[H - 1] = True                                    # the spine: the last plane
    _check_mask(comb, conn)
    rays = np.zeros((H, W, D), dtype=bool)                # three rays that meet only at the last voxel
    rays[:, W - 1, D - 1] = rays[H - 1, :, D - 1] = rays[H - 1, W - 1, :] = True
    got, n = _label(_gpu(rays.astype(np.uint8)), conn)
    assert n == 1
    _check_mask(rays, conn)


# ------------------------------------------------------------------------------------------- 3. multi-value maps
def blob_map(rng, shape, ncls, blobs=12, islands=40):
    lab = np.zeros(shape, dtype=np.int64)
    for _ in range(blobs):
        c = int(rng.integers(1, ncls))
        lo = [int(rng.integers(0, s)) for s in shape]
        hi = [min(s, lo_ + int(rng.integers(1, max(2, s // 3 + 1)))) for s, lo_ in zip(shape, lo)]
        lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = c
    for _ in range(islands):
        p = tuple(int(rng.integers(0, s)) for s in shape)
        lab[p] = int(rng.integers(1, ncls))
    return lab


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64, torch.float32])
@pytest.mark.parametrize("conn", CONN)
def test_multi_value_maps(dtype, conn):
    import mivp_amd  # noqa: F401
    rng = np.random.default_rng(5)
    x = blob_map(rng, (45, 38, 51), 5)
    x[rng.random(x.shape) < 0.05] = 3                     # speckle joining and splitting regions
    want, wn = R.label_by_value(x, conn)
    got, n = _label(_gpu(x, dtype), conn)
    assert n == wn and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------- 4. post-processing
POST = [dict(largest=True), dict(largest=False, min_size=20), dict(largest=True, min_size=50),
        dict(largest=True, classes=[2]), dict(largest=False, min_size=1, connectivity=6),
        dict(largest=True, connectivity=18)]


@pytest.mark.parametrize("kw", POST)
@pytest.mark.parametrize("ncls", [2, 4])
def test_postprocess_equals_restatement(ncls, kw):
    import mivp_amd  # noqa: F401
    from mivp_amd.components import postprocess_labels
    if "classes" in kw and ncls == 2:
        kw = dict(kw, classes=[1])
    rng = np.random.default_rng(ncls * 10 + len(kw))
    x = blob_map(rng, (70, 61, 53), ncls, blobs=16, islands=200)
    want = R.postprocess(x, ncls, **kw)
    for dtype in (torch.uint8, torch.int32, torch.int64, torch.float32):
        t = _gpu(x, dtype).reshape((1, 1) + x.shape)
        before = t.clone()
        out = postprocess_labels(t, ncls, **kw)
        assert out.dtype == dtype and out.shape == t.shape
        assert torch.equal(t, before)                       # the input is not modified
        assert np.array_equal(out[0, 0].cpu().numpy(), want.astype(out[0, 0].cpu().numpy().dtype))


def test_postprocess_bool_ties_and_untouched_values():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import postprocess_labels
    m = np.zeros((20, 18, 40), dtype=bool)
    m[2:5, 2:5, 1:4] = True
    m[2:5, 2:5, 30:33] = True                             # a tie: the first in raster order stays
    m[10, 10, 10] = True
    out = postprocess_labels(_gpu(m), 2)
    assert out.dtype == torch.bool
    assert np.array_equal(out.cpu().numpy(), R.postprocess(m, 2))
    f = np.zeros((20, 18, 40), dtype=np.float32)
    f[m] = 1.0
    f[0, 0, 0], f[19, 17, 39], f[5, 5, 5], f[6, 6, 6] = 1.5, 9.0, -2.0, np.nan
    out = postprocess_labels(_gpu(f), 3, min_size=2).cpu().numpy()
    want = R.postprocess(f, 3, min_size=2)
    assert np.array_equal(out, want, equal_nan=True)
    assert out[0, 0, 0] == 1.5 and out[19, 17, 39] == 9.0 and out[5, 5, 5] == -2.0 and np.isnan(out[6, 6, 6])


def test_large_two_class_map_exact():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import label_components, postprocess_labels
    rng = np.random.default_rng(11)
    x = blob_map(rng, (512, 512, 96), 2, blobs=20, islands=2000).astype(np.uint8)
    t = _gpu(x).reshape((1, 1) + x.shape)
    lab, n = label_components(t, 26)
    want, wn = scipy_ndimage.label(x, R.structure(26))
    assert n == wn and np.array_equal(lab[0, 0].cpu().numpy(), want)
    out = postprocess_labels(t, 2, largest=True, min_size=10)
    assert np.array_equal(out[0, 0].cpu().numpy(), R.postprocess(x, 2, largest=True, min_size=10))


def test_two_runs_are_bitwise_equal():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import label_components, postprocess_labels
    rng = np.random.default_rng(2)
    x = _gpu((rng.random((160, 128, 96)) < 0.3).astype(np.uint8))
    a, na = label_components(x, 26)
    b, nb = label_components(x, 26)
    assert na == nb and torch.equal(a, b)
    y = _gpu(blob_map(rng, (160, 128, 96), 4, islands=500))
    assert torch.equal(postprocess_labels(y, 4, min_size=8), postprocess_labels(y, 4, min_size=8))


def test_postprocess_in_a_graph_equals_eager():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import postprocess_labels
    rng = np.random.default_rng(4)
    shape = (96, 80, 64)
    x1 = _gpu(blob_map(rng, shape, 3, islands=300).astype(np.uint8))
    x2 = _gpu(blob_map(rng, shape, 3, islands=300).astype(np.uint8))
    static = x1.clone()
    kw = dict(largest=True, min_size=4, connectivity=26)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        postprocess_labels(static, 3, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = postprocess_labels(static, 3, **kw)
    for x in (x2, x1):
        static.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, postprocess_labels(x, 3, **kw))


# ------------------------------------------------------------------------------------------- 5. the predictor hook
def _tiny_model(seed=4):
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, _, _ = train.make_conf("tiny")
    torch.manual_seed(seed)
    return SwinUnetR(conf).to(DEV).eval()


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


def _iou_dice(labels, seg, ncls):
    p, t = labels.reshape(-1).long().cpu(), seg.reshape(-1).long().cpu()
    c = torch.zeros((ncls, 3), dtype=torch.float64)
    for k in range(ncls):
        c[k] = torch.tensor([((p == k) & (t == k)).sum(), (p == k).sum(), (t == k).sum()], dtype=torch.float64)
    inter, psum, tsum = c[:, 0], c[:, 1], c[:, 2]
    return float((inter / (psum + tsum - inter + 1e-6)).mean()), float((2 * inter / (psum + tsum + 1e-6)).mean())


def test_predict_with_postprocess_tiny_model_eager_and_graph():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import postprocess_labels
    from mivp_amd.inference import SlidingWindowPredictor, evaluate_volume, predict_volume
    model = _tiny_model()
    g = torch.Generator().manual_seed(7)
    x = torch.rand(1, 1, 56, 48, 40, generator=g).to(DEV)
    seg = torch.randint(0, 2, (1, 1, 56, 48, 40), generator=g).float().to(DEV)
    roi = (32, 32, 32)
    post = dict(largest=True, min_size=3)
    e = SlidingWindowPredictor(model, x.shape[2:], 1, 2, roi, sub_batch=5)
    plain = e.predict(x, return_logits=True)
    want = postprocess_labels(plain["labels"], 2, **post)
    got = e.predict(x, return_logits=True, postprocess=post)
    assert torch.equal(got["labels"], want) and got["labels"].dtype == torch.uint8
    assert torch.equal(got["logits"], plain["logits"])   # the logits stay those before post-processing
    assert e.evaluate(x, seg, postprocess=post) == _iou_dice(want, seg, 2)
    assert e.evaluate(x, seg) == _iou_dice(plain["labels"], seg, 2)          # without the keyword: as before
    gp = SlidingWindowPredictor(model, x.shape[2:], 1, 2, roi, sub_batch=5, graph=True)
    for _ in range(2):                                                        # recording run, then a replay
        assert torch.equal(gp.predict(x, postprocess=post)["labels"], want)
    assert torch.equal(predict_volume(model, x, roi, 2, sub_batch=5, postprocess=post)["labels"], want)
    assert evaluate_volume(model, x, seg, roi, 2, sub_batch=5, postprocess=post) == _iou_dice(want, seg, 2)


def test_evaluate_surface_with_postprocess():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import postprocess_labels
    from mivp_amd.inference import SlidingWindowPredictor, evaluate_volume_surface
    from mivp_amd.surface import surface_metrics
    ncls, image, roi = 3, (40, 28, 20), (16, 16, 8)
    g = torch.Generator().manual_seed(11)
    x = (torch.rand((1, 1) + image, generator=g) * 2 - 1).to(DEV)      # noisy: many islands
    seg = torch.randint(0, ncls, (1, 1) + tuple(s // 4 for s in image), generator=g)
    seg = torch.nn.functional.interpolate(seg.float(), size=image, mode="nearest").to(DEV)
    model = StandIn(ncls).to(DEV).eval()
    post = dict(largest=True, connectivity=6)
    kw = dict(spacing=(0.8, 0.8, 2.5), percentile=95.0, tolerance=2.7)
    e = SlidingWindowPredictor(model, image, 1, ncls, roi, overlap=0.5, sub_batch=3)
    plain = e.predict(x)["labels"]
    labels = postprocess_labels(plain, ncls, **post)
    assert not torch.equal(labels, plain)                 # the noisy input leaves islands to remove
    want = surface_metrics(labels, seg, ncls, **kw)
    for pred in (e, SlidingWindowPredictor(model, image, 1, ncls, roi, overlap=0.5, sub_batch=3, graph=True)):
        got = pred.evaluate_surface(x, seg, postprocess=post, **kw)
        for k in ("hd", "hd_p", "assd", "nsd", "surface_voxels"):
            assert np.array_equal(got[k].numpy(), want[k].numpy(), equal_nan=True), k
        assert (got["iou"], got["dice"]) == _iou_dice(labels, seg, ncls)
    one = evaluate_volume_surface(model, x, seg, roi, ncls, sub_batch=3, postprocess=post, **kw)
    assert np.array_equal(one["hd_p"].numpy(), want["hd_p"].numpy(), equal_nan=True)


# ------------------------------------------------------------------------------------------- 6. argument checks
def test_refuses_bad_arguments_on_the_gpu_path():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import label_components, postprocess_labels
    from mivp_amd.inference import SlidingWindowPredictor
    a = torch.zeros((1, 1, 8, 9, 10), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="GPU"):
        label_components(a.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        postprocess_labels(a.cpu(), 2)
    for bad in (a[0], a[0, 0, 0], torch.zeros((2, 1, 8, 9, 10), device=DEV), torch.zeros((1, 2, 8, 9, 10), device=DEV)):
        with pytest.raises(ValueError):
            label_components(bad)
        with pytest.raises(ValueError):
            postprocess_labels(bad, 2)
    with pytest.raises(ValueError):
        label_components(a, 8)
    with pytest.raises(ValueError):
        postprocess_labels(a, 2, largest=False)
    with pytest.raises(ValueError):
        postprocess_labels(a, 2, classes=[2])
    model = StandIn(2).to(DEV).eval()
    p = SlidingWindowPredictor(model, (8, 9, 10), 1, 2, (8, 8, 8), sub_batch=2)
    x = torch.rand((1, 1, 8, 9, 10), device=DEV)
    for bad in ({"largest": False}, {"classes": [2]}, {"num_classes": 3}, {"bogus": 1}, "largest"):
        with pytest.raises(ValueError):
            p.predict(x, postprocess=bad)
        with pytest.raises(ValueError):
            p.evaluate(x, a.float(), postprocess=bad)
