"""GPU tests of the surface-distance metrics (mivp_amd.surface, csrc/surface.hip): the surface map against the numpy
restatement and scipy's erosion, the exact squared EDT against scipy, the metrics against the brute-force restatement
and scipy, the empty-class rules, run-to-run bitwise equality, SlidingWindowPredictor.evaluate_surface and the argument
checks."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ANISO = (0.8, 0.8, 2.5)


def _blobs(rng, shape, ncls, blobs=5):
    lab = np.zeros(shape, dtype=np.int64)
    for _ in range(blobs):
        c = int(rng.integers(1, ncls))
        lo = [int(rng.integers(0, s)) for s in shape]
        hi = [min(s, l + int(rng.integers(1, max(2, s // 2 + 1)))) for s, l in zip(shape, lo)]
        lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = c
    return lab


def _gpu(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).reshape((1, 1) + a.shape).to(DEV)


def _np(res):
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def _tau_is_valid(tau, spacing, shape):
    """tau is at least 1e-3 away from every distance two voxels of the volume can have."""
    s = np.asarray(spacing, dtype=np.float64)
    g = np.meshgrid(*[np.arange(n) * si for n, si in zip(shape, s)], indexing="ij")
    d = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
    return float(np.abs(d - tau).min()) >= 1e-3


# -------------------------------------------------------------------------------------------------- (a) surface map
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64, torch.float32])
@pytest.mark.parametrize("shape,ncls", [((37, 23, 19), 5), ((20, 16, 13), 2), ((15, 1, 9), 3), ((1, 12, 10), 4),
                                        ((9, 7, 70), 3)])
def test_surface_map_equals_restatement_and_scipy(shape, ncls, dtype):
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import surface_map, surface_metrics
    rng = np.random.default_rng(sum(shape) + ncls)
    lab = _blobs(rng, shape, ncls)
    lab.reshape(-1)[rng.integers(0, lab.size, 5)] = ncls + 1           # out of range: no class
    if dtype != torch.uint8:
        lab.reshape(-1)[rng.integers(0, lab.size, 3)] = -1
    want, counts = R.surface_map(lab, ncls)
    got = surface_map(_gpu(lab, dtype), ncls)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 1) + shape
    assert np.array_equal(got.cpu().numpy()[0, 0], want)
    if _has_scipy():
        for c in range(ncls):
            assert np.array_equal(want == c, R.scipy_surface(lab == c))
    res = surface_metrics(_gpu(lab, dtype), _gpu(lab[::-1].copy(), dtype), ncls)
    assert res["surface_voxels"][:, 0].tolist() == counts.tolist()
    assert res["surface_voxels"][:, 1].tolist() == R.surface_map(lab[::-1], ncls)[1].tolist()


def test_surface_map_float_non_integers_belong_to_no_class():
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import surface_map
    lab = np.ones((6, 7, 8), dtype=np.float32)
    lab[2:4, 2:5, 2:6] = 1.5
    want, _ = R.surface_map(lab, 3)
    assert np.array_equal(surface_map(_gpu(lab, torch.float32), 3).cpu().numpy()[0, 0], want)


def _has_scipy():
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except ImportError:
        return False


# -------------------------------------------------------------------------------------------------- (b) EDT
def _edt_cases():
    rng = np.random.default_rng(3)
    corner = np.zeros((40, 30, 20), dtype=bool)
    corner[0, 0, 0] = True
    far = np.zeros((17, 9, 23), dtype=bool)
    far[16, 8, 22] = True
    full = np.ones((11, 7, 5), dtype=bool)
    line = rng.random((512, 3, 5)) < 0.01
    line[0, 0, 0] = True
    rand96 = rng.random((96, 96, 96)) < 0.0005
    longd = np.zeros((7, 5, 200), dtype=bool)                           # several 64-voxel steps along D, sparse seeds
    longd[3, 2, 150] = longd[0, 0, 5] = longd[6, 4, 199] = True
    return {"corner": corner, "far_corner": far, "all_seeds": full, "line_512x3x5": line, "random_96": rand96,
            "long_d": longd}


@pytest.mark.parametrize("name", list(_edt_cases()))
def test_edt_unit_spacing_is_exact(name):
    ndi = pytest.importorskip("scipy.ndimage")
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import distance_transform_sq
    seeds = _edt_cases()[name]
    assert seeds.any()
    want = np.rint(ndi.distance_transform_edt(~seeds) ** 2).astype(np.float32)
    got = distance_transform_sq(torch.from_numpy(seeds).to(DEV)).cpu().numpy()
    assert got.dtype == np.float32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("name", ["corner", "line_512x3x5", "random_96", "long_d"])
def test_edt_anisotropic_spacing(name):
    ndi = pytest.importorskip("scipy.ndimage")
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import distance_transform_sq
    seeds = _edt_cases()[name]
    want = ndi.distance_transform_edt(~seeds, sampling=ANISO) ** 2
    got = distance_transform_sq(torch.from_numpy(seeds).to(DEV), ANISO).cpu().numpy().astype(np.float64)
    err = np.abs(got - want) / np.maximum(want, 1e-30)
    assert float(err[want > 0].max()) <= 1e-5
    assert np.array_equal(got == 0, want == 0)


def test_edt_without_seeds_is_inf():
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import distance_transform_sq
    for sp in ((1, 1, 1), ANISO):
        got = distance_transform_sq(torch.zeros((13, 9, 70), dtype=torch.uint8, device=DEV), sp)
        assert bool(torch.isinf(got).all()) and bool((got > 0).all())


# -------------------------------------------------------------------------------------------------- (c) metrics
@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), ANISO])
@pytest.mark.parametrize("shape,ncls,seed", [((21, 17, 13), 3, 0), ((16, 20, 11), 4, 1), ((24, 9, 70), 2, 2)])
def test_metrics_match_restatement(shape, ncls, seed, spacing):
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import surface_metrics
    rng = np.random.default_rng(seed)
    tgt = _blobs(rng, shape, ncls)
    pred = tgt.copy()
    pred[_blobs(rng, shape, 2, blobs=3) > 0] = int(rng.integers(0, ncls))       # perturbed copy
    rel = 1e-12 if spacing == (1.0, 1.0, 1.0) else 1e-5
    for tau in (0.5, 1.5, 2.7):
        assert _tau_is_valid(tau, spacing, shape)
    for p in (50.0, 95.0, 100.0):
        for tau in (0.5, 1.5, 2.7):
            got = _np(surface_metrics(_gpu(pred, torch.uint8), _gpu(tgt, torch.float32), ncls, spacing, p, tau))
            assert got["hd"].dtype == np.float64 and got["surface_voxels"].dtype == np.int64
            R.assert_metrics_close(got, R.metrics(pred, tgt, ncls, spacing, p, tau), rel)
    got = _np(surface_metrics(_gpu(pred), _gpu(tgt), ncls, spacing, 95.0, 1.5, include_background=True))
    R.assert_metrics_close(got, R.metrics(pred, tgt, ncls, spacing, 95.0, 1.5, include_background=True), rel)


@pytest.mark.parametrize("spacing", [(1.0, 1.0, 1.0), ANISO])
def test_metrics_large_ellipsoid_against_scipy(spacing):
    pytest.importorskip("scipy.ndimage")
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import surface_metrics
    pred, tgt = R.ellipsoid_pair((256, 256, 160), seed=4)
    rel = 1e-12 if spacing == (1.0, 1.0, 1.0) else 1e-5
    got = _np(surface_metrics(_gpu(pred, torch.uint8), _gpu(tgt, torch.uint8), 2, spacing, 95.0, 2.7))
    assert got["surface_voxels"][1].min() > 20000                     # multi-workgroup select and sums
    R.assert_metrics_close(got, R.scipy_metrics(pred, tgt, 2, spacing, 95.0, 2.7), rel)


# -------------------------------------------------------------------------------------------------- (d) edge cases
def test_edge_cases():
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import surface_metrics
    shape = (12, 10, 9)
    z = np.zeros(shape, dtype=np.int64)
    obj = z.copy()
    obj[3:8, 2:7, 1:6] = 1
    dot = z.copy()
    dot[5, 5, 5] = 1
    dot2 = z.copy()
    dot2[0, 9, 8] = 1
    cases = {"pred_empty": (z, obj), "target_empty": (obj, z), "both_empty": (z, z), "identical": (obj, obj),
             "one_voxel": (dot, dot2), "one_voxel_vs_object": (dot, obj)}
    for name, (p, t) in cases.items():
        for sp in ((1.0, 1.0, 1.0), ANISO):
            got = _np(surface_metrics(_gpu(p), _gpu(t), 2, sp, 95.0, 1.5))
            R.assert_metrics_close(got, R.metrics(p, t, 2, sp, 95.0, 1.5), 1e-12 if sp[2] == 1.0 else 1e-5)
            assert math.isnan(got["hd"][0])                                # background skipped
    both = _np(surface_metrics(_gpu(z), _gpu(z), 2))
    assert all(math.isnan(both[k][1]) for k in R.KEYS)
    pe = _np(surface_metrics(_gpu(z), _gpu(obj), 2))
    assert pe["hd"][1] == math.inf and pe["hd_p"][1] == math.inf and pe["assd"][1] == math.inf and pe["nsd"][1] == 0.0
    same = _np(surface_metrics(_gpu(obj), _gpu(obj), 2, tolerance=0.0))
    assert same["hd"][1] == 0.0 and same["hd_p"][1] == 0.0 and same["assd"][1] == 0.0 and same["nsd"][1] == 1.0


# -------------------------------------------------------------------------------------------------- (e) determinism
def test_two_runs_are_bitwise_equal():
    import mivp_amd  # noqa: F401
    from mivp_amd.surface import surface_metrics
    pred, tgt = R.ellipsoid_pair((160, 128, 96), seed=5)
    p, t = _gpu(pred, torch.uint8), _gpu(tgt, torch.uint8)
    for sp in ((1.0, 1.0, 1.0), ANISO):
        a = _np(surface_metrics(p, t, 2, sp, 95.0, 1.5))
        b = _np(surface_metrics(p, t, 2, sp, 95.0, 1.5))
        for k in R.KEYS:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert np.array_equal(a["surface_voxels"], b["surface_voxels"])


# -------------------------------------------------------------------------------------------------- (f) predictor
class StandIn(torch.nn.Module):
    """A deterministic per-window model (element-wise functions of the first input channel), returned as a
    channels-first view of channels-last fp32 storage like the HIP model's output."""

    K = ((1.7, 0.3), (-2.3, 0.9), (3.1, -1.4), (0.6, 0.1))

    def __init__(self, ncls=3):
        super().__init__()
        self.ncls = ncls
        self.anchor = torch.nn.Parameter(torch.zeros(1), requires_grad=False)

    def forward(self, x):
        x0 = x[:, 0]
        ch = [torch.tanh(x0 * k + b) + 0.25 * torch.sin(x0 * (3.0 + c)) for c, (k, b) in enumerate(self.K[:self.ncls])]
        return {"downstream": torch.stack(ch, dim=-1).permute(0, 4, 1, 2, 3)}


def _smooth_volume(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((1, 1) + tuple(s // 4 for s in shape), generator=g) * 2 - 1
    return torch.nn.functional.interpolate(x, size=shape, mode="trilinear", align_corners=False).to(DEV)


@pytest.mark.parametrize("ncls", [2, 3])
def test_evaluate_surface_equals_surface_metrics_of_predict(ncls):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor, evaluate_volume_surface
    from mivp_amd.surface import surface_metrics
    image, roi = (40, 28, 20), (16, 16, 8)
    x = _smooth_volume(image, 11)
    seg = torch.randint(0, ncls, (1, 1) + tuple(s // 4 for s in image), generator=torch.Generator().manual_seed(12))
    seg = torch.nn.functional.interpolate(seg.float(), size=image, mode="nearest").to(DEV)
    model = StandIn(ncls).to(DEV).eval()
    kw = dict(spacing=ANISO, percentile=95.0, tolerance=2.7, include_background=False)
    e = SlidingWindowPredictor(model, image, 1, ncls, roi, overlap=0.5, sub_batch=3)
    got = e.evaluate_surface(x, seg, **kw)
    labels = e.predict(x)["labels"]
    want = surface_metrics(labels, seg, ncls, **kw)
    for k in R.KEYS + ("surface_voxels",):
        assert np.array_equal(got[k].numpy(), want[k].numpy(), equal_nan=True), k
    assert (got["iou"], got["dice"]) == e.evaluate(x, seg)
    gp = SlidingWindowPredictor(model, image, 1, ncls, roi, overlap=0.5, sub_batch=3, graph=True)
    for _ in range(2):                                                    # recording run, then a replay
        gg = gp.evaluate_surface(x, seg, **kw)
        for k in R.KEYS + ("surface_voxels",):
            assert np.array_equal(gg[k].numpy(), got[k].numpy(), equal_nan=True), k
        assert (gg["iou"], gg["dice"]) == (got["iou"], got["dice"])
    one = evaluate_volume_surface(model, x, seg, roi, ncls, sub_batch=3, **kw)
    for k in R.KEYS:
        assert np.array_equal(one[k].numpy(), got[k].numpy(), equal_nan=True), k


# -------------------------------------------------------------------------------------------------- (g) argument checks
def test_surface_refuses_bad_arguments():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    from mivp_amd.surface import distance_transform_sq, surface_map, surface_metrics
    a = torch.zeros((1, 1, 8, 9, 10), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="GPU"):
        surface_metrics(a.cpu(), a, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        surface_metrics(a, a.cpu(), 2)
    with pytest.raises(RuntimeError, match="GPU"):
        surface_map(a.cpu(), 2)
    with pytest.raises(RuntimeError, match="GPU"):
        distance_transform_sq(a[0, 0].cpu())
    with pytest.raises(ValueError):
        surface_metrics(a, torch.zeros((1, 1, 8, 9, 11), dtype=torch.uint8, device=DEV), 2)     # shape mismatch
    with pytest.raises(ValueError):
        surface_metrics(torch.zeros((2, 1, 8, 9, 10), device=DEV), torch.zeros((2, 1, 8, 9, 10), device=DEV), 2)
    for n in (0, 17):
        with pytest.raises(ValueError):
            surface_metrics(a, a, n)
        with pytest.raises(ValueError):
            surface_map(a, n)
    for sp in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError):
            surface_metrics(a, a, 2, spacing=sp)
        with pytest.raises(ValueError):
            distance_transform_sq(a[0, 0], sp)
    for p in (-0.5, 100.5):
        with pytest.raises(ValueError):
            surface_metrics(a, a, 2, percentile=p)
    with pytest.raises(ValueError):
        surface_metrics(a, a, 2, tolerance=-0.1)
    model = StandIn(2).to(DEV).eval()
    p = SlidingWindowPredictor(model, (8, 9, 10), 1, 2, (8, 8, 8), sub_batch=2)
    x = torch.rand((1, 1, 8, 9, 10), device=DEV)
    with pytest.raises(ValueError):
        p.evaluate_surface(x, a.float(), percentile=101.0)
    with pytest.raises(ValueError):
        p.evaluate_surface(x, torch.zeros((1, 1, 8, 9, 11), device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        p.evaluate_surface(x, a.float().cpu())
