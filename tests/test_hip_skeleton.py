"""GPU tests of the thinning kernels and the centreline counts (mivp_amd.skeleton, csrc/skeleton.hip)
against the Python restatement tests/skeleton_ref.py: skeletons bit for bit in both end-point modes, the two stopping
forms, graph capture, the topological invariants at a size the restatement is too slow for (checked with the project's own
component and shape kernels), the integer counts bit for bit, the float64 metrics within 1 ulp, pooling, and the
predictor's surface."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
scipy_ndimage = pytest.importorskip("scipy.ndimage")
import shape_ref as S  # noqa: E402
import skeleton_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _K():
    import mivp_amd  # noqa: F401
    from mivp_amd import skeleton
    return skeleton


# ---------------------------------------------------------------------------------------------- the volumes and their references
def _last_planes():
    """objects that sit on the last plane of each axis, which is an odd plane (even extents)"""
    x = np.zeros((8, 10, 12), dtype=np.uint8)
    x[3:8, 5:10, 6:12] = 1                                   # the far corner
    x[7, 0:4, 0:5] = 2                                       # a sheet in the last h plane
    x[0:3, 9, 2:9] = 2                                       # a bar in the last w plane
    x[0:6, 0:3, 11] = 3                                      # a sheet in the last d plane
    return x


def _volumes():
    blob = R.blobs((20, 18, 37), 7, num_classes=4)
    flat = R.blobs((9, 33), 3, num_classes=3, sigma=1.5).reshape(1, 9, 33)
    col = np.array([1, 1, 1, 0, 2, 2, 1], dtype=np.uint8).reshape(7, 1, 1)
    return {"blob": (blob, 4, [1, 3]), "flat": (flat, 3, None), "column": (col, 3, [1, 2]), "last": (_last_planes(), 4, None)}


_ref_cache = {}


def _ref(name, keep, max_iter=None):
    key = (name, keep, max_iter)
    if key not in _ref_cache:
        x, ncls, classes = _volumes()[name]
        _ref_cache[key] = R.skeletonize_ref(x, ncls, classes, keep, max_iter)
    return _ref_cache[key]


def test_the_blob_volume_is_the_case_it_is_meant_to_be():
    x, ncls, classes = _volumes()["blob"]
    for m in (x == 1, x != 0):                               # a thinned class touches all six faces of the volume
        assert all(f.any() for f in (m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1]))
    assert (x == 3).sum() > 100
    assert (x == 2).sum() > 100                              # a class that is left out of `classes`


# ---------------------------------------------------------------------------------------------- bit-equality
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", ["blob", "flat", "column", "last"])
def test_skeleton_equals_the_restatement(name, keep):
    K = _K()
    x, ncls, classes = _volumes()[name]
    want, it, conv = _ref(name, keep)
    assert conv and (want.sum() < x.sum() or name == "column")
    src = _gpu(x)
    got = K.skeletonize(src, ncls, classes, keep)
    assert got.skeleton.dtype == torch.uint8 and got.skeleton.shape == src.shape
    assert np.array_equal(got.skeleton.cpu().numpy(), want)
    assert got.iterations == it and got.converged is True
    assert np.array_equal(src.cpu().numpy(), x)              # the input is not modified


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float32, torch.bool])
def test_dtypes_and_5d(dtype):
    K = _K()
    x, ncls, classes = _volumes()["last"]
    if dtype is torch.bool:
        x, ncls, classes = (x != 0).astype(np.uint8), 2, None
        want = R.skeletonize_ref(x, ncls)[0]
    else:
        want = _ref("last", True)[0]
    src = _gpu(x, dtype).reshape((1, 1) + x.shape)
    if dtype is torch.float32:
        src[0, 0, 0, 0, 0] = 0.5                             # no class
        src[0, 0, 0, 5, 0] = float("nan")
        assert x[0, 0, 0] == 0 and x[0, 5, 0] == 0
    got = K.skeletonize(src, ncls, classes)
    assert got.skeleton.shape == src.shape and np.array_equal(got.skeleton[0, 0].cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- the two stopping forms
@pytest.mark.parametrize("keep", [True, False])
def test_fixed_iterations_equal_the_converged_loop(keep):
    K = _K()
    x, ncls, classes = _volumes()["blob"]
    want, it, _ = _ref("blob", keep)
    src = _gpu(x)
    loop = K.skeletonize(src, ncls, classes, keep)
    fixed = K.skeletonize(src, ncls, classes, keep, max_iter=it + 5)
    assert isinstance(fixed.iterations, torch.Tensor) and fixed.iterations.dtype == torch.int32 and fixed.iterations.is_cuda
    assert torch.equal(fixed.skeleton, loop.skeleton) and np.array_equal(fixed.skeleton.cpu().numpy(), want)
    assert int(fixed.converged) == 1 and int(fixed.iterations) == loop.iterations == it
    exact = K.skeletonize(src, ncls, classes, keep, max_iter=it)         # the last one issued is the one that deletes nothing
    assert int(exact.converged) == 1 and int(exact.iterations) == it and torch.equal(exact.skeleton, loop.skeleton)
    short = K.skeletonize(src, ncls, classes, keep, max_iter=it - 1)
    assert int(short.converged) == 0 and int(short.iterations) == it - 1


def test_two_iterations_of_a_thick_object():
    K = _K()
    x = R.bar((13, 12, 30), (11, 9, 26))
    want, it, conv = R.skeletonize_ref(x, 2, max_iter=2)
    assert it == 2 and not conv
    got = K.skeletonize(_gpu(x), 2, max_iter=2)
    assert int(got.converged) == 0 and int(got.iterations) == 2
    assert np.array_equal(got.skeleton.cpu().numpy(), want)
    one = K.skeletonize(_gpu(x), 2, max_iter=1)
    assert np.array_equal(one.skeleton.cpu().numpy(), R.skeletonize_ref(x, 2, max_iter=1)[0]) and int(one.converged) == 0


# ---------------------------------------------------------------------------------------------- counts and metrics
def _pair():
    """(pred, target) 3-class maps that overlap but differ"""
    t = R.blobs((20, 18, 37), 7, num_classes=3)
    p = np.roll(t, (1, -1, 2), axis=(0, 1, 2))
    p[:, :, 17:20] = np.where(p[:, :, 17:20] == 1, 0, p[:, :, 17:20])    # class 1 cut across
    return p, t


_pair_cache = {}


def _pair_ref(keep=True):
    if keep not in _pair_cache:
        p, t = _pair()
        sp, sl = R.skeletonize_ref(p, 3, None, keep)[0], R.skeletonize_ref(t, 3, None, keep)[0]
        _pair_cache[keep] = (p, t, sp, sl, R.centerline_counts(p, t, sp, sl, 3), R.skeleton_stats(sp, 3), R.skeleton_stats(sl, 3))
    return _pair_cache[keep]


def _same_metrics(got, counts, classes):
    want = R.centerline_metrics(counts, classes)
    for k in ("tprec", "tsens", "cldice"):
        assert (S.ulp_distance(got[k], want[k]) <= 1).all(), k
    for k in ("mean_tprec", "mean_tsens", "mean_cldice"):
        assert S.ulp_distance(got[k], want[k]) <= 1, k


def test_centerline_counts_and_metrics():
    K = _K()
    p, t, sp, sl, counts, st_p, st_l = _pair_ref()
    spacing = (0.7, 1.3, 2.5)
    rep = K.centerline_metrics(_gpu(p), _gpu(t), 3, spacing)
    got = rep.cpu()
    assert np.array_equal(rep.pred_skeleton.cpu().numpy(), sp) and np.array_equal(rep.target_skeleton.cpu().numpy(), sl)
    assert np.array_equal(got["counts"], counts) and counts[1:, 0].min() > 20
    assert (counts[1:, 1] < counts[1:, 0]).all() and (counts[1:, 3] < counts[1:, 2]).all()
    _same_metrics(got, counts, [1, 2])
    assert 0 < got["mean_cldice"] < 1
    for side, st in (("pred", st_p), ("target", st_l)):
        for k, col in (("voxels", 0), ("isolated", 1), ("end_points", 2), ("interior", 3), ("branch_points", 4)):
            assert np.array_equal(got[side][k], st[:, col]), (side, k)
        assert np.array_equal(got[side]["edges"], st[:, 5:])
        assert (S.ulp_distance(got[side]["length_mm"], R.length_mm(st, spacing)) <= 1).all()
    assert st_p[1:, 4].min() > 0 and st_p[1:, 2].min() > 0 and (st_p[1:, 5:] > 0).sum() > 20
    assert got["iterations"] == (R.skeletonize_ref(p, 3)[1], R.skeletonize_ref(t, 3)[1]) and got["converged"] == (True, True)
    # a subset of the classes, the other end-point mode, other dtypes
    p0, t0, sp0, sl0, counts0, _, _ = _pair_ref(False)
    sub = K.centerline_metrics(_gpu(p, torch.float32), _gpu(t, torch.int64), 3, classes=[2], keep_endpoints=False).cpu()
    want = counts0.copy()
    want[1] = 0
    assert np.array_equal(sub["counts"], want)
    _same_metrics(sub, want, [2])


def test_skeleton_stats_alone():
    K = _K()
    p, t, sp, sl, _, st_p, _ = _pair_ref()
    spacing = (2.0, 0.5, 1.0)
    a = K.skeleton_stats(_gpu(sp), 3, spacing)
    assert np.array_equal(a.counts.cpu().numpy(), st_p)
    b = K.skeleton_stats(_gpu(sp, torch.int32).reshape((1, 1) + sp.shape), 3, spacing, classes=[2])
    assert np.array_equal(b.counts.cpu().numpy(), R.skeleton_stats(sp, 3, [2]))
    full = K.skeleton_stats(_gpu(p), 3, spacing)                          # any class map: here a thick one
    assert np.array_equal(full.counts.cpu().numpy(), R.skeleton_stats(p, 3))
    assert (S.ulp_distance(full.length_mm.cpu().numpy(), R.length_mm(R.skeleton_stats(p, 3), spacing)) <= 1).all()


def test_identical_maps_give_exactly_one():
    K = _K()
    _, t, _, sl, _, _, _ = _pair_ref()
    rep = K.centerline_metrics(_gpu(t), _gpu(t), 3).cpu()
    assert rep["cldice"][1:].tolist() == [1.0, 1.0] and rep["mean_cldice"] == 1.0
    assert rep["mean_tprec"] == 1.0 and rep["mean_tsens"] == 1.0
    n = [(sl == c).sum() for c in (1, 2)]
    assert rep["counts"][1:].tolist() == [[n[0]] * 4, [n[1]] * 4]
    empty = K.centerline_metrics(_gpu(t), _gpu(np.zeros_like(t)), 3).cpu()
    assert empty["cldice"].tolist() == [0.0, 0.0, 0.0] and empty["mean_cldice"] == 0.0 and not np.isnan(empty["tsens"]).any()


def test_out_pools_two_scans():
    K = _K()
    p, t, _, _, counts, st_p, st_l = _pair_ref()
    p2, t2 = t, p
    rep = K.centerline_metrics(_gpu(p), _gpu(t), 3)
    again = K.centerline_metrics(_gpu(p2), _gpu(t2), 3, out=rep)
    assert again is rep
    swapped = counts[:, [2, 3, 0, 1]]
    got = rep.cpu()
    assert np.array_equal(got["counts"], counts + swapped)
    assert np.array_equal(rep.pred_stats.counts.cpu().numpy(), st_p + st_l)
    assert np.array_equal(rep.target_stats.counts.cpu().numpy(), st_p + st_l)
    _same_metrics(got, counts + swapped, [1, 2])
    st = K.skeleton_stats(rep.pred_skeleton, 3)
    K.skeleton_stats(rep.target_skeleton, 3, out=st)
    assert np.array_equal(st.counts.cpu().numpy(), st_p + st_l)
    with pytest.raises(ValueError, match="out was made for"):
        K.centerline_metrics(_gpu(p), _gpu(t), 3, classes=[1], out=rep)
    with pytest.raises(ValueError, match="same spatial shape"):
        K.centerline_metrics(_gpu(p), _gpu(t[:-1]), 3)


# ---------------------------------------------------------------------------------------------- graph capture
def test_graph_replay_equals_eager():
    K = _K()
    p, t = _pair()
    n = R.skeletonize_ref(t, 3)[1] + 3
    sp, st = _gpu(t), _gpu(p)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.skeletonize(sp, 3, max_iter=2)
        K.centerline_metrics(sp, st, 3, max_iter=2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = K.skeletonize(sp, 3, max_iter=n)
        rep = K.centerline_metrics(sp, st, 3, (1.0, 2.0, 0.5), max_iter=n)
    for a, b in ((p, t), (t, p), (p, p)):
        sp.copy_(_gpu(a)); st.copy_(_gpu(b))
        g.replay()
        torch.cuda.synchronize()
        eager = K.skeletonize(_gpu(a), 3)
        assert torch.equal(res.skeleton, eager.skeleton)
        assert int(res.iterations) == eager.iterations and int(res.converged) == 1
        want = K.centerline_metrics(_gpu(a), _gpu(b), 3, (1.0, 2.0, 0.5)).cpu()
        got = rep.cpu()
        assert np.array_equal(got["counts"], want["counts"]) and got["iterations"] == want["iterations"]
        for k in ("tprec", "tsens", "cldice"):
            assert np.array_equal(got[k], want[k]), k
        for side_ in ("pred", "target"):
            assert np.array_equal(got[side_]["edges"], want[side_]["edges"])
            assert np.array_equal(got[side_]["length_mm"], want[side_]["length_mm"])
    assert np.array_equal(res.skeleton.cpu().numpy(), _pair_ref()[2])     # the last replay thinned p


# ---------------------------------------------------------------------------------------------- invariants at size
def _blobs_and_tubes():
    shape = (64, 64, 48)
    x = R.blobs(shape, 11, num_classes=3, threshold=0.15, sigma=3.0)
    hh, ww, dd = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    helix = (hh - 32 - 18 * np.cos(dd / 6.0)) ** 2 + (ww - 32 - 18 * np.sin(dd / 6.0)) ** 2 <= 9     # a tube of radius 3
    ring = (np.abs(np.sqrt((hh - 32.0) ** 2 + (dd - 24.0) ** 2) - 14) <= 2) & (np.abs(ww - 10) <= 2)
    x[helix] = 1
    x[ring] = 2
    return x


def test_invariants_on_a_large_volume():
    K = _K()
    from mivp_amd.components import label_components
    from mivp_amd.regions import region_shape, region_stats
    x = _blobs_and_tubes()
    src = _gpu(x)
    res = K.skeletonize(src, 3)
    sk = res.skeleton
    assert res.converged and res.iterations >= 4
    assert bool(((sk == src) | (sk == 0)).all()) and int((sk != 0).sum()) * 4 < int((src != 0).sum())
    again = K.skeletonize(sk, 3)
    assert again.iterations == 1 and torch.equal(again.skeleton, sk)
    for c in (1, 2):
        n_in = label_components((src == c).to(torch.uint8), 26)[1]
        n_sk = label_components((sk == c).to(torch.uint8), 26)[1]
        assert n_in == n_sk and n_in >= 1
    tab_in, tab_sk = region_stats(src, 3), region_stats(sk, 3)
    n = int(tab_in.n)
    assert n == int(tab_sk.n) and 2 <= n < 4096
    e_in, e_sk = region_shape(tab_in).euler[:n], region_shape(tab_sk).euler[:n]
    owner = tab_in.labels.reshape(-1)[tab_sk.first[:n].long()].long() - 1      # the input component of each skeleton component
    assert sorted(owner.tolist()) == list(range(n))
    assert torch.equal(e_in[owner], e_sk)
    assert torch.equal(tab_in.cls[:n][owner], tab_sk.cls[:n])
    assert int((e_in < 1).sum()) >= 1                         # the ring (or a blob with a tunnel) is there
    flat = K.skeletonize(src, 3, keep_endpoints=False).skeleton
    tab_f = region_stats(flat, 3)
    assert int(tab_f.n) == n
    assert sorted(region_shape(tab_f).euler[:n].tolist()) == sorted(e_in.tolist())


# ---------------------------------------------------------------------------------------------- the predictor
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
def test_predictor_centerline(graph):
    K = _K()
    from mivp_amd.inference import SlidingWindowPredictor, evaluate_volume_centerline
    ncls, image, roi = 3, (40, 28, 20), (16, 16, 8)
    rng = np.random.default_rng(31)
    field = scipy_ndimage.gaussian_filter(rng.standard_normal(image), 2.0)
    x = _gpu((field / field.std()).astype(np.float32)).reshape((1, 1) + image)
    seg = _gpu(R.blobs(image, 5, num_classes=3)).reshape((1, 1) + image)
    model = StandIn(ncls).to(DEV).eval()
    e = SlidingWindowPredictor(model, image, 1, ncls, roi, overlap=0.5, sub_batch=3, graph=graph)
    post = dict(largest=False, min_size=5)
    kw = dict(spacing=(0.8, 0.8, 2.5), classes=[2, 1], keep_endpoints=True)
    for pp, max_iter in ((None, None), (post, 16)):
        labels = e.predict(x, postprocess=pp)["labels"]
        want = K.centerline_metrics(labels, seg, ncls, max_iter=max_iter, **kw).cpu()
        assert want["counts"][1:, 0].min() > 0
        got = e.evaluate_centerline(x, seg, postprocess=pp, max_iter=max_iter, **kw).cpu()
        assert np.array_equal(got["counts"], want["counts"]) and got["iterations"] == want["iterations"]
        for k in ("tprec", "tsens", "cldice"):
            assert np.array_equal(got[k], want[k]), k
        for side in ("pred", "target"):
            assert np.array_equal(got[side]["edges"], want[side]["edges"])
            assert np.array_equal(got[side]["length_mm"], want[side]["length_mm"])
    lab = labels[0, 0].cpu().numpy()
    sp, sl = R.skeletonize_ref(lab, ncls)[0], R.skeletonize_ref(seg[0, 0].cpu().numpy(), ncls)[0]
    assert np.array_equal(got["counts"], R.centerline_counts(lab, seg[0, 0].cpu().numpy(), sp, sl, ncls))
    one = evaluate_volume_centerline(model, x, seg, roi, ncls, sub_batch=3, graph=graph, postprocess=post, max_iter=16,
                                     **kw).cpu()
    assert np.array_equal(one["counts"], got["counts"])
    with pytest.raises(ValueError, match="max_iter must be"):
        e.evaluate_centerline(x, seg, max_iter=0)
    with pytest.raises(ValueError, match="classes must be ints"):
        e.evaluate_centerline(x, seg, classes=[0])
