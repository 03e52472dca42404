"""CPU: the restatement of the thinning algorithm (tests/skeleton_ref.py) against an independent brute
force and on written-out shapes, the invariants it must keep on random volumes, the clDice example of the README, and the
host side of mivp_amd.skeleton: argument checks, the header wording and the prototype table."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import shape_ref as S
import skeleton_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mivp.h")


# ---------------------------------------------------------------------------------------------- the simple-point predicate
def _brute_simple(obj):
    """(26, 6) simple point by scipy.ndimage.label on the 3 x 3 x 3 block"""
    block = np.zeros((3, 3, 3), dtype=bool)
    for k, o in enumerate(R.OFFSETS26):
        block[o[0] + 1, o[1] + 1, o[2] + 1] = bool((obj >> k) & 1)
    _, n_obj = ndimage.label(block, structure=np.ones((3, 3, 3)))
    if n_obj != 1:
        return False
    n18 = ndimage.generate_binary_structure(3, 2)
    n18[1, 1, 1] = False
    bg = ~block & n18
    lab, _ = ndimage.label(bg, structure=ndimage.generate_binary_structure(3, 1))
    n6 = ndimage.generate_binary_structure(3, 1)
    n6[1, 1, 1] = False
    return len(set(lab[bg & n6].tolist())) == 1


def _configurations():
    few = [sum(1 << k for k in ks) for n in range(4) for ks in itertools.combinations(range(26), n)]
    full = (1 << 26) - 1
    rng = np.random.default_rng(0)
    dense = rng.integers(0, 1 << 26, size=3000).tolist()
    sparse = (rng.integers(0, 1 << 26, size=2500) & rng.integers(0, 1 << 26, size=2500)).tolist()
    return few + [full ^ m for m in few] + dense + sparse


def test_simple_point_against_brute_force():
    cases = _configurations()
    assert len(cases) >= 5000 + 2 * 2952
    wrong = [m for m in cases if R.simple_point(int(m)) != _brute_simple(int(m))]
    assert not wrong, [bin(m) for m in wrong[:5]]
    assert sum(R.simple_point(int(m)) for m in cases) > 500              # both answers occur


def test_neighbourhood_tables():
    assert len(R.OFFSETS26) == 26 and len(R.FORWARD_OFFSETS) == 13
    assert R.FORWARD_OFFSETS[0] == (0, 0, 1) and R.FORWARD_OFFSETS[-1] == (1, 1, 1)
    assert bin(R.N6_MASK).count("1") == 6 and bin(R.N18_MASK).count("1") == 18
    # a corner position touches three edge positions; an edge two corners and two faces; a face four edges (no centre)
    assert sorted(bin(a).count("1") for a in R.ADJ6) == [3] * 8 + [4] * 18
    assert sorted(bin(a).count("1") for a in R.ADJ26) == [6] * 8 + [10] * 12 + [16] * 6
    for k in range(26):
        for j in range(26):
            assert ((R.ADJ26[k] >> j) & 1) == ((R.ADJ26[j] >> k) & 1)


# ---------------------------------------------------------------------------------------------- written-out cases
def test_line_is_unchanged():
    x = np.zeros((1, 1, 9), dtype=np.uint8)
    x[0, 0, 1:8] = 1
    sk, it, conv = R.skeletonize_ref(x, 2)
    assert np.array_equal(sk, x) and it == 1 and conv
    y = np.zeros((5, 5, 11), dtype=np.uint8)
    y[2, 2, 1:10] = 1
    assert np.array_equal(R.skeletonize_ref(y, 2)[0], y)


def test_cube_becomes_one_voxel_without_end_points():
    x = np.zeros((5, 5, 5), dtype=np.uint8)
    x[1:4, 1:4, 1:4] = 1
    sk, _, conv = R.skeletonize_ref(x, 2, keep_endpoints=False)
    assert conv and int(sk.sum()) == 1


def test_bar_becomes_its_centre_line():
    x = np.zeros((11, 11, 22), dtype=np.uint8)
    x[1:8, 2:9, 1:19] = 1                                    # 7 x 7 x 18
    sk, it, conv = R.skeletonize_ref(x, 2)
    idx = np.argwhere(sk)
    assert conv and it == 4 and len(idx) == 14
    on_axis = idx[(idx[:, 0] == 4) & (idx[:, 1] == 5)]
    assert on_axis[:, 2].tolist() == list(range(4, 16))                   # the axis of the bar, 3 voxels short of each end
    rest = sorted(map(tuple, idx[(idx[:, 0] != 4) | (idx[:, 1] != 5)].tolist()))
    assert rest == [(3, 5, 3), (5, 5, 3)]                                 # and a two-voxel fork at one end, one step off it
    assert R.skeleton_stats(sk, 2)[1, :5].tolist() == [14, 0, 3, 10, 1]
    assert S.components_and_cavities(sk) == (1, 0)
    sk, it, conv = R.skeletonize_ref(x, 2, keep_endpoints=False)
    assert conv and it == 7 and int(sk.sum()) == 1


@pytest.mark.parametrize("keep", [True, False])
def test_thick_ring_keeps_its_loop(keep):
    x = R.thick_ring()
    sk, _, conv = R.skeletonize_ref(x, 2, keep_endpoints=keep)
    assert conv and 0 < sk.sum() < x.sum() / 4
    assert S.shape_stats(x.astype(np.int32), 1)["euler"].tolist() == [0]
    assert S.shape_stats(sk.astype(np.int32), 1)["euler"].tolist() == [0]          # one component, one tunnel
    assert S.components_and_cavities(sk) == (1, 0)
    stats = R.skeleton_stats(sk, 2)
    if not keep:                                             # a closed curve: every voxel has two neighbours or more
        assert stats[1, 1] == 0 and stats[1, 2] == 0


@pytest.mark.parametrize("keep", [True, False])
def test_shell_keeps_its_cavity(keep):
    x = R.shell()
    sk, _, conv = R.skeletonize_ref(x, 2, keep_endpoints=keep)
    assert conv and sk.sum() < x.sum()
    assert S.components_and_cavities(x) == (1, 1) and S.components_and_cavities(sk) == (1, 1)
    assert S.shape_stats(sk.astype(np.int32), 1)["euler"].tolist() == [2]


def test_touching_classes_are_thinned_independently():
    x = np.zeros((9, 9, 16), dtype=np.uint8)
    x[1:8, 1:8, 1:8] = 1
    x[1:8, 1:8, 8:15] = 2                                    # face to face
    both = R.skeletonize_ref(x, 3)[0]
    one = R.skeletonize_ref(np.where(x == 1, x, 0), 3)[0]
    two = R.skeletonize_ref(np.where(x == 2, x, 0), 3)[0]
    assert np.array_equal(both, one + two)
    assert np.array_equal(R.skeletonize_ref(x, 3, classes=[2])[0], two)
    f = x.astype(np.float32)
    f[2, 2, 2] = 1.5                                         # no class: background for class 1
    f[0, 0, 0] = 7.0
    g = x.copy()
    g[2, 2, 2] = 0
    assert np.array_equal(R.skeletonize_ref(f, 3)[0], R.skeletonize_ref(g, 3)[0])


# ---------------------------------------------------------------------------------------------- invariants
BLOB_SEEDS = [0, 1, 2, 3]
_blob_cache = {}


def _blob(seed):
    if seed not in _blob_cache:
        x = R.blobs((16, 14, 18), seed)
        history = []
        k = 0
        while True:
            k += 1
            sk, it, conv = R.skeletonize_ref(x, 3, max_iter=k)
            history.append(sk)
            if conv:
                break
        _blob_cache[seed] = (x, history, R.skeletonize_ref(x, 3))
    return _blob_cache[seed]


def _topology(vol, c):
    """(26-components, cavities, sum of the Euler numbers) of class c"""
    m = vol == c
    lab, n = ndimage.label(m, structure=np.ones((3, 3, 3)))
    return S.components_and_cavities(m) + (int(S.shape_stats(lab.astype(np.int32), n)["euler"].sum()),)


@pytest.mark.parametrize("seed", BLOB_SEEDS)
def test_blob_invariants(seed):
    x, history, (sk, it, conv) = _blob(seed)
    assert conv and it == len(history) and it >= 3
    for c in (1, 2):
        assert (x == c).sum() > 200
        assert _topology(x, c) == _topology(sk, c)
    assert ((sk == x) | (sk == 0)).all() and sk.sum() < x.sum()
    again, it2, conv2 = R.skeletonize_ref(sk, 3)
    assert np.array_equal(again, sk) and it2 == 1 and conv2
    assert np.array_equal(history[-1], sk) and np.array_equal(history[-2], sk)       # the last iteration deleted nothing
    for a, b in zip(history, history[1:-1]):
        assert (b <= a).all() and b.sum() < a.sum()
    part, it_k, conv_k = R.skeletonize_ref(x, 3, max_iter=2)
    assert it_k == 2 and not conv_k and np.array_equal(part, history[1])
    assert np.array_equal(R.skeletonize_ref(history[1], 3)[0], sk)      # the iterations compose: no state besides the map


# ---------------------------------------------------------------------------------------------- the clDice example
def test_cldice_notices_a_vessel_cut_by_three_voxels():
    ref = np.zeros((7, 9, 34), dtype=np.uint8)
    ref[3, 3:6, 2:32] = 1                                    # a flat vessel, 3 voxels across, 30 long
    pred = ref.copy()
    pred[3, 3:6, 16] = 0                                     # three voxels missing: two pieces
    assert int(ref.sum()) - int(pred.sum()) == 3
    assert S.components_and_cavities(ref)[0] == 1 and S.components_and_cavities(pred)[0] == 2
    sl, sp = R.skeletonize_ref(ref, 2)[0], R.skeletonize_ref(pred, 2)[0]
    counts = R.centerline_counts(pred, ref, sp, sl, 2)
    assert counts[1].tolist() == CUT_COUNTS
    same = R.centerline_metrics(R.centerline_counts(ref, ref, sl, sl, 2), [1])
    cut = R.centerline_metrics(counts, [1])
    assert same["tsens"][1] == 1.0 and same["cldice"][1] == 1.0
    assert cut["tprec"][1] == 1.0                            # what is predicted lies inside the reference
    drop = 1.0 - cut["tsens"][1]
    assert drop == 1.0 - (CUT_COUNTS[2] - 1) / CUT_COUNTS[2] and drop > 0
    dice_move = 1.0 - R.voxel_dice(pred, ref, 1)
    assert dice_move == 1.0 - 2 * 87 / (90 + 87)
    assert 0 < dice_move < drop
    assert cut["mean_cldice"] == cut["cldice"][1] == 2.0 * cut["tsens"][1] / (1.0 + cut["tsens"][1])


CUT_COUNTS = [34, 34, 33, 32]            # |S_P|, |S_P and V_L|, |S_L|, |S_L and V_P| from the restatement


def test_stats_and_length_by_hand():
    x = np.zeros((4, 5, 6), dtype=np.uint8)
    x[1, 1, 1:4] = 1                                         # three along d
    x[2, 2, 4] = 1                                           # then one diagonal step (1, 1, 1)
    x[3, 4, 0] = 2                                           # an isolated voxel of class 2
    st = R.skeleton_stats(x, 3)
    assert st[1, :5].tolist() == [4, 0, 2, 2, 0] and st[2, :5].tolist() == [1, 1, 0, 0, 0]
    assert st[1, 5 + R.FORWARD_OFFSETS.index((0, 0, 1))] == 2 and st[1, 5 + R.FORWARD_OFFSETS.index((1, 1, 1))] == 1
    assert st[1, 5:].sum() == 3 and st[2, 5:].sum() == 0
    length = R.length_mm(st, (2.0, 3.0, 0.5))
    assert length[1] == 0.5 + 0.5 + np.sqrt(4.0 + 9.0 + 0.25) and length[2] == 0.0
    assert R.skeleton_stats(x, 3, classes=[2])[1].sum() == 0


# ---------------------------------------------------------------------------------------------- the host side of the module
def _mod():
    import mivp_amd  # noqa: F401
    from mivp_amd import skeleton
    return skeleton


def test_argument_checks():
    K = _mod()
    assert K._check_skeleton_args(4) == (4, 0b1110, (1, 2, 3), True, None)
    assert K._check_skeleton_args(4, [3, 1], False, 7) == (4, 0b1010, (1, 3), False, 7)
    assert K._check_skeleton_args(3, None, True, np.int64(4096))[4] == 4096
    for bad in (0, 4097, -1, True, 2.0, "3"):
        with pytest.raises(ValueError, match=r"max_iter must be None or an integer in 1\.\.4096"):
            K._check_skeleton_args(3, None, True, bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="keep_endpoints must be a bool"):
            K._check_skeleton_args(3, None, bad)
    with pytest.raises(ValueError, match=r"classes must be ints in 1\.\.2, got 0"):
        K._check_skeleton_args(3, [0])
    with pytest.raises(ValueError, match=r"classes is empty \(num_classes=1 has no foreground class\)"):
        K._check_skeleton_args(1)
    with pytest.raises(ValueError, match=r"num_classes must be in 1\.\.16, got 17"):
        K._check_skeleton_args(17)
    with pytest.raises(ValueError, match="spacing must be three positive sizes"):
        K.check_centerline_kwargs(3, (1, 1, 0))
    for call in (lambda: K.skeletonize(torch.zeros(4, 4, 4, dtype=torch.uint8), 2),
                 lambda: K.skeleton_stats(torch.zeros(4, 4, 4, dtype=torch.uint8), 2),
                 lambda: K.centerline_metrics(torch.zeros(4, 4, 4), torch.zeros(4, 4, 4), 2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_reports_on_the_host():
    K = _mod()
    assert list(K.FORWARD_OFFSETS) == R.FORWARD_OFFSETS
    rep = K.CenterlineReport(3, (1, 2), (1.0, 1.0, 1.0), "cpu")
    rep.counts.copy_(torch.tensor([[0, 0, 0, 0], [34, 34, 33, 32], [0, 0, 5, 0]]))
    want = R.centerline_metrics(rep.counts.numpy(), [1, 2])
    for k in ("tprec", "tsens", "cldice"):
        assert np.array_equal(getattr(rep, k).numpy(), want[k]), k
    for k in ("mean_tprec", "mean_tsens", "mean_cldice"):
        assert float(getattr(rep, k)) == want[k], k
    assert rep.cldice[2] == 0.0 and rep.cldice[0] == 0.0     # empty sets score 0, not NaN
    st = K.SkeletonStats(3, (1, 2), (2.0, 3.0, 0.5), "cpu")
    st.counts[1, 5:] = torch.arange(1, 14)
    assert np.array_equal(st.length_mm.numpy(), R.length_mm(st.counts.numpy(), (2.0, 3.0, 0.5)))
    with pytest.raises(ValueError, match="out was made for"):
        K._check_out(rep, K.CenterlineReport, 3, (1,))
    with pytest.raises(TypeError, match="out must be a SkeletonStats"):
        K._check_out(rep, K.SkeletonStats, 3, (1, 2))


def test_predictor_surface_and_exports():
    import mivp_amd
    from mivp_amd import inference
    K = _mod()
    for name in ("skeletonize", "skeleton_stats", "centerline_metrics", "evaluate_volume_centerline", "SkeletonResult",
                 "SkeletonStats", "CenterlineReport"):
        assert getattr(mivp_amd, name) is getattr(K, name)
    assert inference.evaluate_volume_centerline is K.evaluate_volume_centerline
    sig = inspect.signature(inference.SlidingWindowPredictor.evaluate_centerline)
    assert list(sig.parameters) == ["self", "x", "seg", "spacing", "classes", "postprocess", "keep_endpoints", "max_iter"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [(1.0, 1.0, 1.0), None, None, True, None]
    one = inspect.signature(K.evaluate_volume_centerline)
    surf = inspect.signature(inference.evaluate_volume_surface)
    assert list(one.parameters)[:10] == list(surf.parameters)[:10]       # model .. graph, as evaluate_volume_surface
    assert {"spacing", "classes", "postprocess", "mirror_axes", "keep_endpoints", "max_iter", "skip", "fit"} <= set(one.parameters)
    assert one.parameters["fit"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(K.skeletonize).parameters) == ["labels", "num_classes", "classes", "keep_endpoints",
                                                                  "max_iter"]


def test_header_and_prototypes():
    from mivp_amd import _lib
    assert _lib.ABI_VERSION == 18
    text = open(HEADER).read()
    block = text[text.index("Centreline extraction by 3-D thinning"):text.index("size_t mivp_skeleton_ws")]
    assert re.search(r"joined ABI 18 without\s+(\*\s+)?a bump", block)
    assert "ABI 19" not in text
    P = _lib.parse_header()
    vp, i32, u32 = _lib.vp, _lib.i32, __import__("ctypes").c_uint32
    import ctypes
    assert P["mivp_skeleton_ws"] == (ctypes.c_size_t, [vp])
    assert P["mivp_skeleton_begin"] == (ctypes.c_int, [vp, i32, vp, i32, u32, vp, vp, vp])
    assert P["mivp_skeleton_iter"] == (ctypes.c_int, [vp, vp, i32, i32, vp, vp])
    assert P["mivp_skeleton_end"] == (ctypes.c_int, [vp, i32, vp, vp, vp])
    assert P["mivp_centerline_counts"] == (ctypes.c_int, [vp, i32, vp, i32, vp, vp, vp, i32, vp, vp])
    assert P["mivp_skeleton_stats"] == (ctypes.c_int, [vp, vp, i32, u32, vp, vp])
