"""CPU: the numpy restatement of the surface-distance metrics (tests/surface_ref.py) against scipy.ndimage and
numpy.percentile, and the empty-class rules it applies."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_ref as R  # noqa: E402


def _random_labels(rng, shape, ncls, blobs=4):
    """Blobby multi-class maps (random boxes painted over background), with objects touching the border."""
    lab = np.zeros(shape, dtype=np.int64)
    for _ in range(blobs):
        c = int(rng.integers(1, ncls))
        lo = [int(rng.integers(0, s)) for s in shape]
        hi = [min(s, l + int(rng.integers(1, max(2, s // 2 + 1)))) for s, l in zip(shape, lo)]
        lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = c
    return lab


CASES = [((9, 11, 7), 3, (1.0, 1.0, 1.0)), ((12, 8, 10), 4, (0.8, 0.8, 2.5)), ((6, 13, 5), 2, (1.5, 0.7, 1.0)),
         ((10, 10, 1), 3, (1.0, 1.0, 1.0))]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape,ncls,spacing", CASES)
def test_restatement_matches_scipy(shape, ncls, spacing, seed):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(seed)
    pred, tgt = _random_labels(rng, shape, ncls), _random_labels(rng, shape, ncls)
    for c in range(ncls):
        m = R.class_mask(tgt, c)
        assert np.array_equal(R.surface(m), R.scipy_surface(m))
    for p in (50.0, 95.0, 100.0):
        got = R.metrics(pred, tgt, ncls, spacing, p, 1.5, include_background=True)
        want = R.scipy_metrics(pred, tgt, ncls, spacing, p, 1.5, include_background=True)
        R.assert_metrics_close(got, want, 1e-12)


def test_surface_marks_border_voxels():
    m = np.ones((4, 5, 3), dtype=bool)
    s = R.surface(m)
    inner = np.zeros_like(m)
    inner[1:-1, 1:-1, 1:-1] = True
    assert np.array_equal(s, m & ~inner)
    assert not R.surface(np.zeros((3, 3, 3), dtype=bool)).any()


def test_directed_distances_by_hand():
    a = np.zeros((5, 5, 5), dtype=bool)
    b = np.zeros_like(a)
    a[0, 0, 0] = True
    b[3, 4, 0] = True
    b[4, 4, 4] = True
    assert R.directed(a, b, (1, 1, 1)).tolist() == [5.0]
    assert np.allclose(R.directed(a, b, (2.0, 1.0, 0.5)), [math.sqrt(36 + 16)])
    assert R.directed(b, a, (1, 1, 1)).tolist() == [5.0, math.sqrt(48)]


def test_empty_class_rules():
    z = np.zeros((6, 6, 6), dtype=np.int64)
    one = z.copy()
    one[2:4, 2:4, 2:4] = 1
    both_empty = R.metrics(z, z, 3)
    assert all(np.isnan(both_empty[k]).all() for k in R.KEYS)        # class 0 skipped, classes 1, 2 empty on both sides
    pred_empty = R.metrics(z, one, 2)
    tgt_empty = R.metrics(one, z, 2)
    for m in (pred_empty, tgt_empty):
        assert math.isnan(m["hd"][0])
        assert m["hd"][1] == math.inf and m["hd_p"][1] == math.inf and m["assd"][1] == math.inf and m["nsd"][1] == 0.0
    same = R.metrics(one, one, 2, tolerance=0.0)
    assert same["hd"][1] == 0.0 and same["assd"][1] == 0.0 and same["nsd"][1] == 1.0
    assert same["surface_voxels"][1].tolist() == [8, 8]
    bg = R.metrics(one, one, 2, include_background=True)
    assert not math.isnan(bg["hd"][0])


def test_percentile_is_numpy_linear():
    d_ab = np.array([0.0, 1.0, 2.0, 10.0])
    d_ba = np.array([3.0])
    v = R.combine(d_ab, d_ba, 50.0, 1.0)
    assert v["hd_p"] == max(np.percentile(d_ab, 50.0), 3.0) == 3.0
    assert v["hd"] == 10.0 and v["assd"] == 16.0 / 5 and v["nsd"] == 2 / 5
