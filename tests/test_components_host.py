"""CPU: the numpy / scipy restatement of connected-component labelling and post-processing (tests/components_ref.py) on
hand-made volumes with known answers, and the argument checks of mivp_amd.components."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytest.importorskip("scipy")
import components_ref as R  # noqa: E402


def test_diagonal_pairs_by_connectivity():
    edge = np.zeros((3, 3, 3), dtype=np.uint8)
    edge[0, 0, 0] = edge[1, 1, 0] = 1                      # share an edge
    corner = np.zeros((3, 3, 3), dtype=np.uint8)
    corner[0, 0, 0] = corner[1, 1, 1] = 1                  # share a corner only
    assert [R.label_by_value(edge, k)[1] for k in (6, 18, 26)] == [2, 1, 1]
    assert [R.label_by_value(corner, k)[1] for k in (6, 18, 26)] == [2, 2, 1]


def test_numbering_follows_first_voxel_and_value():
    x = np.zeros((2, 3, 4), dtype=np.int32)
    x[1, 2, 3] = 5                                         # last voxel: numbered last
    x[0, 0, 2] = 7
    x[0, 0, 3] = 5                                         # adjacent to the 7 but another value: its own component
    x[1, 0, 0] = 7
    lab, n = R.label_by_value(x, 26)
    assert n == 4
    assert (lab[0, 0, 2], lab[0, 0, 3], lab[1, 0, 0], lab[1, 2, 3]) == (1, 2, 3, 4)


def test_scipy_numbering_is_first_appearance():
    """label_by_value of a 0/1 mask is scipy.ndimage.label itself (the numbering the GPU output is compared with)."""
    from scipy import ndimage
    rng = np.random.default_rng(0)
    for k in (6, 18, 26):
        m = rng.random((17, 13, 11)) < 0.35
        want, n = ndimage.label(m, R.structure(k))
        got, gn = R.label_by_value(m.astype(np.uint8), k)
        assert gn == n and np.array_equal(got, want)


def _two_cubes(gap=2):
    x = np.zeros((4, 6, 12), dtype=np.uint8)
    x[1:3, 1:3, 0:2] = 1
    x[1:3, 1:3, 2 + gap:4 + gap] = 1                       # same size, later in raster order
    return x


def test_ties_keep_the_first_in_raster_order():
    x = _two_cubes()
    out = R.postprocess(x, 2, largest=True)
    assert out[1:3, 1:3, 0:2].all() and not out[:, :, 2:].any()


def test_min_size_equal_to_a_size_keeps_it():
    x = _two_cubes()
    x[0, 5, 11] = 1                                        # a single voxel
    out = R.postprocess(x, 2, largest=False, min_size=8)
    assert np.array_equal(out, np.where(np.arange(x.size).reshape(x.shape) == np.ravel_multi_index((0, 5, 11), x.shape),
                                        0, x))
    assert np.array_equal(R.postprocess(x, 2, largest=False, min_size=1), x)
    assert not R.postprocess(x, 2, largest=False, min_size=9).any()


def test_classes_outside_the_selection_are_untouched():
    x = np.zeros((5, 5, 5), dtype=np.int64)
    x[0, 0, 0] = 1
    x[4, 4, 3:5] = 1
    x[2, 2, 2] = 2
    x[0, 4, 4] = 2
    out = R.postprocess(x, 3, largest=True, classes=[1])
    want = x.copy()
    want[0, 0, 0] = 0
    assert np.array_equal(out, want)
    both = R.postprocess(x, 3, largest=True)
    assert both[0, 4, 4] == 2 and both[2, 2, 2] == 0       # ties of class 2: the first in raster order stays


def test_out_of_range_and_non_integer_floats_are_untouched():
    x = np.zeros((4, 4, 4), dtype=np.float32)
    x[0, 0, 0] = 1.0
    x[3, 3, 1:4] = 1.0
    x[1, 1, 1] = 1.5                                       # not a class
    x[2, 2, 2] = 7.0                                       # outside [0, C)
    x[0, 3, 0] = -1.0
    out = R.postprocess(x, 3, largest=True)
    assert (out[1, 1, 1], out[2, 2, 2], out[0, 3, 0], out[0, 0, 0]) == (1.5, 7.0, -1.0, 0.0)
    assert out[3, 3, 1:4].tolist() == [1.0, 1.0, 1.0]
    assert out.dtype == np.float32


# ------------------------------------------------------------------------------------------------------ argument checks
def test_check_post_args_accepts_and_normalises():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import _check_post_args
    assert _check_post_args(4) == (4, 0b1110, 0, True, 26)
    assert _check_post_args(4, largest=False, min_size=5, classes=[3, 1], connectivity=6) == (4, 0b1010, 5, False, 6)
    assert _check_post_args(2, min_size=2 ** 40)[2] == 2 ** 31 - 1
    assert _check_post_args(16, classes=[15])[1] == 1 << 15
    assert _check_post_args(3, min_size=np.int64(3), classes=[np.int32(2)])[1:3] == (0b100, 3)


@pytest.mark.parametrize("kw", [
    dict(num_classes=0), dict(num_classes=17), dict(num_classes=1),            # no foreground class to keep
    dict(num_classes=3, classes=[]), dict(num_classes=3, classes=[0]), dict(num_classes=3, classes=[3]),
    dict(num_classes=3, classes=[1, 1]), dict(num_classes=3, classes=[1.0]), dict(num_classes=3, classes=[True]),
    dict(num_classes=3, min_size=-1), dict(num_classes=3, min_size=2.5), dict(num_classes=3, min_size=True),
    dict(num_classes=3, largest=False), dict(num_classes=3, largest=False, min_size=0), dict(num_classes=3, largest=1),
    dict(num_classes=3, connectivity=8), dict(num_classes=3, connectivity=True), dict(num_classes=3, connectivity="26"),
])
def test_check_post_args_rejects(kw):
    import mivp_amd  # noqa: F401
    from mivp_amd.components import _check_post_args
    with pytest.raises(ValueError):
        _check_post_args(**kw)


def test_check_connectivity():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import _check_connectivity
    assert [_check_connectivity(k) for k in (6, 18, 26)] == [6, 18, 26]
    for bad in (0, 4, 8, 27, None, 6.5, False):
        with pytest.raises(ValueError):
            _check_connectivity(bad)


def test_postprocess_kwargs():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import postprocess_kwargs
    assert postprocess_kwargs(None, 3) is None
    assert postprocess_kwargs({}, 3) == (3, 0b110, 0, True, 26)
    assert postprocess_kwargs({"num_classes": 3, "min_size": 4, "largest": False}, 3) == (3, 0b110, 4, False, 26)
    for bad in ({"num_classes": 4}, {"min_sizes": 3}, {"largest": False}, [("largest", True)], {"classes": [5]}):
        with pytest.raises(ValueError):
            postprocess_kwargs(bad, 3)


def test_cpu_tensors_are_refused():
    import mivp_amd  # noqa: F401
    from mivp_amd.components import label_components, postprocess_labels
    a = torch.zeros((1, 1, 4, 4, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        label_components(a)
    with pytest.raises(RuntimeError, match="GPU"):
        postprocess_labels(a, 2)
