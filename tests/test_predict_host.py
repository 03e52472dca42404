"""CPU: window placement, the padded device table and the importance tables of whole-volume prediction
(mivp_amd.inference.window_origins / window_table / importance_tables), against the rule restated here."""
import itertools
import math

import numpy as np
import pytest

CASES = [((20, 17, 9), (8, 8, 4)), ((13, 30, 11), (6, 10, 4)), ((5, 30, 11), (8, 10, 4)), ((32, 20, 3), (16, 8, 4)),
         ((16, 16, 8), (16, 16, 8))]
OVERLAPS = [0.0, 0.25, 0.5, 0.75]


def _rule(image_size, roi, overlap):
    """The placement rule, written out independently: pad short axes to the roi, interval, count, clamped starts."""
    per_axis = []
    for n, r in zip(image_size, roi):
        n = max(n, r)
        interval = max(int(r * (1 - overlap)), 1)
        count = math.ceil((n - r) / interval) + 1
        per_axis.append([min(i * interval, n - r) for i in range(count)])
    return [list(o) for o in itertools.product(*per_axis)]


@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("image_size,roi", CASES)
def test_window_origins_follow_the_rule_and_cover_the_volume(image_size, roi, overlap):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import window_origins, window_padding
    o = window_origins(image_size, roi, overlap)
    assert o.dtype == np.int32 and o.ndim == 2 and o.shape[1] == 3
    assert o.tolist() == _rule(image_size, roi, overlap)
    pad, pdims = window_padding(image_size, roi)
    for a in range(3):
        n, r = image_size[a], roi[a]
        assert pdims[a] == max(n, r)
        assert pad[a] == ((r - n) // 2 if n < r else 0)
        assert o[:, a].min() == 0 and o[:, a].max() == pdims[a] - r            # the last window is flush with the end
    cover = np.zeros(pdims, dtype=np.int32)
    for s in o:
        cover[s[0]:s[0] + roi[0], s[1]:s[1] + roi[1], s[2]:s[2] + roi[2]] += 1
    assert cover.min() >= 1


def test_roi_equal_to_volume_is_one_window():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import window_origins
    for ov in OVERLAPS:
        assert window_origins((16, 16, 8), (16, 16, 8), ov).tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("sub_batch", [1, 3, 4, 10, 1000])
@pytest.mark.parametrize("image_size,roi", CASES[:3])
def test_window_table_is_padded_to_the_sub_batch(image_size, roi, sub_batch):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import window_origins, window_table
    o = window_origins(image_size, roi, 0.5)
    t = window_table(o, sub_batch)
    n = o.shape[0]
    assert t.dtype == np.int32 and t.shape == (math.ceil(n / sub_batch) * sub_batch, 4)
    assert int(t[:, 3].sum()) == n and (t[:n, 3] == 1).all() and (t[n:, 3] == 0).all()
    assert (t[:n, :3] == o).all()


@pytest.mark.parametrize("roi,sigma_scale", [((8, 8, 4), 0.125), ((6, 10, 4), 0.125), ((96, 96, 96), 0.125),
                                             ((7, 5, 3), 0.3), ((128, 128, 8), 0.125)])
def test_gaussian_tables_match_the_formula(roi, sigma_scale):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import importance_tables
    tabs, floor = importance_tables(roi, "gaussian", sigma_scale)
    mins = []
    for t, r in zip(tabs, roi):
        s = sigma_scale * r
        want = np.array([math.exp(-((i - r // 2) ** 2) / (2 * s * s)) for i in range(r)])
        np.testing.assert_allclose(t, want, rtol=1e-14, atol=0)
        assert t[r // 2] == 1.0
        mins.append(want.min())
    assert floor == max(float(np.prod(mins)), 1e-3)
    full = tabs[0][:, None, None] * tabs[1][None, :, None] * tabs[2][None, None, :]
    assert full.max() == 1.0
    assert np.maximum(full, floor).min() >= 1e-3


def test_gaussian_clamp_engages_for_a_wide_roi():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import importance_tables
    _, floor = importance_tables((96, 96, 96), "gaussian", 0.125)
    assert floor == 1e-3                                                      # exp(-8)^3 ~ 4e-11 < 1e-3


def test_constant_tables_are_ones():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import importance_tables
    tabs, floor = importance_tables((4, 5, 6), "constant")
    assert [t.tolist() for t in tabs] == [[1.0] * 4, [1.0] * 5, [1.0] * 6] and floor == 1.0


def test_invalid_arguments_raise():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import importance_tables, window_origins, window_table
    for ov in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            window_origins((16, 16, 16), (8, 8, 8), ov)
    with pytest.raises(ValueError):
        window_origins((16, 16), (8, 8, 8), 0.5)
    with pytest.raises(ValueError):
        window_origins((16, 16, 16), (8, 0, 8), 0.5)
    with pytest.raises(ValueError):
        window_table(window_origins((16, 16, 16), (8, 8, 8), 0.5), 0)
    with pytest.raises(ValueError):
        importance_tables((8, 8, 8), "triangle")
    with pytest.raises(ValueError):
        importance_tables((8, 8, 8), "gaussian", 0.0)


def test_predictor_refuses_a_cpu_model():
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    model = torch.nn.Conv3d(1, 2, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        SlidingWindowPredictor(model, (16, 16, 16), 1, 2, (8, 8, 8))
    with pytest.raises(ValueError):
        SlidingWindowPredictor(model, (16, 16, 16), 1, 2, (8, 8, 8), overlap=1.0)
