"""CPU: the shared host-side argument checks (mivp_amd._host) -- an accept / reject table per helper with the message each
refusal carries, the same refusal through every caller of a shared check, ``window_table`` as the one-code ``tta_table``,
the frozen call surface of the evaluation modules, and two source checks that keep the helpers in one place."""
import ctypes
import glob
import importlib
import inspect
import math
import os

import numpy as np
import pytest
import torch

MODULES = ("inference", "surface", "components", "regions", "calibration", "scan", "scanstats")


def _host():
    import mivp_amd  # noqa: F401
    from mivp_amd import _host
    return _host


# ---------------------------------------------------------------------------------------------------------------------
# accept / reject tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("good,want", [(1, 1), (16, 16), (np.int64(5), 5), ("3", 3), (True, 1)])
def test_check_classes_accepts(good, want):
    got = _host().check_classes(good)
    assert type(got) is int and got == want


@pytest.mark.parametrize("bad", [0, 17, -1, False, 2 ** 40])
def test_check_classes_rejects(bad):
    with pytest.raises(ValueError, match=rf"num_classes must be in 1\.\.16, got {bad}"):
        _host().check_classes(bad)


@pytest.mark.parametrize("good,want", [((1, 1, 1), (1.0, 1.0, 1.0)), ([0.5, 2, 3], (0.5, 2.0, 3.0)),
                                       (np.array([1e-3, 7, 2.5]), (1e-3, 7.0, 2.5)), ((True, 1, 1), (1.0, 1.0, 1.0))])
def test_check_spacing_accepts(good, want):
    got = _host().check_spacing(good)
    assert got == want and all(type(a) is float for a in got)


@pytest.mark.parametrize("bad", [(1, 1), (1, 1, 1, 1), (1, 1, 0), (1, -1, 1), (1, 1, math.inf), (math.nan, 1, 1),
                                 (False, 1, 1), ()])
def test_check_spacing_rejects(bad):
    with pytest.raises(ValueError, match="spacing must be three positive sizes in mm, got"):
        _host().check_spacing(bad)


@pytest.mark.parametrize("good", [6, 18, 26, np.int32(18)])
def test_check_connectivity_accepts(good):
    got = _host().check_connectivity(good)
    assert type(got) is int and got == good


@pytest.mark.parametrize("bad", [True, False, 0, 7, 27, "6", None, 6.5])
def test_check_connectivity_rejects(bad):
    with pytest.raises(ValueError, match=r"connectivity must be one of \(6, 18, 26\), got"):
        _host().check_connectivity(bad)


@pytest.mark.parametrize("ncls,classes,want", [(4, None, 0b1110), (2, None, 0b10), (4, [3, 1], 0b1010), (4, (2,), 0b100),
                                               (16, [15], 1 << 15), (3, [np.int32(2)], 0b100), (3, iter([1, 2]), 0b110)])
def test_class_mask_accepts(ncls, classes, want):
    got = _host().class_mask(ncls, classes)
    assert type(got) is int and got == want


CLASS_REJECTS = [(1, None, "classes is empty (num_classes=1 has no foreground class)"), (3, [], "classes is empty"),
                 (3, [0], "classes must be ints in 1..2, got 0"), (3, [3], "classes must be ints in 1..2, got 3"),
                 (3, [-1], "classes must be ints in 1..2, got -1"), (3, [True], "classes must be ints in 1..2, got True"),
                 (3, [False], "classes must be ints in 1..2, got False"), (3, [1.0], "classes must be ints in 1..2, got 1.0"),
                 (3, ["1"], "classes must be ints in 1..2, got '1'"), (3, [1, 1], "classes has duplicates: [1, 1]"),
                 (4, [2, 3, 2], "classes has duplicates: [2, 3, 2]")]


@pytest.mark.parametrize("ncls,classes,text", CLASS_REJECTS)
def test_class_mask_rejects(ncls, classes, text):
    with pytest.raises(ValueError) as e:
        _host().class_mask(ncls, classes)
    assert str(e.value) == text
    if classes == []:
        assert "num_classes=1" not in str(e.value)              # the hint is for the default only


@pytest.mark.parametrize("good,want", [(0, 0), (5, 5), (np.int64(3), 3), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31, 2 ** 31 - 1),
                                       (2 ** 40, 2 ** 31 - 1)])
def test_check_min_size_accepts_and_clamps(good, want):
    got = _host().check_min_size(good)
    assert type(got) is int and got == want


MIN_SIZE_REJECTS = [-1, True, False, 1.5, 2.0, "3", None, np.int64(-2)]


@pytest.mark.parametrize("bad", MIN_SIZE_REJECTS)
def test_check_min_size_rejects(bad):
    with pytest.raises(ValueError) as e:
        _host().check_min_size(bad)
    assert str(e.value) == f"min_size must be a non-negative int, got {bad!r}"


@pytest.mark.parametrize("v,want", [(0, True), (-3, True), (2 ** 70, True), (np.int32(4), True), (np.uint8(4), True),
                                    (True, False), (False, False), (np.bool_(True), False), (1.0, False),
                                    (np.float32(1), False), ("1", False), (None, False)])
def test_plain_int(v, want):
    assert _host().plain_int(v) is want


@pytest.mark.parametrize("good,want", [((1, 2, 3), [1, 2, 3]), ([7, 1, 2 ** 31 - 1], [7, 1, 2 ** 31 - 1]),
                                       (np.array([4, 5, 6]), [4, 5, 6]), (torch.Size([2, 3, 4]), [2, 3, 4]),
                                       ((1.9, 2, 3), [1, 2, 3]), ((True, False, 2), [1, 0, 2])])
def test_i3_accepts(good, want):
    a = _host().i3(good)
    assert isinstance(a, ctypes.Array) and a._type_ is ctypes.c_int32 and len(a) == 3 and list(a) == want


@pytest.mark.parametrize("bad,exc", [((1, 2, 3, 4), IndexError), (("a", 2, 3), ValueError), ((None, 2, 3), TypeError),
                                     (5, TypeError)])
def test_i3_rejects(bad, exc):
    with pytest.raises(exc):                                     # the refusals of int() and ctypes: i3 words none itself
        _host().i3(bad)


def test_iou_dice_by_hand():
    # (intersection, predicted, target): class 0 -> IoU 3 / (5 + 4 - 3), Dice 6 / 9; class 1 -> 2 / 6, 4 / 8; class 2 has
    # no voxel on either side: 0 / 1e-6 = 0, not NaN
    table = [[3, 5, 4], [2, 2, 6], [0, 0, 0]]
    want_iou = (3 / (6 + 1e-6) + 2 / (6 + 1e-6) + 0.0) / 3
    want_dice = (6 / (9 + 1e-6) + 4 / (8 + 1e-6) + 0.0) / 3
    for t in (torch.tensor(table, dtype=torch.int64), torch.tensor(table, dtype=torch.float64),
              torch.tensor(table, dtype=torch.int32)):
        iou, dice = _host().iou_dice(t)
        assert type(iou) is float and type(dice) is float
        assert iou == pytest.approx(want_iou, rel=1e-14, abs=0) and dice == pytest.approx(want_dice, rel=1e-14, abs=0)
    assert _host().iou_dice(torch.zeros((2, 3), dtype=torch.int64)) == (0.0, 0.0)
    assert _host().iou_dice(torch.tensor([[7, 7, 7]])) == (pytest.approx(7 / (7 + 1e-6)), pytest.approx(14 / (14 + 1e-6)))


def test_segmetrics_compute_is_iou_dice():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SegMetrics
    m = SegMetrics(2, "cpu")
    m.counts.copy_(torch.tensor([[3, 5, 4], [0, 0, 0]]))
    assert m.compute() == _host().iou_dice(m.counts) == (pytest.approx(0.25, abs=1e-6), pytest.approx(1 / 3, abs=1e-6))


# ---------------------------------------------------------------------------------------------------------------------
# one check, every caller: the same bad input gives the same exception type and text
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls,classes,text", CLASS_REJECTS)
def test_classes_refusal_is_the_same_through_every_caller(ncls, classes, text):
    import mivp_amd  # noqa: F401
    from mivp_amd import components, regions
    seen = []
    for call in (lambda: components._check_post_args(ncls, classes=classes),
                 lambda: components.postprocess_kwargs({"classes": classes}, ncls),
                 lambda: regions.check_region_kwargs(ncls, classes=classes),
                 lambda: regions.check_lesion_kwargs(ncls, classes=classes)):
        with pytest.raises(ValueError) as e:
            call()
        seen.append((type(e.value), str(e.value)))
    assert seen == [(ValueError, text)] * 4


@pytest.mark.parametrize("bad", MIN_SIZE_REJECTS)
def test_min_size_refusal_is_the_same_through_every_caller(bad):
    import mivp_amd  # noqa: F401
    from mivp_amd import components, regions
    seen = []
    for call in (lambda: components._check_post_args(3, min_size=bad), lambda: regions.check_lesion_kwargs(3, min_size=bad)):
        with pytest.raises(ValueError) as e:
            call()
        seen.append((type(e.value), str(e.value)))
    assert seen == [(ValueError, f"min_size must be a non-negative int, got {bad!r}")] * 2


def test_min_size_clamp_is_the_same_through_both_callers():
    import mivp_amd  # noqa: F401
    from mivp_amd import components, regions
    assert components._check_post_args(3, min_size=2 ** 40)[2] == 2 ** 31 - 1
    assert regions._check_lesion_args(0.0, 2 ** 40, 4096, None)[1] == 2 ** 31 - 1


def test_predictor_num_classes_message_keeps_its_old_prefix():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    for bad in (0, 17):
        with pytest.raises(ValueError, match=rf"^num_classes must be in 1\.\.16, got {bad}$"):
            SlidingWindowPredictor(torch.nn.Conv3d(1, 2, 1), (16, 16, 16), 1, bad, (8, 8, 8))


# ---------------------------------------------------------------------------------------------------------------------
# window_table is tta_table with the one code 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub_batch", [1, 3, 10])
def test_window_table_is_the_one_code_tta_table(sub_batch):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import tta_table, window_origins, window_table
    o = window_origins((10, 13, 7), (16, 8, 12), 0.5)
    a, b = window_table(o, sub_batch), tta_table(o, sub_batch, (0,))
    assert a.dtype == b.dtype == np.int32
    assert a.shape == b.shape == (-(-o.shape[0] // sub_batch) * sub_batch, 4)
    assert np.array_equal(a, b)
    assert np.array_equal(a[:o.shape[0], :3], o) and (a[:o.shape[0], 3] == 1).all() and (a[o.shape[0]:] == 0).all()
    with pytest.raises(ValueError, match="sub_batch must be >= 1"):
        window_table(o, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the call surface: every public function of the evaluation modules and every public method of the predictor, as
# str(inspect.signature(fn)), frozen from the commit before the helpers were shared
# ---------------------------------------------------------------------------------------------------------------------
SURFACE = {
    'inference.evaluate_volume':
        "(model, x: 'torch.Tensor', seg: 'torch.Tensor', roi: 'Sequence[int]', num_classes: 'int', "
        "overlap: 'float' = 0.5, mode: 'str' = 'gaussian', sigma_scale: 'float' = 0.125, "
        "sub_batch: 'int' = 10, graph: 'bool' = False, postprocess: 'Optional[Dict]' = None, "
        "mirror_axes: 'Sequence[int]' = (), skip: 'Optional[WindowSkip]' = None, *, "
        "fit: 'Optional[WindowFit]' = None) -> 'Tuple[float, "
        "float]'",
    'inference.evaluate_volume_calibration':
        "(model, x: 'torch.Tensor', seg: 'torch.Tensor', roi: 'Sequence[int]', num_classes: 'int', "
        "overlap: 'float' = 0.5, mode: 'str' = 'gaussian', sigma_scale: 'float' = 0.125, "
        "sub_batch: 'int' = 10, graph: 'bool' = False, mirror_axes: 'Sequence[int]' = (), "
        "n_bins: 'int' = 15, out=None, skip: 'Optional[WindowSkip]' = None, *, fit: 'Optional[WindowFit]' = None)",
    'inference.evaluate_volume_lesions':
        "(model, x: 'torch.Tensor', seg: 'torch.Tensor', roi: 'Sequence[int]', num_classes: 'int', "
        "overlap: 'float' = 0.5, mode: 'str' = 'gaussian', sigma_scale: 'float' = 0.125, "
        "sub_batch: 'int' = 10, graph: 'bool' = False, spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), "
        "postprocess: 'Optional[Dict]' = None, mirror_axes: 'Sequence[int]' = (), "
        "with_scores: 'bool' = False, skip: 'Optional[WindowSkip]' = None, *, "
        "fit: 'Optional[WindowFit]' = None, **lesion_kwargs)",
    'inference.evaluate_volume_surface':
        "(model, x: 'torch.Tensor', seg: 'torch.Tensor', roi: 'Sequence[int]', num_classes: 'int', "
        "overlap: 'float' = 0.5, mode: 'str' = 'gaussian', sigma_scale: 'float' = 0.125, "
        "sub_batch: 'int' = 10, graph: 'bool' = False, spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), "
        "percentile: 'float' = 95.0, tolerance: 'float' = 1.0, include_background: 'bool' = False, "
        "postprocess: 'Optional[Dict]' = None, mirror_axes: 'Sequence[int]' = (), "
        "skip: 'Optional[WindowSkip]' = None, *, fit: 'Optional[WindowFit]' = None) -> 'Dict[str, object]'",
    'inference.flip_codes':
        "(mirror_axes: 'Sequence[int]' = ()) -> 'Tuple[int, ...]'",
    'inference.importance_tables':
        "(roi: 'Sequence[int]', mode: 'str' = 'gaussian', sigma_scale: 'float' = 0.125)",
    'inference.predict_scan_volume':
        "(model, raw: 'torch.Tensor', affine, roi: 'Sequence[int]', num_classes: 'int', out_size=None, "
        "axcodes: 'str' = 'RAS', overlap: 'float' = 0.5, mode: 'str' = 'gaussian', "
        "sigma_scale: 'float' = 0.125, sub_batch: 'int' = 10, graph: 'bool' = False, "
        "restore: 'str' = 'labels', postprocess: 'Optional[Dict]' = None, "
        "mirror_axes: 'Sequence[int]' = (), skip: 'Optional[WindowSkip]' = None, *, "
        "fit: 'Optional[WindowFit]' = None, **intensity) -> 'Dict[str, torch.Tensor]'",
    'inference.predict_volume':
        "(model, x: 'torch.Tensor', roi: 'Sequence[int]', num_classes: 'int', overlap: 'float' = 0.5, "
        "mode: 'str' = 'gaussian', sigma_scale: 'float' = 0.125, sub_batch: 'int' = 10, "
        "graph: 'bool' = False, return_logits: 'bool' = False, postprocess: 'Optional[Dict]' = None, "
        "mirror_axes: 'Sequence[int]' = (), return_probs: 'bool' = False, "
        "return_confidence: 'bool' = False, return_entropy: 'bool' = False, "
        "skip: 'Optional[WindowSkip]' = None, *, fit: 'Optional[WindowFit]' = None) -> 'Dict[str, torch.Tensor]'",
    'inference.sliding_window_view':
        "(x: 'torch.Tensor', roi: 'Sequence[int]') -> 'torch.Tensor'",
    'inference.sliding_windows':
        "(x: 'torch.Tensor', roi: 'Sequence[int]') -> 'torch.Tensor'",
    'inference.summarize':
        "(values: 'List[float]') -> 'Tuple[float, float]'",
    'inference.test_volume':
        "(model, x: 'torch.Tensor', seg: 'torch.Tensor', roi: 'Sequence[int]', num_classes: 'int', "
        "sub_batch: 'int' = 10)",
    'inference.tta_table':
        "(origins: 'np.ndarray', sub_batch: 'int', codes: 'Sequence[int]') -> 'np.ndarray'",
    'inference.window_batch':
        "(win_view: 'torch.Tensor', begin: 'int', end: 'int') -> 'torch.Tensor'",
    'inference.window_grid':
        "(image_size: 'Sequence[int]', roi: 'Sequence[int]') -> 'Tuple[List[slice], List[int], "
        "List[int]]'",
    'inference.window_origins':
        "(image_size: 'Sequence[int]', roi: 'Sequence[int]', overlap: 'float') -> 'np.ndarray'",
    'inference.window_padding':
        "(image_size: 'Sequence[int]', roi: 'Sequence[int]') -> 'Tuple[Tuple[int, int, int], Tuple[int, "
        "int, int]]'",
    'inference.window_table':
        "(origins: 'np.ndarray', sub_batch: 'int') -> 'np.ndarray'",
    'inference.SlidingWindowPredictor.__init__':
        "(self, model, image_size: 'Sequence[int]', in_channels: 'int', num_classes: 'int', "
        "roi: 'Sequence[int]', overlap: 'float' = 0.5, mode: 'str' = 'gaussian', "
        "sigma_scale: 'float' = 0.125, sub_batch: 'int' = 10, graph: 'bool' = False, "
        "mirror_axes: 'Sequence[int]' = (), skip: 'Optional[WindowSkip]' = None, *, fit: 'Optional[WindowFit]' = None)",
    'inference.SlidingWindowPredictor.evaluate':
        "(self, x: 'torch.Tensor', seg: 'torch.Tensor', "
        "postprocess: 'Optional[Dict]' = None) -> 'Tuple[float, float]'",
    'inference.SlidingWindowPredictor.evaluate_calibration':
        "(self, x: 'torch.Tensor', seg: 'torch.Tensor', n_bins: 'int' = 15, out=None)",
    'inference.SlidingWindowPredictor.evaluate_lesions':
        "(self, x: 'torch.Tensor', seg: 'torch.Tensor', spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), "
        "postprocess: 'Optional[Dict]' = None, with_scores: 'bool' = False, **lesion_kwargs)",
    'inference.SlidingWindowPredictor.evaluate_scan':
        "(self, raw: 'torch.Tensor', seg_native: 'torch.Tensor', geom, "
        "postprocess: 'Optional[Dict]' = None, **intensity) -> 'Tuple[float, float]'",
    'inference.SlidingWindowPredictor.evaluate_surface':
        "(self, x: 'torch.Tensor', seg: 'torch.Tensor', spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), "
        "percentile: 'float' = 95.0, tolerance: 'float' = 1.0, include_background: 'bool' = False, "
        "postprocess: 'Optional[Dict]' = None) -> 'Dict[str, object]'",
    'inference.SlidingWindowPredictor.predict':
        "(self, x: 'torch.Tensor', return_logits: 'bool' = False, postprocess: 'Optional[Dict]' = None, "
        "return_probs: 'bool' = False, return_confidence: 'bool' = False, "
        "return_entropy: 'bool' = False) -> 'Dict[str, torch.Tensor]'",
    'inference.SlidingWindowPredictor.predict_regions':
        "(self, x: 'torch.Tensor', return_logits: 'bool' = False, postprocess: 'Optional[Dict]' = None, "
        "return_probs: 'bool' = False, return_confidence: 'bool' = False, "
        "return_entropy: 'bool' = False, spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), "
        "**region_kwargs) -> 'Dict[str, object]'",
    'inference.SlidingWindowPredictor.predict_scan':
        "(self, raw: 'torch.Tensor', geom, restore: 'str' = 'labels', "
        "postprocess: 'Optional[Dict]' = None, **intensity) -> 'Dict[str, torch.Tensor]'",
    'inference.SlidingWindowPredictor.set_region':
        "(self, mask: 'Optional[torch.Tensor]')",
    'surface.distance_transform_sq':
        "(seeds: 'torch.Tensor', spacing: 'Sequence[float]' = (1.0, 1.0, 1.0)) -> 'torch.Tensor'",
    'surface.surface_map':
        "(labels: 'torch.Tensor', num_classes: 'int') -> 'torch.Tensor'",
    'surface.surface_metrics':
        "(pred: 'torch.Tensor', target: 'torch.Tensor', num_classes: 'int', "
        "spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), percentile: 'float' = 95.0, "
        "tolerance: 'float' = 1.0, include_background: 'bool' = False) -> 'Dict[str, torch.Tensor]'",
    'components.label_components':
        "(x: 'torch.Tensor', connectivity: 'int' = 6) -> 'Tuple[torch.Tensor, int]'",
    'components.postprocess_kwargs':
        "(postprocess: 'Optional[Dict]', num_classes: 'int')",
    'components.postprocess_labels':
        "(labels: 'torch.Tensor', num_classes: 'int', largest: 'bool' = True, min_size: 'int' = 0, "
        "classes: 'Optional[Iterable[int]]' = None, connectivity: 'int' = 26) -> 'torch.Tensor'",
    'regions.check_lesion_kwargs':
        '(num_classes, spacing=(1.0, 1.0, 1.0), **kwargs)',
    'regions.check_region_kwargs':
        '(num_classes, spacing=(1.0, 1.0, 1.0), **kwargs)',
    'regions.lesion_metrics':
        "(pred: 'torch.Tensor', target: 'torch.Tensor', num_classes: 'int', "
        "spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), connectivity: 'int' = 26, "
        "iou_threshold: 'float' = 0.0, min_size: 'int' = 0, classes: 'Optional[Iterable[int]]' = None, "
        "max_regions: 'int' = 4096, max_pairs: 'Optional[int]' = None) -> 'LesionReport'",
    'regions.lesion_score_metrics':
        "(pred: 'torch.Tensor', target: 'torch.Tensor', num_classes: 'int', "
        "pred_image: 'Optional[torch.Tensor]', spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), "
        "connectivity: 'int' = 26, iou_threshold: 'float' = 0.0, min_size: 'int' = 0, "
        "classes: 'Optional[Iterable[int]]' = None, max_regions: 'int' = 4096, "
        "max_pairs: 'Optional[int]' = None) -> 'LesionReport'",
    'regions.region_stats':
        "(labels: 'torch.Tensor', num_classes: 'int', image: 'Optional[torch.Tensor]' = None, "
        "spacing: 'Sequence[float]' = (1.0, 1.0, 1.0), connectivity: 'int' = 26, "
        "classes: 'Optional[Iterable[int]]' = None, max_regions: 'int' = 4096) -> 'RegionTable'",
    'calibration.calibration_tables':
        "(probs: 'torch.Tensor', target: 'torch.Tensor', num_classes: 'int', n_bins: 'int' = 15, "
        "out: 'Optional[CalibrationReport]' = None, flags: 'int' = 0) -> 'CalibrationReport'",
    'calibration.table_words':
        "(num_classes: 'int', n_bins: 'int') -> 'int'",
    'scan.check_predict_args':
        "(image_size, in_channels: 'int', raw, geom, restore: 'str', "
        "postprocess=None) -> 'torch.Tensor'",
    'scan.intensity_map':
        "(a_min: 'float' = -1000.0, a_max: 'float' = 1000.0, b_min: 'float' = 0.0, "
        "b_max: 'float' = 1.0)",
    'scan.linear_taps':
        "(n_in: 'int', n_out: 'int') -> 'Tuple[np.ndarray, np.ndarray, np.ndarray]'",
    'scan.nearest_indices':
        "(n_in: 'int', n_out: 'int') -> 'np.ndarray'",
    'scan.prepare_labels':
        "(seg: 'torch.Tensor', geom: 'ScanGeometry', out: 'Optional[torch.Tensor]' = None, "
        "check: 'bool' = True, flags: 'int' = 0) -> 'torch.Tensor'",
    'scan.prepare_scan':
        "(raw: 'torch.Tensor', geom: 'ScanGeometry', a_min: 'Optional[float]' = None, "
        "a_max: 'Optional[float]' = None, b_min: 'float' = 0.0, b_max: 'float' = 1.0, "
        "clip: 'bool' = True, out: 'Optional[torch.Tensor]' = None, flags: 'int' = 0, window=None, "
        "mask: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
    'scan.restore_labels':
        "(labels: 'torch.Tensor', geom: 'ScanGeometry', out: 'Optional[torch.Tensor]' = None, "
        "flags: 'int' = 0) -> 'torch.Tensor'",
    'scan.restore_labels_from_logits':
        "(logits: 'torch.Tensor', geom: 'ScanGeometry', out: 'Optional[torch.Tensor]' = None, "
        "flags: 'int' = 0) -> 'torch.Tensor'",
    'scanstats.check_window_args':
        "(window, raw: 'torch.Tensor', mask, shape) -> 'None'",
    'scanstats.resolve_window':
        "(window, raw: 'torch.Tensor', mask) -> 'WindowSlot'",
    'scanstats.scan_histogram':
        "(raw: 'torch.Tensor', mask: 'Optional[torch.Tensor]' = None, above: 'Optional[int]' = None, "
        "out: 'Optional[ScanHistogram]' = None, base: 'Optional[int]' = None, "
        "flags: 'int' = 0) -> 'ScanHistogram'",
    'scanstats.window_slot':
        "(hist: 'ScanHistogram', spec: 'IntensityWindow', "
        "out: 'Optional[WindowSlot]' = None) -> 'WindowSlot'",
}


def _surface():
    import mivp_amd  # noqa: F401
    out = {}
    for m in MODULES:
        mod = importlib.import_module(f"mivp_amd.{m}")
        for k, v in sorted(vars(mod).items()):
            if inspect.isfunction(v) and not k.startswith("_") and v.__module__ == mod.__name__:
                out[f"{m}.{k}"] = str(inspect.signature(v))
    cls = importlib.import_module("mivp_amd.inference").SlidingWindowPredictor
    for k, v in sorted(vars(cls).items()):
        if inspect.isfunction(v) and (not k.startswith("_") or k == "__init__"):
            out[f"inference.SlidingWindowPredictor.{k}"] = str(inspect.signature(v))
    return out


def test_public_surface_is_frozen():
    got = _surface()
    assert sorted(got) == sorted(SURFACE)
    for k in SURFACE:
        assert got[k] == SURFACE[k], k


def test_package_exports_resolve():
    import mivp_amd
    for name in ("SlidingWindowPredictor", "predict_volume", "evaluate_volume", "evaluate_volume_surface",
                 "predict_scan_volume", "evaluate_volume_lesions", "evaluate_volume_calibration", "WindowSkip",
                 "surface_map", "distance_transform_sq", "surface_metrics", "label_components", "postprocess_labels",
                 "region_stats", "lesion_metrics", "lesion_score_metrics", "RegionTable", "LesionReport",
                 "calibration_tables", "CalibrationReport", "ScanGeometry", "prepare_scan", "prepare_labels",
                 "restore_labels", "restore_labels_from_logits", "scan_histogram", "window_slot", "IntensityWindow",
                 "ScanHistogram", "WindowSlot", "ScanReport"):
        assert callable(getattr(mivp_amd, name)), name


# ---------------------------------------------------------------------------------------------------------------------
# source checks: the helpers live in one place and no module borrows a private name from surface or components
# ---------------------------------------------------------------------------------------------------------------------
def _sources():
    import mivp_amd
    files = sorted(glob.glob(os.path.join(list(mivp_amd.__path__)[0], "*.py")))
    assert len(files) > 10 and any(f.endswith("_host.py") for f in files)
    return {os.path.basename(f): open(f).read() for f in files}


def test_i3_is_defined_once():
    src = _sources()
    assert [n for n, text in src.items() if "def _i3" in text] == []
    assert [n for n, text in src.items() if "def i3(" in text] == ["_host.py"]


def test_no_private_imports_from_surface_or_components():
    for name, text in _sources().items():
        assert "from .surface import _" not in text, name
        assert "from .components import _" not in text, name
