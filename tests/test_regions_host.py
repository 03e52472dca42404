"""CPU: the numpy / scipy restatement of the region statistics and lesion-wise metrics (tests/regions_ref.py) on hand-made
volumes whose answers are written out, the argument checks of mivp_amd.regions, the predictor's new surface and the C ABI
declarations of the region entry points (they joined ABI 18 without a bump)."""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytest.importorskip("scipy.ndimage")
import regions_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mivp_region_stats", "mivp_region_stats_ws", "mivp_region_overlap", "mivp_region_overlap_ws",
           "mivp_lesion_match")


def _line(n, *runs):
    """[1, 1, n] class map with class 1 on the inclusive runs (a, b)."""
    x = np.zeros((1, 1, n), dtype=np.uint8)
    for a, b in runs:
        x[0, 0, a:b + 1] = 1
    return x


# ------------------------------------------------------------------------------------------- the restatement, by hand
def test_two_cubes_and_an_l_shape():
    x = np.zeros((8, 8, 8), dtype=np.uint8)
    x[0:2, 0:2, 0:2] = 1
    x[4:7, 4:7, 4:7] = 2
    for w, d in ((5, 0), (6, 0), (7, 0), (7, 1), (7, 2)):
        x[0, w, d] = 1
    h, w, d = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    img = (100 * h + 10 * w + d).astype(np.int32)
    r = R.region_stats(x, 3, img, spacing=(2.0, 2.0, 0.5), connectivity=6)
    assert r["n"] == 3
    assert r["cls"].tolist() == [1, 1, 2]
    assert r["size"].tolist() == [8, 5, 27]
    assert r["first"].tolist() == [0, 40, 292]
    assert r["bbox"].tolist() == [[0, 0, 0, 1, 1, 1], [0, 5, 0, 0, 7, 2], [4, 4, 4, 6, 6, 6]]
    assert r["coord_sum"].tolist() == [[4, 4, 4], [0, 32, 3], [135, 135, 135]]
    assert r["extent"].tolist() == [[2, 2, 2], [1, 3, 3], [3, 3, 3]]
    assert r["volume_mm3"].tolist() == [16.0, 10.0, 54.0]
    assert r["centroid"][2].tolist() == [5.0, 5.0, 5.0] and r["centroid_mm"][2].tolist() == [10.0, 10.0, 2.5]
    assert r["vmin"].tolist() == [0, 50, 444] and r["vmax"].tolist() == [111, 72, 666]
    assert r["vsum"].tolist() == [444, 323, 27 * 555]
    assert r["vsqsum"][1] == 21225
    assert r["vmean"][1] == 64.6 and math.isclose(r["vstd"][1], math.sqrt(21225 / 5 - 64.6 ** 2), rel_tol=1e-12)
    assert r["labels"][0, 7, 2] == 2 and r["labels"][5, 5, 5] == 3 and r["labels"][1, 1, 1] == 1
    only2 = R.region_stats(x, 3, classes=[2], connectivity=6)              # unlisted classes take no number
    assert only2["n"] == 1 and only2["cls"].tolist() == [2] and only2["labels"][5, 5, 5] == 1
    assert R.region_stats(x, 3, connectivity=26)["n"] == 3


def test_reference_split_across_two_predictions():
    m = R.lesion_metrics(_line(12, (0, 2), (5, 8)), _line(12, (0, 9)), 2, connectivity=6)
    assert m["counts"].tolist() == [[0, 0, 0, 0], [1, 2, 1, 2]]
    assert m["overlap"].tolist() == [7] and m["touching"].tolist() == [7]
    assert m["best_pred"].tolist() == [2] and m["best_overlap"].tolist() == [4]
    assert m["best_iou"].tolist() == [0.4] and m["dice_t"].tolist() == [14 / 17]
    assert m["pairs"].tolist() == [[1, 1, 3], [2, 1, 4]]
    assert m["sensitivity"][1] == 1.0 and m["precision"][1] == 1.0 and m["f1"][1] == 1.0
    assert m["lesion_dice"][1] == 14 / 17


def test_one_prediction_bridging_two_references():
    pred, tgt = _line(12, (2, 7)), _line(12, (0, 3), (6, 9))
    m = R.lesion_metrics(pred, tgt, 2, connectivity=6)
    assert m["counts"][1].tolist() == [2, 1, 2, 1]
    assert m["overlap"].tolist() == [2, 2] and m["touching"].tolist() == [6, 6]
    assert m["best_pred"].tolist() == [1, 1] and m["best_iou"].tolist() == [0.25, 0.25]
    assert m["dice_t"].tolist() == [0.4, 0.4] and m["lesion_dice"][1] == 0.4
    strict = R.lesion_metrics(pred, tgt, 2, connectivity=6, iou_threshold=0.5)
    assert strict["counts"][1].tolist() == [2, 1, 0, 0]
    assert strict["sensitivity"][1] == 0.0 and strict["precision"][1] == 0.0 and strict["f1"][1] == 0.0
    assert strict["lesion_dice"][1] == 0.8 / 3


def test_a_miss_and_a_false_alarm_and_min_size():
    pred, tgt = _line(24, (1, 3), (20, 21)), _line(24, (0, 2), (10, 12))
    m = R.lesion_metrics(pred, tgt, 2, connectivity=6)
    assert m["counts"][1].tolist() == [2, 2, 1, 1]
    assert m["detected"].tolist() == [1, 0] and m["matched"].tolist() == [1, 0]
    assert m["sensitivity"][1] == 0.5 and m["precision"][1] == 0.5 and m["f1"][1] == 0.5
    assert m["dice_t"].tolist() == [4 / 6, 0.0] and m["lesion_dice"][1] == (4 / 6) / 3
    big = R.lesion_metrics(pred, tgt, 2, connectivity=6, min_size=3)       # the 2-voxel false alarm is ignored
    assert big["counts"][1].tolist() == [2, 1, 1, 1] and big["lesion_dice"][1] == (4 / 6) / 2
    none = R.lesion_metrics(pred, tgt, 2, connectivity=6, min_size=4)      # applied on both sides: nothing is left
    assert none["counts"][1].tolist() == [0, 0, 0, 0] and np.isnan(none["sensitivity"][1])
    assert none["overlap"].tolist() == [0, 0] and none["valid"].tolist() == [False, False]


def test_tie_for_best_pred_goes_to_the_smaller_label():
    m = R.lesion_metrics(_line(12, (0, 1), (4, 5)), _line(12, (0, 9)), 2, connectivity=6)
    assert m["best_pred"].tolist() == [1] and m["best_overlap"].tolist() == [2] and m["touching"].tolist() == [4]


def test_iou_of_exactly_one_half_matches_at_one_half():
    m = R.lesion_metrics(_line(8, (2, 7)), _line(8, (0, 5)), 2, connectivity=6, iou_threshold=0.5)
    assert m["pairs"].tolist() == [[1, 1, 4]] and m["best_iou"].tolist() == [0.5]
    assert m["counts"][1].tolist() == [1, 1, 1, 1]


def test_empty_class_gives_nan():
    m = R.lesion_metrics(_line(8, (0, 3)), _line(8, (2, 5)), 3, connectivity=6)
    for k in ("sensitivity", "precision", "f1", "lesion_dice"):
        assert np.isnan(m[k][0]) and np.isnan(m[k][2]) and not np.isnan(m[k][1]), k
    assert m["counts"][2].tolist() == [0, 0, 0, 0]


def test_pairs_of_different_classes_do_not_count():
    pred, tgt = _line(8, (0, 3)), _line(8, (0, 3)) * 2
    m = R.lesion_metrics(pred, tgt, 3, connectivity=6)
    assert m["pairs"].shape == (0, 3) and m["counts"].tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0]]


# ------------------------------------------------------------------------------------------- argument checks
def test_rejected_arguments():
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import regions as G
    ok = G._check_region_args(3, 26, None, 4096, (1, 1, 1))
    assert ok == (3, 0b110, 26, 4096, (1.0, 1.0, 1.0))
    assert G._check_region_args(3, 6, [2], 16, (1, 2, 3))[1] == 0b100
    for kw in (dict(num_classes=0), dict(num_classes=17), dict(connectivity=8), dict(connectivity=True),
               dict(classes=[0]), dict(classes=[3]), dict(classes=[1, 1]), dict(classes=[]), dict(classes=[1.5]),
               dict(num_classes=1), dict(max_regions=0), dict(max_regions=2 ** 24 + 1), dict(max_regions=1.5),
               dict(max_regions=True), dict(spacing=(1, 1)), dict(spacing=(1, 0, 1)), dict(spacing=(1, float("nan"), 1))):
        args = dict(num_classes=3, connectivity=26, classes=None, max_regions=4096, spacing=(1, 1, 1))
        args.update(kw)
        with pytest.raises(ValueError):
            G._check_region_args(**args)
    assert G._check_lesion_args(0.0, 0, 4096, None) == (0.0, 0, 16384)
    assert G._check_lesion_args(0.5, 7, 64, 10) == (0.5, 7, 10)
    for kw in (dict(iou_threshold=-0.1), dict(iou_threshold=1.5), dict(iou_threshold=float("nan")),
               dict(iou_threshold="0.5"), dict(min_size=-1), dict(min_size=1.5), dict(min_size=True),
               dict(max_pairs=0), dict(max_pairs=2 ** 28 + 1), dict(max_pairs=2.5)):
        with pytest.raises(ValueError):
            G._check_lesion_args(**kw)
    G.check_region_kwargs(3, (1, 1, 2), connectivity=6, classes=[2], max_regions=8)
    G.check_lesion_kwargs(3, (1, 1, 2), connectivity=6, iou_threshold=0.5, min_size=2, classes=[1], max_regions=8, max_pairs=9)
    for fn, bad in ((G.check_region_kwargs, dict(bogus=1)), (G.check_region_kwargs, dict(iou_threshold=0.5)),
                    (G.check_region_kwargs, dict(connectivity=7)), (G.check_lesion_kwargs, dict(bogus=1)),
                    (G.check_lesion_kwargs, dict(min_size=-1)), (G.check_lesion_kwargs, dict(classes=[0])),
                    (G.check_lesion_kwargs, dict(max_pairs=0))):
        with pytest.raises(ValueError):
            fn(3, (1, 1, 1), **bad)
    with pytest.raises(ValueError):
        G.check_lesion_kwargs(3, (1, 0, 1))
    x = torch.zeros(4, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        G.region_stats(x, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        G.lesion_metrics(x, x, 2)
    for name in ("region_stats", "lesion_metrics", "RegionTable", "LesionReport", "evaluate_volume_lesions"):
        assert getattr(mivp_amd, name) is not None


def test_public_signatures():
    import mivp_amd  # noqa: F401
    from mivp_amd import inference as I
    from mivp_amd import regions as G
    sig = inspect.signature(G.region_stats).parameters
    assert list(sig) == ["labels", "num_classes", "image", "spacing", "connectivity", "classes", "max_regions"]
    assert sig["connectivity"].default == 26 and sig["max_regions"].default == 4096 and sig["image"].default is None
    sig = inspect.signature(G.lesion_metrics).parameters
    assert list(sig) == ["pred", "target", "num_classes", "spacing", "connectivity", "iou_threshold", "min_size", "classes",
                         "max_regions", "max_pairs"]
    assert sig["iou_threshold"].default == 0.0 and sig["min_size"].default == 0 and sig["max_pairs"].default is None
    # predict keeps the parameters the suite pins; the regions come from predict_regions, which takes them all
    sig = inspect.signature(I.SlidingWindowPredictor.predict).parameters
    assert list(sig)[1:] == ["x", "return_logits", "postprocess", "return_probs", "return_confidence", "return_entropy"]
    sig = inspect.signature(I.SlidingWindowPredictor.predict_regions).parameters
    assert list(sig)[1:8] == ["x", "return_logits", "postprocess", "return_probs", "return_confidence", "return_entropy",
                              "spacing"]
    sig = inspect.signature(I.SlidingWindowPredictor.evaluate_lesions).parameters
    assert list(sig)[1:5] == ["x", "seg", "spacing", "postprocess"] and sig["postprocess"].default is None
    sig = inspect.signature(I.evaluate_volume_lesions).parameters
    assert list(sig)[:5] == ["model", "x", "seg", "roi", "num_classes"] and sig["mirror_axes"].default == ()


# ------------------------------------------------------------------------------------------- C ABI
def test_header_declares_region_symbols_within_abi_18():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    names = set(re.findall(r"\b(mivp_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    assert "ABI 18" in text and "ABI 19" not in text
    assert "joined ABI 18 without a bump" in text
    assert _lib.ABI_VERSION == 18
    for n in ("mivp_region_stats", "mivp_region_overlap", "mivp_lesion_match"):      # the file's conventions
        m = re.search(r"int %s\(([^;]*)\);" % n, text)
        assert m and m.group(1).replace("\n", " ").split(",")[-1].strip() == "mivp_stream_t stream", n


def test_library_exports_region_symbols():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    lib = _lib.lib()
    assert lib.mivp_abi_version() == 18
    for n in SYMBOLS:
        assert hasattr(lib, n), n
    import ctypes as C
    assert lib.mivp_region_overlap_ws(C.c_int64(100)) == (2 + 2 * 256) * 8      # 256 = the power of two >= 2 * 100
    assert lib.mivp_region_overlap_ws(C.c_int64(0)) == 0
    dims = (C.c_int32 * 3)(8, 8, 8)
    assert lib.mivp_region_stats_ws(dims) == 512 + lib.mivp_label_ws(dims)
