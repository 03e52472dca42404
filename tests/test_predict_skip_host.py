"""CPU: the host side of window skipping in whole-volume prediction (mivp_amd.inference.WindowSkip): the numpy restatement
of tests/window_skip_ref.py against a second, voxel-by-voxel form, the value object's checks, the declarations of
include/mivp.h and the package exports."""
import math
import os
import re

import numpy as np
import pytest

from window_skip_ref import compact, covered, fill, occupancy, padded_foreground

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mivp_window_occupancy", "mivp_window_compact", "mivp_stitch_fill", "mivp_window_blend_any")
# (channels, image, roi): the padded shapes of the gather tests
CASES = [(1, (10, 13, 7), (16, 8, 12)), (4, (9, 6, 8), (12, 8, 12)), (4, (20, 12, 16), (16, 8, 8)),
         (1, (21, 11, 9), (8, 8, 4))]


def _volume(cin, image, seed):
    rng = np.random.default_rng(seed)
    v = rng.random((cin,) + image, dtype=np.float32)
    v[v < 0.6] = 0.0                                             # mostly air
    v[:, image[0] // 2:] = 0.0                                   # one half empty, so that some windows hold nothing
    v[-1, 0, 0, 0] = np.float32(0.0025)                          # exactly the threshold: not foreground
    v[-1, 0, 0, 1] = np.nan                                      # not foreground
    return v


def _count_voxelwise(vol, channel, threshold, mask, image, roi, origins):
    """The second form: every voxel of every window on its own, in image coordinates."""
    from mivp_amd.inference import window_padding
    pad, _ = window_padding(image, roi)
    out = []
    for o in origins.tolist():
        n = 0
        for i in range(roi[0]):
            for j in range(roi[1]):
                for k in range(roi[2]):
                    h, w, d = o[0] + i - pad[0], o[1] + j - pad[1], o[2] + k - pad[2]
                    if not (0 <= h < image[0] and 0 <= w < image[1] and 0 <= d < image[2]):
                        continue
                    if mask is not None:
                        n += int(mask[h, w, d] != 0)
                    else:
                        x = np.float32(vol[channel, h, w, d])
                        n += int((not math.isnan(x)) and x > np.float32(threshold))
        out.append(n)
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("cin,image,roi", CASES)
def test_occupancy_restatement_matches_the_voxelwise_form(cin, image, roi):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import window_origins
    o = window_origins(image, roi, 0.5)
    vol = _volume(cin, image, 0)
    ch = cin - 1
    got = occupancy(o, roi, padded_foreground(image, roi, vol=vol, channel=ch, threshold=0.0025))
    want = _count_voxelwise(vol, ch, 0.0025, None, image, roi, o)
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    assert 0 < int((got > 0).sum())
    mask = (np.random.default_rng(1).random(image) > 0.9).astype(np.uint8) * 7
    got = occupancy(o, roi, padded_foreground(image, roi, mask=mask))
    assert got.tolist() == _count_voxelwise(None, 0, 0.0, mask, image, roi, o).tolist()


def test_threshold_and_nan_voxels_do_not_count():
    image, roi = (10, 13, 7), (16, 8, 12)
    vol = np.zeros((1,) + image, dtype=np.float32)
    vol[0, 1, 1, 1] = np.float32(0.0025)
    vol[0, 1, 1, 2] = np.nan
    vol[0, 1, 1, 3] = np.nextafter(np.float32(0.0025), np.float32(1))
    fg = padded_foreground(image, roi, vol=vol, channel=0, threshold=0.0025)
    assert int(fg.sum()) == 1 and fg[1 + 3, 1, 3 + 2]          # pad (3, 0, 2)


@pytest.mark.parametrize("codes", [(0,), (0, 1, 4, 5)])
@pytest.mark.parametrize("min_voxels", [1, 50])
@pytest.mark.parametrize("sub_batch", [1, 4, 7])
def test_compact_restatement_keeps_order_and_zeroes_the_rest(codes, min_voxels, sub_batch):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import tta_table, window_origins
    image, roi = (20, 12, 16), (16, 8, 8)
    o = window_origins(image, roi, 0.5)
    full = tta_table(o, sub_batch, codes)
    f = len(codes)
    vol = np.zeros((4,) + image, dtype=np.float32)
    vol[1, :4, :4, :6] = 1.0                                     # 96 voxels in window (0, 0, 0), 32 in (0, 0, 4)
    counts = occupancy(o, roi, padded_foreground(image, roi, vol=vol, channel=1))
    assert sorted(counts.tolist())[-2:] == [32, 96]
    got, meta = compact(full, counts, f, min_voxels)
    # second form: walk the windows, emit their flips
    want = []
    for w in range(o.shape[0]):
        if counts[w] >= min_voxels:
            want += [[int(o[w, 0]), int(o[w, 1]), int(o[w, 2]), 1 + 2 * m] for m in codes]
    assert 0 < len(want) < o.shape[0] * f
    assert got.shape == full.shape and got.dtype == np.int32
    assert got[:len(want)].tolist() == want
    assert not got[len(want):].any()
    assert meta.tolist() == [len(want) // f, len(want)]


def test_compact_with_everything_kept_is_the_full_table():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import tta_table, window_origins
    o = window_origins((20, 12, 16), (16, 8, 8), 0.5)
    full = tta_table(o, 4, (0, 2))
    got, meta = compact(full, np.ones(o.shape[0], dtype=np.int32), 2, 1)
    assert (got == full).all() and meta.tolist() == [o.shape[0], 2 * o.shape[0]]
    got, meta = compact(full, np.zeros(o.shape[0], dtype=np.int32), 2, 1)
    assert not got.any() and meta.tolist() == [0, 0]


def test_fill_restatement_and_coverage():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import window_origins, window_padding
    image, roi = (10, 13, 7), (16, 8, 12)
    _, pdims = window_padding(image, roi)
    o = window_origins(image, roi, 0.5)
    keep = np.zeros(o.shape[0], dtype=bool)
    keep[0] = True
    cov = covered(o, roi, pdims, keep)
    assert 0 < int(cov.sum()) == int(np.prod(roi)) < int(np.prod(pdims))
    rng = np.random.default_rng(3)
    acc = rng.standard_normal(pdims + (3,)).astype(np.float32) * cov[..., None]
    wsum = (rng.random(pdims).astype(np.float32) + 0.5) * cov
    a2, w2 = fill(acc, wsum, 1, 10.0)
    for idx in np.ndindex(*pdims):                               # second form: voxel by voxel
        if cov[idx]:
            assert (a2[idx] == acc[idx]).all() and w2[idx] == wsum[idx]
        else:
            assert a2[idx].tolist() == [-10.0, 10.0, -10.0] and w2[idx] == 1.0
    assert ((a2 / w2[..., None])[~cov] == np.array([-10.0, 10.0, -10.0], dtype=np.float32)).all()


def test_window_skip_defaults_and_validation():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import WindowSkip
    k = WindowSkip()
    assert (k.threshold, k.channel, k.min_voxels, k.fill_class, k.fill_logit) == (0.0025, 0, 1, 0, 10.0)
    k = WindowSkip(threshold=-1.0, channel=2, min_voxels=50, fill_class=1, fill_logit=4.5)
    assert (k.threshold, k.channel, k.min_voxels, k.fill_class, k.fill_logit) == (-1.0, 2, 50, 1, 4.5)
    assert k == WindowSkip(-1.0, 2, 50, 1, 4.5) and k != WindowSkip()
    with pytest.raises(AttributeError):
        k.channel = 0
    for bad in (dict(channel=-1), dict(channel=1.5), dict(min_voxels=0), dict(min_voxels=-3), dict(fill_class=-1),
                dict(fill_logit=0.0), dict(fill_logit=-2.0), dict(fill_logit=float("inf")), dict(fill_logit=float("nan")),
                dict(fill_logit=1e39), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold="0.1"),
                dict(channel=True), dict(min_voxels=None)):
        with pytest.raises(ValueError):
            WindowSkip(**bad)


def test_header_declares_the_skip_symbols_at_abi_18():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    names = set(re.findall(r"\b(mivp_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for n in SYMBOLS:
        assert n in names, n
        assert hasattr(lib, n), n
        m = re.search(r"int %s\(([^;]*)\);" % n, text)
        assert m, n
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert args[-1] == "mivp_stream_t stream", (n, args[-1])
    assert "ABI 19" not in text
    assert _lib.ABI_VERSION == 18
    assert lib.mivp_abi_version() == 18
    src = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "window_skip.hip")
    body = open(src).read()
    for n in SYMBOLS:
        assert re.search(r'extern "C" int %s\(' % n, body), n


def test_package_exports_and_signatures():
    import inspect
    import mivp_amd
    from mivp_amd import inference
    assert mivp_amd.WindowSkip is inference.WindowSkip
    assert mivp_amd.SlidingWindowPredictor is inference.SlidingWindowPredictor
    p = inspect.signature(inference.SlidingWindowPredictor.__init__).parameters
    assert p["skip"].default is None
    for fn in ("predict_volume", "evaluate_volume", "evaluate_volume_surface", "evaluate_volume_lesions",
               "evaluate_volume_calibration", "predict_scan_volume"):
        q = inspect.signature(getattr(inference, fn)).parameters
        assert "skip" in q and q["skip"].default is None, fn
    assert hasattr(inference.SlidingWindowPredictor, "set_region")
