"""CPU: the host side of fitting the prediction windows to the foreground bounding box (mivp_amd.inference.WindowFit):
the numpy restatement of tests/window_fit_ref.py against window_origins / tta_table and against the properties the
predictor relies on (never more windows per axis than the full tiling, every window inside the padded volume, the grown
box covered), the value object's checks, the refusals that need no device, the declarations of include/mivp.h and the
package exports."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from window_fit_ref import axis_starts, box_of, count_of, covered, fitted_origins, fitted_table, foreground, interval_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mivp_foreground_box", "mivp_window_fit_plan")
# (image, roi): the shapes of tests/test_hip_predict_fit.py -- plain, H shorter than the roi, D % 4 == 0
SHAPES = [((30, 26, 21), (12, 12, 8)), ((13, 30, 11), (16, 10, 4)), ((20, 12, 16), (16, 8, 8))]
OVERLAPS = (0.0, 0.25, 0.5, 0.9)


@pytest.mark.parametrize("image,roi", SHAPES)
@pytest.mark.parametrize("overlap", OVERLAPS)
def test_whole_volume_box_gives_the_full_tiling(image, roi, overlap):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import tta_table, window_origins
    full = window_origins(image, roi, overlap)
    whole = [0, 0, 0] + [n - 1 for n in image]
    for margin in ((0, 0, 0), (3, 0, 50)):                       # a margin past the faces changes nothing
        got = fitted_origins(whole, image, roi, overlap, margin)
        assert got.dtype == np.int32 and got.tolist() == full.tolist()
    for codes, sub_batch in (((0,), 7), ((0, 1, 4, 5), 3)):
        want = tta_table(full, sub_batch, codes)
        table, meta = fitted_table(full, want.shape[0], codes)
        assert table.dtype == np.int32 and table.tolist() == want.tolist()
        assert meta.tolist() == [full.shape[0], full.shape[0] * len(codes)]


@pytest.mark.parametrize("image,roi", SHAPES)
@pytest.mark.parametrize("overlap", OVERLAPS)
def test_no_length_takes_more_windows_than_the_padded_axis(image, roi, overlap):
    """count(n) <= count(p) for every n in r..p: the fitted work list always fits the full one."""
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import window_origins, window_padding
    _, pdims = window_padding(image, roi)
    full = window_origins(image, roi, overlap)
    for a in range(3):
        p, r = pdims[a], roi[a]
        step = interval_of(r, overlap)
        top = count_of(p, r, step)
        assert top == len(set(full[:, a].tolist()))              # the full tiling's own count
        counts = [count_of(n, r, step) for n in range(r, p + 1)]
        assert counts[0] == 1 and max(counts) == counts[-1] == top
        assert all(x <= y for x, y in zip(counts, counts[1:]))


@pytest.mark.parametrize("image,roi", SHAPES)
def test_every_box_is_covered_by_windows_inside_the_padded_volume(image, roi):
    """Exhaustive per axis: every inclusive [lo, hi], margins 0 / 2 / past the axis, overlaps 0 and 0.5."""
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import window_padding
    pad, pdims = window_padding(image, roi)
    for a in range(3):
        n, p, r = image[a], pdims[a], roi[a]
        full = {ov: count_of(p, r, interval_of(r, ov)) for ov in (0.0, 0.5)}
        for lo, hi in itertools.combinations_with_replacement(range(n), 2):
            for m in (0, 2, n):
                for ov in (0.0, 0.5):
                    step = interval_of(r, ov)
                    s = axis_starts(lo, hi, pad[a], p, r, m, step)
                    assert 1 <= len(s) <= full[ov]
                    assert s == sorted(set(s)) and s[0] >= 0 and s[-1] + r <= p
                    assert all(y - x <= step for x, y in zip(s, s[1:]))          # no gap for any overlap >= 0
                    assert s[0] <= max(lo + pad[a] - m, 0) and s[-1] + r >= min(hi + pad[a] + m + 1, p)


def test_box_restatement_and_empty_encoding():
    image = (9, 7, 6)
    vol = np.zeros((2,) + image, dtype=np.float32)
    assert box_of(foreground(vol, 1)).tolist() == [9, 7, 6, -1, -1, -1]
    vol[1, 2, 3, 4] = np.float32(0.0025)                         # exactly the threshold: not foreground
    vol[1, 8, 6, 5] = np.nan                                     # not foreground
    vol[0, 0, 0, 0] = 1.0                                        # another channel
    assert box_of(foreground(vol, 1)).tolist() == [9, 7, 6, -1, -1, -1]
    vol[1, 2, 3, 4] = np.nextafter(np.float32(0.0025), np.float32(1))
    vol[1, 5, 1, 4] = 0.5
    assert box_of(foreground(vol, 1)).tolist() == [2, 1, 4, 5, 3, 4]
    assert box_of(foreground(vol, 0)).tolist() == [0, 0, 0, 0, 0, 0]
    mask = np.zeros(image, dtype=np.uint8)
    mask[8, 0, 5] = 200
    mask[1, 6, 0] = 1
    assert box_of(foreground(mask=mask)).tolist() == [1, 0, 0, 8, 6, 5]
    assert fitted_origins([9, 7, 6, -1, -1, -1], image, (4, 4, 4), 0.5).shape == (0, 3)
    t, meta = fitted_table(np.zeros((0, 3), dtype=np.int32), 6, (0, 1))
    assert not t.any() and meta.tolist() == [0, 0]


def test_fitted_tiling_worked_example_and_coverage():
    """roi 96, overlap 0.5: a 256-long axis takes 5 windows, a 180-long box 3, a 140-long box 2, 160 takes 3."""
    assert [count_of(n, 96, interval_of(96, 0.5)) for n in (256, 180, 140, 160)] == [5, 3, 2, 3]
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import window_padding
    image, roi = (30, 26, 21), (12, 12, 8)
    _, pdims = window_padding(image, roi)
    box = [4, 20, 3, 20, 22, 9]                                  # wider than the roi, thinner (widened), thinner
    o = fitted_origins(box, image, roi, 0.5)
    assert o.tolist() == [[4, 14, 3], [9, 14, 3]]               # W: 20 - 9 // 2 = 16, clamped to 26 - 12; D: 3 - 1 // 2
    cov = covered(o, roi, pdims)
    assert cov[4:21, 20:23, 3:10].all() and int(cov.sum()) == 17 * 12 * 8
    # the far corner: the widened window is clamped into the volume
    o = fitted_origins([29, 25, 20, 29, 25, 20], image, roi, 0.5)
    assert o.tolist() == [[18, 14, 13]]


def test_window_fit_defaults_validation_and_immutability():
    import mivp_amd
    from mivp_amd.inference import WindowFit
    k = WindowFit()
    assert (k.threshold, k.channel, k.margin, k.fill_class, k.fill_logit) == (0.0025, 0, (0, 0, 0), 0, 10.0)
    k = WindowFit(threshold=-1.0, channel=2, margin=(1, 0, 7), fill_class=1, fill_logit=4.5)
    assert (k.threshold, k.channel, k.margin, k.fill_class, k.fill_logit) == (-1.0, 2, (1, 0, 7), 1, 4.5)
    assert k == WindowFit(-1.0, 2, [1, 0, 7], 1, 4.5) and k != WindowFit()
    assert hash(k) == hash(WindowFit(-1.0, 2, np.array([1, 0, 7]), 1, 4.5))
    assert WindowFit(margin=3).margin == (3, 3, 3) and WindowFit(margin=np.int64(2)) == WindowFit(margin=(2, 2, 2))
    assert "margin=(1, 0, 7)" in repr(k)
    for name in ("channel", "margin", "other"):
        with pytest.raises(AttributeError):
            setattr(k, name, 0)
    for bad in (dict(channel=-1), dict(channel=1.5), dict(channel=True), dict(fill_class=-1), dict(fill_class=None),
                dict(fill_logit=0.0), dict(fill_logit=-2.0), dict(fill_logit=float("inf")), dict(fill_logit=float("nan")),
                dict(fill_logit=1e39), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold="0.1"),
                dict(margin=-1), dict(margin=1.5), dict(margin=True), dict(margin=None), dict(margin=(1, 2)),
                dict(margin=(1, 2, -3)), dict(margin=(1, 2, 3.0)), dict(margin=(1, 2, 3, 4)), dict(margin=2 ** 31),
                dict(margin="111")):
        with pytest.raises(ValueError):
            WindowFit(**bad)
    assert mivp_amd.WindowFit is WindowFit


def test_the_value_objects_share_the_checks_of_host():
    """The same bad value is refused with the same text by WindowFit and WindowSkip: one definition in _host.py."""
    import mivp_amd  # noqa: F401
    from mivp_amd import _host
    from mivp_amd.inference import WindowFit, WindowSkip
    for bad in (dict(channel=-1), dict(fill_class=1.5), dict(fill_logit=0.0), dict(fill_logit=float("nan")),
                dict(threshold=float("inf"))):
        seen = []
        for cls in (WindowFit, WindowSkip):
            with pytest.raises(ValueError) as e:
                cls(**bad)
            seen.append(str(e.value))
        assert seen[0] == seen[1], bad
    assert _host.check_finite("t", np.float32(0.5)) == 0.5 and _host.check_int_from("n", np.int32(4), 1) == 4
    assert _host.check_fill_logit(3) == 3.0
    for call in (lambda: _host.check_finite("t", True), lambda: _host.check_int_from("n", 0, 1),
                 lambda: _host.check_int_from("n", 2 ** 31, 0), lambda: _host.check_fill_logit(-1.0),
                 lambda: _host.check_region_mask(np.zeros((2, 2, 2), np.uint8), (2, 2, 2), torch.device("cpu")),
                 lambda: _host.check_region_mask(torch.zeros((2, 2, 2), dtype=torch.uint8), (2, 2, 2), torch.device("cpu"))):
        with pytest.raises(ValueError):
            call()


def test_predictor_refuses_fit_with_skip_and_bad_fit_before_it_needs_a_device():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor, WindowFit, WindowSkip
    model, args = torch.nn.Conv3d(1, 3, 1), ((16, 16, 16), 1, 3, (8, 8, 8))
    with pytest.raises(ValueError, match="fit and skip cannot be combined"):
        SlidingWindowPredictor(model, *args, skip=WindowSkip(), fit=WindowFit())
    with pytest.raises(ValueError, match="fit must be a WindowFit or None"):
        SlidingWindowPredictor(model, *args, fit=WindowSkip())
    with pytest.raises(ValueError, match="fit.channel 1 is not a channel of a 1-channel volume"):
        SlidingWindowPredictor(model, *args, fit=WindowFit(channel=1))
    with pytest.raises(ValueError, match="fit.fill_class 3 is not one of 3 classes"):
        SlidingWindowPredictor(model, *args, fit=WindowFit(fill_class=3))
    with pytest.raises(RuntimeError, match="runs on the GPU"):   # a good fit passes the checks: the CPU model is next
        SlidingWindowPredictor(model, *args, fit=WindowFit(fill_class=2))


def test_foreground_box_refuses_host_tensors():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import foreground_box
    for bad in (torch.zeros((1, 1, 4, 4, 4)), np.zeros((4, 4, 4), dtype=np.uint8)):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            foreground_box(bad)


def test_header_declares_the_fit_symbols_at_abi_18():
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
    body = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "window_fit.hip")).read()
    for n in SYMBOLS:
        assert re.search(r'extern "C" int %s\(' % n, body), n
    assert "asm" not in body                                     # plain C++ HIP


def test_package_exports_and_the_fit_keyword():
    import mivp_amd
    from mivp_amd import inference, window_fit
    assert mivp_amd.WindowFit is inference.WindowFit is window_fit.WindowFit
    assert mivp_amd.foreground_box is inference.foreground_box is window_fit.foreground_box
    q = inspect.signature(inference.foreground_box).parameters
    assert [(k, v.default) for k, v in q.items()][1:] == [("channel", 0), ("threshold", 0.0025), ("out", None)]
    # every one-shot helper hands fit= to the predictor, whose check of it comes before anything needs a device
    model, x = torch.nn.Conv3d(1, 3, 1), torch.zeros((1, 1, 16, 16, 16))
    bad = inference.WindowSkip()
    for call in (lambda **k: inference.predict_volume(model, x, (8, 8, 8), 3, **k),
                 lambda **k: inference.evaluate_volume(model, x, x, (8, 8, 8), 3, **k),
                 lambda **k: inference.evaluate_volume_surface(model, x, x, (8, 8, 8), 3, **k),
                 lambda **k: inference.evaluate_volume_lesions(model, x, x, (8, 8, 8), 3, **k),
                 lambda **k: inference.evaluate_volume_calibration(model, x, x, (8, 8, 8), 3, **k),
                 lambda **k: inference.predict_scan_volume(model, x[0], np.eye(4), (8, 8, 8), 3, **k),
                 lambda **k: inference._one_shot(model, x, None, 3, (8, 8, 8), 0.5, "gaussian", 0.125, 10, False, (), None,
                                                 **k)):
        with pytest.raises(ValueError, match="fit must be a WindowFit or None"):
            call(fit=bad)
        with pytest.raises(RuntimeError, match="runs on the GPU"):              # fit=None and a good fit get further
            call()
        with pytest.raises(RuntimeError, match="runs on the GPU"):
            call(fit=inference.WindowFit())
    with pytest.raises(TypeError):                               # keyword-only: positional callers are unchanged
        inference.SlidingWindowPredictor(model, (16, 16, 16), 1, 3, (8, 8, 8), 0.5, "gaussian", 0.125, 10, False, (), None,
                                         inference.WindowFit())
