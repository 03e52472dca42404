"""CPU: the host side of mirror test-time augmentation (mivp_amd.inference.flip_codes / tta_table, the predictor's
argument checks) and the C ABI 18 declarations of include/mivp.h."""
import itertools
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSETS = [s for n in range(4) for s in itertools.combinations((0, 1, 2), n)]


@pytest.mark.parametrize("axes", SUBSETS)
def test_flip_codes_are_the_subsets_in_increasing_order(axes):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import flip_codes
    want = sorted(sum(1 << a for a in sub) for n in range(len(axes) + 1) for sub in itertools.combinations(axes, n))
    for order in itertools.permutations(axes):                     # the order the axes are named in does not matter
        got = flip_codes(order)
        assert isinstance(got, tuple) and list(got) == want
    assert got[0] == 0 and len(got) == 2 ** len(axes)


@pytest.mark.parametrize("bad", [(3,), (-1,), (0, 0), (1, 2, 1), (0, 1, 2, 2), (0.5,), ("a",), 1])
def test_flip_codes_refuse_bad_axes(bad):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import flip_codes
    with pytest.raises(ValueError):
        flip_codes(bad)


@pytest.mark.parametrize("sub_batch", [1, 3, 4, 8, 10, 1000])
@pytest.mark.parametrize("axes", [(), (2,), (0, 1), (0, 1, 2)])
@pytest.mark.parametrize("image_size,roi", [((20, 17, 9), (8, 8, 4)), ((5, 30, 11), (8, 10, 4))])
def test_tta_table_is_window_major_flip_minor(image_size, roi, axes, sub_batch):
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import flip_codes, tta_table, window_origins, window_table
    o = window_origins(image_size, roi, 0.5)
    codes = flip_codes(axes)
    n, f = o.shape[0], len(codes)
    t = tta_table(o, sub_batch, codes)
    assert t.dtype == np.int32 and t.shape == (math.ceil(n * f / sub_batch) * sub_batch, 4)
    assert t.shape[0] % sub_batch == 0
    for w in range(n):
        for j, m in enumerate(codes):
            e = t[w * f + j]
            assert e[:3].tolist() == o[w].tolist() and e[3] & 1 == 1 and e[3] >> 1 == m
    assert (t[n * f:] == 0).all()                                   # the tail is invalid
    if f == 1:
        assert np.array_equal(t, window_table(o, sub_batch))


def test_tta_table_refuses_bad_arguments():
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import tta_table, window_origins
    o = window_origins((16, 16, 16), (8, 8, 8), 0.5)
    with pytest.raises(ValueError):
        tta_table(o, 0, (0,))
    for codes in ((), (0, 0), (8,), (-1,)):
        with pytest.raises(ValueError):
            tta_table(o, 4, codes)


def test_predictor_checks_mirror_axes_before_it_needs_a_device():
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd.inference import SlidingWindowPredictor
    model = torch.nn.Conv3d(1, 2, 1)
    for bad in ((3,), (0, 0), (-1, 1)):
        with pytest.raises(ValueError, match="mirror_axes"):
            SlidingWindowPredictor(model, (16, 16, 16), 1, 2, (8, 8, 8), mirror_axes=bad)
    with pytest.raises(RuntimeError, match="GPU"):                  # good axes: the next refusal is the CPU model
        SlidingWindowPredictor(model, (16, 16, 16), 1, 2, (8, 8, 8), mirror_axes=(0, 2))


def test_wrappers_take_mirror_axes():
    import inspect
    import mivp_amd  # noqa: F401
    from mivp_amd import inference as I
    for fn in (I.predict_volume, I.evaluate_volume, I.evaluate_volume_surface, I.predict_scan_volume,
               I.SlidingWindowPredictor.__init__):
        assert inspect.signature(fn).parameters["mirror_axes"].default == ()
    sig = inspect.signature(I.SlidingWindowPredictor.predict).parameters
    assert list(sig)[1:] == ["x", "return_logits", "postprocess", "return_probs", "return_confidence", "return_entropy"]
    assert all(sig[k].default is False for k in ("return_probs", "return_confidence", "return_entropy"))


def test_header_declares_abi_18_symbols():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    names = set(re.findall(r"\b(mivp_[a-z0-9_]+)\s*\(", text))
    for n in ("mivp_window_gather_tta", "mivp_window_blend_tta", "mivp_stitch_finalize_probs"):
        assert n in names, n
    assert "ABI 18" in text
    assert _lib.ABI_VERSION == 18
    lib = _lib.lib()
    assert lib.mivp_abi_version() == 18
    for n in ("mivp_window_gather_tta", "mivp_window_blend_tta", "mivp_stitch_finalize_probs"):
        assert hasattr(lib, n), n
    # the new finalize takes the plain one's arguments with the three maps in front of target / counts
    m = re.search(r"int mivp_stitch_finalize_probs\(([^;]*)\);", text)
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["acc", "wsum", "C", "dims", "pad", "pdims", "labels", "logits", "probs", "confidence", "entropy",
                    "target", "counts", "stream"]
