"""CPU: the numpy restatement of the box and scribble prompts (tests/strokes_ref.py) against a brute-force rasteriser, scipy's
distance transform and a set-based box rule, the shared cases' expectations, and the argument refusals of mivp_amd.strokes,
which all happen before any launch or copy (every tensor here is a CPU tensor; the refusals that can only be reached with a
GPU tensor are marked gpu)."""
import itertools
from argparse import Namespace
from fractions import Fraction
from math import floor

import numpy as np
import pytest
import torch
from scipy import ndimage

import strokes_ref as R

CASES = R.scribble_cases()


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _brute_segment(a, b):
    delta = [q - p for p, q in zip(a, b)]
    n = max(abs(v) for v in delta)
    if n == 0:
        return [tuple(a)]
    return [tuple(p + floor(Fraction(2 * i * dl + n, 2 * n)) for p, dl in zip(a, delta)) for i in range(n + 1)]


@pytest.mark.parametrize("signs", list(itertools.product((-1, 1), repeat=3)))
def test_rasteriser_against_a_per_step_loop_in_every_octant(signs):
    rng = np.random.default_rng(sum(s > 0 for s in signs) * 8 + (signs[0] > 0))
    for _ in range(20):
        a = [int(v) for v in rng.integers(20, 40, size=3)]
        mag = [int(v) for v in rng.integers(0, 20, size=3)]
        b = [p + s * m for p, s, m in zip(a, signs, mag)]
        got = [tuple(int(v) for v in r) for r in R.segment_ref(a, b)]
        assert got == _brute_segment(a, b)
        assert got[0] == tuple(a) and got[-1] == tuple(b)
        steps = np.abs(np.diff(np.asarray(got), axis=0))
        assert len(got) == 1 or (steps.max(axis=1) == 1).all()           # 26-connected, no repeated voxel within a segment


def test_rasteriser_ties_round_half_up_on_every_axis():
    # delta = (4, 2, -2): at i = 1, 3 the minor axes sit exactly between two voxels; floor(x + 1/2) decides, also below zero
    got = R.segment_ref((0, 0, 5), (4, 2, 3)).tolist()
    assert got == [[0, 0, 5], [1, 1, 5], [2, 1, 4], [3, 2, 4], [4, 2, 3]]
    assert R.raster_ref([(3, 3, 3)]).tolist() == [[3, 3, 3]]
    assert R.raster_ref([(3, 3, 3), (3, 3, 3)]).tolist() == [[3, 3, 3]]
    m = R.draw_ref(np.zeros((2, 6, 6, 6), dtype=np.uint8), 1, [(0, 0, 0), (5, 5, 5)], 1)
    m = R.draw_ref(m, 1, [(2, 2, 2)], 0)
    assert m[0].sum() == 0 and m[1, 2, 2, 2] == 3 and (m[1] > 0).sum() == 6


@pytest.mark.parametrize("spacing,rtol", [((1, 1, 1), 1e-12), (R.EXACT_SPACING, 1e-12), ((1, 0.8, 2.5), 1e-6)])
def test_stroke_distance_is_the_scipy_transform(spacing, rtol):
    rng = np.random.default_rng(5)
    for density in (0.01, 0.1):
        seeds = rng.random((13, 10, 7)) < density
        seeds[4, 5, 6] = True
        want = ndimage.distance_transform_edt(~seeds, sampling=spacing) ** 2
        assert np.allclose(R.stroke_dist_sq(seeds, spacing), want, rtol=rtol, atol=0)
    assert np.isinf(R.stroke_dist_sq(np.zeros((3, 2, 2), dtype=bool))).all()


@pytest.mark.parametrize("mode", ["filled", "frame"])
def test_box_rules_against_a_set_based_brute_force(mode):
    dims = (7, 6, 5)
    boxes = np.array([[(1, 1, 1, 4, 3, 3, 0), (3, 2, 0, 6, 5, 4, 0), (2, 2, 2, 2, 2, 2, 1), (0, 0, 0, 6, 5, 4, 1)],
                      [(0, 0, 0, 6, 5, 4, 1), (1, 1, 1, 2, 2, 2, 0), (-1,) * 7, (-1,) * 7]], dtype=np.int32)
    count = [3, 1]                                                  # the fourth row of sample 0 and the second of sample 1 are not read
    got = R.box_ref(boxes, count, dims, mode)
    for b in range(2):
        want = [set(), set()]
        for row in boxes[b, :count[b]].tolist():
            lo, hi, ch = row[:3], row[3:6], row[6]
            for v in itertools.product(*[range(lo[a], hi[a] + 1) for a in range(3)]):
                if mode == "filled" or any(v[a] in (lo[a], hi[a]) for a in range(3)):
                    want[ch].add(v)
        for ch in range(2):
            assert {tuple(v) for v in np.argwhere(got[b, ch]).tolist()} == want[ch]
    assert got[0, 1].sum() == 1 and got[1, 0].sum() == 0
    assert R.box_ref(boxes, count, dims, "frame")[0, 0, 2, 2, 2] == 0 and R.box_ref(boxes, count, dims)[0, 0, 2, 2, 2] == 1


def test_encode_restatement_is_the_maximum_of_box_and_stroke():
    dims = (7, 6, 5)
    mask = np.zeros((1, *dims), dtype=np.uint8)
    mask = R.draw_ref(mask, 0, [(0, 0, 0), (6, 0, 0)], 0)
    boxes = np.array([[(2, 2, 2, 4, 4, 4, 0)]], dtype=np.int32)
    out = R.encode_ref(boxes, [1], mask, radius=1.0)
    assert out[0, 0].sum() == 27 + 7 * 3 and not out[0, 1].any() and not np.signbit(out[0, 1]).any()
    g = R.encode_ref(boxes, [0], mask, kind="gaussian", sigma=1.5, spacing=(1, 0.8, 2.5))
    assert g[0, 0, 3, 0, 0] == 1.0 and np.isclose(g[0, 0, 3, 1, 0], np.exp(-R.spacing_sq((1, 0.8, 2.5))[1] / 4.5))


def test_simulated_box_restatement():
    dims = (9, 8, 7)
    t = np.zeros((3, *dims), dtype=np.int64)
    t[0, 2:5, 3:4, 1:6] = 1
    t[2] = 1                                                        # touches every border
    boxes, count = np.full((3, 2, 7), -1, dtype=np.int32), np.array([0, 0, 2], dtype=np.int32)
    jit = np.array([[9, 0, -1, -9, 0, 1], [0] * 6, [3, 3, 3, -3, -3, -3]], dtype=np.int32)      # sample 0: h would invert
    new, cnt, last = R.simulate_box_ref(t, boxes, count, margin=(1, 0, 2), jitter=jit, channel=1)
    assert new[0, 0].tolist() == [4, 3, 0, 4, 3, 6, 1] and cnt.tolist() == [1, 0, 2]
    assert last[0].tolist() == [4, 3, 0, 4, 3, 6, 1, 0] and last[1].tolist() == [-1] * 6 + [0, 0]
    assert last[2].tolist() == [2, 3, 1, 6, 4, 5, 0, 0] and (new[2] == -1).all()    # a full slot: last is still written
    for b in (0, 2):                                                 # never empty, inside the volume, meets the object
        lo, hi = last[b, :3], last[b, 3:6]
        obj = np.argwhere(t[b] > 0)
        assert (lo >= 0).all() and (hi < dims).all() and (lo <= hi).all()
        assert ((obj >= lo) & (obj <= hi)).all(axis=1).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_scribble_case_expectations(name):
    c = CASES[name]
    B = c["pred"].shape[0]
    mask, last = R.simulate_scribbles_ref(c["pred"], c["target"], np.zeros(c["pred"].shape, dtype=np.uint8), **c["kwargs"])
    assert ((mask & 1).reshape(B, -1).sum(axis=1) == last[:, 0]).all() and ((mask >> 1).reshape(B, -1).sum(axis=1) == last[:, 1]).all()
    e_pos, e_neg = R.error_regions(c["pred"][0], c["target"][0], R._object_mask(c["kwargs"].get("object_classes")),
                                   c["kwargs"].get("ignore_index"))
    assert not ((mask[0] & 1) & ~e_pos).any() and not ((mask[0] >> 1) & ~e_neg).any()      # a scribble lies in its region
    if name in ("thick_blob", "odd_batch", "anisotropic", "ignore_and_classes"):
        assert last[0, 0] >= 2 and last[0, 1] == 0 and last[0, 2] == 1
    if name == "sliver":
        assert e_pos.sum() == 32 and last[0, :2].tolist() == [0, 0] and last[1, 0] > 0
    if name == "both_regions":
        assert last[0, 0] > 0 and last[0, 1] > 0
    if name == "no_error":
        assert not mask.any() and last[:, 2].tolist() == [1, 1]
    if name == "one_iteration":
        thin, _ = R.simulate_scribbles_ref(c["pred"], c["target"], np.zeros(c["pred"].shape, dtype=np.uint8))
        assert last[:, 2].tolist() == [0, 0] and last[0, 0] > (thin[0] & 1).sum()
    if name == "odd_batch":
        assert (last[:, 0] > 0).all()
    again, last2 = R.simulate_scribbles_ref(c["pred"], c["target"], mask, **c["kwargs"])     # accumulation: nothing is new
    assert np.array_equal(again, mask) and not last2[:, :2].any()


def test_no_scribble_case_is_left_to_rounding():
    for c in CASES.values():
        sp = c["kwargs"].get("spacing", (1, 1, 1))
        for b in range(c["pred"].shape[0]):
            for reg in R.error_regions(c["pred"][b], c["target"][b], R._object_mask(c["kwargs"].get("object_classes")),
                                       c["kwargs"].get("ignore_index")):
                d = R.depth_sq(reg, sp)
                assert np.array_equal(d.astype(np.float32).astype(np.float64), d)


# ---------------------------------------------------------------------------------------------------------------------
# refusals, all before any launch
# ---------------------------------------------------------------------------------------------------------------------
def _strokes():
    import mivp_amd  # noqa: F401
    from mivp_amd import strokes
    return strokes


def _slot(dims=(8, 8, 8), **kw):
    return _strokes().StrokeSlot(2, dims, device="cpu", **kw)


def _untouched(s):
    return (s.boxes == -1).all() and (s.box_count == 0).all() and (s.mask == 0).all() and (s.last == 0).all()


@pytest.mark.parametrize("bad", [17, 0, -1, True, 2.0, "4"])
def test_slot_refuses_a_bad_capacity(bad):
    with pytest.raises(ValueError, match="max_boxes must be"):
        _slot(max_boxes=bad)


@pytest.mark.parametrize("batch,dims", [(1, (70000, 4, 4)), (1, (4, 0, 4)), (2, (1022, 1024, 1024)), (1, (4, 4)), (1, (4, 4, 2.0)),
                                        (0, (4, 4, 4)), (65536, (1, 1, 1))])
def test_slot_refuses_a_volume_outside_the_range(batch, dims):
    with pytest.raises(ValueError, match="outside the kernels' range|dims must be three integers|batch must be"):
        _strokes().StrokeSlot(batch, dims, device="cpu")


def test_slot_takes_16_boxes_and_keeps_the_layout():
    s = _slot(max_boxes=16)
    assert s.boxes.shape == (2, 16, 7) and s.mask.shape == (2, 8, 8, 8) and s.mask.dtype == torch.uint8
    assert s.last.shape == (2, 8) and s.box_count.dtype == torch.int32 and _untouched(s)
    odd = _strokes().StrokeSlot(1, (3, 3, 3), device="cpu")
    assert odd.mask.is_contiguous() and odd.mask.untyped_storage().nbytes() % 4 == 0      # whole words behind the mask


@pytest.mark.parametrize("bad,text", [((8, 0, 0, 8, 1, 1, 0), "is outside 0 .."), ((0, 0, 0, 1, 8, 1, 1), "is outside 0 .."),
                                      ((-1, 0, 0, 1, 1, 1, 0), "is outside 0 .."), ((0, 0, 0, 1, 1, 70000, 0), "is outside 0 .."),
                                      ((3, 0, 0, 2, 1, 1, 0), "lo > hi"), ((0, 0, 5, 1, 1, 4, 1), "lo > hi"),
                                      ((0, 0, 0, 1, 1, 1, 2), "channel must be 0"), ((0, 0, 0, 1, 1, 1, -1), "channel must be 0"),
                                      ((0, 0, 0, 1, 1, 1), "seven integers"), ((0, 0, 0, 1, 1, 1.0, 0), "seven integers"),
                                      ((0, 0, 0, 1, 1, 1, True), "seven integers"), ("0001110", "seven integers")])
def test_slot_refuses_a_bad_box(bad, text):
    s = _slot()
    with pytest.raises(ValueError, match=text):
        s.set_boxes(1, [(1, 1, 1, 2, 2, 2, 0), bad])
    with pytest.raises(ValueError, match=text):
        s.add_box(0, bad)
    assert _untouched(s)


def test_slot_set_add_clear_cpu():
    s = _slot(max_boxes=3)
    s.set_boxes(1, [(1, 2, 3, 1, 2, 3, 0), (0, 0, 0, 7, 7, 7, 1)])
    s.add_box(1, (4, 4, 4, 5, 6, 7, 0))
    with pytest.raises(ValueError, match="is full"):
        s.add_box(1, (0, 0, 0, 0, 0, 0, 0))
    with pytest.raises(ValueError, match="the slot takes 3"):
        s.set_boxes(0, [(0, 0, 0, 0, 0, 0, 0)] * 4)
    for bad in (2, -1, True, 0.0):
        with pytest.raises(ValueError, match="sample index"):
            s.set_boxes(bad, [])
    rec = s.cpu()
    assert rec.box_count.tolist() == [0, 3]
    assert rec.boxes[1].tolist() == [[1, 2, 3, 1, 2, 3, 0], [0, 0, 0, 7, 7, 7, 1], [4, 4, 4, 5, 6, 7, 0]]
    assert (rec.boxes[0] == -1).all() and rec.mask.shape == (2, 8, 8, 8) and rec.last.shape == (2, 8)
    s.mask[0, 1, 1, 1] = 3
    s.clear_scribbles()
    assert (s.mask == 0).all() and s.box_count.tolist() == [0, 3]
    s.clear()
    assert _untouched(s)


@pytest.mark.parametrize("bad,text", [([(8, 0, 0)], "is outside 0 .."), ([(0, 0, 0), (0, -1, 0)], "is outside 0 .."),
                                      ([], "1 .. 256 points"), ([(1, 1, 1)] * 257, "1 .. 256 points"),
                                      ([(1, 1)], "integer triples"), ([(1, 1, 1.0)], "integer triples"), (5, "integer triples"),
                                      ([(1, 1, True)], "integer triples")])
def test_draw_refuses_bad_points(bad, text):
    s = _slot()
    with pytest.raises(ValueError, match=text):
        s.draw(0, bad, 0)
    assert _untouched(s)


def test_draw_refuses_a_bad_channel_and_a_cpu_slot():
    s = _slot()
    for bad in (2, -1, True, 0.0, None):
        with pytest.raises(ValueError, match="channel must be 0"):
            s.draw(0, [(1, 1, 1)], bad)
    with pytest.raises(ValueError, match="sample index"):
        s.draw(2, [(1, 1, 1)], 0)
    with pytest.raises(RuntimeError, match="GPU tensor"):            # everything else was in order: the last check
        s.draw(0, [(1, 1, 1), (7, 7, 7)], 1)
    assert _untouched(s)


@pytest.mark.parametrize("bad", [-1, 2, 3, True, 1.0, None])
def test_encode_refuses_a_wrong_channel_offset(bad):
    with pytest.raises(ValueError, match=r"channel_offset must be an integer in 0 \.\. 1"):
        _strokes().encode_strokes(_slot((4, 4, 4)), torch.zeros(2, 3, 4, 4, 4), channel_offset=bad)


def test_encode_refuses_other_bad_arguments():
    S = _strokes()
    x = torch.zeros(2, 3, 4, 4, 4)
    s = _slot((4, 4, 4))
    for kw, text in ((dict(kind="box"), "kind must be one of"), (dict(box="hollow"), "box must be one of"),
                     (dict(kind="gaussian", sigma=0.0), "sigma must be > 0"), (dict(radius=-1.0), "radius must be >= 0"),
                     (dict(spacing=(1, 0, 1)), "spacing must be three"), (dict(workspace=torch.zeros(16, dtype=torch.uint8)), "GPU tensor")):
        with pytest.raises((ValueError, RuntimeError), match=text):
            S.encode_strokes(s, x, channel_offset=1, **kw)
    with pytest.raises(ValueError, match="float32"):
        S.encode_strokes(s, x.double(), channel_offset=1)
    with pytest.raises(ValueError, match="float32"):
        S.encode_strokes(s, x[0], channel_offset=1)
    with pytest.raises(ValueError, match="built for a batch of 2"):
        S.encode_strokes(s, torch.zeros(3, 3, 4, 4, 4), channel_offset=1)
    with pytest.raises(ValueError, match="holds strokes of a"):
        S.encode_strokes(s, torch.zeros(2, 3, 4, 4, 5), channel_offset=1)
    with pytest.raises(ValueError, match="must be a StrokeSlot"):
        S.encode_strokes(None, x, channel_offset=1)
    with pytest.raises(RuntimeError, match="GPU tensor"):            # everything in order: the device is the last check
        S.encode_strokes(s, x, channel_offset=1)
    assert (x == 0).all()


def test_simulations_refuse_bad_arguments_on_the_host():
    S = _strokes()
    y = torch.zeros(2, 4, 4, 4)
    with pytest.raises(ValueError, match="must be .B, 1, H, W, D. or .B, H, W, D."):
        S.simulate_box(torch.zeros(4, 4, 4), _slot((4, 4, 4)))
    with pytest.raises(ValueError, match="must be .B, 1, H, W, D. or .B, H, W, D."):
        S.simulate_scribbles(torch.zeros(4, 4, 4), y, _slot((4, 4, 4)))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        S.simulate_box(y, _slot((4, 4, 4)))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        S.simulate_scribbles(y, y, _slot((4, 4, 4)))
    with pytest.raises(ValueError, match="outside the kernels' range"):
        S.strokes_ws(1, (70000, 4, 4))
    with pytest.raises(ValueError, match="max_jitter must be"):
        S.draw_box_jitter(np.random.default_rng(0), 2, -1)
    with pytest.raises(ValueError, match="generator must be"):
        S.draw_box_jitter(object(), 2, 1)
    for gen in (np.random.default_rng(0), np.random.RandomState(0)):
        j = S.draw_box_jitter(gen, 5, 3)
        assert j.shape == (5, 6) and j.dtype == np.int32 and np.abs(j).max() <= 3
    assert not S.draw_box_jitter(np.random.default_rng(0), 2, 0).any()


@pytest.mark.gpu
def test_simulations_refuse_bad_arguments_that_need_a_gpu_tensor():
    S = _strokes()
    y = torch.zeros(2, 4, 4, 4, device="cuda")
    s = S.StrokeSlot(2, (4, 4, 4))
    for kw, text in ((dict(object_classes=[32]), "object_classes"), (dict(object_classes=[]), "object_classes"),
                     (dict(ignore_index=1.0), "ignore_index must be"), (dict(margin=(1, 1)), "margin must be"),
                     (dict(margin=(1, -1, 0)), "margin must be"), (dict(margin=(1, 1.0, 0)), "margin must be"),
                     (dict(channel=2), "channel must be 0"), (dict(jitter=np.zeros((2, 6), dtype=np.int64)), "jitter must be"),
                     (dict(jitter=np.zeros((3, 6), dtype=np.int32)), "jitter must be"),
                     (dict(jitter=torch.zeros((2, 6), dtype=torch.int32, device="cuda")), "jitter must be"),
                     (dict(jitter=np.full((2, 6), 70000, dtype=np.int32)), "jitter must be")):
        with pytest.raises(ValueError, match=text):
            S.simulate_box(y, s, **kw)
    short = torch.zeros(64, dtype=torch.uint8, device="cuda")
    full = S.strokes_ws(2, (4, 4, 4))
    for kw, text in ((dict(object_classes=[1, 1]), "object_classes"), (dict(ignore_index=2 ** 31), "ignore_index must be"),
                     (dict(spacing=(1, 1)), "spacing must be three"), (dict(min_depth=-1.0), "min_depth must be >= 0"),
                     (dict(max_iter=0), "max_iter must be"), (dict(max_iter=4097), "max_iter must be"),
                     (dict(max_iter=2.0), "max_iter must be"), (dict(keep_endpoints=1), "keep_endpoints must be a bool"),
                     (dict(workspace=short), "workspace must be"), (dict(workspace=full[1:]), "workspace must be"),
                     (dict(workspace=full.view(torch.int8)), "workspace must be"),
                     (dict(workspace=torch.zeros(full.numel(), dtype=torch.uint8)), "workspace must be")):
        with pytest.raises(ValueError, match=text):
            S.simulate_scribbles(y, y, s, **kw)
    x = torch.zeros(2, 3, 4, 4, 4, device="cuda")
    for ws in (short, full[1:], full.view(torch.int8)):
        with pytest.raises(ValueError, match="workspace must be"):
            S.encode_strokes(s, x, channel_offset=1, workspace=ws)
    with pytest.raises(ValueError, match="contiguous and on the slot's device"):
        S.encode_strokes(s, x.permute(0, 1, 4, 3, 2), channel_offset=1)
    with pytest.raises(ValueError, match="differ"):
        S.simulate_scribbles(y, torch.zeros(2, 4, 4, 5, device="cuda"), s)
    with pytest.raises(ValueError, match="holds strokes of a"):
        S.simulate_box(torch.zeros(2, 4, 4, 5, device="cuda"), s)
    with pytest.raises(ValueError, match="built for a batch of 2"):
        S.simulate_box(torch.zeros(3, 4, 4, 4, device="cuda"), s)
    rec = s.cpu()
    assert (rec.boxes == -1).all() and not rec.box_count.any() and not rec.mask.any() and not rec.last.any()
    assert not s._scratch.any() and not x.any()


class _Net(torch.nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.conf = Namespace(input_channels=cin)
        self.conv = torch.nn.Conv3d(cin, 2, 1)

    def forward(self, x):
        return self.conv(x)

    def named_parameters_downstream(self):
        return list(self.named_parameters())


def test_stroke_model_refusals_and_forwarding():
    S = _strokes()
    from mivp_amd import clicks
    for cin in (1, 2):
        with pytest.raises(ValueError, match="conf.input_channels >= 3"):
            S.StrokeModel(_Net(cin), _slot())
    with pytest.raises(ValueError, match="conf.input_channels >= 5"):
        S.StrokeModel(_Net(4), _slot(), clicks=clicks.ClickSlot(2, device="cpu"))
    with pytest.raises(ValueError, match="built for a batch of 3"):
        S.StrokeModel(_Net(5), _slot(), clicks=clicks.ClickSlot(3, device="cpu"))
    with pytest.raises(ValueError, match="must be a StrokeSlot"):
        S.StrokeModel(_Net(3), clicks.ClickSlot(2, device="cpu"))
    with pytest.raises(ValueError, match="clicks must be a ClickSlot"):
        S.StrokeModel(_Net(5), _slot(), clicks=_slot())
    with pytest.raises(ValueError, match="unknown encoding keywords"):
        S.StrokeModel(_Net(3), _slot(), channel_offset=1)
    with pytest.raises(ValueError, match="box must be one of"):
        S.StrokeModel(_Net(3), _slot(), box="hollow")
    g = S.StrokeModel(_Net(3), _slot(), kind="gaussian", sigma=1.5)
    with pytest.raises(ValueError, match="already"):
        S.StrokeModel(g, _slot())
    assert g.image_channels == 1 and g.conf.input_channels == 3 and g.encoding["sigma"] == 1.5
    assert [n for n, _ in g.named_parameters_downstream()] == ["conv.weight", "conv.bias"]
    assert S.StrokeModel(_Net(6), _slot(), clicks=clicks.ClickSlot(2, device="cpu")).image_channels == 2
    for cimg in (2, 3):
        with pytest.raises(ValueError, match="the model reads 3 channels = 1 image channels"):
            g(torch.zeros(2, cimg, 8, 8, 8))
    with pytest.raises(ValueError, match="built for a batch of 2"):
        g(torch.zeros(1, 1, 8, 8, 8))
    with pytest.raises(ValueError, match="holds strokes of a"):
        g(torch.zeros(2, 1, 8, 8, 4))
    with pytest.raises(AttributeError):
        g.no_such_attribute
    with pytest.raises(ValueError, match="must be a StrokeModel"):
        S.scribble_rounds(_Net(3), torch.zeros(2, 1, 8, 8, 8), None, _slot(), 1)
    with pytest.raises(ValueError, match="another slot"):
        S.scribble_rounds(g, torch.zeros(2, 1, 8, 8, 8), None, _slot(), 1)
    with pytest.raises(ValueError, match="rounds must be"):
        S.scribble_rounds(g, torch.zeros(2, 1, 8, 8, 8), None, g.slot, -1)


def test_package_exports_the_stroke_calls():
    import mivp_amd
    for name in ("StrokeSlot", "StrokeModel", "encode_strokes", "simulate_box", "simulate_scribbles", "strokes_ws",
                 "draw_box_jitter", "scribble_rounds", "box_then_scribbles"):
        assert callable(getattr(mivp_amd, name)), name


def test_header_declares_the_stroke_entries():
    from mivp_amd import _lib
    protos = _lib.parse_header()
    assert len(protos["mivp_strokes_draw"][1]) == 9 and len(protos["mivp_strokes_encode"][1]) == 15
    assert len(protos["mivp_strokes_box"][1]) == 16 and len(protos["mivp_strokes_scribbles"][1]) == 17
    assert len(protos["mivp_strokes_ws"][1]) == 2
