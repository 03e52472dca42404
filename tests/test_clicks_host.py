"""CPU: the numpy restatement of the click encoding and simulation (tests/clicks_ref.py) against scipy's padded transform
and a brute-force pick, the shared cases' expectations, and the argument refusals of mivp_amd.clicks, which all happen
before any launch (every tensor here is a CPU tensor)."""
import itertools
from argparse import Namespace

import numpy as np
import pytest
import torch
from scipy import ndimage

import clicks_ref as R

CASES = R.simulate_cases()


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,rtol", [((1, 1, 1), 1e-12), (R.EXACT_SPACING, 1e-12), ((1, 0.8, 2.5), 1e-6)])
def test_depth_is_the_padded_scipy_transform(spacing, rtol):
    rng = np.random.default_rng(3)
    for density in (0.5, 0.9, 1.0):
        mask = rng.random((13, 10, 7)) < density
        want = ndimage.distance_transform_edt(np.pad(mask, 1), sampling=spacing)[1:-1, 1:-1, 1:-1] ** 2
        got = R.depth_sq(mask, spacing)
        assert np.allclose(got, want, rtol=rtol, atol=0)
        assert ((got > 0) == mask).all()


@pytest.mark.parametrize("spacing", [(1, 1, 1), R.EXACT_SPACING])
def test_depth_is_the_inner_transform_capped_by_the_faces(spacing):
    # the identity the kernels use: min(transform inside the volume, (distance along an axis to the nearest face)^2)
    rng = np.random.default_rng(4)
    a = R.spacing_sq(spacing)
    for density in (0.6, 1.0):
        mask = rng.random((9, 8, 7)) < density
        if mask.all():
            inner = np.full(mask.shape, np.inf)
        else:
            inner = ndimage.distance_transform_edt(mask, sampling=[np.sqrt(v) for v in a]) ** 2
        g = np.meshgrid(*[np.arange(n) for n in mask.shape], indexing="ij")
        face = np.minimum.reduce([a[k] * np.minimum(g[k] + 1, mask.shape[k] - g[k]) ** 2 for k in range(3)])
        want = np.where(mask, np.minimum(inner, face), 0.0)
        assert np.allclose(R.depth_sq(mask, spacing), want, rtol=1e-12, atol=0)


def _brute_pick(e_pos, e_neg, a):
    best = None                                                    # (depth^2, channel, index): larger depth, then channel 0, then low index
    dims = e_pos.shape
    for ch, reg in ((0, e_pos), (1, e_neg)):
        pad = np.pad(reg, 1)
        outside = np.argwhere(~pad) - 1
        for idx, v in enumerate(itertools.product(*[range(n) for n in dims])):
            if not reg[v]:
                continue
            d = min(float(sum(a[k] * (v[k] - o[k]) ** 2 for k in range(3))) for o in outside)
            if best is None or d > best[0]:
                best = (d, ch, idx)
    return best


@pytest.mark.parametrize("seed", range(6))
def test_pick_against_a_brute_force_loop(seed):
    rng = np.random.default_rng(100 + seed)
    dims = [(6, 5, 4), (4, 4, 4), (5, 3, 2), (6, 5, 4), (3, 5, 4), (2, 2, 2)][seed]
    spacing = (1, 1, 1) if seed % 2 == 0 else R.EXACT_SPACING
    pred = R.blobs(rng, dims, classes=2, cell=2)[None]
    target = R.blobs(rng, dims, classes=2, cell=2)[None]
    if seed == 5:
        pred, target = np.zeros_like(pred), np.ones_like(target)
    e_pos, e_neg = R.error_regions(pred[0], target[0])
    want = _brute_pick(e_pos, e_neg, R.spacing_sq(spacing))
    clicks, count, last = R.simulate_ref(pred, target, np.full((1, 4, 4), -1), np.zeros(1), spacing)
    if want is None:
        assert count[0] == 0 and tuple(last[0]) == (0, -1, -1, 0)
        return
    d, ch, idx = want
    W, D = dims[1], dims[2]
    assert count[0] == 1
    assert tuple(clicks[0, 0]) == (idx // (W * D), (idx // D) % W, idx % D, ch)
    assert tuple(last[0]) == (int(np.float32(d).view(np.int32)), ch, idx, 1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_case_is_left_to_rounding(name):
    c = CASES[name]
    assert R.is_exact(c["pred"], c["target"], c["kwargs"].get("spacing", (1, 1, 1)), c["kwargs"].get("object_classes"),
                      c["kwargs"].get("ignore_index"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_expectations(name):
    c = CASES[name]
    K = c["K"]
    clicks = np.full((2, K, 4), -1, dtype=np.int32)
    count = np.zeros(2, dtype=np.int32)
    for b, rows in enumerate(c["init"]):
        for i, r in enumerate(rows):
            clicks[b, i] = r
        count[b] = len(rows)
    new, cnt, last = R.simulate_ref(c["pred"], c["target"], clicks, count, **c["kwargs"])
    if c["want"] is None:
        assert cnt[0] == count[0] and last[0, 3] == 0 and np.array_equal(new[0], clicks[0])
    elif c["want"] != "any":
        assert cnt[0] == count[0] + 1 and tuple(new[0, count[0]]) == c["want"] and last[0, 3] == 1
    if name in ("min_depth", "full_slot"):
        assert last[0, 1] == 0 and last[0, 2] >= 0                 # a winner was found and not placed
    if name == "no_error":
        assert tuple(last[0]) == (0, -1, -1, 0)
    if name == "tie_regions":
        e_pos, e_neg = R.error_regions(c["pred"][0], c["target"][0])
        assert R.depth_sq(e_pos).max() == R.depth_sq(e_neg).max() == 4.0
        assert np.flatnonzero(e_neg.reshape(-1))[0] < np.flatnonzero(e_pos.reshape(-1))[0]
    if name == "face_slab":
        assert R.depth_sq(R.error_regions(c["pred"][0], c["target"][0])[0])[0].max() == 1.0    # the face h = 0 is shallow


def test_encode_restatement_is_the_maximum_of_the_gaussians():
    clicks = np.array([[(2, 3, 1, 0), (5, 1, 4, 0), (4, 4, 4, 1), (0, 0, 0, -1)]], dtype=np.int32)
    out = R.encode_ref(clicks, [3], (7, 6, 5), spacing=(1, 0.8, 2.5), sigma=1.5)
    a = R.spacing_sq((1, 0.8, 2.5))
    g = np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij")
    each = [np.exp(-sum(a[k] * (g[k] - c[k]) ** 2 for k in range(3)) / 4.5) for c in clicks[0, :2]]
    assert np.allclose(out[0, 0], np.maximum(*each), rtol=1e-14)
    assert out[0, 0, 2, 3, 1] == 1.0 and out[0, 1, 4, 4, 4] == 1.0
    empty = R.encode_ref(clicks, [0], (7, 6, 5))
    assert not empty.any() and not np.signbit(empty).any()
    disk = R.encode_ref(clicks, [3], (7, 6, 5), kind="disk", radius=1.0)
    assert disk[0, 0].sum() == 7 + 6 and disk[0, 1].sum() == 6    # a click at d = 4 loses its neighbour beyond the face


# ---------------------------------------------------------------------------------------------------------------------
# refusals, all before any launch
# ---------------------------------------------------------------------------------------------------------------------
def _clicks():
    import mivp_amd  # noqa: F401
    from mivp_amd import clicks
    return clicks


def _slot(**kw):
    return _clicks().ClickSlot(2, device="cpu", **kw)


@pytest.mark.parametrize("bad", [65, 0, -1, True, 2.0, "8"])
def test_slot_refuses_a_bad_capacity(bad):
    with pytest.raises(ValueError, match="max_clicks must be"):
        _clicks().ClickSlot(2, max_clicks=bad, device="cpu")


def test_slot_takes_64():
    assert _slot(max_clicks=64).clicks.shape == (2, 64, 4)


@pytest.mark.parametrize("bad", [(1, 2, 3, 2), (1, 2, 3, -1), (1, 2, 3, True), (1, 2, 3, 0.0)])
def test_slot_refuses_a_bad_channel(bad):
    s = _slot(dims=(8, 8, 8))
    with pytest.raises(ValueError, match="channel must be 0|must be four integers"):
        s.set(0, [bad])
    with pytest.raises(ValueError, match="channel must be 0|must be four integers"):
        s.add(0, bad)
    assert (s.clicks == -1).all() and (s.count == 0).all()


@pytest.mark.parametrize("bad", [(8, 0, 0, 0), (0, 8, 0, 1), (0, 0, 8, 0), (-1, 0, 0, 0), (0, 0, 70000, 1)])
def test_slot_refuses_a_coordinate_outside_the_volume(bad):
    s = _slot(dims=(8, 8, 8))
    with pytest.raises(ValueError, match="is outside 0 .."):
        s.set(1, [(1, 1, 1, 0), bad])
    assert (s.clicks == -1).all() and (s.count == 0).all()


def test_an_unbound_slot_is_checked_when_it_meets_the_volume():
    C = _clicks()
    s = _slot()
    s.set(0, [(9, 1, 1, 0)])
    with pytest.raises(ValueError, match="outside the volume"):
        C.encode_clicks(s, torch.zeros(2, 3, 8, 8, 8), channel_offset=1)
    s.clear()
    s.set(0, [(7, 7, 7, 1)])
    with pytest.raises(RuntimeError, match="GPU tensor"):            # everything else was in order: the last check
        C.encode_clicks(s, torch.zeros(2, 3, 8, 8, 8), channel_offset=1)
    with pytest.raises(ValueError, match="holds clicks of a"):
        C.encode_clicks(s, torch.zeros(2, 3, 8, 8, 9), channel_offset=1)


def test_slot_set_add_clear_cpu():
    s = _slot(max_clicks=3, dims=(8, 8, 8))
    s.set(1, [(1, 2, 3, 0), (4, 5, 6, 1)])
    s.add(1, (7, 7, 7, 0))
    with pytest.raises(ValueError, match="is full"):
        s.add(1, (0, 0, 0, 0))
    with pytest.raises(ValueError, match="the slot takes 3"):
        s.set(0, [(0, 0, 0, 0)] * 4)
    with pytest.raises(ValueError, match="sample index"):
        s.set(2, [])
    rec = s.cpu()
    assert rec.count.tolist() == [0, 3] and rec.clicks[1].tolist() == [[1, 2, 3, 0], [4, 5, 6, 1], [7, 7, 7, 0]]
    assert (rec.clicks[0] == -1).all()
    s.clear()
    assert (s.clicks == -1).all() and (s.count == 0).all() and (s.last == 0).all()


@pytest.mark.parametrize("bad", [-1, 2, 3, True, 1.0, None])
def test_encode_refuses_a_wrong_channel_offset(bad):
    with pytest.raises(ValueError, match=r"channel_offset must be an integer in 0 \.\. 1"):
        _clicks().encode_clicks(_slot(), torch.zeros(2, 3, 4, 4, 4), channel_offset=bad)


def test_encode_refuses_other_bad_arguments():
    C = _clicks()
    x = torch.zeros(2, 3, 4, 4, 4)
    for kw, text in ((dict(kind="box"), "kind must be one of"), (dict(sigma=0.0), "sigma must be > 0"),
                     (dict(kind="disk", radius=-1.0), "radius must be >= 0"), (dict(spacing=(1, 0, 1)), "spacing must be three")):
        with pytest.raises(ValueError, match=text):
            C.encode_clicks(_slot(), x, channel_offset=1, **kw)
    with pytest.raises(ValueError, match="float32"):
        C.encode_clicks(_slot(), x.double(), channel_offset=1)
    with pytest.raises(ValueError, match="built for a batch of 2"):
        C.encode_clicks(_slot(), torch.zeros(3, 3, 4, 4, 4), channel_offset=1)
    with pytest.raises(ValueError, match="must be a ClickSlot"):
        C.encode_clicks(None, x, channel_offset=1)


def test_simulate_refuses_bad_arguments():
    C = _clicks()
    y = torch.zeros(2, 4, 4, 4)
    with pytest.raises(ValueError, match="must be .B, 1, H, W, D. or .B, H, W, D."):
        C.simulate_clicks(torch.zeros(4, 4, 4), y, _slot())
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.simulate_clicks(y, y, _slot())
    for bad in ([], [32], [-1], [1, 1], [True], [1.0]):
        with pytest.raises(ValueError, match="object_classes"):
            C.object_mask(bad)
    assert C.object_mask(None) == 0xFFFFFFFE and C.object_mask([0, 31]) == (1 << 31) | 1 and C.object_mask((2,)) == 4
    with pytest.raises(ValueError, match="outside the kernels' range"):
        C.simulate_clicks_ws(1, (70000, 4, 4))
    with pytest.raises(ValueError, match="logits must be"):
        C.simulate_clicks_from_logits(torch.zeros(2, 33, 4, 4, 4), y, _slot())


class _Net(torch.nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.conf = Namespace(input_channels=cin)
        self.conv = torch.nn.Conv3d(cin, 2, 1)

    def forward(self, x):
        return self.conv(x)

    def named_parameters_downstream(self):
        return list(self.named_parameters())


@pytest.mark.parametrize("cin", [1, 2])
def test_guided_model_refuses_a_model_without_guidance_channels(cin):
    with pytest.raises(ValueError, match="conf.input_channels >= 3"):
        _clicks().GuidedModel(_Net(cin), _slot())


def test_guided_model_refuses_a_channel_count_mismatch():
    C = _clicks()
    g = C.GuidedModel(_Net(3), _slot())
    assert g.image_channels == 1 and g.conf.input_channels == 3
    assert [n for n, _ in g.named_parameters_downstream()] == ["conv.weight", "conv.bias"]
    for cimg in (2, 3):
        with pytest.raises(ValueError, match="the model reads 3 channels = 1 image channels"):
            g(torch.zeros(2, cimg, 4, 4, 4))
    with pytest.raises(ValueError, match="built for a batch of 2"):
        g(torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(ValueError, match="must be a ClickSlot"):
        C.GuidedModel(_Net(3), None)
    with pytest.raises(ValueError, match="GuidedModel already"):
        C.GuidedModel(g, _slot())
    with pytest.raises(AttributeError):
        g.no_such_attribute


def test_package_exports_the_click_calls():
    import mivp_amd
    for name in ("ClickSlot", "GuidedModel", "encode_clicks", "simulate_clicks", "simulate_clicks_from_logits",
                 "simulate_clicks_ws", "click_rounds", "refine_volume"):
        assert callable(getattr(mivp_amd, name)), name


def test_header_declares_the_click_entries():
    from mivp_amd import _lib
    protos = _lib.parse_header()
    assert len(protos["mivp_clicks_encode"][1]) == 12 and len(protos["mivp_clicks_simulate"][1]) == 18
    assert len(protos["mivp_clicks_simulate_ws"][1]) == 2
