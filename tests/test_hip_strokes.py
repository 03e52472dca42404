"""GPU: box and scribble prompts (mivp_amd.strokes, csrc/strokes.hip) against the numpy restatement of tests/strokes_ref.py.

  draw       the mask bit-equal for axis-aligned, diagonal, steep and single-point strokes, a polyline that revisits voxels
             and both channels on one voxel; other samples untouched.
  encode     disk mode bit-equal at unit spacing (boxes filled and as a frame, a one-voxel box, a box equal to the volume,
             overlapping boxes of both channels); an empty channel is +0; gaussian mode and anisotropic spacing against float64
             with the project's yardstick (the kernel may err 8 x E32, E32 the largest error of the float32 numpy composition
             against float64 on the same inputs; measured ratios: see DESIGN 4.47); the anisotropic disk away from the
             radius; write extent under a NaN pattern with guard elements at every alignment of the tensor's start.
  simulate   boxes / box_count / last and mask / last integer-equal to the restatement on the cases of the issue.
  replay     a recording of [simulate_scribbles -> encode_strokes] on new pred / target over three rounds equals eager.
  end to end the 32^3 configuration with three input channels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strokes_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = 0x7FC0BEEF                                               # a NaN no kernel produces
CASES = R.scribble_cases()
ALL_SHAPES = tuple(R.SHAPES) + tuple(R.DEGENERATE)


def S():
    import mivp_amd  # noqa: F401
    from mivp_amd import strokes
    return strokes


def patterned(B, ctot, dims, lead, guard=7):
    """A [B, ctot, *dims] view at element ``lead`` of a flat buffer filled with PATTERN, and the buffer as int32."""
    n = B * ctot * dims[0] * dims[1] * dims[2]
    flat = torch.full((lead + n + guard,), PATTERN, dtype=torch.int32, device=DEV)
    return flat.view(torch.float32)[lead:lead + n].view(B, ctot, *dims), flat


def random_boxes(rng, B, KB, dims, counts):
    table = np.full((B, KB, 7), -1, dtype=np.int32)
    for b in range(B):
        for i in range(counts[b]):
            p, q = rng.integers(0, dims, size=3), rng.integers(0, dims, size=3)
            table[b, i] = [*np.minimum(p, q), *np.maximum(p, q), rng.integers(0, 2)]
    return table


def random_strokes(rng, dims, n):
    """n short polylines -> [(points, channel)]."""
    out = []
    for i in range(n):
        k = int(rng.integers(1, 4))
        out.append(([tuple(int(v) for v in rng.integers(0, dims, size=3)) for _ in range(k)], i % 2))
    return out


def filled_slot(B, dims, table, counts, strokes_per_sample, KB=4):
    """(slot, numpy mask): boxes of ``table`` and the polylines drawn on both sides."""
    slot = S().StrokeSlot(B, dims, max_boxes=KB)
    mask = np.zeros((B, *dims), dtype=np.uint8)
    for b in range(B):
        slot.set_boxes(b, [tuple(int(v) for v in r) for r in table[b, :counts[b]]])
        for pts, ch in strokes_per_sample[b]:
            slot.draw(b, pts, ch)
            mask = R.draw_ref(mask, b, pts, ch)
    return slot, mask


# =============================================================================================
# draw
# =============================================================================================
@pytest.mark.parametrize("dims", ALL_SHAPES)
def test_draw_is_bit_equal(dims):
    slot = S().StrokeSlot(3, dims)
    want = np.zeros((3, *dims), dtype=np.uint8)
    for name, (pts, ch) in R.strokes_for(dims).items():
        slot.draw(1, pts, ch)
        want = R.draw_ref(want, 1, pts, ch)
        assert np.array_equal(slot.cpu().mask, want), name
    centre = tuple(n // 2 for n in dims)
    for ch in (0, 1):                                              # both channels on one voxel: the value is 3
        slot.draw(1, [centre], ch)
        want = R.draw_ref(want, 1, [centre], ch)
    got = slot.cpu().mask
    assert np.array_equal(got, want) and got[1][centre] == 3
    assert not got[0].any() and not got[2].any() and got.max() <= 3
    last = tuple(n - 1 for n in dims)                              # the last byte of the last sample: its word ends the storage
    slot.draw(2, [last, last], 1)
    assert slot.cpu().mask[2][last] == 2
    slot.clear_scribbles()
    assert not slot.cpu().mask.any()


def test_draw_a_long_polyline_of_256_points():
    dims = R.SHAPES[2]
    rng = np.random.default_rng(4)
    pts = [tuple(int(v) for v in rng.integers(0, dims, size=3)) for _ in range(256)]
    slot = S().StrokeSlot(2, dims)
    slot.draw(0, pts, 1)
    assert np.array_equal(slot.cpu().mask, R.draw_ref(np.zeros((2, *dims), dtype=np.uint8), 0, pts, 1))


# =============================================================================================
# encode
# =============================================================================================
@pytest.mark.parametrize("box", ["filled", "frame"])
@pytest.mark.parametrize("dims,B", [(R.SHAPES[0], 2), (R.SHAPES[1], 3), (R.SHAPES[2], 2)])
def test_encode_disk_is_bit_equal_at_unit_spacing(dims, B, box):
    rng = np.random.default_rng(1)
    counts = [3, 0, 4][:B]
    table = random_boxes(rng, B, 4, dims, counts)
    strokes = [random_strokes(rng, dims, 3), [], random_strokes(rng, dims, 4)][:B]
    slot, mask = filled_slot(B, dims, table, counts, strokes)
    ws = S().strokes_ws(B, dims)
    ws.fill_(0xFF)                                                 # stale workspace contents must not matter
    for radius in (0.0, 2.0, 3.5):
        out = torch.full((B, 3, *dims), 7.0, device=DEV)
        S().encode_strokes(slot, out, channel_offset=1, box=box, kind="disk", radius=radius, workspace=ws)
        want = R.encode_ref(table, counts, mask, box=box, radius=radius, dtype=np.float32)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, 1:].view(np.int32), want.view(np.int32)), radius
        assert (got[:, 0] == 7.0).all()
    assert not got[1, 1:].any() and not np.signbit(got[1, 1:]).any()       # sample 1 has nothing: exact +0


@pytest.mark.parametrize("box", ["filled", "frame"])
def test_encode_special_boxes(box):
    dims = R.SHAPES[0]
    H, W, D = dims
    table = np.full((3, 4, 7), -1, dtype=np.int32)
    table[0, 0] = (5, 4, 3, 5, 4, 3, 0)                            # one voxel
    table[1, 0] = (0, 0, 0, H - 1, W - 1, D - 1, 1)                # the whole volume
    table[2, :4] = [(1, 1, 1, 8, 6, 4, 0), (4, 3, 2, 12, 9, 6, 1), (6, 0, 0, 9, 9, 6, 0), (2, 2, 2, 10, 7, 5, 1)]      # overlapping
    counts = [1, 1, 4]
    slot, mask = filled_slot(3, dims, table, counts, [[], [], []])
    out = torch.full((3, 2, *dims), 7.0, device=DEV)
    S().encode_strokes(slot, out, channel_offset=0, box=box)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.int32), R.encode_ref(table, counts, mask, box=box, dtype=np.float32).view(np.int32))
    assert got[0, 0].sum() == 1 and got[0, 0, 5, 4, 3] == 1 and not got[0, 1].any() and not np.signbit(got[0, 1]).any()
    assert not got[1, 0].any() and got[1, 1].sum() == (H * W * D if box == "filled" else H * W * D - (H - 2) * (W - 2) * (D - 2))
    slot.set_boxes(2, [])                                          # rows beyond box_count are not read
    S().encode_strokes(slot, out, channel_offset=0, box=box)
    assert not out[2].any()


@pytest.mark.parametrize("dims", R.DEGENERATE + ((1, 1, 1),))
def test_encode_degenerate_volumes(dims):
    rng = np.random.default_rng(6)
    table = random_boxes(rng, 2, 2, dims, [1, 0])
    slot, mask = filled_slot(2, dims, table, [1, 0], [[([tuple(n - 1 for n in dims)], 1)], [([(0, 0, 0)], 0)]], KB=2)
    for box, kind in (("filled", "disk"), ("frame", "gaussian")):
        out, flat = patterned(2, 2, dims, 9)
        S().encode_strokes(slot, out, channel_offset=0, box=box, kind=kind, radius=1.0, sigma=1.0)
        want = R.encode_ref(table, [1, 0], mask, box=box, kind=kind, radius=1.0, sigma=1.0, dtype=np.float32)
        assert np.allclose(out.cpu().numpy(), want, rtol=0, atol=0 if kind == "disk" else 1e-6)
        assert (flat[:9] == PATTERN).all() and (flat[9 + out.numel():] == PATTERN).all()


@pytest.mark.parametrize("dims,B,spacing,sigma", [(R.SHAPES[0], 2, (1, 1, 1), 2.0), (R.SHAPES[1], 3, (1, 0.8, 2.5), 1.5),
                                                  (R.SHAPES[2], 2, (1, 0.8, 2.5), 3.0), (R.SHAPES[2], 2, (1, 1, 1), 0.7)])
def test_encode_gaussian_against_float64(dims, B, spacing, sigma):
    rng = np.random.default_rng(2)
    counts = [2, 0, 1][:B]
    table = random_boxes(rng, B, 4, dims, counts)
    strokes = [random_strokes(rng, dims, 4), [([(1, 1, 1), (4, 5, 3)], 0)], random_strokes(rng, dims, 2)][:B]
    slot, mask = filled_slot(B, dims, table, counts, strokes)
    out = torch.full((B, 4, *dims), 7.0, device=DEV)
    S().encode_strokes(slot, out, channel_offset=2, kind="gaussian", sigma=sigma, spacing=spacing)
    got = out.cpu().numpy()[:, 2:].astype(np.float64)
    w64 = R.encode_ref(table, counts, mask, spacing, kind="gaussian", sigma=sigma, dtype=np.float64)
    w32 = R.encode_ref(table, counts, mask, spacing, kind="gaussian", sigma=sigma, dtype=np.float32).astype(np.float64)
    e32, err = np.abs(w32 - w64).max(), np.abs(got - w64).max()
    print(f"encode gaussian {dims} spacing {spacing} sigma {sigma}: err {err:.3e}, E32 {e32:.3e}, ratio {err / e32:.2f}")
    assert e32 > 0 and err <= 8 * e32
    empty = out[1, 3].cpu().numpy()                                # sample 1 has no negative stroke and no box
    assert not empty.any() and not np.signbit(empty).any()
    for b in range(B):                                             # a scribble voxel is exactly 1
        for ch in range(2):
            assert (out[b, 2 + ch].cpu().numpy()[((mask[b] >> ch) & 1) > 0] == 1.0).all()
    assert (out[:, :2] == 7.0).all()


@pytest.mark.parametrize("spacing", [R.EXACT_SPACING, (1, 0.8, 2.5)])
def test_encode_anisotropic_disk_away_from_the_radius(spacing):
    # r^2 = 2.89, 9.61, 22.09: at EXACT_SPACING m is a multiple of 0.25, so no voxel is within 1e-4 r^2 of the radius
    dims, B = R.SHAPES[2], 2
    rng = np.random.default_rng(8)
    table = random_boxes(rng, B, 4, dims, [1, 2])
    slot, mask = filled_slot(B, dims, table, [1, 2], [random_strokes(rng, dims, 4), random_strokes(rng, dims, 3)])
    for radius in (1.7, 3.1, 4.7):
        out = torch.empty((B, 2, *dims), device=DEV)
        S().encode_strokes(slot, out, channel_offset=0, radius=radius, spacing=spacing)
        want = R.encode_ref(table, [1, 2], mask, spacing, radius=radius, dtype=np.float64)
        r2 = radius * radius
        m = np.stack([[R.stroke_dist_sq(((mask[b] >> ch) & 1).astype(bool), spacing) for ch in range(2)] for b in range(B)])
        near = np.abs(m - r2) <= 1e-4 * r2
        print(f"anisotropic disk spacing {spacing} radius {radius}: {int(near.sum())} voxels excluded")
        if spacing == R.EXACT_SPACING:
            assert near.sum() == 0
        assert near.mean() < 0.01
        assert np.array_equal(out.cpu().numpy()[~near], want[~near].astype(np.float32))


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["gaussian", "disk"])
def test_encode_write_extent(lead, kind):
    dims, B, ctot, off = R.SHAPES[0], 2, 4, 1                      # vol = 910: the runs start at every residue of 16 bytes
    rng = np.random.default_rng(3)
    table = random_boxes(rng, B, 4, dims, [2, 0])
    slot, mask = filled_slot(B, dims, table, [2, 0], [random_strokes(rng, dims, 3), []])
    out, flat = patterned(B, ctot, dims, 8 + lead)
    S().encode_strokes(slot, out, channel_offset=off, kind=kind, box="frame")
    bits = out.view(torch.int32)
    assert (flat[:8 + lead] == PATTERN).all() and (flat[8 + lead + out.numel():] == PATTERN).all()
    assert (bits[:, 0] == PATTERN).all() and (bits[:, 3] == PATTERN).all()
    assert not (bits[:, 1:3] == PATTERN).any()
    want = R.encode_ref(table, [2, 0], mask, kind=kind, box="frame", dtype=np.float32)
    assert np.allclose(out[:, 1:3].cpu().numpy(), want, rtol=0, atol=1e-6)


# =============================================================================================
# simulate_box
# =============================================================================================
def box_case(name):
    """-> (target [B, H, W, D], KB, init boxes per sample, kwargs)."""
    dims = R.SHAPES[0]
    H, W, D = dims
    t = np.zeros((3, *dims), dtype=np.int64)
    t[0, 3:9, 2:5, 1:4] = 1
    t[1, 6, 7, 2] = 2
    t[2, 2:11, 1:9, 0:7] = 1
    t[2, 5, 5, 5] = 0
    init, KB, kw = [[], [], []], 2, {}
    if name == "empty_object":
        t[1] = 0
    elif name == "every_border":
        t[0] = 1
        kw = dict(margin=(2, 2, 2))
    elif name == "margin_clamps":
        kw = dict(margin=(4, 1, 9), channel=1)
    elif name == "jitter_inverts":
        kw = dict(jitter=np.array([[9, 9, 9, -9, -9, -9], [5, -5, 5, 5, -5, -5], [-3, 2, 0, 1, -2, 40]], dtype=np.int32),
                  margin=(1, 0, 0))
    elif name == "full_slot":
        init = [[(0, 0, 0, 1, 1, 1, 0), (1, 1, 1, 2, 2, 2, 1)], [(3, 3, 3, 4, 4, 4, 1)], []]
    elif name == "ignore_index":
        t[0, 3] = 4
        t[2, :, :, 0] = 4
        kw = dict(ignore_index=4)
    elif name == "object_classes":
        t[0, 4:6, 3, 2] = 3
        kw = dict(object_classes=(2, 3))
    return t, KB, init, kw


@pytest.mark.parametrize("tdt", ["uint8", "float32"])
@pytest.mark.parametrize("name", ["plain", "empty_object", "every_border", "margin_clamps", "jitter_inverts", "full_slot",
                                  "ignore_index", "object_classes"])
def test_simulate_box_equals_the_restatement(name, tdt):
    t, KB, init, kw = box_case(name)
    t = t.astype(tdt)
    B, dims = t.shape[0], t.shape[1:]
    slot = S().StrokeSlot(B, dims, max_boxes=KB)
    table, count = np.full((B, KB, 7), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, rows in enumerate(init):
        slot.set_boxes(b, rows)
        for i, r in enumerate(rows):
            table[b, i] = r
        count[b] = len(rows)
    target = torch.from_numpy(t).to(DEV)
    for _ in range(2):                                             # twice: the scratch words are clean again after a call
        S().simulate_box(target[:, None], slot, **kw)
        table, count, last = R.simulate_box_ref(t, table, count, **kw)
        got = slot.cpu()
        assert np.array_equal(got.last, last), (got.last, last)
        assert np.array_equal(got.box_count, count) and np.array_equal(got.boxes, table)
    assert not slot._scratch.any()
    if name == "full_slot":
        assert got.last[0, 6] == 0 and got.last[0, 3] >= 0
    if name == "empty_object":
        assert got.last[1].tolist() == [-1] * 6 + [0, 0]
    placed = got.last[:, 6] == 1
    assert (got.last[placed, :3] <= got.last[placed, 3:6]).all()


@pytest.mark.parametrize("dims", R.DEGENERATE)
def test_simulate_box_on_degenerate_volumes(dims):
    rng = np.random.default_rng(9)
    t = (rng.random((2, *dims)) < 0.4).astype(np.int32)
    slot = S().StrokeSlot(2, dims)
    jit = S().draw_box_jitter(np.random.default_rng(1), 2, 3)
    S().simulate_box(torch.from_numpy(t).to(DEV), slot, jitter=jit, margin=(1, 1, 1))
    boxes, count, last = R.simulate_box_ref(t, np.full((2, 4, 7), -1), np.zeros(2), jitter=jit, margin=(1, 1, 1))
    got = slot.cpu()
    assert np.array_equal(got.boxes, boxes) and np.array_equal(got.box_count, count) and np.array_equal(got.last, last)


# =============================================================================================
# simulate_scribbles
# =============================================================================================
def run_scribbles(c, slot=None, mask=None, workspace=None):
    B, dims = c["pred"].shape[0], c["pred"].shape[1:]
    slot = slot or S().StrokeSlot(B, dims)
    mask = np.zeros((B, *dims), dtype=np.uint8) if mask is None else mask
    S().simulate_scribbles(torch.from_numpy(c["pred"]).to(DEV), torch.from_numpy(c["target"]).to(DEV), slot, workspace=workspace,
                           **c["kwargs"])
    return slot, R.simulate_scribbles_ref(c["pred"], c["target"], mask, **c["kwargs"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_simulate_scribbles_equals_the_restatement(name):
    c = CASES[name]
    ws = S().strokes_ws(c["pred"].shape[0], c["pred"].shape[1:])
    ws.fill_(0xFF)                                                 # stale workspace contents must not matter
    slot, (mask, last) = run_scribbles(c, workspace=ws)
    got = slot.cpu()
    assert np.array_equal(got.last, last), (got.last, last)
    assert np.array_equal(got.mask, mask)
    if name == "one_iteration":
        assert (got.last[:, 2] == 0).all()
    if name == "odd_batch":
        assert (got.last[:, 0] > 0).all()


def test_simulate_scribbles_accumulates_over_two_calls():
    first, second = CASES["thick_blob"], CASES["both_regions"]
    slot, (mask, _) = run_scribbles(first)
    slot.draw(1, [(0, 0, 0), (5, 5, 5)], 1)                        # a user's stroke in between stays as well
    mask = R.draw_ref(mask, 1, [(0, 0, 0), (5, 5, 5)], 1)
    slot, (mask, last) = run_scribbles(second, slot, mask)
    got = slot.cpu()
    assert np.array_equal(got.mask, mask) and np.array_equal(got.last, last)
    assert (got.mask[0] & 1).sum() > last[0, 0] > 0                # bits of the first call are still there and were not counted
    slot, (mask, last) = run_scribbles(second, slot, mask)
    assert not slot.cpu().last[:, :2].any() and np.array_equal(slot.cpu().mask, mask)


def test_simulate_scribbles_takes_other_dtypes_and_layouts():
    c = CASES["both_regions"]
    B, dims = c["pred"].shape[0], c["pred"].shape[1:]
    _, (mask, last) = run_scribbles(c)
    for pdt, tdt in ((torch.int64, torch.float32), (torch.int32, torch.int64)):
        slot = S().StrokeSlot(B, dims)
        S().simulate_scribbles(torch.from_numpy(c["pred"]).to(DEV).to(pdt)[:, None], torch.from_numpy(c["target"]).to(DEV).to(tdt),
                               slot)
        assert np.array_equal(slot.cpu().mask, mask) and np.array_equal(slot.cpu().last, last)


@pytest.mark.parametrize("dims", R.DEGENERATE)
def test_simulate_scribbles_on_degenerate_volumes(dims):
    rng = np.random.default_rng(12)
    c = dict(pred=(rng.random((2, *dims)) < 0.3).astype(np.uint8), target=(rng.random((2, *dims)) < 0.7).astype(np.uint8),
             kwargs=dict(min_depth=1.0))
    slot, (mask, last) = run_scribbles(c)
    assert np.array_equal(slot.cpu().mask, mask) and np.array_equal(slot.cpu().last, last)
    assert mask.any()


def test_equal_calls_give_equal_bits():
    c = CASES["odd_batch"]
    a, _ = run_scribbles(c)
    b, _ = run_scribbles(c)
    for x, y in zip(a.cpu(), b.cpu()):
        assert np.array_equal(x, y)
    outs = [S().encode_strokes(a, torch.empty((3, 2, *R.SHAPES[2]), device=DEV), channel_offset=0, kind="gaussian",
                               spacing=(1, 0.8, 2.5)) for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


# =============================================================================================
# replay
# =============================================================================================
def test_recorded_scribbles_and_encode_follow_new_contents():
    dims, B = R.SHAPES[1], 2
    rounds = [CASES["thick_blob"], CASES["both_regions"], CASES["sliver"]]
    pred = torch.from_numpy(rounds[0]["pred"]).to(DEV)
    target = torch.from_numpy(rounds[0]["target"]).to(DEV)
    own, ref = S().StrokeSlot(B, dims), S().StrokeSlot(B, dims)
    own.set_boxes(0, [(1, 1, 1, 5, 5, 5, 1)])
    ref.set_boxes(0, [(1, 1, 1, 5, 5, 5, 1)])
    x_own, x_ref = torch.zeros((B, 3, *dims), device=DEV), torch.zeros((B, 3, *dims), device=DEV)
    ws = S().strokes_ws(B, dims)

    def step(slot, x):
        S().simulate_scribbles(pred, target, slot, workspace=ws, max_iter=12)
        S().encode_strokes(slot, x, channel_offset=1, kind="gaussian", sigma=1.5, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(own, x_own)                                           # warm-up on the slot whose scribbles are then cleared
    torch.cuda.current_stream().wait_stream(side)
    own.clear_scribbles()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(own, x_own)
    own.clear_scribbles()                                          # the capture launched nothing: start from an empty mask
    mask = np.zeros((B, *dims), dtype=np.uint8)
    for r in range(3):
        pred.copy_(torch.from_numpy(rounds[r]["pred"]))
        target.copy_(torch.from_numpy(rounds[r]["target"]))
        graph.replay()
        step(ref, x_ref)
        torch.cuda.synchronize()
        for a, b in zip(own.cpu(), ref.cpu()):
            assert np.array_equal(a, b), r
        assert torch.equal(x_own.view(torch.int32), x_ref.view(torch.int32)), r
        mask, last = R.simulate_scribbles_ref(rounds[r]["pred"], rounds[r]["target"], mask, max_iter=12)
        got = own.cpu()
        assert np.array_equal(got.mask, mask) and np.array_equal(got.last, last), r


# =============================================================================================
# end to end
# =============================================================================================
def stroke_setup(cin=3):
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, size, batch = train.make_conf("tiny")
    conf.input_channels = cin
    torch.manual_seed(0)
    model = SwinUnetR(conf).to(DEV).train()
    g = torch.Generator().manual_seed(5)
    image = torch.rand((batch, 1, size, size, size), generator=g).to(DEV)
    target = torch.zeros((batch, 1, size, size, size))
    target[0, 0, 8:20, 6:18, 10:22] = 1
    target[1, 0, 14:28, 12:24, 4:16] = 1
    return conf, model, image, target.to(DEV), S().StrokeSlot(batch, (size, size, size))


def test_stroke_model_end_to_end():
    from mivp_amd import train
    conf, model, image, target, slot = stroke_setup()
    guided = S().StrokeModel(model, slot, kind="gaussian", sigma=2.0)
    with torch.no_grad():
        got = guided(image)["downstream"]
        want = model(torch.cat([image, torch.zeros_like(image), torch.zeros_like(image)], dim=1))["downstream"]
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    first = got.argmax(dim=1).cpu().numpy()                        # the prediction the first round corrects
    thick = [R.core_map(first[b], target[b, 0].cpu().numpy()).any() for b in range(first.shape[0])]
    logits = S().scribble_rounds(guided, image, target, slot, rounds=2, max_iter=16)
    rec = slot.cpu()
    assert logits.shape == got.shape and any(thick)                # (a 12^3 object: an untrained model misses it or floods it)
    for b, has in enumerate(thick):
        assert not has or rec.mask[b].any()                        # a core's skeleton is never empty
    assert rec.mask.max() <= 3
    with torch.no_grad():                                          # the scribbles now reach the model: another output
        assert not torch.equal(guided(image)["downstream"], want)
    opt = train.build_optimizer(guided, conf)
    loss = train.train_step(guided, opt, conf, image, target)
    assert bool(torch.isfinite(loss))
    before = slot.cpu().mask
    assert S().scribble_rounds(guided, image, None, slot, rounds=1).shape == got.shape      # target=None: the caller's strokes only
    assert np.array_equal(slot.cpu().mask, before)
    S().box_then_scribbles(guided, image, target, slot, rounds=1, max_iter=16, box_kwargs=dict(margin=(2, 2, 2)))
    rec = slot.cpu()
    assert rec.box_count.tolist() == [1, 1] and rec.boxes[0, 0].tolist() == [6, 4, 8, 21, 19, 23, 0]


def test_stroke_model_with_clicks_reads_both_slots():
    from mivp_amd import clicks
    conf, model, image, target, slot = stroke_setup(cin=5)
    cslot = clicks.ClickSlot(image.shape[0], max_clicks=4)
    guided = S().StrokeModel(model, slot, clicks=cslot, kind="gaussian", sigma=2.0)
    zero = torch.zeros_like(image)
    with torch.no_grad():
        got = guided(image)["downstream"]
        want = model(torch.cat([image, zero, zero, zero, zero], dim=1))["downstream"]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    slot.draw(0, [(4, 4, 4), (20, 20, 20)], 0)
    cslot.set(1, [(10, 10, 10, 1)])
    x = guided.model_input(image)
    assert x.shape[1] == 5 and x[0, 1, 4, 4, 4] == 1 and x[1, 4, 10, 10, 10] == 1 and not x[1, 1:3].any() and not x[0, 3:].any()
