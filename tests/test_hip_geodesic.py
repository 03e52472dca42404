"""GPU: geodesic distance guidance (mivp_amd.geodesic, csrc/geodesic.hip) against the restatement of tests/geodesic_ref.py.

  field      the converged field bit-equal to the float32 Dijkstra on every case and both planes (13 x 10 x 7 is below the 16 x 16
             x 32 brick on every axis, 17 x 17 x 33 one voxel above it on every axis; the serpentine crosses brick faces many
             times); info reports converged.
  seeds      the mask bit-equal to the numpy union for strokes, clicks, both, neither; a channel -1 and a count above K.
  blind      max_iter = 2 on the serpentine: not converged, nowhere below the restatement, equal calls equal bits; max_iter =
             n* + 3 gives the converged bits for both parities of n*.
  encode     disk bit-equal to the float32 restatement on the kernel's own field; gaussian within the siblings' bar (the
             kernel may err 8 x E32 against float64, E32 the error of the float32 numpy composition on the same field); an
             empty channel is +0; filled and frame boxes; write extent under a NaN pattern with guard bands.
  replay     a recording of [simulate_clicks_from_logits -> encode_geodesic(max_iter=n)] over three rounds equals eager.
  end to end the 32^3 configuration with three input channels."""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geodesic_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = 0x7FC0BEEF                                               # a NaN no kernel produces


def G():
    import mivp_amd  # noqa: F401
    from mivp_amd import geodesic
    return geodesic


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def device_case(name):
    """-> (image f32 [B, 2, H, W, D] with the case's image in channel 1 and noise in channel 0, seeds u8 [B, H, W, D])"""
    c = R.CASES[name]
    img = torch.from_numpy(c["image"])
    image = torch.stack([torch.rand(img.shape, generator=torch.Generator().manual_seed(1)) * 9, img], dim=1).contiguous().to(DEV)
    return image, torch.from_numpy(c["seeds"]).to(DEV)


def run_field(name, **kw):
    c = R.CASES[name]
    image, seeds = device_case(name)
    f = G().geodesic_distance(image, seeds, image_channel=1, spacing=c["spacing"], gamma=c["gamma"], **kw)
    return f.field.cpu().numpy(), f.info.cpu().numpy()


# =============================================================================================
# the field
# =============================================================================================
def test_the_shapes_cover_the_brick():
    brick = G().BRICK
    assert brick == R.BRICK
    assert any(all(s == b + 1 for s, b in zip(d, brick)) for d in R.SHAPES)
    assert any(all(s < b for s, b in zip(d, brick)) for d in R.SHAPES)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_converged_field_is_bit_equal(name):
    want = R.field(name)
    ws = G().geodesic_ws(want.shape[0], want.shape[2:])
    ws.fill_(0xFF)                                                 # stale workspace contents must not matter
    got, info = run_field(name, workspace=ws)
    diff = bits(got) != bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[0], got[diff][0], want[diff][0])
    assert info[1] == 1 and 0 <= info[0] < G().iteration_cap(want.shape[2:])
    got2, info2 = run_field(name, check_every=1)                   # another cadence of the host read: the same bits
    assert np.array_equal(bits(got2), bits(want)) and info2.tolist() == info.tolist()


def test_special_planes():
    got, _ = run_field("ramp_small")
    seeds = R.CASES["ramp_small"]["seeds"]
    assert got[0, 0, 0, 0, 0] == 0 and got[0, 1, -1, -1, -1] == 0 and np.isfinite(got[0]).all()      # first and last voxel
    assert not got[1, 0].any() and not np.signbit(got[1, 0]).any() and seeds[1].all()                # a seed on every voxel
    assert np.isinf(got[1, 1]).all() and np.isinf(got[2, 1]).all()                                   # planes without seeds


# =============================================================================================
# seeds
# =============================================================================================
def filled_slots(dims, B=2, K=4):
    from mivp_amd import clicks, strokes
    st, ck = strokes.StrokeSlot(B, dims), clicks.ClickSlot(B, max_clicks=K, dims=dims)
    st.draw(0, [(0, 0, 0), tuple(n - 1 for n in dims)], 0)
    st.draw(1, [(dims[0] // 2, 0, dims[2] - 1)], 1)
    st.set_boxes(0, [(0, 0, 0, dims[0] - 1, 0, 0, 1)])             # boxes are no seeds
    ck.set(0, [(dims[0] - 1, dims[1] - 1, dims[2] - 1, 1), (0, 0, 0, 0)])
    ck.set(1, [(0, dims[1] - 1, 0, 0), (dims[0] - 1, 0, 0, 1), (0, 0, dims[2] - 1, 1), (dims[0] // 2, 0, dims[2] - 1, 0)])
    ck.clicks[1, 2, 3] = -1                                        # an entry the device must skip
    ck.count[1] = K + 5                                            # and a count it must clamp
    return st, ck


@pytest.mark.parametrize("dims", [R.SHAPES[0], (5, 3, 3), R.DEGENERATE[1]])
def test_seed_mask_is_the_union(dims):
    st, ck = filled_slots(dims)
    rec, crec = st.cpu(), ck.cpu()
    assert crec.count[1] == 9 and crec.clicks[1, 2, 3] == -1
    for use_st, use_ck in ((True, False), (False, True), (True, True), (False, False)):
        out = None
        if not (use_st or use_ck):
            n = 2 * dims[0] * dims[1] * dims[2]
            out = torch.full(((n + 3) // 4 * 4,), 0xEE, dtype=torch.uint8, device=DEV)[:n].view(2, *dims)
        got = G().seed_mask(dims, strokes=st if use_st else None, clicks=ck if use_ck else None, out=out)
        want = R.seed_union(dims, 2, rec.mask if use_st else None, crec.clicks if use_ck else None, crec.count)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (use_st, use_ck)
        assert want.any() == (use_st or use_ck) and want.max() <= 3
    assert np.array_equal(st.cpu().mask, rec.mask)                 # the slots are read only


@pytest.mark.parametrize("dims", [(5, 3, 3), R.SHAPES[0]])          # 90 bytes (the last word is partial) and 1820
def test_seed_mask_write_extent(dims):
    st, ck = filled_slots(dims)                                    # a click and a stroke end on the last voxel of sample 0
    n, band = 2 * dims[0] * dims[1] * dims[2], 1024
    flat = torch.full((band + n + band,), 0xEE, dtype=torch.uint8, device=DEV)
    out = flat[band:band + n].view(2, *dims)
    ck.set(1, [(dims[0] - 1, dims[1] - 1, dims[2] - 1, 1)])        # and one on the last byte of the mask
    rec, crec = st.cpu(), ck.cpu()
    for use_st, use_ck in ((True, True), (False, True), (True, False)):
        flat.fill_(0xEE)
        G().seed_mask(dims, strokes=st if use_st else None, clicks=ck if use_ck else None, out=out)
        want = R.seed_union(dims, 2, rec.mask if use_st else None, crec.clicks if use_ck else None, crec.count)
        assert np.array_equal(out.cpu().numpy(), want) and (not use_ck or want[1, -1, -1, -1] == 2)
        assert (flat[:band] == 0xEE).all() and (flat[band + n:] == 0xEE).all()     # the bytes behind it, its word's rest included


# =============================================================================================
# blind launches
# =============================================================================================
def test_two_blind_iterations_are_deterministic_and_above_the_fixed_point():
    want = R.field("serpentine")
    a, info = run_field("serpentine", max_iter=2)
    b, _ = run_field("serpentine", max_iter=2)
    assert info.tolist() == [2, 0]
    assert np.array_equal(bits(a), bits(b))
    assert (a >= want).all() and (a > want).any()


def test_blind_launches_behind_the_fixed_point_change_nothing():
    seen = {}
    for name in ("serpentine", "blobs_long", "blocky_over_brick", "blocky_mid_aniso", "ramp_small"):
        nstar = int(run_field(name)[1][0])
        seen.setdefault(nstar & 1, (name, nstar))
    if len(seen) == 1:                                             # every n* has one parity: one launch more reaches the other
        (parity, (name, nstar)), = seen.items()
        seen[parity ^ 1] = (name, nstar + 1)
    assert sorted(seen) == [0, 1]
    for parity, (name, n) in seen.items():
        got, info = run_field(name, max_iter=n + 3)
        print(f"{name}: {n} + 3 blind launches, info {info.tolist()}")
        assert np.array_equal(bits(got), bits(R.field(name))), name
        assert info[1] == 1 and info[0] <= n


# =============================================================================================
# the closing pass
# =============================================================================================
def random_boxes(rng, B, KB, dims, counts):
    table = np.full((B, KB, 7), -1, dtype=np.int32)
    for b in range(B):
        for i in range(counts[b]):
            p, q = rng.integers(0, dims, size=3), rng.integers(0, dims, size=3)
            table[b, i] = [*np.minimum(p, q), *np.maximum(p, q), rng.integers(0, 2)]
    return table


def encode_case(name, counts, **kw):
    """encode_geodesic of a case with random boxes -> (out numpy [B, 4, H, W, D], the kernel's own field, table)"""
    from mivp_amd import strokes
    c = R.CASES[name]
    image, seeds = device_case(name)
    B, dims = image.shape[0], tuple(image.shape[2:])
    st = strokes.StrokeSlot(B, dims)
    st.mask.copy_(seeds)
    table = random_boxes(np.random.default_rng(5), B, 4, dims, counts)
    for b in range(B):
        st.set_boxes(b, [tuple(int(v) for v in r) for r in table[b, :counts[b]]])
    ws = G().geodesic_ws(B, dims)
    out = torch.full((B, 4, *dims), 7.0, device=DEV)
    G().encode_geodesic(image, out, strokes=st, channel_offset=2, image_channel=1, gamma=c["gamma"], spacing=c["spacing"],
                        workspace=ws, **kw)
    assert G().geodesic_info(ws, B, dims)[1] == 1
    field = G()._Layout(B, dims).field_of(ws, 0).cpu().numpy()     # converged: both buffers hold it
    got = out.cpu().numpy()
    assert (got[:, :2] == 7.0).all()
    return got[:, 2:], field, table


@pytest.mark.parametrize("box", ["filled", "frame"])
@pytest.mark.parametrize("name,counts", [("ramp_small", [2, 0, 3]), ("blobs_long", [3, 1])])
def test_encode_disk_is_bit_equal_on_the_kernels_field(name, counts, box):
    for radius in (0.0, 2.0, 5.5):
        got, field, table = encode_case(name, counts, kind="disk", radius=radius, box=box)
        assert np.array_equal(bits(field), bits(R.field(name)))
        want = R.encode_ref(field, table, counts, box=box, kind="disk", radius=radius, dtype=np.float32)
        assert np.array_equal(bits(got), bits(want)), radius
        inside = R.SR.box_ref(table, counts, field.shape[2:], box)
        assert inside.any() and (got[inside] == 1).all()           # the boxes are in it
    if name == "ramp_small":                                       # sample 2 has no negative seed; clear its boxes' channel
        empty = got[2, 1][~R.SR.box_ref(table, counts, field.shape[2:], box)[2, 1]]
        assert not empty.any() and not np.signbit(empty).any()


@pytest.mark.parametrize("name,sigma", [("ramp_small", 2.0), ("blocky_mid_aniso", 1.5), ("blobs_long", 3.0), ("serpentine", 40.0)])
def test_encode_gaussian_against_float64(name, sigma):
    counts = [1, 0, 2][:R.CASES[name]["image"].shape[0]]
    got, field, table = encode_case(name, counts, kind="gaussian", sigma=sigma, box="frame")
    w64 = R.encode_ref(field, table, counts, box="frame", kind="gaussian", sigma=sigma, dtype=np.float64)
    w32 = R.encode_ref(field, table, counts, box="frame", kind="gaussian", sigma=sigma, dtype=np.float32).astype(np.float64)
    e32, err = np.abs(w32 - w64).max(), np.abs(got.astype(np.float64) - w64).max()
    print(f"encode gaussian {name} sigma {sigma}: err {err:.3e}, E32 {e32:.3e}, ratio {err / e32:.2f}")
    assert e32 > 0 and err <= 8 * e32
    seeds = R.CASES[name]["seeds"]
    for b in range(seeds.shape[0]):
        for ch in range(2):
            assert (got[b, ch][((seeds[b] >> ch) & 1) > 0] == 1.0).all()       # a seed is exactly 1
            if not ((seeds[b] >> ch) & 1).any() and not (table[b, :counts[b], 6] == ch).any():
                assert not got[b, ch].any() and not np.signbit(got[b, ch]).any()      # an empty channel is +0


def test_encode_without_slots_is_all_zero():
    image, _ = device_case("ramp_small")
    out = torch.full((3, 3, *image.shape[2:]), 7.0, device=DEV)
    G().encode_geodesic(image, out, channel_offset=1, gamma=1.0, spacing=(1, 1, 1), max_iter=3)
    got = out.cpu().numpy()
    assert (got[:, 0] == 7.0).all() and not got[:, 1:].any() and not np.signbit(got[:, 1:]).any()


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("dims", [R.SHAPES[0], (5, 3, 3)])          # vol = 910 and 45: with the offsets, every alignment
def test_encode_write_extent(dims, off):
    from mivp_amd import clicks, strokes
    g = G()
    B, ctot, lead, band = 2, 5, 8, 4096
    starts = {((b * ctot + o) * v + lead) % 4 for b in range(B) for o in (1, 2) for v in (910, 45)}
    assert starts == {0, 1, 2, 3}                                  # the runs of the four cases start at every residue of 16 bytes
    n = B * ctot * dims[0] * dims[1] * dims[2]
    flat = torch.full((lead + n + 7,), PATTERN, dtype=torch.int32, device=DEV)
    out = flat.view(torch.float32)[lead:lead + n].view(B, ctot, *dims)
    iflat = torch.full((n + 16,), 0.25, device=DEV)                # the image with guard elements around it
    image = iflat[8:8 + n].view(B, ctot, *dims)
    image.copy_(torch.rand(image.shape, generator=torch.Generator().manual_seed(2)))
    ibits = iflat.view(torch.int32).clone()
    size = g._Layout(B, dims).size
    wflat = torch.full((band + size + band,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wflat[band:band + size]                                   # the seed mask is its front
    st, ck = strokes.StrokeSlot(B, dims), clicks.ClickSlot(B, dims=dims)
    st.draw(0, [(0, 0, 0), tuple(s - 1 for s in dims)], 0)
    st.set_boxes(1, [(1, 1, 1, 3, 2, 2, 1)])
    ck.set(1, [(dims[0] - 1, dims[1] - 1, dims[2] - 1, 0)])        # the last byte of the mask
    for kind in ("gaussian", "disk"):
        flat.fill_(PATTERN)
        g.encode_geodesic(image, out, strokes=st, clicks=ck, channel_offset=off, image_channel=0, gamma=30.0, spacing=(1, 0.8, 2.5),
                          kind=kind, box="frame", workspace=ws)
        b32 = out.view(torch.int32)
        assert (flat[:lead] == PATTERN).all() and (flat[lead + n:] == PATTERN).all()
        others = [c for c in range(ctot) if c not in (off, off + 1)]
        assert (b32[:, others] == PATTERN).all() and not (b32[:, off:off + 2] == PATTERN).any()
        assert (wflat[:band] == 0xA5).all() and (wflat[band + size:] == 0xA5).all()
        assert torch.equal(iflat.view(torch.int32), ibits)
        assert out[0, off, 0, 0, 0] == 1 and out[1, off][-1, -1, -1] == 1 and out[1, off + 1, 1, 1, 1] == 1
    assert int(g.geodesic_info(ws, B, dims)[1]) == 1


# =============================================================================================
# replay
# =============================================================================================
def test_recorded_clicks_and_encode_follow_new_contents():
    from mivp_amd import clicks
    g = G()
    dims, B, n = R.SHAPES[3], 2, 6
    rng = np.random.default_rng(7)
    rounds = []
    for r in range(3):
        target = np.zeros((B, *dims), dtype=np.int64)
        target[0, 2 + r:9 + r, 3:12, 5:20] = 1
        target[1, 8:15, 1 + r:9, 12 + r:30] = 1
        logits = rng.standard_normal((B, 2, *dims)).astype(np.float32)
        rounds.append((logits, target, np.stack([R.blocky(dims, 40 + r), R.blobs(dims, 50 + r)])[:, None]))
    logits = torch.from_numpy(rounds[0][0]).to(DEV)
    target = torch.from_numpy(rounds[0][1]).to(DEV)
    image = torch.from_numpy(rounds[0][2]).to(DEV)
    own, ref = clicks.ClickSlot(B, max_clicks=4, dims=dims), clicks.ClickSlot(B, max_clicks=4, dims=dims)
    x_own, x_ref = torch.zeros((B, 3, *dims), device=DEV), torch.zeros((B, 3, *dims), device=DEV)
    ws_own, ws_ref, sim = g.geodesic_ws(B, dims), g.geodesic_ws(B, dims), clicks.simulate_clicks_ws(B, dims)

    def step(slot, x, ws):
        clicks.simulate_clicks_from_logits(logits, target, slot, workspace=sim)
        g.encode_geodesic(image, x, clicks=slot, channel_offset=1, gamma=30.0, spacing=(1, 1, 1), sigma=6.0, max_iter=n, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(own, x_own, ws_own)                                   # warm-up on the slot that is then cleared
    torch.cuda.current_stream().wait_stream(side)
    own.clear()
    own.bind(dims)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(own, x_own, ws_own)
    own.clear()                                                    # the capture launched nothing: start from an empty slot
    own.bind(dims)
    for r in range(3):
        logits.copy_(torch.from_numpy(rounds[r][0]))
        target.copy_(torch.from_numpy(rounds[r][1]))
        image.copy_(torch.from_numpy(rounds[r][2]))
        graph.replay()
        step(ref, x_ref, ws_ref)
        torch.cuda.synchronize()
        for a, b in zip(own.cpu(), ref.cpu()):
            assert np.array_equal(a, b), r
        assert own.cpu().count.tolist() == [r + 1, r + 1]
        assert torch.equal(x_own.view(torch.int32), x_ref.view(torch.int32)), r
        assert torch.equal(g.geodesic_info(ws_own, B, dims), g.geodesic_info(ws_ref, B, dims))
        assert x_own[:, 1:].max() == 1 and not x_own[:, 0].any()


# =============================================================================================
# end to end
# =============================================================================================
def test_geodesic_model_end_to_end():
    from mivp_amd import clicks, strokes, train
    from mivp_amd.swin_unetr import SwinUnetR
    g = G()
    conf, size, batch = train.make_conf("tiny")
    conf.input_channels = 3
    torch.manual_seed(0)
    model = SwinUnetR(conf).to(DEV).train()
    image = torch.rand((batch, 1, size, size, size), generator=torch.Generator().manual_seed(5)).to(DEV)
    target = torch.zeros((batch, 1, size, size, size))
    target[0, 0, 8:20, 6:18, 10:22] = 1
    target[1, 0, 14:28, 12:24, 4:16] = 1
    target = target.to(DEV)
    dims = (size, size, size)
    st, ck = strokes.StrokeSlot(batch, dims), clicks.ClickSlot(batch, max_clicks=4)
    guided = g.GeodesicModel(model, strokes=st, clicks=ck, gamma=10.0, max_iter=8, sigma=4.0)
    zero = torch.zeros_like(image)
    with torch.no_grad():
        got = guided(image)["downstream"]
        want = model(torch.cat([image, zero, zero], dim=1))["downstream"]
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))      # empty slots: the bare model
    assert guided.info.tolist() == [0, 1]
    logits = g.geodesic_rounds(guided, image, target, rounds=2, scribble_kwargs=dict(max_iter=16))
    assert logits.shape == got.shape
    assert (ck.cpu().count >= 1).all() and st.cpu().mask.max() <= 3      # (an untrained model misses the object or floods it)
    x = guided.model_input(image)
    h, w, d, ch = ck.cpu().clicks[0, 0].tolist()
    assert x.shape[1] == 3 and x[0, 1 + ch, h, w, d] == 1 and torch.equal(x[:, :1], image)
    with torch.no_grad():
        assert not torch.equal(guided(image)["downstream"], want)  # the prompts now reach the model
    opt = train.build_optimizer(guided, conf)
    loss = train.train_step(guided, opt, conf, image, target)
    assert bool(torch.isfinite(loss))
    before = ck.cpu().count.copy()
    assert g.geodesic_rounds(guided, image, None, rounds=1).shape == got.shape     # target=None: the caller's prompts only
    assert np.array_equal(ck.cpu().count, before)


def test_geodesic_rounds_on_a_stub_model():
    from mivp_amd import clicks
    g = G()

    class Stub(torch.nn.Module):
        """logits = (-x, x) of the positive guidance channel: the object is predicted where the guidance is above zero"""

        def __init__(self):
            super().__init__()
            self.conf = Namespace(input_channels=3)

        def forward(self, x):
            return torch.stack([0.5 - x[:, 1], x[:, 1]], dim=1)

    dims, B = R.SHAPES[1], 2
    img = np.zeros((B, 1, *dims), dtype=np.float32)
    img[0, 0, 3:11, 4:12, 2:9] = 1
    img[1, 0, 6:15, 1:8, 4:12] = 1
    image = torch.from_numpy(img).to(DEV)
    target = (image[:, 0] > 0.5).to(torch.int64)                   # the bright block
    ck = clicks.ClickSlot(B, max_clicks=4, dims=dims)
    guided = g.GeodesicModel(Stub(), clicks=ck, gamma=1000.0, max_iter=None, kind="disk", radius=30.0)
    logits = g.geodesic_rounds(guided, image, target, rounds=2)
    rec = ck.cpu()
    assert rec.count.tolist() == [1, 1] and (rec.clicks[:, 0, 3] == 0).all()       # one positive click, then nothing is wrong:
    pred = logits.argmax(dim=1)
    assert torch.equal(pred, target)                               # the geodesic disk stops at the block's edge
    assert guided.info.tolist()[1] == 1
