"""GPU: interactive click prompts (mivp_amd.clicks, csrc/clicks.hip) against the numpy restatement of tests/clicks_ref.py.

  encode     disk mode bit-equal at unit spacing; gaussian mode against float64 with the project's yardstick (the kernel may
             err 8 x E32, E32 the largest error of the float32 numpy composition of the same formula against float64 on the
             same inputs); an empty channel is +0; anisotropic spacing; write extent under a NaN pattern with guard bands at
             every alignment of the tensor's start.
  simulate   clicks, count and last integer-equal to the restatement on the cases of clicks_ref.simulate_cases() (every one of
             them exact in float32: test_clicks_host.py), the fused arg-max with logit ties, equal calls give equal bits.
  replay     a recording of [simulate -> encode] on new pred / target over three rounds equals the eager calls in the bits.
  end to end the 32^3 configuration with three input channels: GuidedModel with an empty slot is the bare model bit for bit,
             one train_step gives a finite loss, click_rounds leaves two clicks per sample; refine_volume on a small volume."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clicks_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = 0x7FC0BEEF                                               # a NaN no kernel produces
CASES = R.simulate_cases()


def C():
    import mivp_amd  # noqa: F401
    from mivp_amd import clicks
    return clicks


def random_clicks(rng, B, K, dims, counts):
    table = np.full((B, K, 4), -1, dtype=np.int32)
    for b in range(B):
        for i in range(counts[b]):
            table[b, i] = [rng.integers(0, dims[0]), rng.integers(0, dims[1]), rng.integers(0, dims[2]), rng.integers(0, 2)]
    return table


def fill_slot(slot, table, counts):
    for b in range(table.shape[0]):
        slot.set(b, [tuple(int(v) for v in r) for r in table[b, :counts[b]]])


def patterned(B, ctot, dims, lead, guard=7):
    """A [B, ctot, *dims] view at element ``lead`` of a flat buffer filled with PATTERN, and the buffer as int32."""
    n = B * ctot * dims[0] * dims[1] * dims[2]
    flat = torch.full((lead + n + guard,), PATTERN, dtype=torch.int32, device=DEV)
    return flat.view(torch.float32)[lead:lead + n].view(B, ctot, *dims), flat


# =============================================================================================
# encode
# =============================================================================================
@pytest.mark.parametrize("dims,B", [(R.SHAPES[0], 2), (R.SHAPES[1], 3), (R.SHAPES[2], 2)])
def test_encode_disk_is_bit_equal_at_unit_spacing(dims, B):
    rng = np.random.default_rng(1)
    counts = [5, 0, 8][:B]
    table = random_clicks(rng, B, 8, dims, counts)
    slot = C().ClickSlot(B, max_clicks=8)
    fill_slot(slot, table, counts)
    for radius in (0.0, 2.0, 3.5):
        out = torch.full((B, 3, *dims), 7.0, device=DEV)
        C().encode_clicks(slot, out, channel_offset=1, kind="disk", radius=radius)
        want = R.encode_ref(table, counts, dims, kind="disk", radius=radius, dtype=np.float32)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, 1:].view(np.int32), want.view(np.int32))
        assert (got[:, 0] == 7.0).all()
    assert not got[1, 1:].any() and not np.signbit(got[1, 1:]).any()       # sample 1 has no click: exact +0


@pytest.mark.parametrize("dims,B,spacing,sigma", [(R.SHAPES[0], 2, (1, 1, 1), 2.0), (R.SHAPES[1], 3, (1, 0.8, 2.5), 1.5),
                                                  (R.SHAPES[2], 2, (1, 0.8, 2.5), 3.0), (R.SHAPES[2], 2, (1, 1, 1), 0.7)])
def test_encode_gaussian_against_float64(dims, B, spacing, sigma):
    rng = np.random.default_rng(2)
    counts = [6, 3, 0][:B] if B == 3 else [6, 1]
    table = random_clicks(rng, B, 8, dims, counts)
    if B == 2:
        table[1, 0, 3] = 0                                         # sample 1: one positive click, the negative channel empty
    slot = C().ClickSlot(B, max_clicks=8)
    fill_slot(slot, table, counts)
    out = torch.full((B, 4, *dims), 7.0, device=DEV)
    C().encode_clicks(slot, out, channel_offset=2, sigma=sigma, spacing=spacing)
    got = out.cpu().numpy()[:, 2:].astype(np.float64)
    w64 = R.encode_ref(table, counts, dims, spacing, sigma=sigma, dtype=np.float64)
    w32 = R.encode_ref(table, counts, dims, spacing, sigma=sigma, dtype=np.float32).astype(np.float64)
    e32, err = np.abs(w32 - w64).max(), np.abs(got - w64).max()
    print(f"encode gaussian {dims} spacing {spacing} sigma {sigma}: err {err:.3e}, E32 {e32:.3e}, ratio {err / e32:.2f}")
    assert e32 > 0 and err <= 8 * e32
    if B == 2:
        empty = out[1, 3].cpu().numpy()
        assert not empty.any() and not np.signbit(empty).any()
    for b in range(B):                                             # a click's own voxel is exactly 1
        for h, w, d, ch in table[b, :counts[b]]:
            assert out[b, 2 + ch, h, w, d].item() == 1.0
    assert (out[:, :2] == 7.0).all()


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["gaussian", "disk"])
def test_encode_write_extent(lead, kind):
    dims, B, ctot, off = R.SHAPES[0], 2, 4, 1                      # vol = 910: the runs start at every residue of 16 bytes
    rng = np.random.default_rng(3)
    table = random_clicks(rng, B, 8, dims, [4, 0])
    slot = C().ClickSlot(B, max_clicks=8)
    fill_slot(slot, table, [4, 0])
    out, flat = patterned(B, ctot, dims, 8 + lead)
    C().encode_clicks(slot, out, channel_offset=off, kind=kind)
    bits = out.view(torch.int32)
    assert (flat[:8 + lead] == PATTERN).all() and (flat[8 + lead + out.numel():] == PATTERN).all()
    assert (bits[:, 0] == PATTERN).all() and (bits[:, 3] == PATTERN).all()
    assert not (bits[:, 1:3] == PATTERN).any()
    want = R.encode_ref(table, [4, 0], dims, kind=kind, dtype=np.float32)
    assert np.allclose(out[:, 1:3].cpu().numpy(), want, rtol=0, atol=1e-6)


def test_encode_one_voxel_and_thin_volumes():
    for dims in ((1, 1, 1), (1, 1, 5), (3, 1, 2), (2, 2, 3)):
        slot = C().ClickSlot(1, max_clicks=2)
        slot.set(0, [(0, 0, 0, 1)])
        out, flat = patterned(1, 2, dims, 9)
        C().encode_clicks(slot, out, channel_offset=0, kind="disk", radius=1.0)
        want = R.encode_ref(np.array([[(0, 0, 0, 1), (-1, -1, -1, -1)]]), [1], dims, kind="disk", radius=1.0, dtype=np.float32)
        assert np.array_equal(out.cpu().numpy(), want)
        assert (flat[:9] == PATTERN).all() and (flat[9 + out.numel():] == PATTERN).all()


# =============================================================================================
# simulate
# =============================================================================================
def run_case(c, workspace=None):
    K = c["K"]
    slot = C().ClickSlot(2, max_clicks=K)
    table = np.full((2, K, 4), -1, dtype=np.int32)
    count = np.zeros(2, dtype=np.int32)
    for b, rows in enumerate(c["init"]):
        slot.set(b, rows)
        for i, r in enumerate(rows):
            table[b, i] = r
        count[b] = len(rows)
    pred, target = torch.from_numpy(c["pred"]).to(DEV), torch.from_numpy(c["target"]).to(DEV)
    C().simulate_clicks(pred, target, slot, workspace=workspace, **c["kwargs"])
    return slot.cpu(), R.simulate_ref(c["pred"], c["target"], table, count, **c["kwargs"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_simulate_equals_the_restatement(name):
    c = CASES[name]
    ws = C().simulate_clicks_ws(2, c["target"].shape[1:])
    ws.fill_(0xFF)                                                 # stale workspace contents must not matter
    got, (clicks, count, last) = run_case(c, ws)
    assert np.array_equal(got.last, last), (got.last, last)
    assert np.array_equal(got.count, count)
    assert np.array_equal(got.clicks, clicks)
    if isinstance(c["want"], tuple):
        assert tuple(got.clicks[0, len(c["init"][0])]) == c["want"]


def test_simulate_takes_the_five_dimensional_layout_and_bool_maps():
    c = CASES["tie_index"]
    pred = torch.from_numpy(c["pred"] > 0).to(DEV)[:, None]
    target = torch.from_numpy(c["target"] > 0).to(DEV)[:, None]
    slot = C().ClickSlot(2, max_clicks=4)
    C().simulate_clicks(pred, target, slot)
    clicks, count, last = R.simulate_ref((c["pred"] > 0).astype(np.uint8), (c["target"] > 0).astype(np.uint8),
                                         np.full((2, 4, 4), -1), np.zeros(2))
    got = slot.cpu()
    assert np.array_equal(got.clicks, clicks) and np.array_equal(got.count, count) and np.array_equal(got.last, last)


@pytest.mark.parametrize("dims", R.SHAPES)
@pytest.mark.parametrize("layout", ["channels_last", "channels_first"])
def test_simulate_from_logits_is_the_call_on_the_argmax(dims, layout):
    rng = np.random.default_rng(7)
    B, ncls = 2, 3
    z = (rng.integers(-2, 3, size=(B, ncls, *dims)) * 0.5).astype(np.float32)       # many exact ties between the classes
    z[0, :, 2:5, 2:5, 2:5] = 0.0                                   # a block where all three tie: class 0 wins
    target = R.blobs(rng, dims)[None].repeat(B, 0).astype(np.float32)
    target[1] = R.blobs(rng, dims)
    arg = z.argmax(axis=1)                                         # numpy: the first maximum
    assert ((z == z.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.2
    logits = torch.from_numpy(z).to(DEV)
    if layout == "channels_last":
        logits = logits.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    a, b = C().ClickSlot(B, max_clicks=4), C().ClickSlot(B, max_clicks=4)
    C().simulate_clicks_from_logits(logits, torch.from_numpy(target).to(DEV), a)
    C().simulate_clicks(torch.from_numpy(arg).to(DEV), torch.from_numpy(target).to(DEV), b)
    clicks, count, last = R.simulate_ref(arg, target, np.full((B, 4, 4), -1), np.zeros(B))
    for got in (a.cpu(), b.cpu()):
        assert np.array_equal(got.clicks, clicks) and np.array_equal(got.count, count) and np.array_equal(got.last, last)
    assert count.min() == 1


def test_equal_calls_give_equal_bits():
    c = CASES["random2"]
    first, _ = run_case(c)
    second, _ = run_case(c)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    slot = C().ClickSlot(2, max_clicks=4)
    fill_slot(slot, first.clicks, first.count)
    outs = [C().encode_clicks(slot, torch.empty((2, 2, *R.SHAPES[2]), device=DEV), channel_offset=0, spacing=(1, 0.8, 2.5))
            for _ in range(2)]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


# =============================================================================================
# replay
# =============================================================================================
def test_recorded_simulate_and_encode_follow_new_contents():
    dims, B = R.SHAPES[2], 2
    rng = np.random.default_rng(11)
    preds = [R.blobs(rng, dims)[None].repeat(B, 0).astype(np.uint8) for _ in range(3)]
    for p in preds:
        p[1] = R.blobs(rng, dims)
    targets = [np.stack([R.blobs(rng, dims), R.blobs(rng, dims)]).astype(np.float32) for _ in range(2)]
    pred = torch.from_numpy(preds[0]).to(DEV)
    target = torch.from_numpy(targets[0]).to(DEV)
    own, ref = C().ClickSlot(B, max_clicks=4), C().ClickSlot(B, max_clicks=4)
    x_own, x_ref = torch.zeros((B, 3, *dims), device=DEV), torch.zeros((B, 3, *dims), device=DEV)
    ws = C().simulate_clicks_ws(B, dims)

    def step(slot, x):
        C().simulate_clicks(pred, target, slot, workspace=ws)
        C().encode_clicks(slot, x, channel_offset=1, sigma=1.5)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(own, x_own)                                           # warm-up on the slot that is then cleared
    torch.cuda.current_stream().wait_stream(side)
    own.clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(own, x_own)
    own.clear()                                                    # the capture launched nothing: start from an empty slot
    for r in range(3):
        pred.copy_(torch.from_numpy(preds[r]))
        target.copy_(torch.from_numpy(targets[min(r, 1)]))
        graph.replay()
        step(ref, x_ref)
        torch.cuda.synchronize()
        for a, b in zip(own.cpu(), ref.cpu()):
            assert np.array_equal(a, b), r
        assert torch.equal(x_own.view(torch.int32), x_ref.view(torch.int32)), r
    assert own.cpu().count.tolist() == [3, 3]
    table = np.full((B, 4, 4), -1, dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    for r in range(3):
        table, count, last = R.simulate_ref(preds[r], targets[min(r, 1)], table, count)
    got = own.cpu()
    assert np.array_equal(got.clicks, table) and np.array_equal(got.last, last)


# =============================================================================================
# end to end
# =============================================================================================
def guided_setup():
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, size, batch = train.make_conf("tiny")
    conf.input_channels = 3
    torch.manual_seed(0)
    model = SwinUnetR(conf).to(DEV).train()
    g = torch.Generator().manual_seed(5)
    image = torch.rand((batch, 1, size, size, size), generator=g).to(DEV)
    target = torch.zeros((batch, 1, size, size, size))
    target[0, 0, 8:20, 6:18, 10:22] = 1
    target[1, 0, 14:28, 12:24, 4:16] = 1
    return conf, model, image, target.to(DEV), C().ClickSlot(batch, max_clicks=8)


def test_guided_model_end_to_end():
    from mivp_amd import train
    conf, model, image, target, slot = guided_setup()
    guided = C().GuidedModel(model, slot, sigma=2.0)
    with torch.no_grad():
        got = guided(image)["downstream"]
        want = model(torch.cat([image, torch.zeros_like(image), torch.zeros_like(image)], dim=1))["downstream"]
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    logits = C().click_rounds(guided, image, target, slot, rounds=2)
    rec = slot.cpu()
    assert logits.shape == got.shape
    assert rec.count.tolist() == [2, 2] and (rec.last[:, 3] == 1).all()
    placed = rec.clicks[:, :2]
    assert ((placed[..., :3] >= 0) & (placed[..., :3] < 32)).all() and np.isin(placed[..., 3], (0, 1)).all()
    assert (rec.clicks[:, 2:] == -1).all()
    with torch.no_grad():                                          # the clicks now reach the model: another output
        assert not torch.equal(guided(image)["downstream"], want)
    opt = train.build_optimizer(guided, conf)
    loss = train.train_step(guided, opt, conf, image, target)
    assert bool(torch.isfinite(loss))
    assert C().click_rounds(guided, image, None, slot, rounds=1).shape == got.shape      # target=None: the caller's clicks only
    assert slot.cpu().count.tolist() == [2, 2]


class _Stub(torch.nn.Module):
    """A 'downstream' model of one 1 x 1 x 1 convolution: the object is where image + positive - negative guidance > 0.5."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv3d(3, 2, 1)
        with torch.no_grad():
            self.conv.weight.copy_(torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, -1.0]]).view(2, 3, 1, 1, 1))
            self.conv.bias.copy_(torch.tensor([0.5, 0.0]))

    def forward(self, x):
        return {"downstream": self.conv(x)}


def test_refine_volume_moves_towards_the_target():
    from mivp_amd.inference import SlidingWindowPredictor
    dims = (24, 20, 16)
    target = torch.zeros((1, 1, *dims), dtype=torch.uint8, device=DEV)
    target[0, 0, 6:15, 5:14, 4:12] = 1
    image = torch.zeros((1, 1, *dims), device=DEV)
    predictor = SlidingWindowPredictor(_Stub().to(DEV).eval(), dims, 3, 2, (16, 16, 16), sub_batch=2)
    slot = C().ClickSlot(1, max_clicks=4)
    maps = C().refine_volume(predictor, image, target, slot, rounds=2, sigma=3.0)
    assert len(maps) == 3 and all(m.shape == (1, 1, *dims) and m.dtype == torch.uint8 for m in maps)
    wrong = [int((m != target).sum()) for m in maps]
    rec = slot.cpu()
    assert rec.count[0] == 2 and tuple(rec.clicks[0, 0]) == (9, 8, 7, 0)       # the first of the box's deepest voxels (depth 4)
    assert wrong[0] == int(target.sum()) and wrong[1] < wrong[0]
    assert len(C().refine_volume(predictor, image, None, slot, rounds=2)) == 1
