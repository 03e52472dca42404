"""GPU tests of scan preparation and native-grid restore (mivp_amd.scan, csrc/scan.hip) against tests/scan_ref.py.

Every case runs over the four input dtypes and over geometries that hit both read paths of the kernels (identity, flips
only, innermost axis moved, innermost moved plus flips), on sizes that are multiples of no tile.  Gathers are compared
bit for bit.  Trilinear results have no tolerance chosen in advance: per case ``e_ref`` is the max-abs difference between
torch's CPU fp32 ``F.interpolate`` and the float64 evaluation of the same formula, and the GPU result must be within
``2 * e_ref`` of the float64 evaluation (both figures are printed)."""
import numpy as np
import pytest
import torch

import scan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

GEOMS = {
    "identity": ((0, 1, 2), (False, False, False)),
    "flips": ((0, 1, 2), (True, False, True)),
    "moved": ((2, 0, 1), (False, False, False)),
    "moved_flips": ((1, 2, 0), (True, True, True)),
    "swap02_flip": ((2, 1, 0), (False, True, True)),
}
DTYPES = {"int16": torch.int16, "uint8": torch.uint8, "int32": torch.int32, "float32": torch.float32}
SHAPES = [(50, 44, 23), (97, 75, 33)]
RESIZE = {(50, 44, 23): (61, 37, 40), (97, 75, 33): (64, 90, 41)}


def _geom(name, shape, out_size=None):
    from mivp_amd.scan import ScanGeometry
    perm, flip = GEOMS[name]
    return ScanGeometry(shape, perm, flip, out_size=out_size)


def _native_shape(name, oriented):
    perm, _ = GEOMS[name]
    shape = [0, 0, 0]
    for a in range(3):
        shape[perm[a]] = oriented[a]
    return tuple(shape)


def _scan(shape, dtype, seed, channels=1):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (channels,) + shape, generator=g, dtype=torch.int32).to(torch.uint8)
    x = torch.randint(-1500, 1501, (channels,) + shape, generator=g, dtype=torch.int32)
    if dtype == torch.float32:
        return x.float() + 0.25 * torch.randint(0, 4, x.shape, generator=g).float()
    return x.to(dtype)


def _mask(shape, dtype, seed, hi=256):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, hi, shape, generator=g, dtype=torch.int32).to(dtype)


def _both_paths(fn):
    """The default, the forced direct and the forced staged read path must give the same bits."""
    from mivp_amd.scan import FLAG_DIRECT, FLAG_STAGED
    a, b, c = fn(0), fn(FLAG_DIRECT), fn(FLAG_STAGED)
    assert torch.equal(a, b) and torch.equal(a, c)
    return a


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("gname", sorted(GEOMS))
def test_prepare_without_resize_is_bit_equal(gname, dt, shape):
    from mivp_amd import scan
    geom = _geom(gname, shape)
    raw = _scan(shape, DTYPES[dt], seed=11, channels=2)
    got = _both_paths(lambda f: scan.prepare_scan(raw.to(DEV), geom, flags=f))
    want, _ = scan_ref.prepare_scan(raw, geom)
    assert got.shape == (1, 2) + geom.size and got.dtype == torch.float32
    assert torch.equal(got[0].cpu(), want)
    if dt == "int16":
        assert float(want.min()) == 0.0 and float(want.max()) == 1.0           # the clip is exercised
        got = scan.prepare_scan(raw.to(DEV), geom, a_min=-200.0, a_max=300.0, b_min=-1.0, b_max=2.0, clip=False)
        want, _ = scan_ref.prepare_scan(raw, geom, a_min=-200.0, a_max=300.0, b_min=-1.0, b_max=2.0, clip=False)
        assert torch.equal(got[0].cpu(), want)


@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("gname", sorted(GEOMS))
def test_label_maps_both_ways_are_bit_equal(gname, dt, shape, resize):
    from mivp_amd import scan
    geom = _geom(gname, shape, RESIZE[shape] if resize else None)
    seg = _mask(shape, DTYPES[dt], seed=12)
    got = _both_paths(lambda f: scan.prepare_labels(seg.to(DEV), geom, flags=f))
    want = scan_ref.prepare_labels(seg, geom)
    assert got.shape == (1, 1) + geom.size and got.dtype == torch.uint8
    assert torch.equal(got[0, 0].cpu(), want)
    back = _both_paths(lambda f: scan.restore_labels(got, geom, flags=f))
    assert back.shape == geom.shape and back.dtype == torch.uint8
    assert torch.equal(back.cpu(), scan_ref.restore_labels(want, geom))
    if not resize:
        assert torch.equal(back.cpu(), seg.to(torch.uint8))
    out = torch.empty(geom.shape, dtype=torch.uint8, device=DEV)
    assert scan.restore_labels(got[0, 0], geom, out=out) is out and torch.equal(out, back)


# ------------------------------------------------------------------------------------------------ trilinear cases
def _check_trilinear(tag, got, fp32_ref, f64_ref):
    e_ref = float((fp32_ref.double() - f64_ref).abs().max())
    e_gpu = float((got.double().cpu() - f64_ref).abs().max())
    print(f"[scan trilinear] {tag}: e_ref {e_ref:.3e}  gpu {e_gpu:.3e}  bound {2 * e_ref:.3e}")
    assert e_gpu <= 2 * e_ref, (tag, e_gpu, e_ref)
    return e_ref


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("gname", sorted(GEOMS))
def test_prepare_with_resize_within_twice_torch_error(gname, dt, shape):
    from mivp_amd import scan
    geom = _geom(gname, shape, RESIZE[shape])
    raw = _scan(shape, DTYPES[dt], seed=13)
    got = _both_paths(lambda f: scan.prepare_scan(raw.to(DEV), geom, flags=f))
    fp32_ref, f64_ref = scan_ref.prepare_scan(raw, geom)
    assert got.shape == (1, 1) + geom.size
    _check_trilinear(f"{gname} {dt} {shape}->{geom.size}", got[0], fp32_ref, f64_ref)


@pytest.mark.parametrize("gname", sorted(GEOMS))
def test_clip_happens_before_the_resize(gname):
    from mivp_amd import scan
    shape = (50, 44, 23)
    geom = _geom(gname, shape, (61, 37, 40))
    g = torch.Generator().manual_seed(14)
    raw = (torch.randint(0, 3, (1,) + shape, generator=g, dtype=torch.int32) - 1) * 3000      # -3000, 0, 3000
    raw = raw.to(torch.int16)
    got = scan.prepare_scan(raw.to(DEV), geom)
    fp32_ref, f64_ref = scan_ref.prepare_scan(raw, geom)
    e_ref = _check_trilinear(f"clip order {gname}", got[0], fp32_ref, f64_ref)
    # the wrong order: interpolate the unclipped map, then clip
    wrong = scan_ref.trilinear_f64(scan_ref.orient(scan_ref.intensity(raw, clip=False), geom.perm, geom.flip),
                                   geom.size).clamp(0.0, 1.0)
    gap = float((wrong - f64_ref).abs().max())
    print(f"[scan clip order] {gname}: interpolate-then-clip differs by {gap:.3e}")
    assert gap > 2 * e_ref


# ------------------------------------------------------------------------------------------------ logits -> native labels
LOGIT_CASES = [(2, (40, 36, 20), (97, 75, 33)), (3, (48, 48, 24), (61, 50, 24)), (4, (33, 47, 19), (20, 31, 40))]


@pytest.mark.parametrize("ncls,model_size,oriented", LOGIT_CASES)
@pytest.mark.parametrize("gname", sorted(GEOMS))
def test_restore_from_logits_equals_float64_argmax(gname, ncls, model_size, oriented):
    from mivp_amd import scan
    geom = _geom(gname, _native_shape(gname, oriented), model_size)
    assert geom.oriented_shape == oriented and geom.size == model_size
    torch.manual_seed(100 + ncls)
    logits = torch.randn((1, ncls) + model_size)
    got = _both_paths(lambda f: scan.restore_labels_from_logits(logits.to(DEV), geom, flags=f))
    assert got.shape == geom.shape and got.dtype == torch.uint8
    ref = scan_ref.trilinear_f64(logits[0], oriented)
    top2 = ref.topk(2, dim=0).values
    kept = scan_ref.unorient((top2[0] - top2[1]) >= 1e-4, geom.perm, geom.flip)
    want = scan_ref.unorient(ref.argmax(0), geom.perm, geom.flip)
    left_out = 1.0 - float(kept.double().mean())
    fp32 = scan_ref.unorient(scan_ref.trilinear_torch(logits[0], oriented).argmax(0), geom.perm, geom.flip)
    print(f"[scan argmax] {gname} C={ncls} {model_size}->{oriented}: left out {100 * left_out:.4f} %, torch fp32 differs "
          f"on {int((fp32 != want)[kept].sum())} kept voxels, gpu on {int((got.cpu().long() != want)[kept].sum())}")
    assert left_out <= 1e-3
    assert torch.equal(got.cpu().long()[kept], want[kept])


@pytest.mark.parametrize("gname", sorted(GEOMS))
@pytest.mark.parametrize("resize", [False, True])
def test_restore_from_logits_tie_goes_to_the_lower_class(gname, resize):
    from mivp_amd import scan
    shape = (50, 44, 23)
    geom = _geom(gname, shape, (37, 29, 31) if resize else None)
    torch.manual_seed(3)
    one = torch.randn((1, 1) + geom.size)
    logits = torch.cat([one - 5.0, one, one], dim=1).to(DEV)                     # classes 1 and 2 tie everywhere
    got = _both_paths(lambda f: scan.restore_labels_from_logits(logits, geom, flags=f))
    assert bool((got == 1).all())
    if not resize:                                                               # a pure gather of the arg-max
        lg = torch.randn((1, 4) + geom.size)
        got = scan.restore_labels_from_logits(lg.to(DEV), geom)
        assert torch.equal(got.cpu().long(), scan_ref.unorient(lg[0].argmax(0), geom.perm, geom.flip))


# ------------------------------------------------------------------------------------------------ overflow flag
@pytest.mark.parametrize("gname", ["identity", "moved_flips"])
@pytest.mark.parametrize("dt", ["int16", "int32", "float32"])
def test_out_of_range_labels_raise(gname, dt):
    from mivp_amd import scan
    shape = (50, 44, 23)
    geom = _geom(gname, shape)
    seg = _mask(shape, DTYPES[dt], seed=15, hi=4)
    seg[17, 5, 22] = 255
    out = scan.prepare_labels(seg.to(DEV), geom)                                 # 255 fits
    assert int(out.max()) == 255
    for bad in (300, -1):
        s = seg.clone()
        s[49, 43, 0] = bad
        with pytest.raises(ValueError, match="0..255"):
            scan.prepare_labels(s.to(DEV), geom)
    if dt == "float32":
        s = seg.clone()
        s[0, 0, 0] = 1.5
        with pytest.raises(ValueError, match="0..255"):
            scan.prepare_labels(s.to(DEV), geom)


# ------------------------------------------------------------------------------------------------ predictor
def _tiny_model(seed=4):
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, _, _ = train.make_conf("tiny")
    torch.manual_seed(seed)
    model = SwinUnetR(conf)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["extra_heads.downstream.1.bias"] = torch.tensor([0.3, -0.3])
    model.load_state_dict(sd)
    return model.to(DEV).eval()


LPS = np.diag([-0.8, -0.8, 2.5, 1.0])


def test_predict_scan_equals_the_three_steps_and_graph_equals_eager():
    from mivp_amd import scan
    from mivp_amd.inference import SlidingWindowPredictor
    model = _tiny_model()
    shape, roi = (56, 48, 40), (32, 32, 32)
    geom = scan.ScanGeometry.from_affine(shape, LPS)
    assert geom.flip == (True, True, False) and np.allclose(geom.spacing, (0.8, 0.8, 2.5))
    raws = [_scan(shape, torch.int16, seed=s).to(DEV) for s in (21, 22)]
    seg = _mask(shape, torch.int16, seed=23, hi=2).to(DEV)
    kw = dict(overlap=0.5, mode="gaussian", sub_batch=5)
    e = SlidingWindowPredictor(model, geom.size, 1, 2, roi, **kw)
    gp = SlidingWindowPredictor(model, geom.size, 1, 2, roi, graph=True, **kw)
    for raw in raws:                                                             # the recorded graph serves a second scan
        a = e.predict_scan(raw, geom)
        x = scan.prepare_scan(raw, geom)
        steps = scan.restore_labels(e.predict(x)["labels"], geom)
        assert a["labels"].shape == shape and a["labels_oriented"].shape == (1, 1) + geom.size
        assert torch.equal(a["labels"], steps)
        a2 = e.predict_scan(raw, geom)
        assert a2["labels"].cpu().numpy().tobytes() == a["labels"].cpu().numpy().tobytes()
        b = gp.predict_scan(raw, geom)
        torch.cuda.synchronize()
        assert torch.equal(a["labels"], b["labels"]) and torch.equal(a["labels_oriented"], b["labels_oriented"])
        assert gp.vol is not None and torch.equal(gp.vol, x)
        # without a resize the arg-max of the restored logits is the restored arg-max
        c = e.predict_scan(raw, geom, restore="logits")
        assert torch.equal(c["labels"], a["labels"])
        d = e.predict_scan(raw, geom, postprocess={"largest": True})
        want = scan.restore_labels(e.predict(x, postprocess={"largest": True})["labels"], geom)
        assert torch.equal(d["labels"], want)
    raw = raws[0]
    got = e.evaluate_scan(raw, seg, geom)
    assert got == e.evaluate(scan.prepare_scan(raw, geom), scan.prepare_labels(seg, geom))
    assert gp.evaluate_scan(raw, seg, geom) == got
    m = e.evaluate_surface(scan.prepare_scan(raw, geom), scan.prepare_labels(seg, geom), spacing=geom.spacing)
    assert m["iou"] == got[0] and m["dice"] == got[1] and m["hd"].shape == (2,)


def test_predict_scan_volume_with_resize_and_moved_axis():
    import mivp_amd
    from mivp_amd import scan
    model = _tiny_model()
    shape = (37, 61, 50)
    aff = scan_ref.affine_for((1, 2, 0), (True, False, True), zooms=(2.0, 0.9, 0.9))
    raw = _scan(shape, torch.int16, seed=31).to(DEV)
    out = mivp_amd.predict_scan_volume(model, raw[0], aff, (32, 32, 32), 2, out_size=(56, 48, 40), sub_batch=4)
    geom = out["geometry"]
    assert geom.perm == (1, 2, 0) and geom.size == (56, 48, 40) and geom.oriented_shape == (61, 50, 37)
    assert out["labels"].shape == shape and out["labels"].dtype == torch.uint8
    assert torch.equal(out["labels"], scan.restore_labels(out["labels_oriented"], geom))
    lg = mivp_amd.predict_scan_volume(model, raw, aff, (32, 32, 32), 2, out_size=(56, 48, 40), sub_batch=4,
                                      restore="logits")
    assert lg["labels"].shape == shape and torch.equal(lg["labels_oriented"], out["labels_oriented"])
    agree = float((lg["labels"] == out["labels"]).double().mean())
    print(f"[scan predict] restore='logits' agrees with restore='labels' on {agree:.4f} of the native voxels")
