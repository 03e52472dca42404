"""GPU tests of the scan statistics and data-driven windows (mivp_amd.scanstats, csrc/scanstats.hip, the device-map
entry of csrc/scan.hip) against tests/scanstats_ref.py.

Everything integer is compared bitwise: the histogram, the order statistics, and every prepared volume.  So are the float
words of a plan.  ``mean``, ``std`` and the z-score ``s``, ``t`` pass through one float64 divide, multiply, subtract and
square root; were each only within 1 ulp of float64, their fp32 rounding could move by one step at a rounding boundary
(the derived bound: 1 fp32 ulp).  The float64 divide and square root of the gfx950 compiler are correctly rounded (every
case here came out 0 ulp from numpy's), so the comparison is bitwise, up to the sign of a zero; the distance is printed."""
import numpy as np
import pytest
import torch

import scanstats_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 13, 10, 9), (2, 8, 8, 1), (1, 40, 36, 33), (2, 5, 3, 7)]
DTYPES = {"int16": torch.int16, "uint8": torch.uint8}
VALUES = ("consecutive", "full", "constant", "saturated", "straddle")
# the LDS window is [base, base + 16384): int16 defaults to -4096; for uint8 the base is given so that the values fall
# on both sides of it ("straddle") or all outside it ("full")
INT16_BASE = -4096
UINT8_BASE = {"consecutive": None, "full": 16384, "constant": None, "saturated": None, "straddle": 128}


def _values(kind, dt, shape, seed):
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if dt == "int16":
        if kind == "consecutive":
            v = rs.randint(-1000, 3000, size=n)
        elif kind == "full":
            v = rs.randint(-32768, 32768, size=n)
            v[rs.permutation(n)[:2]] = (-32768, 32767)
        elif kind == "constant":
            v = np.full(n, 41)
        elif kind == "saturated":
            v = np.where(rs.rand(n) < 0.95, -1024, rs.randint(-1000, 2000, size=n))
        else:
            lo, hi = INT16_BASE, INT16_BASE + 16384
            v = np.where(rs.rand(n) < 0.5, rs.randint(lo - 6, lo + 6, size=n), rs.randint(hi - 6, hi + 6, size=n))
            v[rs.permutation(n)[:4]] = (lo - 1, lo, hi - 1, hi)
        return v.astype(np.int16).reshape(shape)
    if kind == "constant":
        v = np.full(n, 41)
    elif kind == "saturated":
        v = np.where(rs.rand(n) < 0.95, 0, rs.randint(0, 256, size=n))
    elif kind == "straddle":
        v = rs.randint(120, 136, size=n)
        v[rs.permutation(n)[:2]] = (127, 128)
    else:
        v = rs.randint(0, 256, size=n)
        v[rs.permutation(n)[:2]] = (0, 255)
    return v.astype(np.uint8).reshape(shape)


def _mask(shape, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 4, size=shape[1:]) * (rs.rand(*shape[1:]) < 0.7)).astype(np.uint8)       # a label map


def _S():
    from mivp_amd import scanstats
    return scanstats


def _hist(raw, mask=None, above=None, **kw):
    S = _S()
    h = S.scan_histogram(torch.from_numpy(raw).to(DEV), mask=None if mask is None else torch.from_numpy(mask).to(DEV),
                         above=above, **kw)
    return h


# ------------------------------------------------------------------------------------------------ histogram
@pytest.mark.parametrize("kind", VALUES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_histogram_is_exact(shape, dt, kind):
    S = _S()
    raw = _values(kind, dt, shape, seed=5)
    mask = _mask(shape, seed=6)
    base = UINT8_BASE[kind] if dt == "uint8" else None
    for m, above in ((None, None), (None, 0), (mask, None), (mask, 0)):
        want = R.histogram(raw, m, above)
        got = _hist(raw, m, above, base=base)
        assert got.table.shape == (shape[0], 65536) and got.table.dtype == torch.int64
        assert np.array_equal(got.table.cpu().numpy(), want), (m is not None, above)
        per_value = _hist(raw, m, above, base=base, flags=S.FLAG_PER_VALUE)
        assert torch.equal(per_value.table, got.table)
    if kind == "full" and dt == "int16":
        t = R.histogram(raw)
        assert t[:, 0].sum() >= 1 and t[:, 65535].sum() >= 1                     # -32768 and 32767 are present
    # any window base gives the same table
    for b in (-32768, 0, 20000, 32767):
        assert np.array_equal(_hist(raw, mask, None, base=b).table.cpu().numpy(), R.histogram(raw, mask, None))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_histogram_of_an_unaligned_scan_and_mask(dt):
    """A scan that starts 1..3 elements into its allocation: the planes begin off a 16-byte boundary, and so does the mask."""
    shape = (2, 7, 5, 11)
    n = int(np.prod(shape))
    for off in (1, 2, 3):
        flat = np.concatenate([np.full(off, 99), _values("saturated", dt, (n,), seed=7 + off)]).astype(
            np.int16 if dt == "int16" else np.uint8)
        mflat = np.concatenate([np.full(off, 1), _mask((1, n), seed=8).reshape(-1)]).astype(np.uint8)[:off + n // 2]
        raw = torch.from_numpy(flat).to(DEV)[off:].view(shape)
        mask = torch.from_numpy(mflat).to(DEV)[off:].view(shape[1:])
        assert raw.is_contiguous() and raw.data_ptr() % 16 != 0
        got = _S().scan_histogram(raw, mask=mask, above=-2000)
        want = R.histogram(flat[off:].reshape(shape), mflat[off:].reshape(shape[1:]), -2000)
        assert np.array_equal(got.table.cpu().numpy(), want)


def test_empty_selection_pooling_and_report():
    S = _S()
    shape = (1, 40, 36, 33)
    a, b = _values("consecutive", "int16", shape, seed=9), _values("saturated", "int16", shape, seed=10)
    none = _hist(a, np.zeros(shape[1:], dtype=np.uint8))
    assert int(none.table.abs().sum()) == 0                                       # a mask that selects nothing
    assert int(_hist(a, above=32767).table.sum()) == 0
    pooled = _hist(a)
    assert _S().scan_histogram(torch.from_numpy(b).to(DEV), out=pooled) is pooled
    assert np.array_equal(pooled.table.cpu().numpy(), R.histogram(a) + R.histogram(b))
    rep = pooled.cpu()
    both = np.concatenate([a.reshape(-1), b.reshape(-1)])
    n, _, _, mean, std = R.moments(both)
    assert rep.count.tolist() == [n] and (rep.min[0], rep.max[0]) == (both.min(), both.max())
    assert (rep.mean[0], rep.std[0]) == (mean, std) and rep.percentile(0.995)[0] == R.order_statistic(both, 0.995)
    assert int(pooled.zero_().table.sum()) == 0
    with pytest.raises(ValueError):
        S.scan_histogram(torch.from_numpy(a).to(DEV), out=S.ScanHistogram(2, DEV))


# ------------------------------------------------------------------------------------------------ plan
QS = [(0.005, 0.995), (0.0, 1.0), (0.5, 0.5)]


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _two_channels(spatial=(17, 12, 9), seed=11):
    """int16 [2, H, W, D]: a CT-like channel (half air) and an MR-like one (background exactly 0)."""
    rs = np.random.RandomState(seed)
    shape = (2,) + tuple(spatial)
    n = int(np.prod(spatial))
    ct = np.where(rs.rand(n) < 0.5, -1024, rs.randint(-200, 1500, size=n))
    mr = np.where(rs.rand(n) < 0.4, 0, rs.randint(30, 4000, size=n))
    return np.stack([ct, mr]).astype(np.int16).reshape(shape)


def test_percentile_plan_words_are_bitwise():
    S = _S()
    raw = _two_channels()
    for above in (None, 0):
        hist = _hist(raw, above=above)
        for q_lo, q_hi in QS:
            for b_min, b_max in ((0.0, 1.0), (-1.0, 2.0), (0.1, 0.7)):         # b_min != 0: t is a product and a difference
                spec = S.IntensityWindow.percentile(q_lo, q_hi, b_min, b_max, above=above)
                got = S.window_slot(hist, spec).cpu()
                assert got.shape == (2, 8) and got.dtype == np.float32
                for c in range(2):
                    want = R.percentile_plan(R.selected(raw[c], None, above), q_lo, q_hi, b_min, b_max)
                    assert np.array_equal(_bits(got[c, :6]), _bits(want[:6])), (above, q_lo, q_hi, b_min, c, got[c], want)
                    for k in (6, 7):                                             # mean, std
                        assert R.ulp_distance(got[c, k], np.float32(want[k])) == 0, (k, got[c, k], want[k])
    assert not np.array_equal(got[0], got[1])                                     # each channel has its own window


def test_degenerate_plans():
    S = _S()
    const = np.full((1, 6, 5, 4), -7, dtype=np.int16)
    cases = [("constant", _hist(const), const.reshape(-1).astype(np.int64)),
             ("one voxel", _hist(const, above=-8, mask=np.eye(1, 120, 5, dtype=np.uint8).reshape(6, 5, 4)), np.array([-7])),
             ("empty", _hist(const, above=0), np.zeros(0, dtype=np.int64))]
    for tag, hist, v in cases:
        for q_lo, q_hi in QS:
            got = S.window_slot(hist, S.IntensityWindow.percentile(q_lo, q_hi, 0.25, 1.0)).cpu()[0]
            want = R.percentile_plan(v, q_lo, q_hi, 0.25, 1.0)
            assert np.array_equal(_bits(got), _bits(want)), (tag, got, want)
            assert tuple(got[:4]) == (0.0, 0.25, 0.25, 1.0)
        for clip in (None, (0.005, 0.995)):
            got = S.window_slot(hist, S.IntensityWindow.zscore(clip=clip)).cpu()[0]
            want = R.zscore_plan(v, clip)
            assert np.array_equal(got, want.astype(np.float32)), (tag, clip, got, want)      # (-0.0 == 0.0)
            assert got[0] == 1.0 and got[1] == (7.0 if v.size else 0.0) and got[7] == 0.0


def test_zscore_plan_words():
    S = _S()
    raw = _two_channels(seed=12)
    worst = 0
    for above, clip in ((None, None), (0, None), (None, (0.005, 0.995)), (0, (0.0, 1.0)), (None, (0.5, 0.5))):
        hist = _hist(raw, above=above)
        got = S.window_slot(hist, S.IntensityWindow.zscore(above=above, clip=clip)).cpu()
        for c in range(2):
            want = R.zscore_plan(R.selected(raw[c], None, above), clip)
            assert np.array_equal(_bits(got[c, 4:6]), _bits(want[4:6])), (above, clip, c)     # a_lo, a_hi
            for k in (0, 1, 6, 7):                                                           # s, t, mean, std
                d = R.ulp_distance(got[c, k], np.float32(want[k]))
                worst = max(worst, d)
                assert d == 0, (above, clip, c, k, got[c, k], want[k])
            # lo, hi: the fp32 fma of the slot's own s and t on the order statistics, or -FLT_MAX / FLT_MAX
            if clip is None:
                assert (got[c, 2], got[c, 3]) == (np.float32(-R.FLT_MAX), np.float32(R.FLT_MAX))
            else:
                assert got[c, 2] == R.fma_f32(got[c, 4], got[c, 0], got[c, 1])
                assert got[c, 3] == R.fma_f32(got[c, 5], got[c, 0], got[c, 1])
    print(f"[scanstats plan] z-score words: worst distance from the float64 restatement {worst} fp32 ulp (1 if the divide and the "
          f"square root were merely within 1 ulp)")


# ------------------------------------------------------------------------------------------------ prepare
GEOMS = {
    "identity": ((0, 1, 2), (False, False, False), None),
    "moved": ((2, 0, 1), (False, True, False), None),             # the innermost axis moves: the staged read path
    "resized": ((1, 2, 0), (True, False, True), (20, 26, 15)),    # moved, flipped and a trilinear resize
}
NATIVE = (24, 19, 33)


def _geom(name):
    from mivp_amd.scan import ScanGeometry
    perm, flip, out_size = GEOMS[name]
    return ScanGeometry(NATIVE, perm, flip, out_size=out_size)


def _orient(x, geom):
    """numpy [C, H, W, D] on the native grid -> the oriented grid (no resize)."""
    y = np.transpose(x, (0,) + tuple(1 + p for p in geom.perm))
    for a in range(3):
        if geom.flip[a]:
            y = np.flip(y, axis=1 + a)
    return np.ascontiguousarray(y)


@pytest.mark.parametrize("gname", sorted(GEOMS))
def test_percentile_window_equals_the_fixed_window_of_its_order_statistics(gname, monkeypatch):
    from mivp_amd import _lib, scan
    S = _S()
    geom = _geom(gname)
    raw_np = _two_channels(NATIVE, seed=13)[:1]
    raw = torch.from_numpy(raw_np).to(DEV)
    calls = []
    plain = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), plain(name, *a))[1])
    for q_lo, q_hi, b_min, b_max, above in ((0.005, 0.995, 0.0, 1.0, None), (0.02, 0.9, -1.0, 2.0, 0)):
        v = R.selected(raw_np[0], None, above)
        A, B = R.order_statistic(v, q_lo), R.order_statistic(v, q_hi)
        del calls[:]
        want = scan.prepare_scan(raw, geom, a_min=float(A), a_max=float(B), b_min=b_min, b_max=b_max)
        assert calls == ["mivp_scan_prepare"]                                    # window=None: the call it always was
        del calls[:]
        spec = S.IntensityWindow.percentile(q_lo, q_hi, b_min, b_max, above=above)
        got = scan.prepare_scan(raw, geom, window=spec)
        assert calls == ["mivp_scan_hist", "mivp_scan_window_plan", "mivp_scan_prepare_dev"]
        assert got.shape == (1, 1) + geom.size and got.dtype == torch.float32
        assert torch.equal(got, want)
        if not geom.resized:
            assert float(got.min()) == b_min and float(got.max()) == b_max       # the clip is exercised
        for f in (scan.FLAG_DIRECT, scan.FLAG_STAGED):                            # both read paths, the same bits
            assert torch.equal(scan.prepare_scan(raw, geom, window=spec, flags=f), want)
        # a slot from a pooled histogram, the pool being this one scan
        slot = S.window_slot(S.scan_histogram(raw, above=above), spec)
        del calls[:]
        assert torch.equal(scan.prepare_scan(raw, geom, window=slot), want)
        assert calls == ["mivp_scan_prepare_dev"]
        # clip=False holds for a percentile window as for a fixed one
        assert torch.equal(scan.prepare_scan(raw, geom, window=spec, clip=False),
                           scan.prepare_scan(raw, geom, a_min=float(A), a_max=float(B), b_min=b_min, b_max=b_max, clip=False))


def test_mask_selects_the_voxels_of_the_window():
    from mivp_amd import scan
    S = _S()
    geom = _geom("moved")
    raw_np = _two_channels(NATIVE, seed=14)[:1]
    mask_np = (_mask((1,) + NATIVE, seed=15) * (raw_np[0] > -1024)).astype(np.uint8)     # a label map of the body: no air
    v = R.selected(raw_np[0], mask_np, None)
    A, B = R.order_statistic(v, 0.05), R.order_statistic(v, 0.95)
    assert A > -1024 == R.order_statistic(raw_np[0], 0.05)                                 # the mask moves the window
    raw, mask = torch.from_numpy(raw_np).to(DEV), torch.from_numpy(mask_np).to(DEV)
    got = scan.prepare_scan(raw, geom, window=S.IntensityWindow.percentile(0.05, 0.95), mask=mask)
    assert torch.equal(got, scan.prepare_scan(raw, geom, a_min=float(A), a_max=float(B)))
    assert not torch.equal(got, scan.prepare_scan(raw, geom, window=S.IntensityWindow.percentile(0.05, 0.95)))


@pytest.mark.parametrize("gname", ["identity", "moved"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_two_channels_get_their_own_windows(gname, dt):
    """Per channel the output is fma / clamp in fp32 with that channel's slot words, for both modes, bit for bit."""
    from mivp_amd import scan
    S = _S()
    geom = _geom(gname)
    raw_np = _two_channels(NATIVE, seed=16)
    if dt == "uint8":
        raw_np = np.stack([(raw_np[0] // 16) & 0xFF, (raw_np[1] // 32) & 0x7F]).astype(np.uint8)
    raw = torch.from_numpy(raw_np).to(DEV)
    for spec in (S.IntensityWindow.zscore(), S.IntensityWindow.zscore(above=0, clip=(0.01, 0.99)),
                 S.IntensityWindow.percentile(0.01, 0.99, -1.0, 1.0)):
        got = scan.prepare_scan(raw, geom, window=spec)
        words = spec.buffers(2, raw.device)[1].cpu()                             # the slot this call wrote
        assert not np.array_equal(words[0], words[1])
        x = _orient(raw_np, geom)
        for c in range(2):
            want = R.apply_map(x[c], words[c])
            assert np.array_equal(got[0, c].cpu().numpy().view(np.uint32), want.view(np.uint32)), (spec, c)
        if spec.mode == S.MODE_ZSCORE and not spec.clip:
            y = got[0].double()
            assert float(y.mean(dim=(1, 2, 3)).abs().max()) < 1e-4 and float((y.std(dim=(1, 2, 3), unbiased=False) - 1).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ graph
def test_the_three_launch_chain_records_and_replays():
    from mivp_amd import scan
    S = _S()
    geom = _geom("resized")
    scans = [torch.from_numpy(_two_channels(NATIVE, seed=s)[:1] + np.int16(k)).to(DEV) for s, k in ((17, 0), (18, 300))]
    mask = torch.from_numpy((_mask((1,) + NATIVE, seed=19) > 0).astype(np.uint8)).to(DEV)
    spec = S.IntensityWindow.percentile(0.01, 0.99, above=-1000)
    eager = [scan.prepare_scan(r, geom, window=S.IntensityWindow.percentile(0.01, 0.99, above=-1000), mask=mask).clone()
             for r in scans]
    assert not torch.equal(eager[0], eager[1])
    fixed = scans[0].clone()
    out = torch.empty((1, 1) + geom.size, dtype=torch.float32, device=DEV)
    scan.prepare_scan(fixed, geom, window=spec, mask=mask, out=out)               # eager warm-up: buffers and tables exist now
    slot = spec.buffers(1, fixed.device)[1]

    def record(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g, torch.cuda.memory_allocated() - before

    # (a process's first capture allocates torch's own generator state: take that out with a capture of one in-place op)
    idle, first = record(lambda: out.zero_())
    graph, used = record(lambda: scan.prepare_scan(fixed, geom, window=spec, mask=mask, out=out))
    print(f"[scanstats graph] bytes allocated by a first capture {first}, by the recording of the chain {used}")
    assert used == 0                                                             # the recording allocated nothing
    assert spec.buffers(1, fixed.device)[1] is slot
    words = []
    for i in (0, 1, 0):
        fixed.copy_(scans[i])
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), i
        words.append(slot.cpu().copy())
    assert not np.array_equal(words[0], words[1]) and np.array_equal(words[0], words[2])


# ------------------------------------------------------------------------------------------------ predictor
def _tiny_model(seed=4):
    """The model of tests/test_hip_scan.py, built the same way."""
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, _, _ = train.make_conf("tiny")
    torch.manual_seed(seed)
    model = SwinUnetR(conf)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["extra_heads.downstream.1.bias"] = torch.tensor([0.3, -0.3])
    model.load_state_dict(sd)
    return model.to(DEV).eval()


def test_predict_scan_with_a_window_equals_the_fixed_window():
    from mivp_amd import scan
    from mivp_amd.inference import SlidingWindowPredictor
    S = _S()
    model = _tiny_model()
    shape, roi = (56, 48, 40), (32, 32, 32)
    geom = scan.ScanGeometry.from_affine(shape, np.diag([-0.8, -0.8, 2.5, 1.0]))
    g = torch.Generator().manual_seed(21)
    raw = torch.randint(-1500, 1501, (1,) + shape, generator=g, dtype=torch.int32).to(torch.int16)
    A, B = R.order_statistic(raw.numpy(), 0.005), R.order_statistic(raw.numpy(), 0.995)
    raw = raw.to(DEV)
    spec = S.IntensityWindow.percentile()
    kw = dict(overlap=0.5, mode="gaussian", sub_batch=5)
    e = SlidingWindowPredictor(model, geom.size, 1, 2, roi, **kw)
    want = e.predict_scan(raw, geom, a_min=float(A), a_max=float(B))
    got = e.predict_scan(raw, geom, window=spec)
    assert torch.equal(got["labels"], want["labels"]) and torch.equal(got["labels_oriented"], want["labels_oriented"])
    print(f"[scanstats predict] window {A}..{B}, foreground voxels {int(want['labels'].sum())} of {want['labels'].numel()}")
    # graph mode: the prepare launches write the predictor's resident volume, the recorded prediction reads it
    gp = SlidingWindowPredictor(model, geom.size, 1, 2, roi, graph=True, **kw)
    b = gp.predict_scan(raw, geom, window=spec)
    torch.cuda.synchronize()
    assert torch.equal(b["labels"], want["labels"])
    assert torch.equal(gp.vol, scan.prepare_scan(raw, geom, a_min=float(A), a_max=float(B)))
