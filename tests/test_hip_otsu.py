"""GPU tests of the Otsu foreground thresholds (mivp_amd.scanstats otsu_slot / foreground_mask / foreground="otsu",
SlidingWindowPredictor.predict_scan(foreground=AutoForeground()); csrc/scanstats.hip) against the
Python-integer restatement tests/otsu_ref.py.

Everything is compared in the bits.  The record and the mask are integers.  The restricted window plan is compared with the
unrestricted plan kernel on a histogram counted with ``above=t`` (``t`` read back in the test only): the same integer sums
enter the same float64 operations, so the words are equal, not merely close."""
import functools

import numpy as np
import pytest
import torch

import otsu_ref as O
import scanstats_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ODD, TINY, U8 = (1, 37, 29, 23), (1, 1, 1, 5), (2, 20, 17, 9)     # 37 x 29 x 23 = 24679 voxels: no multiple of 8 or 16


def _S():
    from mivp_amd import scanstats
    return scanstats


# ------------------------------------------------------------------------------------------------ scans (built once)
@functools.lru_cache(maxsize=None)
def _scan(kind):
    """name -> a read-only numpy scan [C, H, W, D]."""
    rs = np.random.RandomState({"ct": 1, "mr": 2, "tiny": 3, "u8": 4, "const": 5, "mr2": 6}[kind])
    if kind == "ct":                                              # padding, air, soft tissue, bone
        n = int(np.prod(ODD))
        u = rs.rand(n)
        body = np.where(u < 0.93, rs.randint(-120, 140, size=n), rs.randint(300, 1600, size=n))
        v = np.where(u < 0.15, -1024, np.where(u < 0.55, rs.randint(-1010, -980, size=n), body))
        a = v.astype(np.int16).reshape(ODD)
    elif kind in ("mr", "mr2"):                                   # zeros, a dark gamma rim, a bright mode
        n = int(np.prod(ODD))
        u = rs.rand(n)
        rim, mode = (9.0, 700) if kind == "mr" else (30.0, 1100)
        v = np.where(u < 0.35, 0, np.where(u < 0.6, 1 + rs.gamma(2.0, rim, size=n).astype(np.int64),
                                           rs.normal(mode, 90, size=n).astype(np.int64)))
        a = np.clip(v, 0, 4000).astype(np.int16).reshape(ODD)
    elif kind == "tiny":
        a = np.array([3, -7, 3, 250, 249], dtype=np.int16).reshape(TINY)
    elif kind == "u8":                                            # two channels with different thresholds
        n = int(np.prod(U8[1:]))
        c0 = np.where(rs.rand(n) < 0.5, rs.randint(0, 20, size=n), rs.randint(90, 200, size=n))
        c1 = np.where(rs.rand(n) < 0.3, rs.randint(30, 60, size=n), rs.randint(200, 256, size=n))
        a = np.stack([c0, c1]).astype(np.uint8).reshape(U8)
    else:
        a = np.full(ODD, 41, dtype=np.int16)
    a.setflags(write=False)
    return a


CASES = [("ct", None), ("mr", None), ("mr", 0), ("tiny", None), ("u8", None), ("const", None), ("ct", 32767)]
IDS = [f"{k}-above{a}" for k, a in CASES]


@functools.lru_cache(maxsize=None)
def _want(kind, above):
    """(table, record) of the restatement, computed once per case."""
    table = R.histogram(_scan(kind), None, above)
    return table, O.otsu_record(table)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                   # (a copy: the cached scans are read-only)


def _hist_of(table):
    """A ScanHistogram holding ``table``: pooled histograms are plain tensors."""
    S = _S()
    h = S.ScanHistogram(table.shape[0], DEV)
    h.table.copy_(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)))
    return h


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the record
@pytest.mark.parametrize("kind,above", CASES, ids=IDS)
def test_record_equals_the_restatement(kind, above):
    S = _S()
    table, want = _want(kind, above)
    hist = S.scan_histogram(_dev(_scan(kind)), above=above)
    slot = S.otsu_slot(hist)
    got = slot.cpu()
    print(f"[otsu] {kind} above={above}: record {got.tolist()}")
    assert got.dtype == np.int64 and got.shape == (table.shape[0], 4)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(got[:, 1] + got[:, 2], table.sum(axis=1))
    if kind == "const" or above == 32767:                         # a constant scan, an empty selection: no threshold
        assert got[:, 3].tolist() == [0] and got[0, 0] == (41 if kind == "const" else 0)
    else:
        assert got[:, 3].all()
    if (kind, above) == ("mr", 0):                                # Otsu acts on what was counted: the zeros are not
        assert got[0, 0] > 0 and got[0, 1] < _want("mr", None)[1][0, 1] and got[0, 2] == _want("mr", None)[1][0, 2]
    # two equal calls give equal bits; out= is written in place
    again = S.otsu_slot(hist, out=S.OtsuSlot(table.shape[0], DEV))
    assert torch.equal(again.words, slot.words)
    assert S.otsu_slot(hist, out=slot) is slot and np.array_equal(slot.cpu(), want)


def test_record_of_tables_written_straight_into_the_histogram():
    S = _S()
    gap = {v: 5 for v in range(10, 14)}
    gap.update({v: 5 for v in range(200, 204)})
    rows = {"tie": O.table_of({0: 7, 1: 7, 2: 7}), "gap": O.table_of(gap), "big": O.big_table(),
            "ends": O.table_of({-32768: 3, -32767: 1, 32766: 2, 32767: 5}), "empty": O.table_of({}),
            "too many": O.table_of({0: 2 ** 32, 5: 2 ** 32})}
    names = sorted(rows)
    for i in range(0, len(names), 4):                             # four channels a launch
        table = np.stack([rows[n] for n in names[i:i + 4]])
        got = S.otsu_slot(_hist_of(table)).cpu()
        for n, g, row in zip(names[i:i + 4], got, table):
            want, bits = O.otsu(row)
            print(f"[otsu] table {n}: record {g.tolist()}, compared products up to {bits} bits")
            assert tuple(int(x) for x in g) == want, (n, g, want)
    assert O.otsu(rows["tie"])[0] == (0, 7, 14, 1) and O.otsu(rows["gap"])[0] == (13, 20, 20, 1)
    assert O.otsu(rows["big"])[1] > 192                           # the 256-bit path decides this one
    assert O.otsu(rows["too many"])[0][3] == 0 == O.otsu(rows["empty"])[0][3]


def test_record_of_a_histogram_pooled_from_two_scans():
    S = _S()
    a, b = _scan("mr"), _scan("mr2")
    pooled = S.scan_histogram(_dev(a), above=0)
    S.scan_histogram(_dev(b), above=0, out=pooled)
    table = R.histogram(a, None, 0) + R.histogram(b, None, 0)
    want = O.otsu_record(table)
    got = S.otsu_slot(pooled).cpu()
    assert np.array_equal(got, want)
    assert not np.array_equal(want[:, :1], _want("mr", 0)[1][:, :1])                 # the pool moved the threshold


# ------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("kind,above", CASES, ids=IDS)
def test_mask_equals_the_comparison(kind, above):
    S = _S()
    raw_np = _scan(kind)
    _, want = _want(kind, above)
    raw = _dev(raw_np)
    slot = S.otsu_slot(S.scan_histogram(raw, above=above))
    for c in range(raw_np.shape[0]):
        got = S.foreground_mask(raw, slot, channel=c)
        assert got.dtype == torch.uint8 and tuple(got.shape) == raw_np.shape[1:]
        ref = O.mask(raw_np[c], want[c])
        assert np.array_equal(got.cpu().numpy(), ref), (kind, c)
        if want[c, 3]:
            assert int(ref.sum()) == int((raw_np[c].astype(np.int64) > want[c, 0]).sum()) and 0 < ref.sum() < ref.size
        else:
            assert ref.all()                                      # no threshold: everything is foreground
        out = torch.full(raw_np.shape[1:], 7, dtype=torch.uint8, device=DEV)
        assert S.foreground_mask(raw, slot, channel=c, out=out) is out and torch.equal(out, got)
    if raw_np.shape[0] == 2:
        assert want[0, 0] != want[1, 0]                           # each channel has its own threshold


@pytest.mark.parametrize("kind", ["ct", "u8"])
def test_mask_of_unaligned_views(kind):
    """The scan starts 1..3 elements into its allocation, and so does ``out``: heads, tails and the byte-store path."""
    S = _S()
    raw_np = _scan(kind)
    _, want = _want(kind, None)
    flat = raw_np.reshape(-1)
    for off in (1, 2, 3):
        store = torch.from_numpy(np.concatenate([np.full(off, 99, dtype=flat.dtype), flat])).to(DEV)
        raw = store[off:].view(raw_np.shape)
        assert raw.is_contiguous() and raw.data_ptr() % 16 != 0
        slot = S.otsu_slot(S.scan_histogram(raw))
        assert np.array_equal(slot.cpu(), want)
        obuf = torch.full((off + flat.size // raw_np.shape[0] + 5,), 7, dtype=torch.uint8, device=DEV)
        out = obuf[off:off + flat.size // raw_np.shape[0]].view(raw_np.shape[1:])
        c = raw_np.shape[0] - 1
        S.foreground_mask(raw, slot, channel=c, out=out)
        assert np.array_equal(out.cpu().numpy(), O.mask(raw_np[c], want[c])), off
        assert (obuf[:off] == 7).all() and (obuf[off + out.numel():] == 7).all()       # nothing written outside


# ------------------------------------------------------------------------------------------------ the restricted plan
def _specs(S, above):
    W = S.IntensityWindow
    return [W.percentile(0.005, 0.995, above=above), W.percentile(0.0, 1.0, -1.0, 2.0, above=above), W.zscore(above=above),
            W.zscore(above=above, clip=(0.01, 0.99))]


@pytest.mark.parametrize("kind,above", CASES, ids=IDS)
def test_restricted_plan_equals_the_plan_of_a_histogram_above_the_threshold(kind, above):
    S = _S()
    raw_np = _scan(kind)
    raw = _dev(raw_np)
    hist = S.scan_histogram(raw, above=above)
    slot = S.otsu_slot(hist)
    rec = slot.cpu()                                              # read back in the test only
    for spec in _specs(S, above):
        got = S.window_slot_above(hist, spec, slot).cpu()
        plain = S.window_slot(hist, spec).cpu()
        for c in range(raw_np.shape[0]):
            if rec[c, 3]:
                assert above is None or rec[c, 0] >= above
                want = S.window_slot(S.scan_histogram(raw, above=int(rec[c, 0])), spec).cpu()[c]
                assert not np.array_equal(_bits(want), _bits(plain[c])), (spec, c)
                # and the restatement over the values themselves agrees on the order statistics
                v = O.restricted_values(raw_np[c], above)
                assert (got[c, 4], got[c, 5]) == (R.order_statistic(v, spec.q_lo), R.order_statistic(v, spec.q_hi))
            else:
                want = plain[c]                                   # no threshold: the unrestricted plan
            assert np.array_equal(_bits(got[c]), _bits(want)), (spec, c, got[c], want)
    out = S.WindowSlot(raw_np.shape[0], DEV)
    assert S.window_slot_above(hist, spec, slot, out=out) is out and np.array_equal(_bits(out.cpu()), _bits(got))


# ------------------------------------------------------------------------------------------------ prepare_scan
NATIVE = ODD[1:]


def _geom(resized=True):
    from mivp_amd.scan import ScanGeometry
    return ScanGeometry(NATIVE, (1, 2, 0), (True, False, True), out_size=(20, 26, 15) if resized else None)


@pytest.mark.parametrize("kind,above", [("ct", None), ("mr", 0), ("const", None)], ids=["ct", "mr-above0", "const"])
def test_prepare_scan_with_an_otsu_window_equals_the_two_step_form(kind, above, monkeypatch):
    from mivp_amd import _lib, scan
    S = _S()
    geom = _geom()
    raw = _dev(_scan(kind))
    rec = _want(kind, above)[1]
    calls = []
    plain = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), plain(name, *a))[1])
    for mk in (lambda **kw: S.IntensityWindow.zscore(**kw), lambda **kw: S.IntensityWindow.zscore(clip=(0.01, 0.99), **kw),
               lambda **kw: S.IntensityWindow.percentile(0.02, 0.98, **kw)):
        del calls[:]
        got = scan.prepare_scan(raw, geom, window=mk(above=above, foreground="otsu"))
        assert calls == ["mivp_scan_hist", "mivp_scan_otsu_plan", "mivp_scan_window_plan_above", "mivp_scan_prepare_dev"]
        t_host = int(rec[0, 0]) if rec[0, 3] else above
        want = scan.prepare_scan(raw, geom, window=S.window_slot(S.scan_histogram(raw, above=t_host), mk(above=t_host)))
        assert torch.equal(got, want)
        del calls[:]
        unrestricted = scan.prepare_scan(raw, geom, window=mk(above=above))
        assert calls == ["mivp_scan_hist", "mivp_scan_window_plan", "mivp_scan_prepare_dev"]      # no keyword: as before
        assert torch.equal(got, unrestricted) == (not rec[0, 3])


def test_the_four_launch_chain_records_and_replays():
    from mivp_amd import scan
    S = _S()
    geom = _geom()
    scans = [_dev(_scan("mr")), _dev(_scan("mr2"))]
    mk = lambda: S.IntensityWindow.zscore(above=0, foreground="otsu")   # noqa: E731
    eager = [scan.prepare_scan(r, geom, window=mk()).clone() for r in scans]
    assert not torch.equal(eager[0], eager[1])
    spec = mk()
    fixed = scans[0].clone()
    out = torch.empty((1, 1) + geom.size, dtype=torch.float32, device=DEV)
    scan.prepare_scan(fixed, geom, window=spec, out=out)          # eager warm-up: buffers and tables exist now
    rec = spec.buffers(1, fixed.device)[2]

    def record(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g, torch.cuda.memory_allocated() - before

    # (a process's first capture allocates torch's own generator state: take that out with a capture of one in-place op)
    idle, first = record(lambda: out.zero_())
    graph, used = record(lambda: scan.prepare_scan(fixed, geom, window=spec, out=out))
    print(f"[otsu graph] bytes allocated by a first capture {first}, by the recording of the chain {used}")
    assert used == 0                                              # the recording allocated nothing
    thresholds = []
    for i in (0, 1, 0):
        fixed.copy_(scans[i])
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), i
        thresholds.append(int(rec.cpu()[0, 0]))
    assert thresholds[0] != thresholds[1] and thresholds[0] == thresholds[2]
    assert thresholds[:2] == [int(_want("mr", 0)[1][0, 0]), int(O.otsu_record(R.histogram(_scan("mr2"), None, 0))[0, 0])]


# ------------------------------------------------------------------------------------------------ the predictor
IMAGE, ROI = (30, 26, 21), (12, 12, 8)                            # the sizes of tests/test_hip_predict_fit.py: 80 windows
PERM, FLIP = (2, 0, 1), (False, True, False)


class StandIn(torch.nn.Module):
    """A deterministic per-window model: element-wise functions of the input (no reduction, so a window's logits do not
    depend on the batch it runs in), returned as a channels-first view of channels-last fp32 storage."""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1), requires_grad=False)

    def forward(self, x):
        x0 = x[:, 0]
        ch = [torch.tanh(x0 * k + b) + 0.25 * torch.sin(x0 * (3.0 + c)) for c, (k, b) in
              enumerate(((1.7, 0.3), (-2.3, 0.9), (3.1, -1.4)))]
        return {"downstream": torch.stack(ch, dim=-1).permute(0, 4, 1, 2, 3)}


@functools.lru_cache(maxsize=None)
def _body():
    """An int16 MR-like scan on its native grid: a bright body box (600..900) in a corner of noisy air (0..50), with one
    speckle of 300 in every 6 x 6 x 4 cell of the air.  A speckle lies above the scan's mean, so after a z-score it passes
    the fixed ``> 0.0025`` rule in every window; it lies below the Otsu threshold, which separates the body."""
    from mivp_amd.scan import ScanGeometry
    geom = ScanGeometry(tuple(IMAGE[PERM.index(a)] for a in range(3)), PERM, FLIP)
    assert geom.size == IMAGE
    rs = np.random.RandomState(7)
    n = geom.shape
    a = rs.randint(0, 51, size=n)
    a[2::6, 2::6, 1::4] = 300
    a[0, 0, 0] = a[-1, -1, -1] = 300                               # the fixed rule's bounding box is the whole volume
    lo, hi = [1, 1, 1], [s // 3 for s in n]
    a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rs.randint(600, 901, size=[h - l for l, h in zip(lo, hi)])
    a = a.astype(np.int16)[None]
    a.setflags(write=False)
    return a, geom


@pytest.mark.parametrize("rule", ["fit", "skip"])
def test_predict_scan_with_auto_foreground_equals_the_region_set_by_hand(rule):
    from mivp_amd import scan
    from mivp_amd.inference import AutoForeground, SlidingWindowPredictor, WindowFit, WindowSkip
    S = _S()
    raw_np, geom = _body()
    raw = _dev(raw_np)
    kw = {rule: WindowFit() if rule == "fit" else WindowSkip()}
    spec = S.IntensityWindow.zscore()
    model = StandIn().to(DEV).eval()
    p = SlidingWindowPredictor(model, IMAGE, 1, 3, ROI, overlap=0.5, sub_batch=7, **kw)
    # the parent's fixed rule on the z-scored volume keeps every window
    fixed = p.predict_scan(raw, geom, window=spec)
    assert p.n_kept == p.n_windows == 80
    # by hand: the public pieces, then set_region
    rec = S.otsu_slot(S.scan_histogram(raw))
    region = scan.prepare_labels(S.foreground_mask(raw, rec, 0), geom)[0, 0]
    t = int(rec.cpu()[0, 0])
    assert 300 <= t < 600 and t == int(O.otsu_record(R.histogram(raw_np))[0, 0])
    p.set_region(region)
    want = p.predict_scan(raw, geom, window=spec, restore="logits")
    want_l = p.predict_scan(raw, geom, window=spec)
    kept = p.n_kept
    p.set_region(None)
    assert 0 < kept < p.n_windows                                 # the Otsu region keeps fewer: the case is not vacuous
    got = p.predict_scan(raw, geom, window=spec, restore="logits", foreground=AutoForeground())
    assert p.n_kept == kept and p.region is None
    got_l = p.predict_scan(raw, geom, window=spec, foreground=AutoForeground())
    for k in ("labels", "labels_oriented"):
        assert torch.equal(got[k], want[k]) and torch.equal(got_l[k], want_l[k]), k
    assert fixed["labels"].shape == got_l["labels"].shape == raw_np.shape[1:]
    print(f"[otsu predict] {rule}: threshold {t}, windows kept {kept} of {p.n_windows} (fixed rule: all)")
    # the metrics entry and the one-shot wrapper take the same keyword
    seg = _dev((raw_np[0] > t).astype(np.uint8))
    p.set_region(region)
    score = p.evaluate_scan(raw, seg, geom, window=spec)
    p.set_region(None)
    fg = AutoForeground()
    assert p.evaluate_scan(raw, seg, geom, window=spec, foreground=fg) == score
    # graph mode: the region is the predictor's own buffer, the result the eager one
    gp = SlidingWindowPredictor(model, IMAGE, 1, 3, ROI, overlap=0.5, sub_batch=7, graph=True, **kw)
    for _ in range(2):
        b = gp.predict_scan(raw, geom, window=spec, foreground=fg)
        torch.cuda.synchronize()
        assert torch.equal(b["labels"], want_l["labels"]) and gp.n_kept == kept
    assert torch.equal(gp._auto_mask[0, 0], region) and gp.region is None
