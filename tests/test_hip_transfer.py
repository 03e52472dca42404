"""GPU tests of the intensity transfer tables (mivp_amd.transfer; csrc/scan_transfer.hip) against the
restatement tests/transfer_ref.py.

Everything is compared in the bits.  The tables are float32 words from integer sums through float64 operations the
restatement repeats one by one; the match integers are read through a reference slot that holds the identity map, and the
float stage is compared with the existing ``prepare_scan(window=slot)`` on a volume that holds those integers."""
import functools

import numpy as np
import pytest
import torch

import otsu_ref as O
import scanstats_ref as R
import transfer_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
ODD, TINY, U8, WIDE = (1, 37, 29, 23), (1, 1, 1, 5), (2, 20, 17, 9), (1, 16, 16, 33)
FLT_MAX = float(np.finfo(np.float32).max)
N_Q = len(T.DEFAULT_Q)


def _tr():
    from mivp_amd import transfer
    return transfer


def _S():
    from mivp_amd import scanstats
    return scanstats


# ------------------------------------------------------------------------------------------------ scans (built once)
@functools.lru_cache(maxsize=None)
def _scan(kind):
    """name -> a read-only numpy scan [C, H, W, D] (the scans of tests/test_hip_otsu.py, and WIDE)."""
    rs = np.random.RandomState({"ct": 1, "mr": 2, "tiny": 3, "u8": 4, "const": 5, "mr2": 6, "wide": 7, "mr3": 8, "mr4": 9}[kind])
    if kind == "ct":                                              # padding, air, soft tissue, bone
        n = int(np.prod(ODD))
        u = rs.rand(n)
        body = np.where(u < 0.93, rs.randint(-120, 140, size=n), rs.randint(300, 1600, size=n))
        v = np.where(u < 0.15, -1024, np.where(u < 0.55, rs.randint(-1010, -980, size=n), body))
        a = v.astype(np.int16).reshape(ODD)
    elif kind in ("mr", "mr2", "mr3", "mr4"):                     # zeros, a dark gamma rim, a bright mode
        n = int(np.prod(ODD))
        u = rs.rand(n)
        rim, mode = {"mr": (9.0, 700), "mr2": (30.0, 1100), "mr3": (15.0, 900), "mr4": (12.0, 500)}[kind]
        v = np.where(u < 0.35, 0, np.where(u < 0.6, 1 + rs.gamma(2.0, rim, size=n).astype(np.int64),
                                           rs.normal(mode, 90, size=n).astype(np.int64)))
        a = np.clip(v, 0, 4000).astype(np.int16).reshape(ODD)
    elif kind == "tiny":
        a = np.array([3, -7, 3, 250, 249], dtype=np.int16).reshape(TINY)
    elif kind == "u8":                                            # two channels with different histograms
        n = int(np.prod(U8[1:]))
        c0 = np.where(rs.rand(n) < 0.5, rs.randint(0, 20, size=n), rs.randint(90, 200, size=n))
        c1 = np.where(rs.rand(n) < 0.3, rs.randint(30, 60, size=n), rs.randint(200, 256, size=n))
        a = np.stack([c0, c1]).astype(np.uint8).reshape(U8)
    elif kind == "wide":                                          # uniform over int16: most values miss the LDS window
        a = rs.randint(-32768, 32768, size=WIDE).astype(np.int16)
        a[0, 0, 0, :2] = (-32768, 32767)
    else:
        a = np.full(ODD, 41, dtype=np.int16)
    a.setflags(write=False)
    return a


CASES = [(k, a) for k in ("ct", "mr", "tiny", "u8", "const", "wide") for a in (None, 0)] + [("ct", 32767)]
IDS = [f"{k}-above{a}" for k, a in CASES]


@functools.lru_cache(maxsize=None)
def _table(kind, above):
    return R.histogram(_scan(kind), None, above)


@functools.lru_cache(maxsize=None)
def _bank_rows():
    """The three scans the bank learns from, in a fixed order, as histogram rows counted above 0."""
    return tuple(_table(k, 0)[0] for k in ("mr2", "mr3", "mr4"))


@functools.lru_cache(maxsize=None)
def _ref_bank():
    return T.default_bank(_bank_rows())


@functools.lru_cache(maxsize=None)
def _want_equalize(kind, above):
    return [T.equalize(row, -1.0, 2.5) for row in _table(kind, above)]


@functools.lru_cache(maxsize=None)
def _want_landmark_table(kind, above, clip):
    return [T.landmark_table(row, T.landmarks(row), _ref_bank(), N_Q, clip) for row in _table(kind, above)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                   # (a copy: the cached scans are read-only)


def _hist_of(table):
    """A ScanHistogram holding ``table``: pooled histograms are plain tensors."""
    S = _S()
    h = S.ScanHistogram(table.shape[0], DEV)
    h.table.copy_(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)))
    return h


def _bank(channels=1):
    """A device bank of ``channels`` equal channels learnt from the three scans through ``add_scan``."""
    tr = _tr()
    bank = tr.LandmarkBank(channels, device=DEV)
    for k in ("mr2", "mr3", "mr4"):
        bank.add_scan(_dev(np.repeat(_scan(k), channels, axis=0)), above=0)
    return bank


def _bits(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _identity_slot(channels):
    S = _S()
    slot = S.WindowSlot(channels, DEV)
    slot.words[:, :4] = torch.tensor([1.0, 0.0, -FLT_MAX, FLT_MAX], device=DEV)
    return slot


def _same_table(got, want, what):
    gt, gm = got.cpu()
    for c, (wt, wm) in enumerate(want):
        bad = np.flatnonzero(_bits(gt[c]) != _bits(wt))
        assert bad.size == 0, (what, c, bad[:5] - T.OFFSET, gt[c][bad[:5]], wt[bad[:5]])
        assert gm[c].tolist() == wm.tolist(), (what, c, gm[c], wm)
        assert np.all(np.diff(gt[c]) >= 0), (what, c)                             # 7: monotone along v


# ------------------------------------------------------------------------------------------------ 1. tables in the bits
@pytest.mark.parametrize("kind,above", CASES, ids=IDS)
def test_equalize_table_equals_the_restatement(kind, above):
    tr, S = _tr(), _S()
    hist = S.scan_histogram(_dev(_scan(kind)), above=above)
    got = tr.equalize_table(hist, -1.0, 2.5)
    _same_table(got, _want_equalize(kind, above), "equalize")
    again = tr.TransferTable(hist.channels, DEV)
    assert tr.equalize_table(hist, -1.0, 2.5, out=again) is again
    assert torch.equal(again.table, got.table) and torch.equal(again.meta, got.meta)     # equal calls, equal bits


@pytest.mark.parametrize("kind,above", CASES, ids=IDS)
def test_landmark_record_and_table_equal_the_restatement(kind, above):
    tr, S = _tr(), _S()
    table = _table(kind, above)
    channels = table.shape[0]
    bank = _bank(channels)
    hist = S.scan_histogram(_dev(_scan(kind)), above=above)
    lm = tr.scan_landmarks(hist)
    assert np.array_equal(lm.cpu(), np.stack([T.landmarks(row) for row in table]))
    for clip in (False, True):
        _same_table(tr.landmark_table(lm, bank, clip=clip), _want_landmark_table(kind, above, clip), f"landmarks clip={clip}")
    empty = tr.landmark_table(lm, tr.LandmarkBank(channels, device=DEV))          # an empty bank: zeros, not valid
    et, em = empty.cpu()
    assert not et.any() and not em[:, 2].any()


def test_landmark_records_and_bank_of_three_scans():
    tr, S = _tr(), _S()
    bank = tr.LandmarkBank(1, s_lo=-1.0, s_hi=3.0, device=DEV)
    want = np.zeros(T.LM_WORDS)
    for k in ("mr2", "mr3", "mr4", "const"):                      # the constant scan's record is not valid: adds nothing
        lm = tr.scan_landmarks(S.scan_histogram(_dev(_scan(k)), above=0))
        rec = T.landmarks(_table(k, 0)[0])
        assert np.array_equal(lm.cpu()[0], rec)
        bank.add(lm)
        want = T.bank_add(want, rec, N_Q, -1.0, 3.0)
    got = bank.cpu()
    assert got.dtype == np.float64 and got[0, 0] == 3.0
    assert np.array_equal(got[0].view(np.uint64), want.view(np.uint64)), (got, want)
    assert np.array_equal(_bank().cpu()[0].view(np.uint64), _ref_bank().view(np.uint64))     # add_scan: the same chain
    # a saved bank handed back through words= is the same bank
    back = tr.LandmarkBank(1, s_lo=-1.0, s_hi=3.0, device=DEV, words=bank.words.clone())
    lm = tr.scan_landmarks(S.scan_histogram(_dev(_scan("mr")), above=0))
    assert torch.equal(tr.landmark_table(lm, back).table, tr.landmark_table(lm, bank).table)
    # other quantiles
    q = (0.0, 0.25, 0.5, 1.0)
    lm = tr.scan_landmarks(S.scan_histogram(_dev(_scan("ct"))), quantiles=q)
    assert np.array_equal(lm.cpu()[0], T.landmarks(_table("ct", None)[0], q))


MATCH = [("mr", 0, "mr2", 0), ("ct", None, "mr", None), ("u8", None, "u8", None), ("tiny", None, "ct", None),
         ("wide", None, "mr", 0), ("mr", 0, "wide", None), ("const", None, "ct", None), ("ct", 32767, "ct", None),
         ("ct", None, "ct", 32767)]


@pytest.mark.parametrize("src,sa,ref,ra", MATCH, ids=[f"{s}{a}-to-{r}{b}" for s, a, r, b in MATCH])
def test_match_integers_equal_the_restatement_and_the_float_stage_is_the_prepare_map(src, sa, ref, ra):
    from mivp_amd import scan
    tr, S = _tr(), _S()
    st, rt = _table(src, sa), _table(ref, ra)
    channels = st.shape[0]
    if rt.shape[0] != channels:
        rt = np.repeat(rt, channels, axis=0)
    hist, ref_hist = _hist_of(st), _hist_of(rt)
    got = tr.match_table(hist, ref_hist, _identity_slot(channels), clip=False)
    gt, gm = got.cpu()
    want = [T.match_integers(st[c], rt[c]) for c in range(channels)]
    for c, (u, valid) in enumerate(want):
        assert np.array_equal(gt[c].astype(np.int64), u) and np.array_equal(gt[c], u.astype(np.float32)), (c,)
        assert gm[c].tolist() == T.meta(st[c], valid).tolist()
        assert np.all(np.diff(gt[c]) >= 0)
    # the float stage: the reference's own window, against the existing prepare launch on a volume that holds u
    for spec, clip in ((S.IntensityWindow.percentile(0.02, 0.98), True), (S.IntensityWindow.percentile(0.02, 0.98), False),
                       (S.IntensityWindow.zscore(clip=(0.01, 0.99)), True)):
        slot = S.window_slot(ref_hist, spec)
        tab = tr.match_table(hist, ref_hist, slot, clip=clip).cpu()[0]
        vol = _dev(np.stack([u for u, _ in want]).astype(np.int16).reshape(channels, 64, 32, 32))
        ref_out = scan.prepare_scan(vol, scan.ScanGeometry.identity((64, 32, 32)), window=slot, clip=clip)
        assert np.array_equal(_bits(tab), _bits(ref_out.reshape(channels, -1))), (spec, clip)


def test_match_refuses_nothing_but_marks_a_histogram_of_2_33_voxels():
    tr = _tr()
    big = np.stack([O.table_of({0: 2 ** 32, 5: 2 ** 32}), O.table_of({0: 3, 5: 1})])
    ref = np.stack([O.table_of({1: 2, 9: 2}), O.table_of({1: 2 ** 33})])
    gt, gm = tr.match_table(_hist_of(big), _hist_of(ref), _identity_slot(2), clip=False).cpu()
    for c in range(2):
        assert np.array_equal(gt[c].astype(np.int64), T.VALUES) and gm[c].tolist() == [0, 5, 0, 0]


# ------------------------------------------------------------------------------------------------ 2. Otsu restriction
@pytest.mark.parametrize("kind,above", [("ct", None), ("mr", 0), ("u8", None), ("const", None), ("tiny", None)],
                         ids=["ct", "mr-above0", "u8", "const", "tiny"])
def test_plans_with_an_otsu_record_equal_the_plans_counted_above_the_threshold(kind, above):
    tr, S = _tr(), _S()
    raw_np = _scan(kind)
    raw = _dev(raw_np)
    channels = raw_np.shape[0]
    hist = S.scan_histogram(raw, above=above)
    otsu = S.otsu_slot(hist)
    rec = otsu.cpu()                                              # read back in the test only
    bank = _bank(channels)
    ref_hist = _hist_of(np.repeat(_table("mr2", 0), channels, axis=0))
    ref_slot = S.window_slot(ref_hist, S.IntensityWindow.zscore(clip=(0.01, 0.99)))
    got = (tr.equalize_table(hist, otsu=otsu), tr.match_table(hist, ref_hist, ref_slot, otsu=otsu),
           tr.landmark_table(tr.scan_landmarks(hist, otsu=otsu), bank))
    plain = (tr.equalize_table(hist), tr.match_table(hist, ref_hist, ref_slot), tr.landmark_table(tr.scan_landmarks(hist), bank))
    for c in range(channels):
        if rec[c, 3]:
            h = S.scan_histogram(raw, above=int(rec[c, 0]))
            want = (tr.equalize_table(h), tr.match_table(h, ref_hist, ref_slot), tr.landmark_table(tr.scan_landmarks(h), bank))
        else:
            want = plain                                          # no threshold: the unrestricted plan
        for name, g, w, p in zip(("equalize", "match", "landmarks"), got, want, plain):
            assert torch.equal(g.table[c].view(torch.int32), w.table[c].view(torch.int32)), (name, c)
            assert torch.equal(g.meta[c], w.meta[c]), (name, c)
            if rec[c, 3]:
                assert not torch.equal(g.table[c], p.table[c]), (name, c)         # the case is not vacuous
    assert rec[:, 3].all() == (kind != "const")


# ------------------------------------------------------------------------------------------------ 3. apply
@pytest.mark.parametrize("kind", ["ct", "mr", "tiny", "u8", "wide", "const"])
def test_apply_equals_the_gather_on_both_read_paths(kind):
    tr, S = _tr(), _S()
    raw_np = _scan(kind)
    raw = _dev(raw_np)
    channels = raw_np.shape[0]
    tab = tr.equalize_table(S.scan_histogram(raw), -1.0, 2.5)
    # every entry its own value, so that a wrong index cannot hide behind equal neighbours
    tab.table.copy_(torch.arange(channels * 65536, device=DEV, dtype=torch.float32).reshape(channels, 65536) * 0.5 - 7.0)
    want = torch.stack([tab.table[c][raw[c].long() + 32768] for c in range(channels)])
    for flags in (0, tr.FLAG_GLOBAL):
        got = tr.apply_table(raw, tab, flags=flags)
        assert got.dtype == torch.float32 and tuple(got.shape) == raw_np.shape
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, flags)
        out = torch.full(raw_np.shape, 7.0, device=DEV)
        assert tr.apply_table(raw, tab, out=out, flags=flags) is out and torch.equal(out, got)
    if kind == "wide":                                            # most values fall outside the 16384 staged entries
        lo, hi = tab.meta[0, :2].tolist()
        assert (lo, hi) == (-32768, 32767) and float((raw[0].long() >= lo + 16384).float().mean()) > 0.5


@pytest.mark.parametrize("kind", ["ct", "u8", "wide"])
def test_apply_on_unaligned_views(kind):
    """The scan starts 1..3 elements into its allocation, and so does ``out``: heads, tails and the scalar-store path."""
    tr, S = _tr(), _S()
    raw_np = _scan(kind)
    flat = raw_np.reshape(-1)
    channels = raw_np.shape[0]
    tab = tr.equalize_table(S.scan_histogram(_dev(raw_np)), -1.0, 2.5)
    tab.table.copy_(torch.arange(channels * 65536, device=DEV, dtype=torch.float32).reshape(channels, 65536) * 0.25 + 3.0)
    for off in (1, 2, 3):
        store = torch.from_numpy(np.concatenate([np.full(off, 99, dtype=flat.dtype), flat])).to(DEV)
        raw = store[off:].view(raw_np.shape)
        assert raw.is_contiguous() and raw.data_ptr() % 16 != 0
        want = torch.stack([tab.table[c][raw[c].long() + 32768] for c in range(channels)])
        obuf = torch.full((off + flat.size + 5,), 7.0, device=DEV)
        out = obuf[off:off + flat.size].view(raw_np.shape)
        for flags in (0, tr.FLAG_GLOBAL):
            obuf.fill_(7.0)
            tr.apply_table(raw, tab, out=out, flags=flags)
            assert torch.equal(out, want), (off, flags)
            assert (obuf[:off] == 7.0).all() and (obuf[off + flat.size:] == 7.0).all()       # nothing written outside
            assert torch.equal(tr.apply_table(raw, tab, flags=flags), want)                  # an aligned out, the same raw


# ------------------------------------------------------------------------------------------------ 4. the chain
NATIVE = ODD[1:]


def _geom():
    from mivp_amd.scan import ScanGeometry
    return ScanGeometry(NATIVE, (2, 0, 1), (True, False, True), out_size=(24, 20, 16))


def _specs(tr, S, raw):
    """name -> a fresh spec of each mode (the match reference is the scan's own histogram counted above 0)."""
    own = S.scan_histogram(raw, above=0)
    return {"equalize": tr.IntensityTransfer.equalize(-1.0, 2.5, above=0),
            "match": tr.IntensityTransfer.match(own, S.IntensityWindow.zscore(clip=(0.01, 0.99)), above=0),
            "landmarks": tr.IntensityTransfer.landmarks(_bank(), above=0),
            "landmarks-otsu": tr.IntensityTransfer.landmarks(_bank(), clip=True, foreground="otsu")}


@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
def test_prepare_scan_with_a_transfer_equals_the_two_step_form(aa, monkeypatch):
    from mivp_amd import _lib, scan
    tr, S = _tr(), _S()
    geom = _geom()
    flags = scan.FLAG_ANTIALIAS if aa else 0
    raw = _dev(_scan("mr"))
    calls = []
    plain = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), plain(name, *a))[1])
    last = "mivp_scan_prepare_aa" if aa else "mivp_scan_prepare"
    chains = {"equalize": ["mivp_scan_hist", "mivp_scan_transfer_equalize"],
              "match": ["mivp_scan_hist", "mivp_scan_transfer_match"],
              "landmarks": ["mivp_scan_hist", "mivp_scan_landmarks", "mivp_scan_transfer_landmarks"],
              "landmarks-otsu": ["mivp_scan_hist", "mivp_scan_otsu_plan", "mivp_scan_landmarks", "mivp_scan_transfer_landmarks"]}
    seen = []
    for name, spec in _specs(tr, S, raw).items():
        if name == "match":
            spec.ref_slot()                                       # the reference's window is planned once, ahead
        del calls[:]
        got = scan.prepare_scan(raw, geom, window=spec, flags=flags)
        assert calls == chains[name] + ["mivp_scan_transfer_apply", last], (name, calls)
        table = spec.buffers(1, raw.device)[1]
        want = scan.prepare_scan(tr.apply_table(raw, table), geom, a_min=0, a_max=1, clip=False, flags=flags)
        assert tuple(got.shape) == (1, 1) + geom.size and torch.equal(got.view(torch.int32), want.view(torch.int32)), name
        del calls[:]
        direct = scan.prepare_scan(raw, geom, window=table, flags=flags)                 # a TransferTable as it is
        assert calls == ["mivp_scan_transfer_apply", last] and torch.equal(direct, got), name
        assert all(not torch.equal(got, s) for s in seen), name                           # the modes differ
        seen.append(got)
    # calls without the new types issue the launches they issued before
    del calls[:]
    scan.prepare_scan(raw, geom, window=S.IntensityWindow.percentile(), flags=flags)
    scan.prepare_scan(raw, geom, flags=flags)
    assert calls == ["mivp_scan_hist", "mivp_scan_window_plan", last + "_dev", last]


def test_prepare_scan_with_a_mask_and_two_channels():
    from mivp_amd import scan
    tr, S = _tr(), _S()
    raw_np = _scan("u8")
    raw = _dev(raw_np)
    geom = scan.ScanGeometry.identity(U8[1:])
    mask_np = (np.random.RandomState(3).rand(*U8[1:]) < 0.6).astype(np.uint8)
    got = scan.prepare_scan(raw, geom, window=tr.IntensityTransfer.equalize(), mask=_dev(mask_np))
    want = np.stack([T.equalize(row)[0][raw_np[c].astype(np.int64) + T.OFFSET]
                     for c, row in enumerate(R.histogram(raw_np, mask_np))])
    assert np.array_equal(_bits(got[0]), _bits(want))


# ------------------------------------------------------------------------------------------------ 5. self-match
@pytest.mark.parametrize("kind,above", [("mr", 0), ("ct", None), ("u8", None)], ids=["mr-above0", "ct", "u8"])
def test_matching_a_scan_to_its_own_histogram_reproduces_the_window(kind, above):
    from mivp_amd import scan
    tr, S = _tr(), _S()
    raw = _dev(_scan(kind))
    geom = scan.ScanGeometry.identity(_scan(kind).shape[1:])
    own = S.scan_histogram(raw, above=above)
    for mk in (lambda: S.IntensityWindow.percentile(above=above), lambda: S.IntensityWindow.zscore(above=above, clip=(0.01, 0.99)),
               lambda: S.IntensityWindow.percentile(0.1, 0.9, -1.0, 1.0, above=above, foreground="otsu")):
        want = scan.prepare_scan(raw, geom, window=mk())
        got = scan.prepare_scan(raw, geom, window=tr.IntensityTransfer.match(own, mk(), above=above))
        if above is not None:                                     # an uncounted value maps to the counted value below it
            keep = (raw > above)[None]
            assert keep.any() and torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32))
        else:
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6. gain invariance
def test_landmark_standardisation_is_invariant_to_gain_and_shift():
    from mivp_amd import scan
    tr = _tr()
    a_np = _scan("mr")
    b_np = (2 * a_np.astype(np.int64) + 50).astype(np.int16)
    assert a_np.max() <= 4000
    geom = scan.ScanGeometry.identity(NATIVE)
    spec = tr.IntensityTransfer.landmarks(_bank())
    a = scan.prepare_scan(_dev(a_np), geom, window=spec).clone()
    b = scan.prepare_scan(_dev(b_np), geom, window=spec).clone()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # the ratios of the formula are the same rationals
    assert float(a.max() - a.min()) > 0.5
    fa = scan.prepare_scan(_dev(a_np), geom, a_min=0.0, a_max=4000.0)
    fb = scan.prepare_scan(_dev(b_np), geom, a_min=0.0, a_max=4000.0)
    assert not torch.equal(fa, fb) and float((fa - fb).abs().max()) > 0.01       # what a fixed window makes of the gain


# ------------------------------------------------------------------------------------------------ 8. recording
def test_the_chains_record_and_replay_and_allocate_nothing():
    from mivp_amd import scan
    tr, S = _tr(), _S()
    geom = _geom()
    scans = [_dev(_scan("mr")), _dev(_scan("mr2"))]
    fixed = scans[0].clone()
    out = torch.empty((1, 1) + geom.size, dtype=torch.float32, device=DEV)

    def record(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g, torch.cuda.memory_allocated() - before

    # (a process's first capture allocates torch's own generator state: take that out with a capture of one in-place op)
    idle, first = record(lambda: out.zero_())
    for name, spec in _specs(tr, S, scans[0]).items():
        fresh = _specs(tr, S, scans[0])[name]
        eager = [scan.prepare_scan(r, geom, window=fresh).clone() for r in scans]
        assert not torch.equal(eager[0], eager[1])
        scan.prepare_scan(fixed, geom, window=spec, out=out)      # eager warm-up: buffers, tables and workspace exist now
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        for r in scans:
            fixed.copy_(r)
            scan.prepare_scan(fixed, geom, window=spec, out=out)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == held, name        # eager calls after the first allocate nothing
        graph, used = record(lambda: scan.prepare_scan(fixed, geom, window=spec, out=out))
        print(f"[transfer graph] {name}: bytes allocated by the recording {used} (a first capture: {first})")
        assert used == 0, name
        for i in (0, 1, 0):
            fixed.copy_(scans[i])
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), eager[i].view(torch.int32)), (name, i)


# ------------------------------------------------------------------------------------------------ 9. C-ABI refusals
def test_cabi_refusals_return_einval_and_launch_nothing():
    import ctypes as C
    from mivp_amd import _lib
    lib = _lib.lib()
    EINVAL = -1                                                   # MIVP_EINVAL of include/mivp.h
    hist = torch.zeros((4, 65536), dtype=torch.int64, device=DEV)
    slot = torch.zeros((4, 8), dtype=torch.float32, device=DEV)
    otsu = torch.zeros((4, 4), dtype=torch.int64, device=DEV)
    rec = torch.zeros((4, 17), dtype=torch.int64, device=DEV)
    bank = torch.zeros((4, 17), dtype=torch.float64, device=DEV)
    table = torch.full((4, 65536), 5.0, device=DEV)
    meta = torch.full((4, 4), 9, dtype=torch.int32, device=DEV)
    raw = torch.zeros((1, 4, 4, 4), dtype=torch.int16, device=DEV)
    out = torch.full((1, 4, 4, 4), 5.0, device=DEV)
    p = lambda t, off=0: t.data_ptr() + off                       # noqa: E731
    q = (C.c_double * 3)(0.1, 0.5, 0.9)
    dims = (C.c_int32 * 3)(4, 4, 4)
    st = _lib.stream()
    eq, ma, lm = lib.mivp_scan_transfer_equalize, lib.mivp_scan_transfer_match, lib.mivp_scan_landmarks
    ad, tl, ap = lib.mivp_scan_landmark_bank_add, lib.mivp_scan_transfer_landmarks, lib.mivp_scan_transfer_apply
    bad = [
        eq(None, 1, 0.0, 1.0, None, p(table), p(meta), st), eq(p(hist), 1, 0.0, 1.0, None, None, p(meta), st),
        eq(p(hist), 1, 0.0, 1.0, None, p(table), None, st), eq(p(hist), 0, 0.0, 1.0, None, p(table), p(meta), st),
        eq(p(hist), 5, 0.0, 1.0, None, p(table), p(meta), st), eq(p(hist, 4), 1, 0.0, 1.0, None, p(table), p(meta), st),
        eq(p(hist), 1, 0.0, 1.0, p(otsu, 4), p(table), p(meta), st), eq(p(hist), 1, 0.0, 1.0, None, p(table, 2), p(meta), st),
        eq(p(hist), 1, 0.0, 1.0, None, p(table), p(meta, 2), st), eq(p(hist), 1, 1.0, 0.0, None, p(table), p(meta), st),
        eq(p(hist), 1, 0.0, float("nan"), None, p(table), p(meta), st),
        ma(None, p(hist), p(slot), 1, 1, None, p(table), p(meta), st), ma(p(hist), None, p(slot), 1, 1, None, p(table), p(meta), st),
        ma(p(hist), p(hist), None, 1, 1, None, p(table), p(meta), st), ma(p(hist), p(hist), p(slot), 5, 1, None, p(table), p(meta), st),
        ma(p(hist), p(hist, 4), p(slot), 1, 1, None, p(table), p(meta), st),
        ma(p(hist), p(hist), p(slot, 2), 1, 1, None, p(table), p(meta), st),
        ma(p(hist), p(hist), p(slot), 1, 1, None, None, p(meta), st),
        lm(None, 1, q, 3, None, p(rec), st), lm(p(hist), 1, None, 3, None, p(rec), st), lm(p(hist), 1, q, 3, None, None, st),
        lm(p(hist), 0, q, 3, None, p(rec), st), lm(p(hist), 1, q, 1, None, p(rec), st), lm(p(hist), 1, q, 17, None, p(rec), st),
        lm(p(hist), 1, (C.c_double * 3)(0.1, 0.1, 0.9), 3, None, p(rec), st),
        lm(p(hist), 1, (C.c_double * 3)(0.5, 0.4, 0.9), 3, None, p(rec), st),
        lm(p(hist), 1, (C.c_double * 3)(-0.1, 0.4, 0.9), 3, None, p(rec), st),
        lm(p(hist), 1, (C.c_double * 3)(0.1, 0.4, 1.5), 3, None, p(rec), st),
        lm(p(hist), 1, (C.c_double * 3)(0.1, float("nan"), 0.9), 3, None, p(rec), st),
        lm(p(hist), 1, q, 3, None, p(rec, 4), st), lm(p(hist), 1, q, 3, p(otsu, 4), p(rec), st),
        ad(None, 1, 3, 0.0, 1.0, p(bank), st), ad(p(rec), 1, 3, 0.0, 1.0, None, st), ad(p(rec), 5, 3, 0.0, 1.0, p(bank), st),
        ad(p(rec), 1, 1, 0.0, 1.0, p(bank), st), ad(p(rec), 1, 17, 0.0, 1.0, p(bank), st), ad(p(rec), 1, 3, 0.0, 1.0, p(bank, 4), st),
        ad(p(rec), 1, 3, 1.0, 0.0, p(bank), st),
        tl(None, p(rec), p(bank), 1, 3, 0, None, p(table), p(meta), st), tl(p(hist), None, p(bank), 1, 3, 0, None, p(table), p(meta), st),
        tl(p(hist), p(rec), None, 1, 3, 0, None, p(table), p(meta), st), tl(p(hist), p(rec), p(bank), 0, 3, 0, None, p(table), p(meta), st),
        tl(p(hist), p(rec), p(bank), 1, 1, 0, None, p(table), p(meta), st), tl(p(hist), p(rec), p(bank), 1, 17, 0, None, p(table), p(meta), st),
        tl(p(hist), p(rec), p(bank, 4), 1, 3, 0, None, p(table), p(meta), st),
        tl(p(hist), p(rec), p(bank), 1, 3, 0, None, None, p(meta), st),
        ap(None, 4, 1, dims, p(table), p(meta), 0, p(out), st), ap(p(raw), 4, 1, None, p(table), p(meta), 0, p(out), st),
        ap(p(raw), 4, 1, dims, None, p(meta), 0, p(out), st), ap(p(raw), 4, 1, dims, p(table), None, 0, p(out), st),
        ap(p(raw), 4, 1, dims, p(table), p(meta), 0, None, st), ap(p(raw), 3, 1, dims, p(table), p(meta), 0, p(out), st),
        ap(p(raw), 4, 5, dims, p(table), p(meta), 0, p(out), st), ap(p(raw), 4, 1, dims, p(table), p(meta), 2, p(out), st),
        ap(p(raw, 1), 4, 1, dims, p(table), p(meta), 0, p(out), st), ap(p(raw), 4, 1, dims, p(table), p(meta), 0, p(out, 2), st),
        ap(p(raw), 4, 1, (C.c_int32 * 3)(4, 0, 4), p(table), p(meta), 0, p(out), st),
    ]
    assert len(bad) > 50 and all(rc == EINVAL for rc in bad), bad
    assert b"contract violated" in lib.mivp_last_error()
    torch.cuda.synchronize()
    # nothing was launched: no output word changed
    assert (table == 5.0).all() and (meta == 9).all() and (out == 5.0).all() and not rec.any() and not bank.any()
