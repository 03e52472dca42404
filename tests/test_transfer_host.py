"""CPU: the restatement tests/transfer_ref.py of mivp_amd.transfer against independent formulations (equalisation against a
``np.cumsum`` form, the match integers against a brute-force search over exact ``Fraction`` s, the landmark table against
``np.interp``), every host-side argument refusal, the exported names and the forwarding through ``predict_scan``."""
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import scanstats_ref as R
import transfer_ref as T
from conftest import ROOT

SYMBOLS = ("mivp_scan_transfer_equalize", "mivp_scan_transfer_match", "mivp_scan_landmarks", "mivp_scan_landmark_bank_add",
           "mivp_scan_transfer_landmarks", "mivp_scan_transfer_apply")


def _tr():
    import mivp_amd  # noqa: F401
    from mivp_amd import transfer
    return transfer


def _ss():
    from mivp_amd import scanstats
    return scanstats


def _row(counts):
    row = np.zeros(T.NBINS, dtype=np.int64)
    for v, k in counts.items():
        row[v + T.OFFSET] = k
    return row


def _mr_row(seed, n=20000, gain=1, shift=0, zeros=0.4):
    rs = np.random.RandomState(seed)
    v = np.where(rs.rand(n) < zeros, 0, rs.normal(700, 120, size=n).astype(np.int64).clip(1, 4000)) * gain + shift
    return np.bincount(v + T.OFFSET, minlength=T.NBINS).astype(np.int64)


ROWS = {"few": _row({-5: 3, 0: 1, 7: 4, 8: 2}), "one": _row({41: 9}), "empty": _row({}), "mr": _mr_row(1),
        "ends": _row({-32768: 3, -32767: 1, 32766: 2, 32767: 5})}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", sorted(ROWS))
def test_equalize_against_a_cumsum_form(name):
    row = ROWS[name]
    for b_min, b_max in ((0.0, 1.0), (-1.0, 2.5)):
        got, meta = T.equalize(row, b_min, b_max)
        cum = np.cumsum(row)
        occ = np.flatnonzero(row)
        c0 = row[occ[0]] if occ.size else 0
        d = cum[-1] - c0
        r = np.maximum(cum - c0, 0).astype(np.float64) / np.float64(d) if d else np.zeros(T.NBINS)
        want = (r * (np.float64(b_max) - np.float64(b_min)) + np.float64(b_min)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.all(np.diff(got) >= 0)
        if occ.size:
            assert got[occ[0]] == np.float32(b_min) and (d == 0 or got[occ[-1]] == np.float32(b_max))
            assert meta.tolist() == [occ[0] - T.OFFSET, occ[-1] - T.OFFSET, 1, 0]
        else:
            assert meta.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("src,ref", [("few", "few"), ("few", "mr"), ("mr", "few"), ("one", "few"), ("few", "one"),
                                     ("ends", "few"), ("few", "ends")])
def test_match_integers_against_exact_fractions(src, ref):
    row, rrow = ROWS[src], ROWS[ref]
    got, valid = T.match_integers(row, rrow)
    assert valid == 1
    ns, nr = int(row.sum()), int(rrow.sum())
    rocc = np.flatnonzero(rrow)
    cdf = [Fraction(int(rrow[:b + 1].sum()), nr) for b in rocc]   # the reference's distribution at its counted values
    cum = np.cumsum(row)
    for b in np.unique(np.concatenate([np.flatnonzero(row), np.flatnonzero(row) - 1, [0, T.NBINS - 1]]).clip(0)):
        f = Fraction(max(int(cum[b]), 1), ns)
        want = next(int(rocc[i]) for i, g in enumerate(cdf) if g >= f) - T.OFFSET
        assert got[b] == want, (b, got[b], want)
    assert np.all(np.diff(got) >= 0)
    if src == ref:                                                # to itself: every counted value stays
        occ = np.flatnonzero(row)
        assert np.array_equal(got[occ], occ - T.OFFSET)


def test_match_degenerate_tables():
    same, valid = T.match_integers(ROWS["empty"], ROWS["few"])
    assert np.array_equal(same, T.VALUES) and valid == 0
    same, valid = T.match_integers(ROWS["few"], ROWS["empty"])
    assert np.array_equal(same, T.VALUES) and valid == 0
    same, valid = T.match_integers(_row({0: 2 ** 32, 5: 2 ** 32}), ROWS["few"])
    assert np.array_equal(same, T.VALUES) and valid == 0


def test_landmarks_are_order_statistics():
    row = ROWS["mr"]
    values = np.repeat(T.VALUES, row)
    rec = T.landmarks(row)
    assert rec[0] == 1 and rec[12:].tolist() == [0] * 5
    for i, q in enumerate(T.DEFAULT_Q):
        assert rec[1 + i] == R.order_statistic(values, q)
    assert T.landmarks(ROWS["empty"]).tolist() == [0] * 17
    one = T.landmarks(ROWS["one"])
    assert one[0] == 0 and one[1:12].tolist() == [41] * 11        # a constant scan: landmarks, but no scale


def test_bank_and_landmark_table_against_interp():
    n = len(T.DEFAULT_Q)
    rows = [_mr_row(s, zeros=0.0) for s in (2, 3, 4)]
    bank = T.default_bank(rows + [ROWS["one"], ROWS["empty"]], s_lo=0.0, s_hi=100.0)
    assert bank[0] == 3.0                                         # the constant and the empty scan add nothing
    std = bank[1:1 + n] / bank[0]
    assert std[0] == 0.0 and std[-1] == 100.0 and np.all(np.diff(std) > 0)
    row = _mr_row(1, zeros=0.0)
    rec = T.landmarks(row)
    got, meta = T.landmark_table(row, rec, bank, n)
    ms, ts = T.knots(rec, bank, n)
    assert len(ms) == n and meta[2] == 1
    at = np.array(ms) + T.OFFSET
    assert np.array_equal(got[at], np.array(ts).astype(np.float32))                      # exact at the knots
    inside = np.arange(ms[0], ms[-1] + 1)
    want = np.interp(inside, ms, ts).astype(np.float32)
    ulps = max(R.ulp_distance(a, b) for a, b in zip(got[inside + T.OFFSET], want))
    assert ulps <= 2, ulps
    assert np.all(np.diff(got) >= 0)
    assert got[0] < ts[0] and got[-1] > ts[-1]                    # both ends extrapolate
    clipped, _ = T.landmark_table(row, rec, bank, n, clip=True)
    assert clipped[0] == np.float32(ts[0]) and clipped[-1] == np.float32(ts[-1])
    assert np.array_equal(clipped[at[0]:at[-1] + 1], got[at[0]:at[-1] + 1])
    # shared landmark values become one knot with the mean standard value
    few = _row({0: 50, 10: 30, 20: 20})
    frec = T.landmarks(few)
    fm, ft = T.knots(frec, bank, n)
    assert fm == [0, 10, 20] and frec[1:12].tolist() == [0] * 6 + [10] * 3 + [20] * 2
    assert ft[0] == sum(std[1:6], std[0]) / 6 and ft[2] == (std[9] + std[10]) / 2
    # degenerate: one knot, nothing counted, an empty bank
    const, cmeta = T.landmark_table(ROWS["one"], T.landmarks(ROWS["one"]), bank, n)
    assert np.all(const == const[0]) and cmeta.tolist() == [41, 41, 0, 0]
    zero, zmeta = T.landmark_table(ROWS["empty"], T.landmarks(ROWS["empty"]), bank, n)
    assert not zero.any() and zmeta.tolist() == [0, 0, 0, 0]
    none, nmeta = T.landmark_table(row, rec, np.zeros(17), n)
    assert not none.any() and nmeta[2] == 0


def test_gain_and_shift_leave_the_landmark_table_values():
    """B = 2 A + 50: the ratios of the landmark formula are the same rationals, so a voxel's standard value is equal."""
    n = len(T.DEFAULT_Q)
    bank = T.default_bank([_mr_row(s) for s in (2, 3, 4)])
    a, b = _mr_row(9), _mr_row(9, gain=2, shift=50)
    ta, _ = T.landmark_table(a, T.landmarks(a), bank, n)
    tb, _ = T.landmark_table(b, T.landmarks(b), bank, n)
    va = np.flatnonzero(a) - T.OFFSET
    assert np.array_equal(ta[va + T.OFFSET].view(np.uint32), tb[2 * va + 50 + T.OFFSET].view(np.uint32))


def test_restrict_zeroes_the_bins_up_to_a_valid_threshold():
    row = ROWS["few"]
    assert T.restrict(row, None) is not None and np.array_equal(T.restrict(row, (0, 4, 6, 0)), row)
    cut = T.restrict(row, (0, 4, 6, 1))
    assert cut[:T.OFFSET + 1].sum() == 0 and np.array_equal(cut[T.OFFSET + 1:], row[T.OFFSET + 1:])


# ------------------------------------------------------------------------------------------------ C ABI and exports
def test_header_declares_transfer_symbols_within_abi_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    for name in SYMBOLS:
        m = re.search(r"int %s\(([^;]*)\);" % name, text)
        assert m and m.group(1).replace("\n", " ").split(",")[-1].strip() == "mivp_stream_t stream", name
    assert _lib.ABI_VERSION == 18
    protos = _lib.parse_header()
    for name in SYMBOLS[:3] + SYMBOLS[4:5]:                       # the plan entries and the landmarks take a nullable otsu
        assert "const int64_t* otsu" in re.search(r"int %s\(([^;]*)\);" % name, text).group(1), name
    assert len(protos["mivp_scan_transfer_apply"][1]) == 9


def test_library_exports_transfer_symbols():
    from mivp_amd import _lib
    lib = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_package_exports():
    import mivp_amd
    tr = _tr()
    for name in ("IntensityTransfer", "TransferTable", "LandmarkSlot", "LandmarkBank", "equalize_table", "match_table",
                 "scan_landmarks", "landmark_table", "apply_table"):
        assert getattr(mivp_amd, name) is getattr(tr, name)
    assert mivp_amd.transfer is tr
    assert tr.DEFAULT_Q == T.DEFAULT_Q and tr.LM_WORDS == T.LM_WORDS


# ------------------------------------------------------------------------------------------------ arguments
def test_containers_and_spec_checks():
    tr, S = _tr(), _ss()
    t = tr.TransferTable(2, "cpu")
    assert t.table.shape == (2, 65536) and t.table.dtype == torch.float32
    assert t.meta.shape == (2, 4) and t.meta.dtype == torch.int32
    assert tr.LandmarkSlot(1, "cpu").words.shape == (1, 17) and tr.LandmarkSlot(1, "cpu").words.dtype == torch.int64
    bank = tr.LandmarkBank(3, device="cpu")
    assert bank.words.shape == (3, 17) and bank.words.dtype == torch.float64 and bank.cpu()[:, 0].tolist() == [0.0] * 3
    words = torch.arange(17, dtype=torch.float64)[None].clone()
    assert tr.LandmarkBank(1, device="cpu", words=words).words is words
    for bad in (dict(channels=5), dict(channels=0), dict(quantiles=(0.5,)), dict(quantiles=tuple(i / 20 for i in range(17))),
                dict(quantiles=(0.5, 0.5)), dict(quantiles=(0.6, 0.4)), dict(quantiles=(0.0, 1.5)),
                dict(quantiles=(float("nan"), 0.5)), dict(quantiles=0.5), dict(s_lo=1.0, s_hi=0.0), dict(s_hi=float("inf")),
                dict(words=torch.zeros((1, 17))), dict(words=torch.zeros((2, 17), dtype=torch.float64))):
        kw = dict(channels=1, device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            tr.LandmarkBank(**kw)
    with pytest.raises(ValueError):
        tr.TransferTable(5, "cpu")
    with pytest.raises(ValueError):
        tr.LandmarkSlot(1, "cpu", quantiles=(0.2, 0.1))
    X = tr.IntensityTransfer
    e = X.equalize()
    assert (e.mode, e.b_min, e.b_max, e.above, e.foreground, e.channels) == (tr.MODE_EQUALIZE, 0.0, 1.0, None, None, None)
    for bad in (dict(b_min=1.0, b_max=0.0), dict(b_max=float("nan")), dict(b_min="0"), dict(above=0.5),
                dict(foreground="li")):
        with pytest.raises(ValueError):
            X.equalize(**bad)
    h = S.ScanHistogram(1, "cpu")
    m = X.match(h, S.IntensityWindow.percentile(), above=0, foreground="otsu")
    assert (m.mode, m.clip, m.above, m.foreground, m.channels) == (tr.MODE_MATCH, True, 0, "otsu", 1)
    assert X.match(h, S.WindowSlot(1, "cpu"), clip=False).clip is False
    for bad in ((h.table, S.IntensityWindow.zscore()), (h, "zscore"), (h, S.WindowSlot(2, "cpu"))):
        with pytest.raises(ValueError):
            X.match(*bad)
    lm = X.landmarks(bank)
    assert (lm.mode, lm.clip, lm.channels) == (tr.MODE_LANDMARKS, False, 3)
    with pytest.raises(ValueError):
        X.landmarks(bank.words)
    assert e.buffers(1, "cpu") is e.buffers(1, torch.device("cpu")) and e.buffers(2, "cpu") is not e.buffers(1, "cpu")
    hist, tab, otsu, slot = X.landmarks(tr.LandmarkBank(1, device="cpu"), foreground="otsu").buffers(1, "cpu")
    assert isinstance(hist, S.ScanHistogram) and isinstance(tab, tr.TransferTable) and isinstance(otsu, S.OtsuSlot) \
        and isinstance(slot, tr.LandmarkSlot)
    assert e.buffers(1, "cpu")[2:] == (None, None)


def test_function_argument_errors():
    tr, S = _tr(), _ss()
    h, h2 = S.ScanHistogram(1, "cpu"), S.ScanHistogram(2, "cpu")
    slot = S.WindowSlot(1, "cpu")
    bank = tr.LandmarkBank(1, device="cpu")
    for call in (lambda: tr.equalize_table(h.table), lambda: tr.equalize_table(h, 1.0, 0.0),
                 lambda: tr.equalize_table(h, otsu=S.OtsuSlot(2, "cpu")), lambda: tr.equalize_table(h, otsu="otsu"),
                 lambda: tr.equalize_table(h, out=tr.TransferTable(2, "cpu")), lambda: tr.equalize_table(h, out=h.table),
                 lambda: tr.match_table(h, h.table, slot), lambda: tr.match_table(h, h, slot.words),
                 lambda: tr.match_table(h, h2, slot), lambda: tr.match_table(h, h, S.WindowSlot(2, "cpu")),
                 lambda: tr.match_table(h.table, h, slot), lambda: tr.scan_landmarks(h.table),
                 lambda: tr.scan_landmarks(h, quantiles=(0.5,)), lambda: tr.scan_landmarks(h, quantiles=(0.5, 0.4)),
                 lambda: tr.scan_landmarks(h, out=tr.LandmarkSlot(2, "cpu")),
                 lambda: tr.landmark_table(h, bank), lambda: tr.landmark_table(tr.LandmarkSlot(1, "cpu"), bank.words),
                 lambda: tr.landmark_table(tr.LandmarkSlot(2, "cpu"), bank),
                 lambda: tr.landmark_table(tr.LandmarkSlot(1, "cpu", (0.1, 0.9)), bank),
                 lambda: tr.landmark_table(tr.LandmarkSlot(1, "cpu"), bank),               # no record yet
                 lambda: bank.add(h), lambda: bank.add(tr.LandmarkSlot(2, "cpu")),
                 lambda: bank.add_scan(torch.zeros((2, 3, 4, 5), dtype=torch.int16)),
                 lambda: bank.add_scan(torch.zeros((1, 3, 4, 5))),
                 lambda: bank.add_scan(torch.zeros((1, 3, 4, 5), dtype=torch.int16), foreground="li")):
        with pytest.raises(ValueError):
            call()
    ok = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    tab = tr.TransferTable(1, "cpu")
    for call in (lambda: tr.apply_table(ok.float(), tab), lambda: tr.apply_table(ok, tab.table),
                 lambda: tr.apply_table(ok, tr.TransferTable(2, "cpu")), lambda: tr.apply_table(ok, tab, flags=2),
                 lambda: tr.apply_table(ok, tab, flags=True), lambda: tr.apply_table(ok, tab, out=torch.zeros((1, 5, 6, 8))),
                 lambda: tr.apply_table(ok, tab, out=torch.zeros((1, 5, 6, 7), dtype=torch.float64)),
                 lambda: tr.apply_table(ok, tab, out=torch.zeros((1, 5, 6, 14))[..., ::2])):
        with pytest.raises(ValueError):
            call()
    # the product path has no CPU fallback: valid arguments on the host reach the device check
    for call in (lambda: tr.equalize_table(h), lambda: tr.match_table(h, h, slot), lambda: tr.scan_landmarks(h),
                 lambda: tr.apply_table(ok, tab), lambda: bank.add(tr.LandmarkSlot(1, "cpu")), lambda: bank.add_scan(ok)):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()


def test_prepare_scan_transfer_argument_errors():
    tr, S = _tr(), _ss()
    from mivp_amd import scan
    g = scan.ScanGeometry((5, 6, 7), (2, 0, 1), (False, True, False))
    ok = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    spec, tab = tr.IntensityTransfer.equalize(), tr.TransferTable(1, "cpu")
    mask = torch.ones((5, 6, 7), dtype=torch.uint8)
    for window in (spec, tab):
        for kw in (dict(a_min=-100.0), dict(a_max=400.0)):
            with pytest.raises(ValueError, match="a_min"):
                scan.prepare_scan(ok, g, window=window, **kw)
        for kw in (dict(b_min=-1.0), dict(b_max=2.0)):
            with pytest.raises(ValueError, match="b_min"):
                scan.prepare_scan(ok, g, window=window, **kw)
        for bad in (ok.float(), ok.int()):
            with pytest.raises(ValueError, match="int16"):
                scan.prepare_scan(bad, g, window=window)
    with pytest.raises(ValueError, match="already computed"):
        scan.prepare_scan(ok, g, window=tab, mask=mask)
    with pytest.raises(ValueError, match="channels"):
        scan.prepare_scan(ok, g, window=tr.TransferTable(2, "cpu"))
    with pytest.raises(ValueError, match="channels"):
        scan.prepare_scan(ok, g, window=tr.IntensityTransfer.landmarks(tr.LandmarkBank(2, device="cpu")))
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, window=spec, mask=torch.ones((7, 5, 6), dtype=torch.uint8))
    with pytest.raises(ValueError, match="IntensityTransfer"):
        scan.prepare_scan(ok, g, window="equalize")
    for window, kw in ((spec, {}), (spec, dict(mask=mask)), (tab, {})):
        with pytest.raises(RuntimeError, match="no CPU"):
            scan.prepare_scan(ok, g, window=window, **kw)
    assert list(inspect.signature(scan.prepare_scan).parameters) == ["raw", "geom", "a_min", "a_max", "b_min", "b_max", "clip",
                                                                     "out", "flags", "window", "mask"]


def test_predictor_forwards_a_transfer_to_prepare_scan():
    """predict_scan's checks need no device: a predictor shell with the fields they read (as tests/test_scanstats_host.py)."""
    tr = _tr()
    from mivp_amd import scan
    from mivp_amd.inference import SlidingWindowPredictor
    p = object.__new__(SlidingWindowPredictor)
    p.image_size, p.cin, p.ncls, p.graph_mode, p.vol = (7, 5, 6), 1, 2, False, None
    g = scan.ScanGeometry((5, 6, 7), (2, 0, 1), (False, True, False))
    raw = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    spec = tr.IntensityTransfer.equalize(above=0)
    with pytest.raises(ValueError, match="a_min"):
        p.predict_scan(raw, g, window=spec, a_min=0.0)
    with pytest.raises(ValueError, match="int16"):
        p.predict_scan(raw.float(), g, window=spec)
    with pytest.raises(ValueError, match="already computed"):
        p.predict_scan(raw, g, window=tr.TransferTable(1, "cpu"), mask=torch.ones((5, 6, 7), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU"):                            # accepted, and stopped at the device check
        p.predict_scan(raw, g, window=spec)
    with pytest.raises(RuntimeError, match="no CPU"):
        p.predict_scan(raw, g, window=tr.TransferTable(1, "cpu"), antialias=True)
    with pytest.raises(RuntimeError, match="no CPU"):
        p.evaluate_scan(raw, torch.zeros((5, 6, 7), dtype=torch.uint8), g, window=spec,
                        mask=torch.ones((5, 6, 7), dtype=torch.uint8))
