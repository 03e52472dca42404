"""Host side of the Otsu foreground thresholds (mivp_amd.scanstats otsu_slot / foreground_mask / foreground="otsu",
mivp_amd.inference AutoForeground): the Python-integer restatement the GPU tests compare with
(tests/otsu_ref.py) against a brute-force maximisation in Fractions, the tie, gap and degenerate cases, a table whose
compared products need more than 192 bits, the host report, the C ABI declarations and the argument checks."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import otsu_ref as O
import scanstats_ref as R
from conftest import ROOT

SYMBOLS = ("mivp_scan_otsu_plan", "mivp_scan_window_plan_above", "mivp_scan_threshold_mask")


def _ss():
    import mivp_amd  # noqa: F401
    from mivp_amd import scanstats
    return scanstats


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_agrees_with_brute_force():
    rs = np.random.RandomState(0)
    for n, spread, top in ((2, 3, 4), (3, 2, 2), (5, 40, 9), (12, 300, 50), (30, 2000, 1000), (6, 4, 1)):
        for _ in range(4):
            vals = rs.randint(-spread, spread + 1, size=n) + rs.randint(-500, 500)
            row = O.table_of({int(v): int(rs.randint(1, top + 1)) for v in vals})
            rec, _ = O.otsu(row)
            t = O.brute_force(row)
            if t is None:
                assert rec[3] == 0 and np.count_nonzero(row) < 2
                continue
            assert rec == (t, int(row[:t + O.OFFSET + 1].sum()), int(row[t + O.OFFSET + 1:].sum()), 1), (vals, rec, t)
            assert row[t + O.OFFSET] > 0 and rec[1] + rec[2] == row.sum()
    # the ends of the value range
    row = O.table_of({-32768: 3, -32767: 1, 32766: 2, 32767: 5})
    assert O.otsu(row)[0][0] == O.brute_force(row) == -32767


def test_tie_picks_the_lower_value():
    row = O.table_of({0: 7, 1: 7, 2: 7})                          # cuts after 0 and after 1 are mirror images
    rec, _ = O.otsu(row)
    assert rec == (0, 7, 14, 1) and O.brute_force(row) == 0
    n0, N, S = 7, 21, 21
    assert (0 * N - S * n0) ** 2 * (14 * 7) == (7 * N - S * 14) ** 2 * (7 * 14)      # the compared integers are equal


def test_gap_picks_the_top_of_the_lower_mode():
    pairs = {v: 5 for v in range(10, 14)}
    pairs.update({v: 5 for v in range(200, 204)})
    row = O.table_of(pairs)
    rec, _ = O.otsu(row)
    assert rec == (13, 20, 20, 1) and O.brute_force(row) == 13


def test_degenerate_tables_have_no_threshold():
    assert O.otsu(O.table_of({41: 120}))[0] == (41, 120, 0, 0)                        # a constant scan
    assert O.otsu(O.table_of({}))[0] == (0, 0, 0, 0)                                  # N = 0
    assert O.otsu(O.table_of({-3: 1, 9: 4}))[0] == (-3, 1, 4, 1)                      # two distinct values: the lower one
    assert O.brute_force(O.table_of({41: 120})) is None and O.brute_force(O.table_of({-3: 1, 9: 4})) == -3
    assert O.otsu(O.table_of({0: 2 ** 32, 5: 2 ** 32}))[0] == (5, 2 ** 33, 0, 0)      # N >= 2^33: beyond the exact range
    assert O.otsu(O.table_of({0: 2 ** 32, 5: 2 ** 32 - 1}))[0] == (0, 2 ** 32, 2 ** 32 - 1, 1)


def test_big_table_needs_more_than_192_bits():
    row = O.big_table()
    rec, bits = O.otsu(row)
    print(f"[otsu ref] big table: N = {int(row.sum())}, record {rec}, compared products up to {bits} bits")
    assert 192 < bits < 256 and rec[3] == 1
    assert rec[0] == O.brute_force(row)
    assert row[0] > 2 ** 31 and row[-1] > 2 ** 31 and np.count_nonzero(row) > 30


def test_mask_and_restricted_values():
    rs = np.random.RandomState(1)
    raw = np.where(rs.rand(6, 5, 4) < 0.5, rs.randint(-1024, -1000, size=(6, 5, 4)), rs.randint(0, 300, size=(6, 5, 4)))
    rec, _ = O.otsu(R.histogram(raw[None].astype(np.int16))[0])
    assert -1024 <= rec[0] < 0 and rec[3] == 1
    m = O.mask(raw, rec)
    assert m.dtype == np.uint8 and np.array_equal(m, (raw >= 0).astype(np.uint8))
    assert np.array_equal(O.mask(raw, (7, 120, 0, 0)), np.ones(raw.shape, dtype=np.uint8))
    assert np.array_equal(np.sort(O.restricted_values(raw)), np.sort(raw[raw >= 0]))
    const = np.full((3, 3, 3), 9)
    assert np.array_equal(O.restricted_values(const), const.reshape(-1))              # no threshold: no restriction
    # above= selects what is counted, Otsu acts on what was counted
    mr = np.where(rs.rand(6, 5, 4) < 0.3, 0, np.where(rs.rand(6, 5, 4) < 0.4, rs.randint(1, 30, size=(6, 5, 4)),
                                                      rs.randint(400, 900, size=(6, 5, 4))))
    v = O.restricted_values(mr, above=0)
    assert v.min() >= 400 and v.size == int((mr >= 400).sum())


# ------------------------------------------------------------------------------------------------ the host report
def test_report_otsu_equals_the_restatement():
    S = _ss()
    rs = np.random.RandomState(2)
    ct = np.where(rs.rand(500) < 0.5, -1024, rs.randint(-200, 1500, size=500))
    tables = np.stack([np.bincount(ct + O.OFFSET, minlength=O.NBINS), O.table_of({0: 7, 1: 7, 2: 7}), O.table_of({41: 9}),
                       O.table_of({})]).astype(np.int64)
    got = S.ScanReport(tables).otsu()
    want = O.otsu_record(tables)
    for k, name in enumerate(("t", "n_le", "n_gt", "valid")):
        assert got[name].dtype == np.int64 and got[name].tolist() == want[:, k].tolist(), name
    assert got["valid"].tolist() == [1, 1, 0, 0]
    # eta = sigma_b^2 / sigma_total^2 of the chosen threshold, in float64
    t = int(want[0, 0])
    lo, hi = ct[ct <= t].astype(np.float64), ct[ct > t].astype(np.float64)
    var_b = lo.size * hi.size / ct.size ** 2 * (lo.mean() - hi.mean()) ** 2
    assert abs(got["eta"][0] - var_b / ct.astype(np.float64).var()) < 1e-12
    assert got["eta"][1] == 0.75 and got["eta"][2] == 0.0 and got["eta"][3] == 0.0
    assert S.ScanReport(O.big_table()[None]).otsu()["t"][0] == O.otsu(O.big_table())[0][0]


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_entries_within_abi_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    protos = _lib.parse_header()
    for n in SYMBOLS:
        assert n in protos, n
        m = re.search(r"int %s\(([^;]*)\);" % n, text)
        assert m and m.group(1).replace("\n", " ").split(",")[-1].strip() == "mivp_stream_t stream", n
    assert [len(protos[n][1]) for n in SYMBOLS] == [4, 11, 8]
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    # the restricted plan has the plan's parameters, with the record in front of the slot
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]   # noqa: E731
    plain = norm(re.search(r"int mivp_scan_window_plan\(([^;]*)\);", text).group(1))
    above = norm(re.search(r"int mivp_scan_window_plan_above\(([^;]*)\);", text).group(1))
    assert above[:8] == plain[:8] and above[8] == "const int64_t* otsu" and above[9:] == plain[8:]


def test_library_exports_the_entries():
    from mivp_amd import _lib
    lib = _lib.lib()
    assert lib.mivp_abi_version() == 18
    for n in SYMBOLS:
        assert hasattr(lib, n), n


def test_package_exports():
    import mivp_amd
    S = _ss()
    from mivp_amd import otsu
    for n in ("OtsuSlot", "otsu_slot", "foreground_mask", "window_slot_above"):
        assert getattr(mivp_amd, n) is getattr(S, n)
    for n in ("otsu_slot", "foreground_mask", "window_slot_above"):              # they live in mivp_amd/otsu.py
        assert getattr(S, n) is getattr(otsu, n)
    with pytest.raises(AttributeError):
        S.no_such_name
    from mivp_amd import inference
    assert mivp_amd.AutoForeground is inference.AutoForeground


# ------------------------------------------------------------------------------------------------ arguments
def test_spec_takes_foreground():
    S = _ss()
    W = S.IntensityWindow
    assert W.percentile().foreground is None and W.zscore().foreground is None
    assert W.percentile(foreground="otsu").foreground == "otsu" and W.zscore(above=0, foreground="otsu").foreground == "otsu"
    assert W.zscore(above=0, clip=(0.01, 0.99), foreground="otsu").above == 0
    for bad in ("x", "Otsu", 1, True):
        with pytest.raises(ValueError, match="foreground"):
            W.percentile(foreground=bad)
        with pytest.raises(ValueError, match="foreground"):
            W.zscore(foreground=bad)
    assert "foreground='otsu'" in repr(W.zscore(foreground="otsu")) and "foreground" not in repr(W.zscore())
    # the buffers gain the record, and only then
    plain, auto = W.percentile().buffers(2, "cpu"), W.percentile(foreground="otsu").buffers(2, "cpu")
    assert len(plain) == 2 and len(auto) == 3
    assert isinstance(auto[0], S.ScanHistogram) and isinstance(auto[1], S.WindowSlot) and isinstance(auto[2], S.OtsuSlot)
    assert auto[2].words.shape == (2, 4) and auto[2].words.dtype == torch.int64
    assert list(inspect.signature(S.window_slot_above).parameters) == ["hist", "spec", "otsu", "out"]
    assert list(inspect.signature(S.window_slot).parameters) == ["hist", "spec", "out"]      # as it was


def test_slot_and_mask_argument_errors():
    S = _ss()
    h = S.ScanHistogram(1, "cpu")
    spec = S.IntensityWindow.zscore()
    with pytest.raises(ValueError):
        S.OtsuSlot(0, "cpu")
    with pytest.raises(ValueError):
        S.OtsuSlot(5, "cpu")
    with pytest.raises(ValueError):
        S.otsu_slot(h.table)                                                     # a tensor, not a ScanHistogram
    with pytest.raises(ValueError):
        S.otsu_slot(h, out=S.OtsuSlot(2, "cpu"))                                 # channel count
    with pytest.raises(ValueError):
        S.otsu_slot(h, out=torch.zeros((1, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        S.otsu_slot(h, out=S.OtsuSlot(1, "meta"))                                # device mismatch
    with pytest.raises(RuntimeError, match="no CPU"):
        S.otsu_slot(h)
    with pytest.raises(ValueError):
        S.window_slot_above(h, spec, torch.zeros((1, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        S.window_slot_above(h, spec, S.OtsuSlot(2, "cpu"))
    with pytest.raises(ValueError):
        S.window_slot_above(h, spec, S.OtsuSlot(1, "meta"))
    with pytest.raises(RuntimeError, match="no CPU"):
        S.window_slot_above(h, spec, S.OtsuSlot(1, "cpu"))
    ok = torch.zeros((2, 5, 6, 7), dtype=torch.int16)
    rec = S.OtsuSlot(2, "cpu")
    for bad in (ok.numpy(), ok.float(), ok.int(), torch.zeros((5, 5, 6, 7), dtype=torch.int16)):
        with pytest.raises(ValueError):
            S.foreground_mask(bad, rec)
    for ch in (-1, 2, 0.0, True, "0"):
        with pytest.raises(ValueError, match="channel"):
            S.foreground_mask(ok, rec, channel=ch)
    with pytest.raises(ValueError):
        S.foreground_mask(ok, rec.words)
    with pytest.raises(ValueError):
        S.foreground_mask(ok, S.OtsuSlot(1, "cpu"))                              # channel count
    with pytest.raises(ValueError):
        S.foreground_mask(ok, S.OtsuSlot(2, "meta"))                             # device mismatch
    for out in (torch.zeros((5, 6, 7)), torch.zeros((5, 6, 8), dtype=torch.uint8), np.zeros((5, 6, 7), dtype=np.uint8),
                torch.zeros((7, 6, 5), dtype=torch.uint8).permute(2, 1, 0),
                torch.zeros((5, 6, 7), dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError):
            S.foreground_mask(ok, rec, out=out)
    with pytest.raises(RuntimeError, match="no CPU"):
        S.foreground_mask(ok, rec, channel=1)


def test_prepare_scan_reaches_the_device_check_with_an_otsu_window():
    S = _ss()
    from mivp_amd import scan
    g = scan.ScanGeometry((5, 6, 7), (2, 0, 1), (False, True, False))
    ok = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    with pytest.raises(RuntimeError, match="no CPU"):
        scan.prepare_scan(ok, g, window=S.IntensityWindow.zscore(foreground="otsu"))
    with pytest.raises(ValueError, match="int16"):
        scan.prepare_scan(ok.float(), g, window=S.IntensityWindow.zscore(foreground="otsu"))


def test_predictor_foreground_checks():
    """The checks of ``foreground=`` need no device: a predictor shell with the fields they read."""
    from mivp_amd import scan
    from mivp_amd.inference import AutoForeground, SlidingWindowPredictor, WindowFit, predict_scan_volume
    fg = AutoForeground()
    assert (fg.channel, fg.above) == (0, None) and (AutoForeground(1, above=0).channel, AutoForeground(above=0).above) == (1, 0)
    assert repr(AutoForeground(1, 0)) == "AutoForeground(channel=1, above=0)"
    for bad in (dict(channel=-1), dict(channel=0.5), dict(above=0.5), dict(above="0")):
        with pytest.raises(ValueError):
            AutoForeground(**bad)
    b = fg.buffers(2, (5, 6, 7), (7, 5, 6), "cpu")
    assert b is fg.buffers(2, (5, 6, 7), (7, 5, 6), torch.device("cpu")) and b is not fg.buffers(1, (5, 6, 7), (7, 5, 6), "cpu")
    assert b[0].table.shape == (2, 65536) and b[1].words.shape == (2, 4)
    assert (b[2].shape, b[2].dtype, b[3].shape, b[3].dtype) == ((5, 6, 7), torch.uint8, (1, 1, 7, 5, 6), torch.uint8)

    p = object.__new__(SlidingWindowPredictor)
    p.image_size, p.cin, p.ncls, p.graph_mode, p.vol = (7, 5, 6), 1, 2, False, None
    p._rule, p.region = None, None
    g = scan.ScanGeometry((5, 6, 7), (2, 0, 1), (False, True, False))
    raw = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    seg = torch.zeros((5, 6, 7), dtype=torch.uint8)
    with pytest.raises(ValueError, match="skip=WindowSkip"):                      # neither skip nor fit, as set_region
        p.predict_scan(raw, g, foreground=fg)
    with pytest.raises(ValueError, match="skip=WindowSkip"):
        p.evaluate_scan(raw, seg, g, foreground=fg)
    p._rule = WindowFit()
    with pytest.raises(ValueError, match="AutoForeground"):
        p.predict_scan(raw, g, foreground="otsu")
    with pytest.raises(ValueError, match="channel"):
        p.predict_scan(raw, g, foreground=AutoForeground(channel=1))
    with pytest.raises(ValueError, match="int16"):
        p.predict_scan(raw.float(), g, foreground=fg)
    with pytest.raises(ValueError, match="int16"):
        p.evaluate_scan(raw.int(), seg, g, foreground=fg)
    with pytest.raises(RuntimeError, match="no CPU"):                            # accepted, and stopped at the device check
        p.predict_scan(raw, g, foreground=fg)
    assert p.region is None
    # foreground= travels with the intensity keywords: the three signatures are the ones they were
    for fn in (SlidingWindowPredictor.predict_scan, SlidingWindowPredictor.evaluate_scan, predict_scan_volume):
        par = inspect.signature(fn).parameters
        assert "foreground" not in par and par["intensity"].kind is inspect.Parameter.VAR_KEYWORD
    with pytest.raises(ValueError, match="unknown intensity"):
        p.predict_scan(raw, g, foregrund=fg)
