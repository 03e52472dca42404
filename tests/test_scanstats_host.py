"""Host side of the scan statistics and data-driven windows (mivp_amd.scanstats): the numpy restatement the GPU tests
compare with (tests/scanstats_ref.py) against brute force, the host report, the C ABI declarations and the argument
checks."""
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import scanstats_ref as R
from conftest import ROOT

SYMBOLS = ("mivp_scan_hist", "mivp_scan_window_plan", "mivp_scan_prepare_dev")


def _ss():
    import mivp_amd  # noqa: F401
    from mivp_amd import scanstats
    return scanstats


# ------------------------------------------------------------------------------------------------ restatement
def _kth_smallest(values, k):
    """The k-th smallest by repeated removal of the minimum: no sort, no cumulative sum."""
    left = list(values)
    for _ in range(k - 1):
        left.remove(min(left))
    return min(left)


def test_order_statistic_against_brute_force():
    rs = np.random.RandomState(0)
    for n in (1, 2, 3, 7, 40):
        for hi in (2, 5, 3000):                                   # hi = 2: almost everything ties
            v = rs.randint(-hi, hi, size=n)
            for q in (0.0, 1.0, 0.5, 0.005, 0.995, 1.0 / 3.0, 0.25):
                k = R.rank(q, n)
                assert 1 <= k <= n
                # k is the smallest integer >= q n, never below 1
                assert Fraction(k) >= Fraction(float(q)) * n or k == 1
                assert k == 1 or Fraction(k - 1) < Fraction(float(q) * float(n))
                assert R.order_statistic(v, q) == _kth_smallest(v.tolist(), k), (n, hi, q)
    v = np.array([4, -2, 9, -2, 4])
    assert R.order_statistic(v, 0.0) == -2 == v.min() and R.order_statistic(v, 1.0) == 9 == v.max()
    assert R.order_statistic(v, 0.4) == -2 and R.order_statistic(v, 0.41) == 4 and R.order_statistic(v, 0.8) == 4
    assert R.order_statistic(np.array([7]), 0.0) == 7 == R.order_statistic(np.array([7]), 1.0)       # N = 1
    assert R.order_statistic(np.zeros(0, dtype=np.int64), 0.5) == 0                                   # N = 0
    # nearest rank, not numpy's interpolating default
    assert R.order_statistic(np.array([0, 10]), 0.75) == 10 and np.percentile([0, 10], 75) == 7.5


def test_histogram_and_moments_against_brute_force():
    rs = np.random.RandomState(1)
    raw = rs.randint(-5, 6, size=(2, 3, 4, 5)).astype(np.int16)
    raw[0, 0, 0, 0], raw[1, 2, 3, 4] = -32768, 32767
    mask = (rs.rand(3, 4, 5) < 0.6).astype(np.uint8) * 3
    for m, above in ((None, None), (mask, None), (None, 0), (mask, 0), (np.zeros_like(mask), None)):
        h = R.histogram(raw, m, above)
        assert h.shape == (2, 65536) and h.dtype == np.int64
        for c in range(2):
            want = {}
            for idx in np.ndindex(3, 4, 5):
                x = int(raw[(c,) + idx])
                if (m is None or m[idx]) and (above is None or x > above):
                    want[x] = want.get(x, 0) + 1
            assert {int(b) - 32768: int(h[c, b]) for b in np.flatnonzero(h[c])} == want
            vals = [x for x, k in want.items() for _ in range(k)]
            n, s1, s2, mean, std = R.moments(R.selected(raw[c], m, above))
            assert (n, s1, s2) == (len(vals), sum(vals), sum(x * x for x in vals))
            if n:
                assert mean == s1 / n and abs(std - float(np.std(np.array(vals, dtype=np.float64)))) < 1e-9 * (1 + std)
            else:
                assert (mean, std) == (0.0, 0.0)
    u8 = rs.randint(0, 256, size=(1, 2, 3, 4)).astype(np.uint8)
    h = R.histogram(u8)
    assert h[0, :32768].sum() == 0 and h[0, 32768 + 256:].sum() == 0 and h.sum() == 24      # one layout for both dtypes


def test_fma_f32_is_the_correctly_rounded_fma():
    rs = np.random.RandomState(2)
    x = rs.randint(-32768, 32768, size=4000)
    worst = 0
    for s, t in ((np.float32(1 / 3), np.float32(-0.7)), (np.float32(0.00048828125), np.float32(0.5)),
                 (np.float32(1.0 / 517.3), np.float32(-1.2345678)), (np.float32(1e-5), np.float32(1e4))):
        got = R.fma_f32(x, s, t)
        assert got.dtype == np.float32
        for xi, gi in zip(x[:400].tolist(), got[:400].tolist()):
            exact = Fraction(xi) * Fraction(float(s)) + Fraction(float(t))
            lo, hi = np.nextafter(np.float32(gi), np.float32(-np.inf)), np.nextafter(np.float32(gi), np.float32(np.inf))
            # no neighbour is closer to the exact value
            assert abs(Fraction(gi) - exact) <= abs(Fraction(float(lo)) - exact)
            assert abs(Fraction(gi) - exact) <= abs(Fraction(float(hi)) - exact)
        worst = max(worst, int((got != (x * np.float64(s) + np.float64(t)).astype(np.float32)).sum()))
    print(f"[scanstats ref] double rounding would have differed on {worst} of 4000 values")


def test_plans_follow_the_formulas():
    from mivp_amd.scan import intensity_map
    rs = np.random.RandomState(3)
    v = rs.randint(-1200, 2500, size=5000)
    a_lo, a_hi = R.order_statistic(v, 0.005), R.order_statistic(v, 0.995)
    p = R.percentile_plan(v, 0.005, 0.995, -1.0, 2.0)
    assert tuple(p[:4]) == intensity_map(a_lo, a_hi, -1.0, 2.0) and (p[4], p[5]) == (a_lo, a_hi)
    assert a_lo < np.percentile(v, 50) < a_hi and v.min() <= a_lo and a_hi <= v.max()
    # the window's ends map to b_min and b_max (to fp32 rounding), everything outside is clipped
    y = R.apply_map(np.array([v.min(), a_lo, a_hi, v.max()]), p)
    assert y[0] == -1.0 and y[3] == 2.0 and abs(y[1] + 1.0) < 1e-6 and abs(y[2] - 2.0) < 1e-6
    # degenerate: a constant selection, an empty one, q_lo == q_hi
    for vv in (np.full(9, 41), np.zeros(0, dtype=np.int64)):
        p = R.percentile_plan(vv, 0.005, 0.995, 0.25, 1.0)
        assert tuple(p[:4]) == (0.0, 0.25, 0.25, 1.0)
        assert (R.apply_map(np.array([-5, 41, 900]), p) == 0.25).all()
    assert tuple(R.percentile_plan(v, 0.5, 0.5)[:2]) == (0.0, 0.0)
    z = R.zscore_plan(v)
    _, _, _, mean, std = R.moments(v)
    assert (z[0], z[1]) == (1.0 / std, -mean / std) and z[2] == -R.FLT_MAX and z[3] == R.FLT_MAX
    assert (z[4], z[5]) == (v.min(), v.max()) and (z[6], z[7]) == (mean, std)
    out = R.apply_map(v, z).astype(np.float64)
    assert abs(out.mean()) < 1e-5 and abs(out.std() - 1.0) < 1e-5
    zc = R.zscore_plan(v, (0.01, 0.99))
    b_lo, b_hi = R.order_statistic(v, 0.01), R.order_statistic(v, 0.99)
    assert zc[2] == float(R.fma_f32(b_lo, zc[0], zc[1])) and zc[3] == float(R.fma_f32(b_hi, zc[0], zc[1]))
    out = R.apply_map(v, zc)
    assert out.min() == np.float32(zc[2]) and out.max() == np.float32(zc[3])
    assert tuple(R.zscore_plan(np.full(5, -3))[:2]) == (1.0, 3.0)            # std == 0: s = 1, t = -mean
    assert tuple(R.zscore_plan(np.zeros(0, dtype=np.int64))[:2]) == (1.0, 0.0) or \
        tuple(R.zscore_plan(np.zeros(0, dtype=np.int64))[:2]) == (1.0, -0.0)


def test_ulp_distance():
    one = np.float32(1.0)
    assert R.ulp_distance(one, one) == 0 and R.ulp_distance(one, np.nextafter(one, np.float32(2))) == 1
    assert R.ulp_distance(np.float32(-0.0), np.float32(0.0)) == 0
    tiny = np.nextafter(np.float32(0), np.float32(1))
    assert R.ulp_distance(-tiny, tiny) == 2


# ------------------------------------------------------------------------------------------------ the host report
def test_report_matches_the_restatement():
    S = _ss()
    rs = np.random.RandomState(4)
    raw = rs.randint(-900, 1800, size=(2, 6, 5, 4)).astype(np.int16)
    raw[1] = 17
    mask = (rs.rand(6, 5, 4) < 0.5).astype(np.uint8)
    table = R.histogram(raw, mask, None)
    table[1] = 0                                                                     # an empty channel
    rep = S.ScanReport(table)
    v = R.selected(raw[0], mask)
    n, _, _, mean, std = R.moments(v)
    assert rep.channels == 2 and rep.count.tolist() == [n, 0]
    assert (rep.min[0], rep.max[0]) == (v.min(), v.max()) and (rep.mean[0], rep.std[0]) == (mean, std)
    assert (rep.min[1], rep.max[1], rep.mean[1], rep.std[1]) == (0, 0, 0.0, 0.0)
    for q in (0.0, 0.005, 0.5, 0.995, 1.0):
        assert rep.percentile(q).tolist() == [R.order_statistic(v, q), 0]
    assert rep.values[0][0] == v.min() and rep.values[0][-1] == v.max() and len(rep.counts[0]) == v.max() - v.min() + 1
    assert rep.counts[0].sum() == n and rep.counts[0][0] > 0 and rep.counts[0][-1] > 0 and len(rep.counts[1]) == 0
    assert np.array_equal(rep.counts[0], np.bincount(v - v.min()))
    with pytest.raises(ValueError):
        rep.percentile(1.5)


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_scanstats_symbols_within_abi_18():
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    names = set(re.findall(r"\b(mivp_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
        m = re.search(r"int %s\(([^;]*)\);" % n, text)
        assert m and m.group(1).replace("\n", " ").split(",")[-1].strip() == "mivp_stream_t stream", n
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    # the device-map entry has the host-map entry's parameters, with the map a device slot
    host = re.search(r"int mivp_scan_prepare\(([^;]*)\);", text).group(1)
    dev = re.search(r"int mivp_scan_prepare_dev\(([^;]*)\);", text).group(1)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]   # noqa: E731
    assert [a.replace("const float* slot", "const float* map") for a in norm(dev)] == norm(host)
    assert "[C][65536]" in text and "[C][8]" in text


def test_library_exports_scanstats_symbols():
    S = _ss()
    from mivp_amd import _lib
    lib = _lib.lib()
    assert lib.mivp_abi_version() == 18
    for n in SYMBOLS + ("mivp_scan_prepare",):
        assert hasattr(lib, n), n
    assert S.NBINS == 65536 and S.OFFSET == 32768


def test_package_exports():
    import mivp_amd
    S = _ss()
    for n in ("scan_histogram", "window_slot", "IntensityWindow", "ScanHistogram", "WindowSlot"):
        assert getattr(mivp_amd, n) is getattr(S, n)
    assert mivp_amd.scanstats is S


# ------------------------------------------------------------------------------------------------ arguments
def test_window_spec_checks():
    S = _ss()
    W = S.IntensityWindow
    w = W.percentile()
    assert (w.q_lo, w.q_hi, w.b_min, w.b_max, w.above, w.mode) == (0.005, 0.995, 0.0, 1.0, None, S.MODE_PERCENTILE)
    z = W.zscore()
    assert (z.q_lo, z.q_hi, z.clip, z.mode) == (0.0, 1.0, False, S.MODE_ZSCORE)
    zc = W.zscore(above=0, clip=(0.01, 0.99))
    assert (zc.q_lo, zc.q_hi, zc.clip, zc.above) == (0.01, 0.99, True, 0)
    assert (W.percentile(0.5, 0.5).q_lo, W.percentile(0, 1).q_hi) == (0.5, 1.0)
    for bad in (dict(q_lo=-0.1), dict(q_hi=1.5), dict(q_lo=0.6, q_hi=0.4), dict(b_min=1.0, b_max=0.0),
                dict(q_lo=float("nan")), dict(b_max=float("inf")), dict(above=0.5), dict(q_lo="low")):
        with pytest.raises(ValueError):
            W.percentile(**bad)
    for bad in (dict(clip=(0.9, 0.1)), dict(clip=(0.1, 1.1)), dict(clip=0.5), dict(clip=(0.1, 0.2, 0.3)), dict(above="0")):
        with pytest.raises(ValueError):
            W.zscore(**bad)


def test_histogram_and_slot_argument_errors():
    S = _ss()
    ok = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    for bad in (ok.numpy(), ok.float(), ok.int(), torch.zeros((5, 5, 6, 7), dtype=torch.int16),
                torch.zeros((2, 1, 5, 6, 7), dtype=torch.int16), torch.zeros((6, 7), dtype=torch.int16)):
        with pytest.raises(ValueError):
            S.scan_histogram(bad)
    for mask in (torch.zeros((5, 6, 7)), torch.zeros((5, 6, 8), dtype=torch.uint8), np.zeros((5, 6, 7), dtype=np.uint8)):
        with pytest.raises(ValueError):
            S.scan_histogram(ok, mask=mask)
    with pytest.raises(ValueError):
        S.scan_histogram(ok, above=0.5)
    with pytest.raises(ValueError):
        S.scan_histogram(ok, base="low")
    with pytest.raises(ValueError):
        S.scan_histogram(ok, out=S.ScanHistogram(2, "cpu"))
    with pytest.raises(ValueError):
        S.scan_histogram(ok, out=torch.zeros((1, 65536), dtype=torch.int64))
    with pytest.raises(ValueError):
        S.ScanHistogram(5, "cpu")
    h = S.ScanHistogram(1, "cpu")
    assert h.table.shape == (1, 65536) and h.table.dtype == torch.int64 and S.WindowSlot(3, "cpu").words.shape == (3, 8)
    spec = S.IntensityWindow.percentile()
    assert spec.buffers(1, "cpu") is spec.buffers(1, torch.device("cpu")) and spec.buffers(2, "cpu") is not spec.buffers(1, "cpu")
    with pytest.raises(ValueError):
        S.window_slot(h.table, spec)
    with pytest.raises(ValueError):
        S.window_slot(h, "percentile")
    with pytest.raises(ValueError):
        S.window_slot(h, spec, out=S.WindowSlot(2, "cpu"))
    # the product path has no CPU fallback: valid arguments on the host reach the device check
    with pytest.raises(RuntimeError):
        S.scan_histogram(ok)
    with pytest.raises(RuntimeError):
        S.window_slot(h, spec)


def test_prepare_scan_window_argument_errors():
    S = _ss()
    from mivp_amd import scan
    g = scan.ScanGeometry((5, 6, 7), (2, 0, 1), (False, True, False))
    ok = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    spec = S.IntensityWindow.percentile()
    for kw in (dict(a_min=-100.0), dict(a_max=400.0), dict(a_min=-100.0, a_max=400.0)):
        with pytest.raises(ValueError, match="a_min"):
            scan.prepare_scan(ok, g, window=spec, **kw)
    for bad in (ok.float(), ok.int()):                                           # int16 / uint8 only
        with pytest.raises(ValueError, match="int16"):
            scan.prepare_scan(bad, g, window=spec)
    for kw in (dict(b_min=-1.0), dict(b_max=2.0), dict(b_min=0.5, b_max=0.75)):     # the output range belongs to the spec
        with pytest.raises(ValueError, match="b_min"):
            scan.prepare_scan(ok, g, window=spec, **kw)
        with pytest.raises(ValueError, match="b_min"):
            scan.prepare_scan(ok, g, window=S.WindowSlot(1, "cpu"), **kw)
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, window="percentile")
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, window=spec, mask=torch.zeros((7, 5, 6), dtype=torch.uint8))     # not the native grid
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, window=spec, mask=torch.zeros((5, 6, 7), dtype=torch.int16))
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, mask=torch.zeros((5, 6, 7), dtype=torch.uint8))                  # a mask without a window
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, window=S.WindowSlot(2, "cpu"))                                   # two channels, one in raw
    with pytest.raises(ValueError):
        scan.prepare_scan(ok, g, window=S.WindowSlot(1, "cpu"), mask=torch.zeros((5, 6, 7), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU"):
        scan.prepare_scan(ok, g, window=spec)
    with pytest.raises(RuntimeError, match="no CPU"):
        scan.prepare_scan(ok.to(torch.uint8), g, window=S.WindowSlot(1, "cpu"))
    p = inspect.signature(scan.prepare_scan).parameters
    assert p["window"].default is None and p["mask"].default is None


def test_predictor_forwards_window_to_prepare_scan():
    """predict_scan's checks need no device: a predictor shell with the fields they read (as tests/test_scan_host.py)."""
    S = _ss()
    from mivp_amd import scan
    from mivp_amd.inference import SlidingWindowPredictor
    p = object.__new__(SlidingWindowPredictor)
    p.image_size, p.cin, p.ncls, p.graph_mode, p.vol = (7, 5, 6), 1, 2, False, None
    g = scan.ScanGeometry((5, 6, 7), (2, 0, 1), (False, True, False))
    raw = torch.zeros((1, 5, 6, 7), dtype=torch.int16)
    spec = S.IntensityWindow.zscore()
    with pytest.raises(ValueError, match="a_min"):
        p.predict_scan(raw, g, window=spec, a_min=0.0)
    with pytest.raises(ValueError, match="int16"):
        p.predict_scan(raw.float(), g, window=spec)
    with pytest.raises(RuntimeError, match="no CPU"):                            # accepted, and stopped at the device check
        p.predict_scan(raw, g, window=spec)
    with pytest.raises(RuntimeError, match="no CPU"):
        p.evaluate_scan(raw, torch.zeros((5, 6, 7), dtype=torch.uint8), g, window=spec,
                        mask=torch.ones((5, 6, 7), dtype=torch.uint8))
