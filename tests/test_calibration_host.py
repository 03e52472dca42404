"""CPU: the numpy restatement tests/calibration_ref.py against independent definitions on small random inputs (rank-based
AUC, float Brier score, Python-int squared error, literal ECE, a brute-force FROC), and the argument checks of
mivp_amd.calibration, which must refuse bad arguments before the library or the GPU is touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_ref as CR  # noqa: E402

Q = CR.Q
CASES = [(1, 1), (2, 10), (3, 15), (5, 64), (2, 1024)]


def _inputs(seed, ncls, n=300, sharp=2.0):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((ncls, n)).astype(np.float32) * np.float32(sharp)
    p = torch.softmax(torch.from_numpy(z), 0).numpy().reshape(ncls, 5, 6, n // 30)
    t = rng.integers(0, max(ncls - 1, 1), p.shape[1:]).astype(np.uint8)         # the last class is absent
    t[rng.random(t.shape) < 0.05] = 255
    p[0][rng.random(t.shape) < 0.02] = np.nan
    p[ncls - 1][rng.random(t.shape) < 0.02] = 1.5
    return p, t


@pytest.mark.parametrize("ncls,n_bins", CASES)
@pytest.mark.parametrize("sharp", [0.5, 8.0])
def test_restatement_against_independent_definitions(ncls, n_bins, sharp):
    p, t = _inputs(ncls * 1000 + n_bins, ncls, sharp=sharp)
    rep = CR.calibration(p, t, ncls, n_bins)
    rows, n_ignored, n_invalid = CR.rows(p, t, ncls)
    flat_p, flat_t = p.reshape(ncls, -1), t.reshape(-1).astype(np.int64)
    bad = ~np.all((flat_p >= 0) & (flat_p <= 1), axis=0)
    assert n_invalid == bad.sum() > 0 and n_ignored == (~bad & (flat_t == 255)).sum() > 0
    assert rep["n_invalid"] == n_invalid and rep["n_ignored"] == n_ignored
    for r, (q, y) in enumerate(rows):
        assert rep["n"][r] == q.size == flat_t.size - n_invalid - n_ignored
        b = CR.bin_of(q, n_bins)
        assert b.min() >= 0 and b.max() < n_bins
        # the squared error: Python integers
        e2 = sum(int(abs(int(a) - int(c) * Q)) ** 2 for a, c in zip(q, y))
        assert int(rep["sq_hi"][r]) * Q + int(rep["sq_lo"][r]) == e2
        # Brier: the float64 mean of (q / Q - y)^2
        want = np.mean((q.astype(np.float64) / Q - y) ** 2)
        np.testing.assert_allclose(rep["brier"][r], want, rtol=1e-12, atol=0)
        # ECE / MCE as written, in floats: each bin's term is off by a few ulp of its own size at most
        terms, gaps = [], []
        for k in range(n_bins):
            m = b == k
            if m.any():
                gaps.append(abs(y[m].mean() - (q[m].astype(np.float64) / Q).mean()))
                terms.append(m.sum() / q.size * gaps[-1])
        assert abs(rep["ece"][r] - sum(terms)) <= 1e-14 and abs(rep["mce"][r] - max(gaps)) <= 1e-14
        # ROC: the rank statistic of the bin indices, ties counted half
        bp, bn = b[y == 1], b[y == 0]
        if bp.size and bn.size:
            u = (bp[:, None] > bn[None, :]).sum() + 0.5 * (bp[:, None] == bn[None, :]).sum()
            assert abs(rep["roc_auc"][r] - u / (bp.size * bn.size)) <= 1e-12
        else:
            assert np.isnan(rep["roc_auc"][r])
        # the sweep, threshold by threshold
        for k in range(n_bins):
            tp, fp, fn = ((b >= k) & (y == 1)).sum(), ((b >= k) & (y == 0)).sum(), ((b < k) & (y == 1)).sum()
            assert (rep["tp"][r, k], rep["fp"][r, k], rep["fn"][r, k]) == (tp, fp, fn)
            if 2 * tp + fp + fn:
                assert rep["dice_curve"][r, k] == 2 * tp / (2 * tp + fp + fn)
            else:
                assert np.isnan(rep["dice_curve"][r, k])
        d = rep["dice_curve"][r]
        if np.isnan(d).all():
            assert np.isnan(rep["best_threshold"][r])
        else:
            k = int(np.nanargmax(d))
            assert rep["best_threshold"][r] == k / n_bins and rep["best_dice"][r] == d[k]
        # average precision: the step sum over recall
        if bp.size:
            ap, prev = 0.0, 0.0
            for k in range(n_bins - 1, -1, -1):
                tp, fp = ((b >= k) & (y == 1)).sum(), ((b >= k) & (y == 0)).sum()
                if tp + fp:
                    ap += (tp / bp.size - prev) * tp / (tp + fp)
                    prev = tp / bp.size
            assert abs(rep["average_precision"][r] - ap) <= 1e-12
        else:
            assert np.isnan(rep["average_precision"][r])
    if ncls > 1:                                          # the absent class: undefined where nothing is positive
        assert rep["n_pos"][ncls - 1] == 0 and np.isnan(rep["roc_auc"][ncls - 1])
        assert np.isnan(rep["average_precision"][ncls - 1])


def test_tables_add():
    p1, t1 = _inputs(1, 3)
    p2, t2 = _inputs(2, 3)
    both = CR.tables(np.concatenate([p1, p2], 1), np.concatenate([t1, t2], 0), 3, 15)
    added = CR.add_tables(CR.tables(p1, t1, 3, 15), CR.tables(p2, t2, 3, 15))
    for k in CR.INT_FIELDS:
        assert np.array_equal(both[k], added[k]), k


@pytest.mark.parametrize("seed", range(6))
def test_froc_restatement_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    ncls, npred, nref = 3, 25, 18
    score = (rng.integers(1, 9, npred) / 8).astype(np.float32)           # many ties
    cls_p, cls_t = rng.integers(1, ncls, npred), rng.integers(1, ncls, nref)
    if seed == 4:
        cls_p[:] = 1                                                      # class 2 without predictions
    if seed == 5:
        cls_t[:] = 1                                                      # class 2 without reference lesions
    valid_p, valid_t = rng.random(npred) < 0.9, rng.random(nref) < 0.9
    matched = ((rng.random(npred) < 0.5) & valid_p).astype(np.int32)
    best = np.full(nref, -np.inf, dtype=np.float32)
    for t in range(nref):
        cand = score[(matched > 0) & (cls_p == cls_t[t])]
        if cand.size and rng.random() < 0.7:
            best[t] = rng.choice(cand)
    got = CR.froc(score, matched, valid_p, cls_p, best, valid_t, cls_t, ncls)
    levels = (0.125, 0.25, 0.5, 1, 2, 4, 8)
    fs = CR.froc_score(got, levels)
    for c in range(ncls):
        vp, vt = valid_p & (cls_p == c), valid_t & (cls_t == c)
        thr = sorted(set(score[vp].tolist()), reverse=True)
        assert got["n_thresholds"][c] == len(thr)
        ap, prev, sens_at = 0.0, 0.0, []
        for i, tau in enumerate(thr):
            det = sum(1 for t in range(nref) if vt[t] and best[t] >= tau)
            fp = sum(1 for p in range(npred) if vp[p] and not matched[p] and score[p] >= tau)
            tpp = sum(1 for p in range(npred) if vp[p] and matched[p] and score[p] >= tau)
            assert got["thresholds"][c, i] == np.float32(tau) and got["fp"][c, i] == fp
            assert got["precision"][c, i] == tpp / (tpp + fp)
            if vt.sum():
                assert got["sensitivity"][c, i] == det / vt.sum()
                ap += (det / vt.sum() - prev) * tpp / (tpp + fp)
                prev = det / vt.sum()
                sens_at.append((fp, det / vt.sum()))
            else:
                assert np.isnan(got["sensitivity"][c, i])
        assert np.isnan(got["thresholds"][c, len(thr):]).all() and (got["fp"][c, len(thr):] == -1).all()
        if vt.sum():
            assert abs(got["average_precision"][c] - ap) <= 1e-12
            want = np.mean([max([s for f, s in sens_at if f <= a], default=0.0) for a in levels])
            assert abs(fs[c] - want) <= 1e-12
        else:
            assert np.isnan(got["average_precision"][c]) and np.isnan(fs[c])


def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib, calibration as K

    def never(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", never)
    monkeypatch.setattr(_lib, "call", never)
    p = torch.zeros((2, 4, 5, 6), dtype=torch.float32)
    t = torch.zeros((4, 5, 6), dtype=torch.uint8)
    with pytest.raises(ValueError, match="class planes"):
        K.calibration_tables(p, t, 3)
    with pytest.raises(ValueError, match="class planes"):
        K.calibration_tables(p[None], t[None, None], 3)
    for bad in (0, 1025, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="n_bins"):
            K.calibration_tables(p, t, 2, n_bins=bad)
    with pytest.raises(ValueError, match="num_classes"):
        K.calibration_tables(torch.zeros((17, 2, 2, 2)), torch.zeros((2, 2, 2)), 17)
    with pytest.raises(TypeError, match="float32"):
        K.calibration_tables(p.double(), t, 2)
    with pytest.raises(TypeError, match="float32"):
        K.calibration_tables(p.half(), t, 2)
    with pytest.raises(TypeError, match="tensors"):
        K.calibration_tables(p.numpy(), t, 2)
    with pytest.raises(ValueError, match="spatial shape"):
        K.calibration_tables(p, torch.zeros((4, 5, 7), dtype=torch.uint8), 2)
    with pytest.raises(ValueError, match=r"\[C, H, W, D\]"):
        K.calibration_tables(p[0], t, 2)
    other = K.CalibrationReport(2, 10, "cpu")
    with pytest.raises(ValueError, match="out was made for"):
        K.calibration_tables(p, t, 2, n_bins=15, out=other)
    with pytest.raises(ValueError, match="out was made for"):
        K.calibration_tables(p, t, 2, n_bins=10, out=K.CalibrationReport(3, 10, "cpu"))
    with pytest.raises(TypeError, match="CalibrationReport"):
        K.calibration_tables(p, t, 2, out=torch.zeros(4))
    with pytest.raises(RuntimeError, match="GPU"):                     # valid arguments, CPU tensors: no fallback
        K.calibration_tables(p, t, 2)


def test_report_properties_equal_the_restatement_on_the_host():
    """The torch formulas of CalibrationReport, run on CPU tensors filled from the restatement's tables."""
    import mivp_amd  # noqa: F401
    from mivp_amd import calibration as K
    for ncls, n_bins in CASES:
        p, t = _inputs(7 * ncls + n_bins, ncls, sharp=3.0)
        want = CR.calibration(p, t, ncls, n_bins)
        rep = K.CalibrationReport(ncls, n_bins, "cpu")
        assert rep.tables.numel() == K.table_words(ncls, n_bins)
        for k in CR.INT_FIELDS[:7]:
            getattr(rep, k).copy_(torch.from_numpy(want[k]))
        rep.tables[-2], rep.tables[-1] = want["n_ignored"], want["n_invalid"]
        got = rep.cpu()
        for k in CR.INT_FIELDS:
            assert np.array_equal(got[k], want[k]), k
        for k in CR.DERIVED:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
