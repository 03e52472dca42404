"""numpy restatement of mivp_amd.calibration and of the lesion scores / FROC of mivp_amd.regions for the
tests.  It does not import the package.

- ``tables``: the integer tables by the definitions of the package's docstring (Q = 2^20, q = rint(p32 * Q), valid voxels,
  bin = min(n_bins - 1, q * n_bins >> 20), C one-vs-rest rows and the top-label row).
- ``derived``: the float64 values from the integer tables, with the package's formulas.
- ``lesion_scores`` / ``froc``: score, best_score and the free-response curve on top of ``regions_ref.lesion_metrics``."""
import numpy as np

QBITS = 20
Q = 1 << QBITS
INT_FIELDS = ("count", "pos", "qsum", "n", "n_pos", "sq_hi", "sq_lo", "n_ignored", "n_invalid")
DERIVED = ("bin_confidence", "bin_accuracy", "ece", "mce", "brier", "tp", "fp", "fn", "dice_curve", "roc_auc",
           "average_precision", "best_threshold", "best_dice")


def class_map(x, num_classes):
    x = np.asarray(x)
    if x.dtype == bool:
        x = x.astype(np.uint8)
    if np.issubdtype(x.dtype, np.floating):
        with np.errstate(invalid="ignore"):
            ok = (x >= 0) & (x < num_classes) & (x == np.floor(x))
    else:
        ok = (x >= 0) & (x < num_classes)
    c = np.full(x.shape, -1, dtype=np.int64)
    c[ok] = x[ok].astype(np.int64)
    return c


def quantise(p32):
    return np.rint(np.asarray(p32, dtype=np.float32) * np.float32(Q)).astype(np.int64)


def bin_of(q, n_bins):
    return np.minimum(n_bins - 1, (q * n_bins) >> QBITS)


def rows(probs, target, num_classes):
    """-> (list of (q, y) per row over the valid voxels, n_ignored, n_invalid)."""
    p = np.asarray(probs, dtype=np.float32).reshape(num_classes, -1)
    t = class_map(np.asarray(target).reshape(-1), num_classes)
    with np.errstate(invalid="ignore"):
        good = np.all((p >= 0) & (p <= 1), axis=0)
    valid = good & (t >= 0)
    n_ignored, n_invalid = int((good & (t < 0)).sum()), int((~good).sum())
    p, t = p[:, valid], t[valid]
    out = [(quantise(p[c]), (t == c).astype(np.int64)) for c in range(num_classes)]
    out.append((quantise(p.max(0)), (p.argmax(0) == t).astype(np.int64)))         # argmax: the first among equals
    return out, n_ignored, n_invalid


def tables(probs, target, num_classes, n_bins):
    rws, n_ignored, n_invalid = rows(probs, target, num_classes)
    R = num_classes + 1
    out = {k: np.zeros((R, n_bins), dtype=np.int64) for k in ("count", "pos", "qsum")}
    out.update({k: np.zeros(R, dtype=np.int64) for k in ("n", "n_pos", "sq_hi", "sq_lo")})
    for r, (q, y) in enumerate(rws):
        b = bin_of(q, n_bins)
        np.add.at(out["count"][r], b, 1)
        np.add.at(out["pos"][r], b, y)
        np.add.at(out["qsum"][r], b, q)
        e = np.abs(q - y * Q)
        e2 = e * e
        out["n"][r], out["n_pos"][r] = q.size, y.sum()
        out["sq_hi"][r], out["sq_lo"][r] = (e2 >> QBITS).sum(), (e2 & (Q - 1)).sum()
    out["n_ignored"], out["n_invalid"] = n_ignored, n_invalid
    return out


def add_tables(a, b):
    return {k: a[k] + b[k] for k in INT_FIELDS}


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    num, den = np.broadcast_arrays(num, den)
    out = np.full(den.shape, np.nan)
    ok = den > 0
    out[ok] = num[ok] / den[ok]
    return out


def _tail(a):
    return np.cumsum(a[:, ::-1], axis=1)[:, ::-1]


def derived(tab, n_bins):
    count, pos, qsum, n, n_pos = tab["count"], tab["pos"], tab["qsum"], tab["n"], tab["n_pos"]
    out = dict(bin_confidence=_ratio(qsum, count * Q), bin_accuracy=_ratio(pos, count))
    gap = np.abs(pos * Q - qsum)                                     # |pos / count - qsum / (count Q)| * count * Q, exact
    out["ece"] = _ratio(gap.sum(1), n * Q)
    g = _ratio(gap, count * Q)
    out["mce"] = np.where(n > 0, np.where(np.isnan(g), -1.0, g).max(1), np.nan)
    out["brier"] = _ratio(tab["sq_hi"].astype(np.float64) * float(Q) + tab["sq_lo"].astype(np.float64),
                          n.astype(np.float64) * float(Q) * float(Q))
    tp, fp = _tail(pos), _tail(count - pos)
    fn = n_pos[:, None] - tp
    dice = _ratio(2 * tp, 2 * tp + fp + fn)
    out.update(tp=tp, fp=fp, fn=fn, dice_curve=dice)
    best_k = np.zeros(len(n), dtype=np.int64)
    best_thr, best_dice = np.full(len(n), np.nan), np.full(len(n), np.nan)
    for r in range(len(n)):
        for k in range(n_bins):                                      # the first maximum among the defined entries
            if not np.isnan(dice[r, k]) and (np.isnan(best_dice[r]) or dice[r, k] > best_dice[r]):
                best_k[r], best_dice[r], best_thr[r] = k, dice[r, k], k / float(n_bins)
    out.update(best_threshold=best_thr, best_dice=best_dice)
    zero = np.zeros((len(n), 1), dtype=np.int64)
    tp1, fp1 = np.concatenate([tp[:, 1:], zero], 1), np.concatenate([fp[:, 1:], zero], 1)
    area = ((fp - fp1).astype(np.float64) * (tp + tp1).astype(np.float64)).sum(1)
    out["roc_auc"] = _ratio(area, 2.0 * (n - n_pos).astype(np.float64) * n_pos.astype(np.float64))
    prec = _ratio(tp, tp + fp)
    term = (tp - tp1).astype(np.float64) * np.where(np.isnan(prec), 0.0, prec)
    out["average_precision"] = _ratio(term.sum(1), n_pos)
    return out


def calibration(probs, target, num_classes, n_bins):
    tab = tables(probs, target, num_classes, n_bins)
    tab.update(derived(tab, n_bins))
    return tab


# ------------------------------------------------------------------------------------------- lesion scores and FROC
def froc(score, matched, valid_p, cls_p, best_score, valid_t, cls_t, num_classes):
    """Per class: the distinct scores of the valid predictions, descending, and the curve at each of them (padded to the
    longest curve: thresholds / sensitivity / precision with NaN, fp with -1)."""
    curves = []
    for c in range(num_classes):
        vp, vt = valid_p & (cls_p == c), valid_t & (cls_t == c)
        thr = np.unique(score[vp])[::-1].astype(np.float32)
        n_ref = int(vt.sum())
        hit = matched > 0
        asc_t = np.sort(best_score[vt])
        asc_fp, asc_tp = np.sort(score[vp & ~hit]), np.sort(score[vp & hit])
        det = asc_t.size - np.searchsorted(asc_t, thr, "left")
        fp = asc_fp.size - np.searchsorted(asc_fp, thr, "left")
        tpp = asc_tp.size - np.searchsorted(asc_tp, thr, "left")
        sens = _ratio(det, np.full(det.shape, n_ref))
        prec = _ratio(tpp, tpp + fp)
        step = det - np.concatenate([[0], det[:-1]])
        ap = _ratio((step.astype(np.float64) * prec).sum(), n_ref)
        curves.append(dict(thresholds=thr, sensitivity=sens, fp=fp.astype(np.int64), precision=prec, ap=float(ap),
                           n_ref=n_ref))
    kmax = max(len(c["thresholds"]) for c in curves) if curves else 0
    pad = lambda a, fill, dt: np.concatenate([a.astype(dt), np.full(kmax - len(a), fill, dtype=dt)])   # noqa: E731
    return dict(thresholds=np.stack([pad(c["thresholds"], np.nan, np.float32) for c in curves]),
                n_thresholds=np.array([len(c["thresholds"]) for c in curves], dtype=np.int64),
                sensitivity=np.stack([pad(c["sensitivity"], np.nan, np.float64) for c in curves]),
                fp=np.stack([pad(c["fp"], -1, np.int64) for c in curves]),
                precision=np.stack([pad(c["precision"], np.nan, np.float64) for c in curves]),
                average_precision=np.array([c["ap"] for c in curves]),
                n_ref=np.array([c["n_ref"] for c in curves], dtype=np.int64))


def froc_score(curve, fp_levels=(0.125, 0.25, 0.5, 1, 2, 4, 8)):
    out = np.full(len(curve["n_ref"]), np.nan)
    for c in range(len(out)):
        if curve["n_ref"][c] == 0:
            continue
        k = curve["n_thresholds"][c]
        sens, fp = curve["sensitivity"][c, :k], curve["fp"][c, :k]
        out[c] = np.mean([sens[fp <= a].max() if (fp <= a).any() else 0.0 for a in fp_levels])
    return out


def lesion_scores(pred, target, image, num_classes, connectivity=26, iou_threshold=0.0, min_size=0):
    """``regions_ref.lesion_metrics`` plus ``score``, ``best_score``, ``froc`` and ``froc_score``."""
    import regions_ref as R
    rep = R.lesion_metrics(pred, target, num_classes, connectivity=connectivity, iou_threshold=iou_threshold,
                           min_size=min_size)
    P = R.region_stats(pred, num_classes, image, connectivity=connectivity)
    T = rep["target_regions"]
    score = P["vmax"].astype(np.float32)
    best = np.full(T["n"], -np.inf, dtype=np.float32)
    for p, t, n in rep["pairs"]:
        sp, st = P["size"][p - 1], T["size"][t - 1]
        if sp < min_size or st < min_size:
            continue
        iou = np.float64(n) / np.float64(sp + st - n)
        if (iou > 0.0) if iou_threshold == 0 else (iou >= iou_threshold):
            best[t - 1] = max(best[t - 1], score[p - 1])
    rep["pred_regions"] = P
    rep["score"], rep["best_score"] = score, best
    valid_p = (P["size"] >= min_size) & (P["size"] > 0)
    rep["froc"] = froc(score, rep["matched"], valid_p, P["cls"], best, rep["valid"] & (T["size"] > 0), T["cls"],
                       num_classes)
    rep["froc_score"] = froc_score(rep["froc"])
    return rep
