"""numpy / scipy restatement of mivp_amd.regions for the tests.  It does not import the package.

- ``label_classes``: the voxels whose class is listed, labelled per class value (scipy.ndimage.label per class), numbered
  1..n in the raster order of each region's first voxel over all listed classes.
- ``region_stats``: per region cls, size, first, bbox, coord_sum (+ vmin, vmax, vsum, vsqsum of an image) and the derived
  float64 values by the formulas of the package's docstring.
- ``lesion_metrics``: pair counts from ``np.unique`` over (lp, lt) where both are nonzero, then the matching rules."""
import numpy as np
from scipy import ndimage

CONNECTIVITY = {6: 1, 18: 2, 26: 3}


def structure(connectivity):
    return ndimage.generate_binary_structure(3, CONNECTIVITY[connectivity])


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


def label_classes(x, num_classes, connectivity=26, classes=None):
    """x [H, W, D] -> (int32 labels, n, class of each region 1..n)."""
    cm = class_map(x, num_classes)
    flat = np.zeros(cm.size, dtype=np.int64)
    firsts, clss, base = [], [], 0
    for c in (range(1, num_classes) if classes is None else classes):
        lab, n = ndimage.label(cm == c, structure(connectivity))
        if n == 0:
            continue
        lf = lab.ravel()
        idx = np.flatnonzero(lf)
        first = np.full(n + 1, np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(first, lf[idx], idx)
        flat[idx] = lf[idx] + base
        firsts.append(first[1:])
        clss.append(np.full(n, c, dtype=np.int32))
        base += n
    out = np.zeros(cm.size, dtype=np.int32)
    cls = np.zeros(0, dtype=np.int32)
    if base:
        first = np.concatenate(firsts)
        order = np.argsort(first, kind="stable")
        rank = np.empty(base, dtype=np.int64)
        rank[order] = np.arange(base)
        sel = flat > 0
        out[sel] = rank[flat[sel] - 1] + 1
        cls = np.concatenate(clss)[order]
    return out.reshape(cm.shape), base, cls


def region_stats(x, num_classes, image=None, spacing=(1.0, 1.0, 1.0), connectivity=26, classes=None):
    lab, n, cls = label_classes(x, num_classes, connectivity, classes)
    lf = lab.ravel().astype(np.int64)
    idx = np.flatnonzero(lf)
    r = lf[idx] - 1
    h, w, d = np.unravel_index(idx, lab.shape)
    coords = np.stack([h, w, d], 1).astype(np.int64)
    size = np.bincount(r, minlength=n).astype(np.int64)
    first = np.full(n, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, r, idx)
    mn = np.full((n, 3), np.iinfo(np.int64).max, dtype=np.int64)
    mx = np.full((n, 3), -1, dtype=np.int64)
    csum = np.zeros((n, 3), dtype=np.int64)
    for a in range(3):
        np.minimum.at(mn[:, a], r, coords[:, a])
        np.maximum.at(mx[:, a], r, coords[:, a])
        np.add.at(csum[:, a], r, coords[:, a])
    sp = np.asarray(spacing, dtype=np.float64)
    out = dict(n=n, labels=lab, cls=cls, size=size, first=first, bbox=np.concatenate([mn, mx], 1).astype(np.int32),
               coord_sum=csum)
    fsize = size.astype(np.float64)
    out["volume_mm3"] = fsize * (float(spacing[0]) * float(spacing[1]) * float(spacing[2]))
    out["centroid"] = csum.astype(np.float64) / fsize[:, None]
    out["centroid_mm"] = out["centroid"] * sp
    out["extent"] = (mx - mn + 1).astype(np.int32)
    if image is not None:
        img = np.asarray(image).ravel()[idx]
        isf = np.issubdtype(img.dtype, np.floating)
        acc = np.float64 if isf else np.int64
        v = img.astype(acc)
        vsum, vsq = np.zeros(n, dtype=acc), np.zeros(n, dtype=acc)
        np.add.at(vsum, r, v)
        np.add.at(vsq, r, v * v)
        vmin = np.full(n, np.inf if isf else np.iinfo(np.int32).max, dtype=np.float32 if isf else np.int32)
        vmax = np.full(n, -np.inf if isf else np.iinfo(np.int32).min, dtype=vmin.dtype)
        np.minimum.at(vmin, r, img.astype(vmin.dtype))
        np.maximum.at(vmax, r, img.astype(vmin.dtype))
        out.update(vmin=vmin, vmax=vmax, vsum=vsum, vsqsum=vsq)
        out["vmean"] = vsum.astype(np.float64) / fsize
        out["vstd"] = np.sqrt(np.maximum(vsq.astype(np.float64) / fsize - out["vmean"] * out["vmean"], 0.0))
        if isf:                      # the bounds of any float64 summation order (tests)
            ab, sq = np.zeros(n), np.zeros(n)
            np.add.at(ab, r, np.abs(v))
            np.add.at(sq, r, v * v)
            out["_abs_sum"], out["_sq_sum"] = ab, sq
    return out


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(den.shape, np.nan)
    ok = den > 0
    out[ok] = num[ok] / den[ok]
    return out


def lesion_metrics(pred, target, num_classes, spacing=(1.0, 1.0, 1.0), connectivity=26, iou_threshold=0.0, min_size=0,
                   classes=None):
    P = region_stats(pred, num_classes, None, spacing, connectivity, classes)
    T = region_stats(target, num_classes, None, spacing, connectivity, classes)
    lp, lt = P["labels"].ravel().astype(np.int64), T["labels"].ravel().astype(np.int64)
    both = (lp > 0) & (lt > 0)
    pairs, cnt = np.unique(np.stack([lp[both], lt[both]], 1), axis=0, return_counts=True)
    if pairs.size == 0:
        pairs = np.zeros((0, 2), dtype=np.int64)
    same = P["cls"][pairs[:, 0] - 1] == T["cls"][pairs[:, 1] - 1]
    pairs, cnt = pairs[same], cnt[same].astype(np.int64)
    nt, npred = T["n"], P["n"]
    overlap = np.zeros(nt, dtype=np.int64)
    touching = np.zeros(nt, dtype=np.int64)
    best_pred = np.zeros(nt, dtype=np.int32)
    best_overlap = np.zeros(nt, dtype=np.int64)
    detected = np.zeros(nt, dtype=np.int32)
    matched = np.zeros(npred, dtype=np.int32)
    for (p, t), n in zip(pairs, cnt):                    # sorted by p, then t
        sp, st = P["size"][p - 1], T["size"][t - 1]
        if sp < min_size or st < min_size:
            continue
        overlap[t - 1] += n
        touching[t - 1] += sp
        if n > best_overlap[t - 1]:                      # ties keep the smaller p (visited first)
            best_overlap[t - 1], best_pred[t - 1] = n, p
        iou = np.float64(n) / np.float64(sp + st - n)
        if (iou > 0.0) if iou_threshold == 0 else (iou >= iou_threshold):
            detected[t - 1] = 1
            matched[p - 1] = 1
    valid_t = T["size"] >= min_size
    valid_p = P["size"] >= min_size
    counts = np.zeros((num_classes, 4), dtype=np.int64)
    for c in range(1, num_classes):
        tc, pc = valid_t & (T["cls"] == c), valid_p & (P["cls"] == c)
        counts[c] = (tc.sum(), pc.sum(), detected[tc].sum(), matched[pc].sum())
    fsize = T["size"].astype(np.float64)
    bo = best_overlap.astype(np.float64)
    spb = P["size"][np.maximum(best_pred.astype(np.int64) - 1, 0)].astype(np.float64) if npred else np.zeros(nt)
    with np.errstate(invalid="ignore", divide="ignore"):
        best_iou = np.where(best_pred > 0, bo / (spb + fsize - bo), 0.0)
        dice_t = np.where(valid_t, 2.0 * overlap.astype(np.float64) / (T["size"] + touching).astype(np.float64), 0.0)
    total = np.zeros(num_classes)
    for c in range(num_classes):
        total[c] = dice_t[T["cls"] == c].sum()
    det, fn, fp = counts[:, 2], counts[:, 0] - counts[:, 2], counts[:, 1] - counts[:, 3]
    return dict(counts=counts, sensitivity=_ratio(counts[:, 2], counts[:, 0]), precision=_ratio(counts[:, 3], counts[:, 1]),
                f1=_ratio(2 * det, 2 * det + fn + fp), lesion_dice=_ratio(total, counts[:, 0] + fp),
                size=T["size"], valid=valid_t, overlap=overlap, touching=touching, best_pred=best_pred,
                best_overlap=best_overlap, best_iou=best_iou, dice_t=dice_t, detected=detected, matched=matched,
                pairs=np.concatenate([pairs, cnt[:, None]], 1).reshape(-1, 3), pred_regions=P, target_regions=T)
