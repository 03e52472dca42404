"""numpy / Python-integer restatement of mivp_amd.transfer (the module docstring there has the definitions): the
equalisation table, the integers ``u(v)`` of histogram matching and its float stage, the landmark record, the bank and the
piecewise-linear landmark table.  Everything takes one channel's numpy int64 table ``[65536]`` (``table[v + 32768]`` counts
value ``v``).  The integer stages use Python integers, the float stages float64 operations written one by one (numpy rounds
each on its own) with one rounding to float32 at the end."""
import numpy as np

import scanstats_ref as R

NBINS, OFFSET = 65536, 32768
DEFAULT_Q = (0.01, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.99)
LM_WORDS = 17
VALUES = np.arange(NBINS, dtype=np.int64) - OFFSET


def restrict(row, otsu=None):
    """The row with the bins at or below a valid Otsu threshold read as zero.  ``otsu``: (t, n_le, n_gt, valid) or None."""
    row = np.asarray(row, dtype=np.int64)
    if otsu is None or not int(otsu[3]):
        return row
    out = row.copy()
    out[:int(otsu[0]) + OFFSET + 1] = 0
    return out


def meta(row, valid):
    """(lowest counted value, highest counted value, valid, 0); both values 0 when nothing is counted."""
    occ = np.flatnonzero(row)
    if occ.size == 0:
        return np.array([0, 0, int(valid), 0], dtype=np.int32)
    return np.array([occ[0] - OFFSET, occ[-1] - OFFSET, int(valid), 0], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ equalise
def equalize(row, b_min=0.0, b_max=1.0):
    """fp32 [65536]: r = max(C(v) - c0, 0) / d, y = r * (b_max - b_min) + b_min; and the meta record."""
    row = np.asarray(row, dtype=np.int64)
    occ = np.flatnonzero(row)
    n = int(row.sum())
    c0 = int(row[occ[0]]) if occ.size else 0
    d = n - c0
    y = np.empty(NBINS, dtype=np.float64)
    width = np.float64(b_max) - np.float64(b_min)
    run, cur = 0, None
    for b in range(NBINS):
        if cur is None or row[b]:                                 # C(v) moves at counted values only
            run += int(row[b])
            r = np.float64(0.0) if d == 0 else np.float64(max(run - c0, 0)) / np.float64(d)
            cur = r * width + np.float64(b_min)
        y[b] = cur
    return y.astype(np.float32), meta(row, n > 0)


# ------------------------------------------------------------------------------------------------ match
def match_integers(row, ref):
    """int64 [65536]: u(v), the smallest value u with C_ref(u) N_src >= max(C_src(v), 1) N_ref, in Python integers; and
    the valid word."""
    row, ref = np.asarray(row, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    ns, nr = sum(int(k) for k in row), sum(int(k) for k in ref)
    exact = ns < 2 ** 33 and nr < 2 ** 33
    if not exact or ns == 0 or nr == 0:
        return VALUES.copy(), int(exact and ns > 0 and nr > 0)
    out = np.empty(NBINS, dtype=np.int64)
    cs, u, cr = 0, 0, int(ref[0])                                 # u is non-decreasing in v: one forward walk
    for b in range(NBINS):
        cs += int(row[b])
        target = max(cs, 1) * nr
        while cr * ns < target:
            u += 1
            cr += int(ref[u])
        out[b] = u - OFFSET
    return out, 1


def match_float(u, words, clip=True):
    """fp32: y = fmaf((float)u, s, t), clamped to [lo, hi] with clip (words = the reference slot's s, t, lo, hi, ...)."""
    return R.apply_map(np.asarray(u, dtype=np.int64), words, clip)


# ------------------------------------------------------------------------------------------------ landmarks
def landmarks(row, quantiles=DEFAULT_Q):
    """int64 [17]: (valid, m_0 .. m_{n-1}, zero padded), m_i the k-th smallest counted value, k = max(1, ceil(q N))."""
    row = np.asarray(row, dtype=np.int64)
    n = int(row.sum())
    rec = np.zeros(LM_WORDS, dtype=np.int64)
    if n == 0:
        return rec
    cum = np.cumsum(row)
    for i, q in enumerate(quantiles):
        rec[1 + i] = int(np.searchsorted(cum, R.rank(q, n), side="left")) - OFFSET
    rec[0] = int(rec[len(quantiles)] > rec[1])
    return rec


def bank_add(bank, rec, n, s_lo=0.0, s_hi=1.0):
    """The float64 [17] bank (count, sums) after adding one record, operation by operation."""
    bank = np.array(bank, dtype=np.float64)
    if not int(rec[0]):
        return bank
    m0, ml = int(rec[1]), int(rec[n])
    for i in range(n):
        ratio = np.float64(int(rec[1 + i]) - m0) / np.float64(ml - m0)
        bank[1 + i] = bank[1 + i] + (np.float64(s_lo) + ratio * (np.float64(s_hi) - np.float64(s_lo)))
    bank[0] = bank[0] + np.float64(1.0)
    return bank


def knots(rec, bank, n):
    """(M_j, T_j): the distinct landmark values in increasing order and the mean standard value of each."""
    count = np.float64(bank[0])
    ms, ts = [], []
    i = 0
    while i < n:
        m, s, share = int(rec[1 + i]), np.float64(0.0), 0
        while i < n and int(rec[1 + i]) == m:
            s = s + np.float64(bank[1 + i]) / count
            share += 1
            i += 1
        ms.append(m)
        ts.append(s / np.float64(share))
    return ms, ts


def landmark_table(row, rec, bank, n, clip=False):
    """fp32 [65536] and the meta record: the piecewise-linear map through the knots, extrapolating at both ends."""
    row = np.asarray(row, dtype=np.int64)
    total = int(row.sum())
    if not np.float64(bank[0]) > 0:
        return np.zeros(NBINS, dtype=np.float32), meta(row, False)
    ms, ts = knots(rec, bank, n)
    if len(ms) < 2:
        y = np.float32(ts[0]) if total else np.float32(0.0)
        return np.full(NBINS, y, dtype=np.float32), meta(row, False)
    m = np.array(ms, dtype=np.int64)
    t = np.array(ts, dtype=np.float64)
    j = np.clip(np.searchsorted(m, VALUES, side="right") - 1, 0, len(ms) - 2)
    frac = (VALUES - m[j]).astype(np.float64) / (m[j + 1] - m[j]).astype(np.float64)
    y = t[j] + frac * (t[j + 1] - t[j])
    if clip:
        y = np.minimum(np.maximum(y, t[0]), t[-1])
    return y.astype(np.float32), meta(row, total > 0)


def default_bank(scan_rows, quantiles=DEFAULT_Q, s_lo=0.0, s_hi=1.0):
    """The bank learnt from the rows in order (float64 [17])."""
    bank = np.zeros(LM_WORDS, dtype=np.float64)
    for row in scan_rows:
        bank = bank_add(bank, landmarks(row, quantiles), len(quantiles), s_lo, s_hi)
    return bank
