"""Python-integer restatement of the Otsu foreground threshold of mivp_amd.scanstats, with a mask helper and
a restricted-window helper built on tests/scanstats_ref.py.

Per channel, from ``table[v + 32768] = n_v``: ``N = sum n_v``, ``S = sum v n_v``.  A candidate ``t`` is a counted value that
is not the largest counted value; ``n0 = sum_{v<=t} n_v``, ``A = sum_{v<=t} v n_v``, ``P = A N - S n0``, ``q = n0 (N - n0)``.
The threshold maximises ``P^2 / q`` (the between-class variance is ``P^2 / (N^2 q)``), candidates compared by the integers
``P_a^2 q_b`` and ``P_b^2 q_a``, equal values picking the lower ``t``.  Fewer than two distinct counted values, ``N == 0`` or
``N >= 2^33``: no threshold (``valid = 0``, ``t`` = the largest counted value or 0, ``n_le = N``, ``n_gt = 0``)."""
from fractions import Fraction

import numpy as np

import scanstats_ref as R

NBINS, OFFSET = R.NBINS, R.OFFSET


def otsu(row):
    """One channel's table (65536 counts) -> ((t, n_le, n_gt, valid), the largest bit length of a compared product)."""
    row = np.asarray(row).reshape(-1)
    assert row.size == NBINS
    occ = [(int(b) - OFFSET, int(row[b])) for b in np.flatnonzero(row)]
    N = sum(k for _, k in occ)
    S = sum(v * k for v, k in occ)
    if len(occ) < 2 or N >= 2 ** 33:
        return (occ[-1][0] if occ else 0, N, 0, 0), 0
    best, bits, n0, A = None, 0, 0, 0
    for v, k in occ[:-1]:                                        # the largest counted value is no candidate
        n0 += k
        A += v * k
        P2, q = (A * N - S * n0) ** 2, n0 * (N - n0)
        if best is None:
            best = (P2, q, v, n0)
            continue
        lhs, rhs = P2 * best[1], best[0] * q
        bits = max(bits, lhs.bit_length(), rhs.bit_length())
        if lhs > rhs:                                            # equal: the earlier, lower t stays
            best = (P2, q, v, n0)
    return (best[2], best[3], N - best[3], 1), bits


def otsu_record(table):
    """int64 [C, 4] of a table [C, 65536]: what mivp_scan_otsu_plan writes."""
    return np.array([otsu(row)[0] for row in np.asarray(table)], dtype=np.int64)


def brute_force(row):
    """The lowest counted value that maximises sigma_b^2 = w0 w1 (mu0 - mu1)^2 over ALL 65535 cut points, in Fractions
    (None when no cut point separates two non-empty classes).  A maximum over an empty gap is attained at the counted
    value below the gap as well, so the lowest maximiser that is a counted value is Otsu's threshold."""
    row = [int(k) for k in np.asarray(row).reshape(-1)]
    N = sum(row)
    S = sum((b - OFFSET) * k for b, k in enumerate(row))
    best, best_t, n0, A = None, None, 0, 0
    for b in range(NBINS - 1):                                   # cut after bin b
        n0 += row[b]
        A += (b - OFFSET) * row[b]
        if n0 == 0 or n0 == N:
            continue
        w0, w1 = Fraction(n0, N), Fraction(N - n0, N)
        var = w0 * w1 * (Fraction(A, n0) - Fraction(S - A, N - n0)) ** 2
        if row[b] and (best is None or var > best):
            best, best_t = var, b - OFFSET
        elif best is not None and var > best:                    # an uncounted cut point never beats the counted one below
            raise AssertionError("a cut point in a gap has a larger variance than the counted value below it")
    return best_t


def table_of(pairs):
    """{value: count} -> one channel's int64 table."""
    row = np.zeros(NBINS, dtype=np.int64)
    for v, k in pairs.items():
        row[v + OFFSET] = k
    return row


def mask(raw_c, rec):
    """uint8 [H, W, D]: raw_c > t, all ones when the record is not valid."""
    raw_c = np.asarray(raw_c)
    if not rec[3]:
        return np.ones(raw_c.shape, dtype=np.uint8)
    return (raw_c.astype(np.int64) > int(rec[0])).astype(np.uint8)


def restricted_values(raw_c, above=None, mask=None):
    """The selected values of one channel that lie above the Otsu threshold of their own histogram (all of them when it
    has none): what a window with foreground="otsu" takes its statistics over."""
    v = R.selected(raw_c, mask, above)
    rec, _ = otsu(np.bincount(v + OFFSET, minlength=NBINS))
    return v[v > rec[0]] if rec[3] else v


def big_table():
    """Counts near 2^32 at -32768 and 32767 and a scattered middle: N < 2^33, and the compared products pass 192 bits."""
    rs = np.random.RandomState(41)
    pairs = {-32768: 2 ** 32 - 2 ** 26 - 5, 32767: 2 ** 32 - 2 ** 26 - 11}
    for v in rs.randint(-30000, 30000, size=40):
        pairs[int(v)] = int(rs.randint(1, 2 ** 20))                  # 40 * 2^20 < 2^26: N stays below 2^33
    row = table_of(pairs)
    assert 2 ** 32 < int(row.sum()) < 2 ** 33
    return row
