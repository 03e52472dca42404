"""Float64 restatement of the window-attention kernels from their OPERANDS, and operand builders whose softmax is exact.

The kernels (include/mivp.h: mivp_win_attn_fwd / _bwd_dq / _bwd_dkv / _bwd_fused / _bwd_prompt / _fwd_fp8) are pure
functions of ``q, k, v, kp, vp, qa, ka, tok_rid, mask_words, cut_flags`` and the descriptor.  Conventions restated here:

* logits in log2 units, ``S = q . k' + qa . ka`` (k, kp and ka are stored multiplied by log2 e);
* the shift mask MULTIPLIES the logit by 0 (swin_block.py:187-200): query class = region id (0 for rows >= Nq), key class =
  region id for content keys, 254 for prompt keys and key rows >= Nq (never masked; padding keys leave through their bias);
* ``lse`` in natural log; ``dq`` w.r.t. the stored, pre-scaled q (hence a factor ln 2 on ``dS k'``); ``dk`` / ``dkp_part`` w.r.t.
  the un-scaled k; ``dkp_part`` / ``dvp_part`` / ``dtok_part`` per (window, head); ``dka_part`` as ``[.., Nkp, 32]``;
* dropout through an explicit keep mask (1 = kept) and the scale of the descriptor.

Exact operands (``build_case``).  Every key j carries the bits of its own row index as +-1 entries of K' (``code columns``,
some in the head dims, some in the bias columns), a query carries ``g`` times the bits of the key it selects (0 on the
bits it does not care about), one constant-1 query column meets a per-key offset ``b`` (and the padding bias), and in
shifted blocks one more column of magnitude 12 g separates the two region groups of a window so that every masked key
of the other group has a raw logit at least 6 * 2 g above the winner (a decoy the mask must remove).  Then in every row a
set W of 2^m keys holds the integer logit L and every other key -- masked ones at logit 0 and padding keys included -- sits
at least 32 below (asserted; 2 g = 36 by construction -- nine neighbours at - 32 would already hold 2^-29 of the mass): P is 1 on W and absorbed elsewhere for any reference point and summation order, and ``o`` is
the mean of v over W, a bf16 number.  ``Case.check()`` asserts the preconditions (a)-(d) of DESIGN.md 5.2 on every row.
"""
import itertools
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

F64 = torch.float64
LN2 = math.log(2.0)
PAD_BIAS = -43264.0            # bf16 value next to -30000 log2 e (what mivp_relbias_aug stores for padding key rows)


def r16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def is_bf16(t):
    return bool((r16(t) == t).all())


def is_e4m3(t):
    """Every element is an E4M3 (fn) number: |x| <= 448, four significant bits, a multiple of 2^-9."""
    m, _ = torch.frexp(t)
    return bool(((t.abs() <= 448) & ((m * 16) == (m * 16).round()) & ((t * 512) == (t * 512).round())).all())


def near_bf16(t, rel=2.0 ** -20):
    """Precondition (c): the reference is a bf16 number up to the absorbed terms (or below bf16's range, i.e. zero)."""
    t0 = torch.where(t.abs() < 2.0 ** -140, torch.zeros_like(t), t)
    return bool(((r16(t0) - t0).abs() <= rel * t0.abs()).all())


def round_up(v, m):
    return (v + m - 1) // m * m


@dataclass
class Case:
    name: str
    B: int
    P: int
    heads: int
    hd: int
    Nq: int
    Nqp: int
    Np: int
    Npp: int
    Nkp: int
    aug: int
    augp: int
    win: tuple
    has_mask: bool
    q: torch.Tensor                   # f64 [BP, heads, Nqp, hd]
    k: torch.Tensor                   # stored k' (log2 units)
    v: torch.Tensor
    kp: Optional[torch.Tensor]        # [heads, Npp, hd]
    vp: Optional[torch.Tensor]
    qa: torch.Tensor                  # [Nqp, augp]
    ka: torch.Tensor                  # [heads, Nkp, augp]
    rid: np.ndarray                   # int32 [P, Nqp]
    L: Optional[torch.Tensor] = None  # [BP, heads, Nq] the winners' logit
    nwin: Optional[torch.Tensor] = None   # [BP, heads, Nq] |W|
    walk: str = "optimistic"
    fp8: bool = False
    extra: dict = field(default_factory=dict)

    @property
    def BP(self):
        return self.B * self.P

    @property
    def C(self):
        return self.heads * self.hd

    # ---- the reference ----
    def live(self):
        """[P, Nqp, Nkp] bool: the logit survives the multiplicative mask (class compare)."""
        if "live" in self.extra:                                          # (tests: a corrupted mask)
            return self.extra["live"]
        if not self.has_mask:
            return None
        rid = torch.from_numpy(self.rid.astype(np.int64))
        slot = torch.arange(self.Nqp)
        qcls = torch.where(slot[None] < self.Nq, rid, torch.zeros_like(rid))
        kcls = torch.full((self.P, self.Nkp), 254, dtype=torch.int64)
        kcls[:, :self.Nqp] = torch.where(slot[None] < self.Nq, rid, torch.full_like(rid, 254))
        return (kcls[:, None, :] == 254) | (kcls[:, None, :] == qcls[:, :, None])

    def keys(self):
        K = torch.zeros((self.BP, self.heads, self.Nkp, self.hd), dtype=F64)
        V = torch.zeros_like(K)
        K[:, :, :self.Nqp] = self.k
        V[:, :, :self.Nqp] = self.v
        if self.Np:
            K[:, :, self.Nqp:self.Nqp + self.Npp] = self.kp[None]
            V[:, :, self.Nqp:self.Nqp + self.Npp] = self.vp[None]
        return K, V

    def raw_logits(self):
        K, _ = self.keys()
        return self.q @ K.transpose(-1, -2) + (self.qa @ self.ka.transpose(-1, -2))[None]

    def logits(self):
        S = self.raw_logits()
        lv = self.live()
        if lv is not None:
            S = S * lv.repeat(self.B, 1, 1)[:, None].to(F64)
        return S

    def forward(self, keep=None, scale=1.0):
        """-> o [BP, Nqp, C], lse [BP, heads, Nqp] (natural log), P [BP, heads, Nqp, Nkp]."""
        S = self.logits()
        m = S.amax(dim=-1, keepdim=True)
        e = torch.exp2(S - m)
        den = e.sum(dim=-1, keepdim=True)
        Pm = e / den
        lse = (m + torch.log2(den)).squeeze(-1) * LN2
        _, V = self.keys()
        Pd = Pm if keep is None else Pm * keep.to(F64) * scale
        o = (Pd @ V).permute(0, 2, 1, 3).reshape(self.BP, self.Nqp, self.C)
        return o, lse, Pm

    def backward(self, d_o, keep=None, scale=1.0):
        """Autograd of ``forward`` for dO [BP, Nqp, C] (rows >= Nq must be zero).  Returns a dict of float64 tensors laid out
        as the kernels write them."""
        K, V = self.keys()
        o, lse, Pm = self.forward(keep, scale)
        dO = d_o.reshape(self.BP, self.Nqp, self.heads, self.hd).permute(0, 2, 1, 3)
        oh = o.reshape(self.BP, self.Nqp, self.heads, self.hd).permute(0, 2, 1, 3)
        delta = (dO * oh).sum(-1)                                        # [BP, heads, Nqp]
        drop = 1.0 if keep is None else keep.to(F64) * scale
        dP = (dO @ V.transpose(-1, -2)) * drop
        dS = Pm * (dP - delta[..., None])                                # w.r.t. the natural-log logit
        lv = self.live()
        if lv is not None:
            dS = dS * lv.repeat(self.B, 1, 1)[:, None].to(F64)
        rows = (torch.arange(self.Nqp) < self.Nq).to(F64)[None, None, :, None]
        dSk = dS * rows                                                  # key-side sums run over the valid query rows
        Pk = Pm * drop * rows
        dK = dSk.transpose(-1, -2) @ self.q                              # [BP, heads, Nkp, hd]
        dV = Pk.transpose(-1, -2) @ dO
        out = dict(delta=delta, dq=(dS @ K) * LN2, dk=dK[:, :, :self.Nqp], dv=dV[:, :, :self.Nqp], dS=dS)
        dka = torch.zeros((self.BP, self.heads, self.Nkp, 32), dtype=F64)
        dka[..., :self.augp] = dSk.transpose(-1, -2) @ self.qa
        out["dka_part"] = dka
        if self.Np:
            sl = slice(self.Nqp, self.Nqp + self.Npp)
            out["dkp_part"], out["dvp_part"] = dK[:, :, sl], dV[:, :, sl]
            out["dtok_part"] = dSk.sum(dim=2)[:, :, sl]
        return out

    # ---- preconditions (a)-(d), on every row, before any kernel output is looked at ----
    def check(self, equality=True):
        ops = [self.q, self.k, self.v, self.qa, self.ka] + ([self.kp, self.vp] if self.Np else [])
        for t in ops:                                                     # (a)
            assert is_e4m3(t) if self.fp8 else is_bf16(t), self.name
        S = self.logits()[:, :, :self.Nq]
        top = S.amax(dim=-1, keepdim=True)
        W = S == top
        assert bool((top.squeeze(-1) == self.L).all()) and bool((W.sum(-1) == self.nwin).all()), self.name
        assert bool((S == S.round()).all()), self.name
        other = torch.where(W, torch.full_like(S, -1e9), S)
        assert bool((other.amax(-1) <= self.L - 32).all()), self.name    # every other key at least 32 log2 units below
        mass = torch.exp2(other - top).sum(-1) / self.nwin                # (b): the losers' share, relative to the winners'
        assert bool((mass <= 2.0 ** -30).all()), (self.name, float(mass.max()))
        if equality:
            o, _, _ = self.forward()
            assert near_bf16(o[:, :self.Nq]), self.name                  # (c)
        if self.extra.get("mode") == "route" and self.extra.get("carried") is None:
            missing = {kk: vv for kk, vv in self.coverage().items() if vv}
            assert not missing, (self.name, missing)
        elif self.extra.get("mode") == "tie":
            self.check_tie_spread(W)
        if self.walk == "optimistic":                                     # (d): the row sum 2^L |W| stays inside [2^-100, 2^100)
            assert bool((self.L.abs() <= 90).all()), self.name
        elif self.walk == "tested":
            assert bool((self.L >= 130).all()), self.name
        return self                                                       # (walk "any": dropout calls never take the zero-reference walk)


    def coverage(self):
        """Routing cases: per (batch, window), the selectable keys of each class that NO row of any head selects.  Classes:
        every content key, every prompt key, the first and last key of every 16- and 32-key tile, and the live keys on both
        sides of the Nq | padding | prompt boundaries (Nq - 1, the first and the last prompt key)."""
        sel, live = self.extra["sel"], self.extra["live_sel"]
        j = np.arange(self.Nkp)
        edge = [e for e in (self.Nq - 1, self.Nqp, self.Nqp + self.Np - 1) if e < self.Nkp]
        classes = {"content": live & (j < self.Nq), "prompt": live & (j >= self.Nqp),
                   "tile16": live & np.isin(j % 16, (0, 15)), "tile32": live & np.isin(j % 32, (0, 31)),
                   "boundary": live & np.isin(j, edge)}
        out = {}
        for bp in range(self.BP):
            hit = np.zeros(self.Nkp, bool)
            hit[sel[bp].reshape(-1)] = True
            for kk, need in classes.items():
                miss = np.nonzero(need & ~hit)[0]
                if miss.size:
                    out.setdefault(kk, []).append((bp, miss.tolist()))
        return out

    def check_tie_spread(self, W):
        """Tie cases: some winner set spans different 16-key tiles, winners fall in the first and the last live key tile,
        and both content and prompt keys take part in ties."""
        tied = W & (self.nwin[..., None] > 1)
        keys = tied.reshape(-1, self.Nkp).any(0).numpy()
        live = self.extra["live_sel"]
        first, last = np.nonzero(live)[0][[0, -1]] // 16
        j = np.arange(self.Nkp)
        assert keys[j // 16 == first].any() and keys[j // 16 == last].any(), self.name
        assert keys[:self.Nq].any() and (not self.Np or keys[self.Nqp:].any()), self.name
        tiles = tied.reshape(*tied.shape[:-1], self.Nkp // 16, 16).any(-1)
        assert bool((tiles.sum(-1) > 1).any()), self.name


# ------------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------------
def _spaced(lo, hi, n):
    """n distinct column indices spread over [lo, hi) ending at hi - 1."""
    assert hi - lo >= n
    if n == 0:
        return []
    if n == 1:
        return [hi - 1]
    return [lo + (i * (hi - 1 - lo)) // (n - 1) for i in range(n)]


def v_ids(count, hd, base, first=0):
    """[count, hd] integers in [1, base) naming ``first + i``: digits (+ 1: a zero channel would leave the absorbed keys'
    2^-36 share as the whole value) in the leading channels, then a running check digit in every further channel."""
    ids = torch.arange(first, first + count, dtype=torch.int64)
    nd = min(hd, 6)
    nb = base - 1
    assert first + count <= nb ** nd
    out = torch.zeros((count, hd), dtype=torch.int64)
    for c in range(hd):
        out[:, c] = 1 + ((ids // nb ** c) % nb if c < nd else (ids * (2 * c + 1) + c) % nb)
    return out.to(F64)


def build_case(name, rid, P, Nq, win, B, heads, hd, Np, mode="route", g=18, L0=None, walk="optimistic", fp8=False,
               vbase=32, seed=0, carried=None):
    """``rid``: int32 [P, Nqp] region ids or None (un-shifted block).  ``mode``: "route" (|W| = 1) or "tie" (|W| in
    {1, 2, 4, 8} cycling over the rows).  ``L0``: the winners' logit of a routing row (a tie over 2^m keys sits g m lower).
    ``walk`` = "tested": the keys of the first 32-key step sit far below zero and are never selected, L0 >= 130.
    ``carried``: a region id of a one-window table.  Rows of every OTHER region get -40 on every surviving key (own region,
    prompt keys), so the masked keys of region ``carried`` -- at logit exactly 0 through the multiplicative mask -- carry
    the row: |W| = the size of that region, L = 0.  Rows of region ``carried`` route as usual.  There is no region-group
    column in such a case, and v of the carrying keys is 1..3 so that their sum fits 8 bits and the mean is a bf16 number."""
    assert carried is None or (rid is not None and P == 1)
    rng = np.random.RandomState(seed)
    if L0 is None:                                             # ties sit g m lower: 90, 72, 54, 36 (316 masked keys at 0 against 8 winners: 2^-30.7)
        L0 = 184 if walk == "tested" else (90 if mode == "tie" else 64)
    Nqp = round_up(Nq, 16)
    Npp = round_up(Np, 16) if Np else 0
    Nkp = round_up(Nqp + Npp, 32)
    aug = win[0] + win[1] + win[2] - 1
    augp = round_up(aug, 4)
    has_mask = rid is not None
    BP = B * P
    nbits = max(1, (Nkp - 1).bit_length())
    nhd_cols = hd - (1 if has_mask else 0)                     # the last head dim is the region-group column
    a = max(nbits - nhd_cols, min(3, augp - 1, nbits - 1))     # bits [0, a) sit in the bias columns, [a, nbits) in the head dims
    assert a <= augp - 1 and nbits - a <= nhd_cols
    col_hd = _spaced(0, nhd_cols, nbits - a)                   # head-dim column of bit a + i
    col_aug = _spaced(1, augp, a)                              # bias column of bit i (column 0 is the constant one)
    live_key = np.zeros(Nkp, bool)
    live_key[:Nq] = True
    live_key[Nqp:Nqp + Np] = True
    if walk == "tested":
        live_sel = live_key.copy()
        live_sel[:32] = False
    else:
        live_sel = live_key
    ridn = None if rid is None else np.asarray(rid).reshape(P, Nqp)
    # region groups (+-1) of every content key of every window: regions ranked by id, alternating
    grp = np.ones((P, Nqp), np.int64)
    if has_mask:
        for p in range(P):
            ids = np.unique(ridn[p, :Nq])
            rank = np.searchsorted(ids, ridn[p, :Nq])
            grp[p, :Nq] = 1 - 2 * (rank & 1)
    keybits = ((np.arange(Nkp)[:, None] >> np.arange(nbits)[None]) & 1) * 2 - 1       # [Nkp, nbits] +-1

    # ---- pick the winners of every (work item, row): low bits from the row, high bits rotate with the work item ----
    nhi = (Nkp + (1 << a) - 1) >> a
    tie_masks = {m: [] for m in range(4)}
    hib = list(range(a, nbits))
    tie_masks[0] = [0]
    for m in (1, 2, 3):
        for comb in itertools.combinations(reversed(hib), m):
            tie_masks[m].append(sum(1 << b for b in comb))
    sel = np.zeros((BP, heads, Nq), np.int64)
    care = np.zeros((BP, heads, Nq), np.int64)                 # bit mask of the cared-for bits
    mlog = np.zeros((BP, heads, Nq), np.int64)
    full = (1 << nbits) - 1
    # single selections: a row may only select keys that share its low ``a`` bits (the bias columns are shared by every work
    # item) and, in a cut window, its region (or a prompt key).  Within each (low bits, region) class the rows are rotated
    # over the class's own content keys -- a permutation, so every work item of an even head covers every selectable content
    # key of its window -- and in the odd heads a rotating set of rows of each low-bits class takes that class's prompt keys.
    lowmask = (1 << a) - 1
    prompts_c = [[j for j in range(Nqp, Nqp + Np) if (j & lowmask) == c and live_sel[j]] for c in range(1 << a)]
    rows_c = [[n for n in range(Nq) if (n & lowmask) == c] for c in range(1 << a)]
    idx_c = {n: i for c in range(1 << a) for i, n in enumerate(rows_c[c])}
    single = []
    for p in range(P):
        reg = ridn[p, :Nq] if has_mask else np.zeros(Nq, np.int64)
        rows_cr, keys_cr, idx_cr = {}, {}, {}
        for n in range(Nq):
            key = (n & lowmask, int(reg[n]))
            idx_cr[n] = len(rows_cr.setdefault(key, []))
            rows_cr[key].append(n)
            if live_sel[n]:
                keys_cr.setdefault(key, []).append(n)
        single.append((reg, keys_cr, idx_cr))

    def pick_single(bp, h, n):
        reg, keys_cr, idx_cr = single[bp % P]
        c = n & lowmask
        S = keys_cr.get((c, int(reg[n])), [])
        Pc = prompts_c[c]
        slot = (idx_c[n] + bp) % len(rows_c[c])
        if Pc and (h & 1 or not S) and (slot < len(Pc) or not S):
            return Pc[slot % len(Pc)]
        assert S, (name, bp, h, n)
        return S[(idx_cr[n] + bp * heads + h) % len(S)]

    for bp in range(BP):
        p = bp % P
        for h in range(heads):
            bph = bp * heads + h
            for n in range(Nq):
                if carried is not None and ridn[p, n] != carried:      # a row carried by its masked keys selects nothing
                    care[bp, h, n] = 0
                    continue

                def ok(j):
                    return j < Nkp and live_sel[j] and (not has_mask or j >= Nq or ridn[p, j] == ridn[p, n])
                want = (n + bph) % 4 if mode == "tie" else 0
                done = False
                for m in range(want, 0, -1):
                    masks = tie_masks[m]
                    for t in range(nhi * max(1, min(len(masks), 6))):
                        hi = ((n >> a) + 5 * bph + t) % nhi
                        j0 = (hi << a) | (n & lowmask)
                        M = masks[(n + t) % len(masks)]
                        members = [j0 ^ s for s in _subsets(M)]
                        if all(ok(j) for j in members):
                            sel[bp, h, n], care[bp, h, n], mlog[bp, h, n] = j0, full & ~M, m
                            done = True
                            break
                    if done:
                        break
                if not done:
                    sel[bp, h, n], care[bp, h, n], mlog[bp, h, n] = pick_single(bp, h, n), full, 0

    # ---- operands ----
    q = torch.zeros((BP, heads, Nqp, hd), dtype=F64)
    k = torch.zeros((BP, heads, Nqp, hd), dtype=F64)
    qa = torch.zeros((Nqp, augp), dtype=F64)
    ka = torch.zeros((heads, Nkp, augp), dtype=F64)
    kp = torch.zeros((heads, Npp, hd), dtype=F64) if Np else None
    selbits = keybits[sel]                                     # [BP, heads, Nq, nbits]
    cared = (care[..., None] >> np.arange(nbits)) & 1
    qdir = torch.from_numpy(selbits * cared * g).to(F64)
    kb = torch.from_numpy(keybits).to(F64)
    for i, c in enumerate(col_hd):
        q[:, :, :Nq, c] = qdir[..., a + i]
        k[:, :, :Nq, c] = kb[:Nq, a + i]
        if Np:
            kp[:, :Np, c] = kb[Nqp:Nqp + Np, a + i]
    for i, c in enumerate(col_aug):
        # the bias columns are shared by every work item: their bits depend on the row alone (by construction of sel)
        assert bool((qdir[..., i] == qdir[:1, :1, :, i]).all()), name
        qa[:Nq, c] = qdir[0, 0, :, i]
        ka[:, :, c] = kb[:, i]
    X = 0 if carried is not None else 12 * g                   # region-group column: other-group keys rise by X, own-group keys sink by X
    if has_mask and X:
        for bp in range(BP):
            p = bp % P
            q[bp, :, :Nq, hd - 1] = torch.from_numpy(grp[p, :Nq] * X).to(F64)[None]
            k[bp, :, :Nq, hd - 1] = torch.from_numpy(-grp[p, :Nq]).to(F64)[None]
    # spare head-dim columns: values that meet a zero on the other side (a shifted column would let them in)
    used = set(col_hd) | ({hd - 1} if has_mask else set())
    for c in range(hd):
        if c in used:
            continue
        if c & 1:
            k[:, :, :Nq, c] = torch.from_numpy(rng.randint(-3, 4, size=(BP, heads, Nq))).to(F64)
            if Np:
                kp[:, :Np, c] = torch.from_numpy(rng.randint(-3, 4, size=(heads, Np))).to(F64)
        else:
            q[:, :, :Nq, c] = torch.from_numpy(rng.randint(-3, 4, size=(BP, heads, Nq))).to(F64)
    for c in range(1, augp):
        if c in col_aug:
            continue
        if c & 1:
            ka[:, :, c] = torch.from_numpy(rng.randint(-3, 4, size=(heads, Nkp))).to(F64)
        else:
            qa[:Nq, c] = torch.from_numpy(rng.randint(-3, 4, size=(Nq,))).to(F64)
    # constant column: offset of every live key, the padding bias elsewhere.  A routing row has logit g nbits + b (own-group
    # content keys: - X with the region column; prompt keys do not take part in it, so they carry the - X in their offset).
    qa[:Nq, 0] = 1.0
    b = L0 - g * nbits + (X if has_mask else 0)
    off = torch.full((Nkp,), float(b), dtype=F64)
    if has_mask:
        off[Nqp:] -= X
    if walk == "tested":
        off[:32] = -384.0
    ka[:, :, 0] = off[None]
    ka[:, ~torch.from_numpy(live_key), 0] = -448.0 if fp8 else PAD_BIAS
    Lrow = torch.from_numpy(L0 - g * mlog).to(F64)
    nwin = torch.from_numpy(1 << mlog).to(F64)
    if carried is not None:
        # one spare bias column (one window: qa may depend on the row's region) lifts every surviving key of a carried row
        # from its offset b to -40; the carrying keys are the other regions' masked ones
        cs = next(c for c in range(1, augp) if c not in col_aug)
        others = torch.from_numpy(ridn[0, :Nq] != carried)
        ka[:, :, cs] = 1.0
        qa[:Nq, cs] = torch.where(others, torch.full((Nq,), -40.0 - b, dtype=F64), torch.zeros(Nq, dtype=F64))
        q[:, :, :Nq][:, :, others] = 0
        Lrow[:, :, others] = 0.0
        nwin[:, :, others] = float((~others).sum())

    v = torch.zeros((BP, heads, Nqp, hd), dtype=F64)
    v[:, :, :Nq] = v_ids(BP * heads * Nq, hd, vbase).reshape(BP, heads, Nq, hd)
    vp = None
    if Np:
        vp = torch.zeros((heads, Npp, hd), dtype=F64)
        vp[:, :Np] = v_ids(heads * Np, hd, vbase, first=BP * heads * Nq).reshape(heads, Np, hd)
    if carried is not None:
        car = torch.from_numpy(ridn[0, :Nq] == carried)
        v[:, :, :Nq][:, :, car] = 1 + v[:, :, :Nq][:, :, car] % 3
    rid_out = np.zeros((P, Nqp), np.int32) if rid is None else ridn.astype(np.int32)
    case = Case(name=name, B=B, P=P, heads=heads, hd=hd, Nq=Nq, Nqp=Nqp, Np=Np, Npp=Npp, Nkp=Nkp, aug=aug, augp=augp,
                win=tuple(win), has_mask=has_mask, q=q, k=k, v=v, kp=kp, vp=vp, qa=qa, ka=ka, rid=rid_out, L=Lrow,
                nwin=nwin, walk=walk, fp8=fp8)
    case.extra = dict(sel=sel, care=care, mlog=mlog, g=g, X=X if has_mask else 0, a=a, nbits=nbits, mode=mode,
                      live_sel=live_sel, carried=carried)
    return case


def _subsets(M):
    s = M
    out = [0]
    while s:
        out.append(s)
        s = (s - 1) & M
    return out


def winners(case):
    """[BP, heads, Nq, Nkp] bool of the reference's winner sets."""
    S = case.logits()[:, :, :case.Nq]
    return S == S.amax(dim=-1, keepdim=True)


def int_grad(case, seed=1):
    """Integer dO [BP, Nqp, C]: +-1 in one channel per (row, head), zero rows >= Nq -- so that dP - delta times 1 / |W| is a
    bf16 number for v < 32 and |W| <= 8 (the kernels round dS to bf16 before the dq / dk products)."""
    rng = np.random.RandomState(seed)
    d = torch.zeros((case.BP, case.Nqp, case.heads, case.hd), dtype=F64)
    ch = torch.from_numpy(rng.randint(0, case.hd, size=(case.BP, case.Nq, case.heads)))
    sg = torch.from_numpy(rng.randint(0, 2, size=(case.BP, case.Nq, case.heads)) * 2 - 1).to(F64)
    d[:, :case.Nq].scatter_(3, ch[..., None], sg[..., None])
    return d.reshape(case.BP, case.Nqp, case.C)


def synthetic_rid(P, Nq, Nqp, borders):
    """Region ids whose borders fall INSIDE 16-slot tiles: window p cuts its slots at ``borders[p]`` (sorted slot indices)."""
    rid = np.zeros((P, Nqp), np.int32)
    for p in range(P):
        ids = np.searchsorted(np.asarray(borders[p]), np.arange(Nq), side="right")
        rid[p, :Nq] = 3 * ids + p
    return rid


def random_case(name, rid, P, Nq, win, B, heads, hd, Np, seed=0):
    """A realistic block input in kernel-operand form: normal q (pre-scaled), k' and v rounded to bf16, the query one-hots
    and table-valued key columns of mivp_relbias_aug (tables ~ N(0, 0.1)), the padding bias in the w0 query-h columns."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    Nqp, Npp = round_up(Nq, 16), (round_up(Np, 16) if Np else 0)
    Nkp = round_up(Nqp + Npp, 32)
    aug = win[0] + win[1] + win[2] - 1
    augp = round_up(aug, 4)
    BP = B * P
    q = torch.zeros((BP, heads, Nqp, hd), dtype=F64)
    k, v = torch.zeros_like(q), torch.zeros_like(q)
    q[:, :, :Nq] = r16(rn(BP, heads, Nq, hd) * 0.25 * hd ** -0.5)    # logit std 0.25: every weight near 1 / 400
    k[:, :, :Nq] = r16(rn(BP, heads, Nq, hd) / LN2)
    v[:, :, :Nq] = r16(rn(BP, heads, Nq, hd))
    kp = vp = None
    if Np:
        kp, vp = torch.zeros((heads, Npp, hd), dtype=F64), torch.zeros((heads, Npp, hd), dtype=F64)
        kp[:, :Np], vp[:, :Np] = r16(rn(heads, Np, hd) / LN2), r16(rn(heads, Np, hd))
    n = torch.arange(Nq)
    coords = [n // (win[1] * win[2]), (n // win[2]) % win[1], n % win[2]]
    qa = torch.zeros((Nqp, augp), dtype=F64)
    ka = torch.zeros((heads, Nkp, augp), dtype=F64)
    base = 0
    for a in range(3):
        width = win[a] if a < 2 else win[a] - 1
        tab = rn(heads, 2 * win[a] - 1) * 0.1 / LN2
        for i in range(width):
            qa[:Nq, base + i] = (coords[a] == i).to(F64)
            ka[:, :Nq, base + i] = tab[:, coords[a] - i + win[a] - 1]
        base += width
    if Np:
        ka[:, Nqp:Nqp + Np, :win[0]] = (rn(heads, Np) * 0.1 / LN2)[..., None]
    ka = r16(ka)
    ka[:, Nq:Nqp, :win[0]] = PAD_BIAS
    ka[:, Nqp + Np:, :win[0]] = PAD_BIAS
    has_mask = rid is not None
    rid_out = np.zeros((P, Nqp), np.int32) if rid is None else np.asarray(rid).reshape(P, Nqp).astype(np.int32)
    return Case(name=name, B=B, P=P, heads=heads, hd=hd, Nq=Nq, Nqp=Nqp, Np=Np, Npp=Npp, Nkp=Nkp, aug=aug, augp=augp,
                win=tuple(win), has_mask=has_mask, q=q, k=k, v=v, kp=kp, vp=vp, qa=qa, ka=ka, rid=rid_out)
