"""Numpy oracle of what pass 2 and the extract leg of the symmetric path see per entry, and the generators of the tables that
fill their LDS structures -- TEST INFRASTRUCTURE ONLY, held to independent code (oracle/brute.py) and to its promises by
tests/test_pass2_oracle_host.py.  Nothing here knows a constant of the engine: the tests hand the thresholds in.

Pass 1 leaves one code byte per entry: the number of its pairs at positions p >= k // 2 (none, one, several) and, for one,
where the partner is; the look-ups add whether it owns a pair at p < k // 2.  `classify` restates that from the table alone.
"""
from typing import NamedTuple

import numpy as np

from smudgeplot_amd import ktab

SMAX = 1000
REACH = 30                                # a code byte names a partner up to this many entries away


class Classes(NamedTuple):
    s_all: np.ndarray                     # pairs at p >= k // 2
    pre: np.ndarray                       # pairs at p < k // 2
    partner: np.ndarray                   # the partner of the only pair at p >= k // 2, else -1
    pos: np.ndarray                       # where that pair differs, else -1


def classify(packed, counts, k):
    """per entry of a table (packed [n, kbyte], in table order): the pairs it owns on either side of k // 2 -- grouped like
    brute.unique_pairs groups them (the k-mers with base p blanked), the sum limit of 1000 applied"""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n, kb = packed.shape
    cnt = np.asarray(counts).astype(np.int64)
    s_all, pre = np.zeros(n, np.int64), np.zeros(n, np.int64)
    partner, pos = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for p in range(k):
        m = packed.copy()
        m[:, p >> 2] &= np.uint8(~(3 << (6 - 2 * (p & 3))) & 0xFF)
        v = m.view(np.dtype((np.void, kb))).ravel()
        order = np.argsort(v, kind="stable")
        vs = v[order]
        new = np.ones(n, dtype=bool)
        new[1:] = vs[1:] != vs[:-1]
        gid = np.cumsum(new) - 1
        for d in (1, 2, 3):
            same = gid[d:] == gid[:-d]
            a, b = order[:-d][same], order[d:][same]
            ok = cnt[a] + cnt[b] <= SMAX
            a, b = a[ok], b[ok]
            side = s_all if p >= k // 2 else pre
            np.add.at(side, a, 1)
            np.add.at(side, b, 1)
            if p >= k // 2:
                partner[a], partner[b] = b, a
                pos[a], pos[b] = p, p
    partner[s_all != 1] = -1
    pos[s_all != 1] = -1
    return Classes(s_all, pre, partner, pos)


def candidates(c):
    """entries pass 2 queues: one pair at p >= k // 2, none in front, the partner ahead and within the code's reach"""
    d = c.partner - np.arange(len(c.partner))
    return (c.s_all == 1) & (c.pre == 0) & (d > 0) & (d <= REACH)


def far(c):
    """entries whose only pair at p >= k // 2 has its partner ahead and out of the code's reach (whatever `pre` says)"""
    return (c.s_all == 1) & (c.partner - np.arange(len(c.partner)) > REACH)


def counting(c):
    """entries with a partner that has one pair at p >= k // 2 and none in front as well"""
    j = np.where(c.partner >= 0, c.partner, 0)
    return (c.partner >= 0) & (c.s_all[j] == 1) & (c.pre[j] == 0)


def cells(counts, c, mask):
    """(sum, min) of the pairs of the entries in `mask` (which all have a partner)"""
    cnt = np.asarray(counts).astype(np.int64)
    i = np.flatnonzero(mask)
    a, b = cnt[i], cnt[c.partner[i]]
    return a + b, np.minimum(a, b)


def records_of(packed, counts, k, c, labelled):
    """per entry, the records the extract leg stages for it: a counting candidate or far entry without a pair in front,
    on a labelled pixel (labelled: bool [1001, 501], [sum, min]), writes its pair -- and the mirror image of a pair that
    is not its own mirror image"""
    take = (candidates(c) | (far(c) & (c.pre == 0))) & counting(c)
    s, m = cells(counts, c, take)
    i = np.flatnonzero(take)
    nrec = np.zeros(len(c.partner), np.int64)
    nrec[i] = np.where(labelled[s, m], np.where(c.pos[i] != k - 1 - c.pos[i], 2, 1), 0)
    return nrec


# ---- generators -----------------------------------------------------------------------------------------------------

def _forward(rng, n, k):
    """n random k-mers that begin and end with a or c: their complements begin and end with g or t, so after
    ktab.symmetrize the k-mers made here are the first half of the table, in their own order"""
    rows = rng.integers(0, 4, size=(n, k), dtype=np.uint8)
    rows[:, 0] = rng.integers(0, 2, size=n)
    rows[:, k - 1] = rng.integers(0, 2, size=n)
    return rows


def _pairs(rng, n, k):
    """n disjoint pairs that differ at a random position in [k // 2, k - 2] (for odd k that includes the middle position,
    the pair that is its own mirror image): -> (lower members, upper members) [n, k]"""
    x = _forward(rng, n, k)
    p = rng.integers(k // 2, k - 1, size=n)
    y = x.copy()
    r = np.arange(n)
    y[r, p] = (x[r, p] + rng.integers(1, 4, size=n)) & 3
    low = x[r, p] < y[r, p]
    return np.where(low[:, None], x, y), np.where(low[:, None], y, x)


def _finish(bases, counts, k):
    packed, cnt = ktab.sort_unique_packed(ktab.pack_bases(bases), np.asarray(counts).astype(np.uint16))
    packed, cnt = ktab.symmetrize(packed, cnt, k)
    return packed, cnt.astype(np.uint16)


def star_pair_table(k, n_star, m, n_pair, seed, cnt_lo, cnt_hi, fixed=None, extra=None):
    """A table whose first half is dense in queue candidates: n_star star families -- a centre and m leaves, each leaf at a
    position of its own in [k // 2, k - 2] with a smaller base than the centre's, so that it stands in front of the centre,
    has the centre for its only partner and is a candidate that does not count (the centre owns m pairs) -- and n_pair
    disjoint pairs, whose lower members are candidates that count.  Counts uniform in [cnt_lo, cnt_hi).
    fixed = (a, b): the disjoint pairs carry these two counts instead (one pixel of the plot takes them all);
    extra = (pairs, pixels, s_lo): that many more disjoint pairs, on about `pixels` random pixels with sum >= s_lo."""
    rng = np.random.default_rng(seed)
    lo, span = k // 2, k - 1 - k // 2
    assert m <= span
    centre = _forward(rng, n_star, k)
    r = np.arange(n_star)[:, None]
    at = np.argsort(rng.random((n_star, span)), axis=1)[:, :m] + lo
    cb = rng.integers(1, 4, size=(n_star, m))
    centre[r, at] = cb
    leaves = np.repeat(centre[:, None, :], m, axis=1)
    leaves[r, np.arange(m)[None, :], at] = np.floor(rng.random((n_star, m)) * cb).astype(np.uint8)
    n_extra = extra[0] if extra else 0
    pa, pb = _pairs(rng, n_pair + n_extra, k)
    bases = np.concatenate([centre, leaves.reshape(-1, k), pa, pb])
    counts = rng.integers(cnt_lo, cnt_hi, size=len(bases))
    ca, cb2 = counts[-2 * len(pa): -len(pa)], counts[-len(pa):]             # (views: the pairs' lower and upper members)
    if fixed:
        ca[:n_pair], cb2[:n_pair] = fixed
    if extra:
        s = rng.integers(extra[2], SMAX + 1, size=extra[1])
        mn = (1 + np.floor(rng.random(extra[1]) * (s // 2))).astype(np.int64)
        pick = rng.integers(0, extra[1], size=n_extra)
        swap = rng.random(n_extra) < 0.5
        ca[n_pair:] = np.where(swap, mn[pick], s[pick] - mn[pick])
        cb2[n_pair:] = np.where(swap, s[pick] - mn[pick], mn[pick])
    return _finish(bases, counts, k)


def far_flag_families(k, seed):
    """Far entries on either side of the look-ups' flag: 12 blocks of 300 .. 600 k-mers that share their first k // 2 + 1
    bases and have random tails (one window block each, far longer than a code byte reaches).  45 pairs per block differ
    at position k // 2 + 1 with the bases a and t, the first free one: the members stand at opposite ends of their block.
    A third of the lower members own a one-base variant at a position < k // 2 as well, another third of the upper members
    do, the last third of the pairs count.  Some counts beyond the sum limit, a random background."""
    rng = np.random.default_rng(seed)
    share = k // 2 + 1
    rows = []
    for f in range(12):
        size = int(rng.integers(300, 601))
        base = rng.integers(0, 4, k, dtype=np.uint8)
        base[0], base[1] = f & 3, f >> 2                        # (a leading 2-mer of its own: one block, one bucket)
        fam = np.tile(base, (size, 1))
        fam[:, share:] = rng.integers(0, 4, (size, k - share), dtype=np.uint8)
        var = []
        for j in range(45):
            fam[2 * j, share] = 0
            fam[2 * j + 1] = fam[2 * j]
            fam[2 * j + 1, share] = 3
            if j % 3 < 2:
                v = fam[2 * j + j % 3].copy()
                q = int(rng.integers(0, k // 2))
                v[q] = (v[q] + rng.integers(1, 4)) & 3
                var.append(v)
        rows += [fam, np.array(var)]
    rows.append(rng.integers(0, 4, (3000, k), dtype=np.uint8))
    bases = np.concatenate(rows)
    counts = rng.integers(5, 60, size=len(bases))
    counts[rng.random(len(counts)) < 0.04] = 700                # (two such counts exceed the sum limit)
    return _finish(bases, counts, k)


EDGE_CELLS = [(1000, 500), (1000, 499), (999, 499), (1000, 1)]
BEYOND = [(500, 501), (501, 501)]                               # sums 1001 and 1002: no pixel of the plot


def every_cell_table(k, seed, s_full):
    """1 + (7 s + m) % 3 disjoint pairs with the counts (m, s - m) for every pixel 2 <= s <= s_full, 1 <= m <= s // 2; one pair
    on each of EDGE_CELLS, the corners of the plot; one with each of the count pairs BEYOND, which must not appear.
    -> (packed, counts, planted), planted = the (sum, min, pairs) rows of what was planted"""
    rng = np.random.default_rng(seed)
    planted = [(s, m, 1 + (7 * s + m) % 3) for s in range(2, s_full + 1) for m in range(1, s // 2 + 1)]
    planted += [(s, m, 1) for s, m in EDGE_CELLS]
    lo = np.concatenate([np.full(c, m) for s, m, c in planted] + [[a for a, b in BEYOND]])
    hi = np.concatenate([np.full(c, s - m) for s, m, c in planted] + [[b for a, b in BEYOND]])
    pa, pb = _pairs(rng, len(lo), k)
    swap = rng.random(len(lo)) < 0.5
    counts = np.concatenate([np.where(swap, lo, hi), np.where(swap, hi, lo)])
    packed, cnt = _finish(np.concatenate([pa, pb]), counts, k)
    return packed, cnt, np.array(planted, dtype=np.int64)


def staged_flushes(nrec, grid, tpb, stage):
    """The extract leg's staging, replayed: `grid` workgroups of `tpb` threads take one entry per thread and round, stage the
    records of their entries (nrec, from records_of) and write them out once another round might not fit the `stage`
    records of the buffer, and after the last round.  -> (flushes before a workgroup's last round, the most records
    a workgroup ever held)"""
    n = len(nrec)
    step = grid * tpb
    rounds = -(-n // step)
    pad = np.zeros(rounds * step, np.int64)
    pad[:n] = nrec
    per = pad.reshape(rounds, grid, tpb).sum(axis=2)
    have = np.zeros(grid, np.int64)
    early, most = 0, 0
    for rd in range(rounds):
        have += per[rd]
        most = max(most, int(have.max()))
        full = have + 2 * tpb > stage
        if rd + 1 < rounds:
            early += int((full & (have > 0)).sum())
        have[full] = 0
    return early, most
