"""Numpy oracle of what the kernels of three-word k-mers (k = 65 .. 85: kf_pass1<3>, kf_filter<4>, the routing kernels, kf_apply<3> /
kf_apply_indexed<3>, kf_pass2_farscan<3>, kf_extract<3>) hand from one to the next, and the generators of the tables that put known
entries where those kernels change regime -- TEST INFRASTRUCTURE ONLY, held to independent code (oracle/brute.py) and to its promises
by tests/test_wide_oracle_host.py.  Nothing here knows a constant of the engine: the callers hand in engine.wide_limits().

Per entry x of a closed table, with pairs = k-mers of the table one base away whose counts sum to at most 1000:
  s_all  pairs at p >= k // 2          pre   pairs at p < k // 2          (tests/pass2_oracle.classify)
  mid    pairs at the middle position of an odd k (p == k - 1 - p: the pair is its own mirror image)
  s_hi   s_all - mid: pairs at p >= k // 2 that are not their own mirror image -- x then tells rc(x), which owns the mirror image
         on its prefix side, by a request record (rc(x) as three words, count | (s_hi > 0) << 16).
"""
import functools
from typing import NamedTuple

import numpy as np

import brute
import lookup_oracle as lo
import pass2_oracle as po
from smudgeplot_amd import ktab, synth

U = np.uint64
A, C, G, T = 0, 1, 2, 3
KS = (65, 66, 85)
SMAX = 1000
BLOCK = 40                                # entries of a seam block
LADDER = (31, 32, 33, 34, 63, 64, 65, 66, 128, 129, 130)
FAR_STEPS = (0, 1, 2)                     # distances reach + 0, 1, 2 of the pairs inside a ladder block


class Wide(NamedTuple):
    k: int
    packed: np.ndarray
    cnt: np.ndarray
    words: np.ndarray                     # uint64[n, 3], left aligned
    cls: po.Classes
    mid: np.ndarray
    s_hi: np.ndarray
    plot: np.ndarray                      # brute.hetmers_plot


def mid_pairs(packed, counts, k):
    """per entry: its pairs at the middle position of an odd k (none where k is even)"""
    n = len(counts)
    out = np.zeros(n, np.int64)
    if k % 2 == 0:
        return out
    p = k // 2
    cnt = np.asarray(counts).astype(np.int64)
    m = np.ascontiguousarray(packed, dtype=np.uint8).copy()
    m[:, p >> 2] &= np.uint8(~(3 << (6 - 2 * (p & 3))) & 0xFF)
    _, gid = np.unique(m, axis=0, return_inverse=True)
    gid = np.asarray(gid).ravel()
    order = np.argsort(gid, kind="stable")
    g = gid[order]
    for d in (1, 2, 3):
        same = g[d:] == g[:-d]
        a, b = order[:-d][same], order[d:][same]
        ok = cnt[a] + cnt[b] <= SMAX
        np.add.at(out, a[ok], 1)
        np.add.at(out, b[ok], 1)
    return out


def analyse(packed, cnt, k):
    cls = po.classify(packed, cnt, k)
    mid = mid_pairs(packed, cnt, k)
    t = Wide(k, packed, cnt, lo.packed_to_words(packed, k), cls, mid, cls.s_all - mid, brute.hetmers_plot(packed, cnt, k))
    for a in (t.packed, t.cnt, t.words, t.mid, t.s_hi, t.plot, *t.cls):
        a.setflags(write=False)
    return t


# ---- what the kernels hand on ------------------------------------------------------------------------------------------------

def emitted_rows(t, exact):
    """the request list of pass 1, sorted: every entry under the exact proof, the entries with s_hi > 0 under the hash proof"""
    send = np.ones(len(t.cnt), bool) if exact else t.s_hi > 0
    rc = lo.packed_to_words(ktab.revcomp_packed(t.packed, t.k), t.k)
    meta = t.cnt.astype(U) | ((t.s_hi > 0).astype(U) << U(16))
    return lo.sort_rows(np.concatenate([rc, meta[:, None]], axis=1)[send])


def senders_per_tile(t, exact, tile):
    send = np.ones(len(t.cnt), bool) if exact else t.s_hi > 0
    ntiles = -(-len(t.cnt) // tile)
    return np.bincount(np.flatnonzero(send) // tile, minlength=ntiles)


def map_bits(t, bits):
    """the candidate map as (word index, word value) of its nonzero 32-bit words: bit id is set <=> an entry with s_all == 1 has
    the leading `bits` bits id"""
    ids = np.unique(t.words[t.cls.s_all == 1, 0] >> U(64 - bits)).astype(np.int64)
    w, first = np.unique(ids >> 5, return_index=True)
    val = np.bitwise_or.reduceat(np.left_shift(np.int64(1), ids & 31), first) if len(ids) else np.zeros(0, np.int64)
    return w, val


def ids_of(rows, bits):
    return (rows[:, 0] >> U(64 - bits)).astype(np.int64)


def chunk_replay(per_tile, grid, f_ch):
    """The chunk rule of pass 1, replayed: workgroup wg takes the tiles wg, wg + grid, ..; the requests of a tile go to the
    workgroup's open chunk, to a new one when they do not fit (used + qn > f_ch), and a tile without requests opens nothing.
    -> the fills of the chunks opened, workgroup by workgroup"""
    fills = []
    for wg in range(min(grid, len(per_tile))):
        used = None
        for qn in per_tile[wg::grid].tolist():
            if qn == 0:
                continue
            if used is None or used + qn > f_ch:
                if used is not None:
                    fills.append(used)
                used = 0
            used += qn
        if used is not None:
            fills.append(used)
    return fills


def index_of_rows(t, rows):
    """table index of the k-mer of every row (-1: absent)"""
    at = {tuple(w): i for i, w in enumerate(t.words.tolist())}
    return np.array([at.get(tuple(r[:3]), -1) for r in rows.tolist()], np.int64)


def flagged_by(t, rows):
    """the entries that carry the prefix-side flag after these rows were applied: the targets of the rows with bit 16 set"""
    f = np.zeros(len(t.cnt), bool)
    j = index_of_rows(t, rows)
    f[j[(j >= 0) & ((rows[:, 3] >> U(16)) & U(1) == 1)]] = True
    return f


def mutual_pairs(t):
    """(i, j, weight): i < j, each the other's only pair at p >= k // 2; weight 2 where the pair stands for its mirror image too"""
    c = t.cls
    i = np.flatnonzero((c.s_all == 1) & (c.partner > np.arange(len(c.partner))))
    j = c.partner[i]
    ok = (c.s_all[j] == 1) & (c.partner[j] == i)
    i, j = i[ok], j[ok]
    return i, j, np.where(c.pos[i] != t.k - 1 - c.pos[i], 2, 1)


def flag_plot(t, flagged):
    """the plot when exactly the entries `flagged` carry the prefix-side flag: a pair enters when both members have s_all == 1,
    name each other and neither is flagged"""
    i, j, w = mutual_pairs(t)
    ok = ~flagged[i] & ~flagged[j]
    cnt = t.cnt.astype(np.int64)
    plot = np.zeros((brute.SMAX + 1, brute.FMAX + 1), np.int64)
    np.add.at(plot, (cnt[i[ok]] + cnt[j[ok]], np.minimum(cnt[i[ok]], cnt[j[ok]])), w[ok])
    return plot


def held_by_flag_alone(t):
    """the pairs that only the prefix-side flag keeps out of the plot"""
    i, j, _ = mutual_pairs(t)
    return int(((t.cls.pre[i] > 0) | (t.cls.pre[j] > 0)).sum())


def apply_list(t, rows, m):
    """`rows` reordered so that row m - 1 and the last row each decide a pair alone: their targets are members of a pair whose
    other member has no pair in front of k // 2, so the plot changes with either row"""
    i, j, _ = mutual_pairs(t)
    alone = np.concatenate([i[(t.cls.pre[i] > 0) & (t.cls.pre[j] == 0)], j[(t.cls.pre[j] > 0) & (t.cls.pre[i] == 0)]])
    dec = np.isin(index_of_rows(t, rows), alone)
    d, rest = rows[dec], rows[~dec]
    assert len(d) >= 2 and len(rest) >= m - 1
    return np.concatenate([rest[: m - 1], d[:1], rest[m - 1:], d[1:]])


def ranks_of(rows, splitters):
    """destination of every row: the number of splitters (uint64[s, 3], ascending) that are <= its k-mer"""
    r = np.zeros(len(rows), np.int64)
    for sp in splitters.reshape(-1, 3):
        ge = np.zeros(len(rows), bool)
        eq = np.ones(len(rows), bool)
        for w in range(3):
            ge |= eq & (rows[:, w] > sp[w])
            eq &= rows[:, w] == sp[w]
        r += ge | eq
    return r


def two_word_family(t):
    """the longest run of entries that agree in their first two words (64 bases) -> (first, last + 1)"""
    same = (t.words[1:, 0] == t.words[:-1, 0]) & (t.words[1:, 1] == t.words[:-1, 1])
    best, start = (0, 0), 0
    for i in range(len(same) + 1):
        if i == len(same) or not same[i]:
            if i + 1 - start > best[1] - best[0]:
                best = (start, i + 1)
            start = i + 1
    return best


def blocks(t):
    """window blocks (entries that share their first k // 2 bases) -> (start of every block, its length)"""
    pre = ktab.unpack_bases(t.packed, t.k)[:, : t.k // 2]
    new = np.r_[True, (pre[1:] != pre[:-1]).any(axis=1)]
    start = np.flatnonzero(new)
    return start, np.diff(np.r_[start, len(pre)])


# ---- generators ------------------------------------------------------------------------------------------------------------

def closed(rows, counts, k):
    packed, cnt = ktab.sort_unique_packed(ktab.pack_bases(rows), np.asarray(counts).astype(np.uint16))
    assert len(cnt) == len(rows), "two k-mers of the table are equal"
    packed, cnt = ktab.symmetrize(packed, cnt, k)
    return packed, cnt.astype(np.uint16)


# a. sizes

@functools.lru_cache(maxsize=None)
def units(k):
    """random k-mers, every other one followed by a one-base variant of itself; for even k, in front, a k-mer that is its own
    reverse complement (a closed table that holds it has an odd number of entries)"""
    rng = np.random.default_rng(9100 + k)
    rows = []
    for j in range(1500):
        z = rng.integers(0, 4, k, dtype=np.uint8)
        rows.append(z)
        if j % 2 == 0:
            y = z.copy()
            p = int(rng.integers(0, k)) if j % 8 else k // 2          # (every fourth pair at the middle position)
            y[p] = (y[p] + int(rng.integers(1, 4))) & 3
            rows.append(y)
    rows = np.array(rows, dtype=np.uint8)
    own = None
    if k % 2 == 0:
        half = rng.integers(0, 4, k // 2, dtype=np.uint8)
        own = np.concatenate([half, 3 - half[::-1]]).astype(np.uint8)
    return rows, own


@functools.lru_cache(maxsize=None)
def cut(k, n):
    """the closed table of n entries (n + 1 where k is odd and n is: such a table has an even number) of the leading rows of
    units(k) -> Wide"""
    rows, own = units(k)
    counts = np.random.default_rng(k).integers(20, 60, len(rows) + 1).astype(np.uint16)
    odd = n % 2 == 1 and own is not None
    m = (n + (0 if odd else 1)) // 2
    take = np.concatenate([own[None, :], rows[:m]]) if odd else rows[:m]
    packed, cnt = closed(take, counts[: len(take)], k)
    assert n <= len(cnt) <= n + 1
    return analyse(packed, cnt, k)


def size_list(tile):
    return [tile + d for d in range(-3, 6)] + [2 * tile + d for d in range(-3, 4)] + [4 * tile + 1, 4 * tile + 5]


# b, c: window blocks with known entries at known places

def _digits(key):
    return [(key >> 4) & 3, (key >> 2) & 3, key & 3]


def _ranked_keys(size, fixed, twins=()):
    """ascending keys < 64 for the ranks 0 .. size - 1 of a group; fixed = {rank: key}; a rank in `twins` takes the key of the rank
    in front of it (the two differ behind the key)"""
    keys = [None] * size
    for r, key in fixed.items():
        if r < size:
            keys[r] = key
    prev = -1
    for r in range(size):
        if r in twins:
            keys[r] = prev
            continue
        if keys[r] is None:
            nf = next((q for q in range(r + 1, size) if keys[q] is not None), None)
            keys[r] = prev + 1 if nf is None else max(prev + 1, keys[nf] - (nf - r) + sum(1 for q in twins if r < q <= nf))
        assert keys[r] > prev, (size, fixed, twins)
        prev = keys[r]
    assert prev < 64
    return keys


def _rows(rng, k, head, specs):
    """members of one window block: head = the bases 0 .. lead - 1 they share; spec = (base at lead, key in the three bases
    behind it, id of the random rest -- members with the same id share it --, {position: base} to override).  The last base
    is a (the complement starts with t) unless overridden, and then the base in front of it is a (.. with gt)."""
    lead = len(head)
    rests = {}
    out = np.empty((len(specs), k), np.uint8)
    for r, (g, key, rid, over) in enumerate(specs):
        if rid not in rests:
            rest = rng.integers(0, 4, k - lead - 4, dtype=np.uint8)
            rest[-1] = A
            if len(rest) > 1:
                rest[-2] = A
            rests[rid] = rest
        out[r] = np.concatenate([head, [g], _digits(key), rests[rid]])
        for p, b in over.items():
            out[r, p] = b
    return out


def seam_block(rng, k, head2, reach, halo):
    """BLOCK entries that share their first k // 2 bases.  In block order: the pair (1, 1 + reach) -- the last near code, found from
    entry 1 by the block walk and from the other end by the linear scan --, the pair (BLOCK - 2 - reach, BLOCK - 1) at distance
    reach + 1 -- found by the linear scan of its lower member, coded far --, and the neighbours (mid - 1, mid) at the last base,
    mid = BLOCK // 2 + 1; all six have no other pair.  A seam that cuts the block in front of entry `mid` is crossed by all three.
    -> (rows in block order, mid)"""
    p0 = k // 2
    a1, b1, a2, b2, mid = 1, 1 + reach, BLOCK - 2 - reach, BLOCK - 1, BLOCK // 2 + 1
    assert a1 < a2 < mid - 1 and mid < b1 < b2
    assert BLOCK - 1 - a1 >= halo and b2 >= halo                 # entries 1 and BLOCK - 1: the walk
    assert b1 < halo and BLOCK - 1 - b1 < halo and a2 < halo and BLOCK - 1 - a2 < halo      # the others: the linear scan
    head = rng.integers(0, 4, p0 + 1, dtype=np.uint8)
    head[: len(head2)] = head2
    n_a, c_end = a2 + 2, b1 - 5                               # groups at the base behind the head: a, c (holds mid), g (ends with b1), t
    assert mid + 1 < c_end
    sizes = {A: n_a, C: c_end - n_a, G: b1 + 1 - c_end, T: BLOCK - b1 - 1}
    keys = {A: _ranked_keys(sizes[A], {a1: 20, a2: 40}), C: _ranked_keys(sizes[C], {}, twins=(mid - n_a,)),
            G: _ranked_keys(sizes[G], {sizes[G] - 1: 20}), T: _ranked_keys(sizes[T], {sizes[T] - 1: 40})}
    specs = []
    for g in (A, C, G, T):
        for r, key in enumerate(keys[g]):
            j = len(specs)
            rid = "near" if j in (a1, b1) else "far" if j in (a2, b2) else "one" if j in (mid - 1, mid) else j
            specs.append((g, key, rid, {k - 1: C} if j == mid else {}))
    return _rows(rng, k, head, specs), mid


def fillers(rng, k, m, head, tail, p0):
    """m k-mers that begin with `head` and end with `tail`; every third one is a one-base variant of the one in front of it, at the
    middle position, the base behind it, position 40, or the last base but one in turn (both in one window block of two)"""
    rows = rng.integers(0, 4, (m, k), dtype=np.uint8)
    rows[:, : len(head)] = head
    rows[:, k - len(tail):] = tail
    where = (p0, p0 + 1, max(40, p0 + 2), k - 1 - max(2, len(tail)))
    for j in range(2, m, 3):
        p = where[(j // 3) % 4]
        rows[j] = rows[j - 1]
        rows[j, p] = (rows[j - 1, p] + 1 + (j // 12) % 3) & 3
    return rows


@functools.lru_cache(maxsize=None)
def seam_table(k, tile, halo, reach):
    """About three tiles whose two inner seams each cut a seam_block in front of its entry `mid`.  In table order: k-mers a.. (the
    complements of most of them, ct.., between the blocks), block one (ca..), k-mers cc.., those complements, block two (ga..),
    k-mers gc.., and, from gt.. on, the complements of everything else.  -> (Wide, (seam, seam), mid)"""
    p0 = k // 2
    rng = np.random.default_rng([k, 77])
    b1, mid = seam_block(rng, k, [C, A], reach, halo)
    b2, _ = seam_block(rng, k, [G, A], reach, halo)
    n_a = tile - mid
    n_c = 50
    n_mid = tile - BLOCK - n_c
    n_g = max(0, (3 * tile - 20) // 2 - (n_a + n_c + 2 * BLOCK))
    rows = np.concatenate([fillers(rng, k, n_mid, [A], [A, G], p0), fillers(rng, k, n_a - n_mid, [A], [A], p0), b1,
                           fillers(rng, k, n_c, [C, C], [A], p0), b2, fillers(rng, k, n_g, [G, C], [A], p0)])
    packed, cnt = closed(rows, rng.integers(5, 60, len(rows)), k)
    return analyse(packed, cnt, k), (tile, 2 * tile), mid


def ladder_block(rng, k, size, head, lead, reach):
    """`size` entries that share their first k // 2 bases (and all bases in front of `lead`).  The first and the last differ at
    position k // 2 alone (a and t; everybody else has c there).  The others, by their rank among themselves: the pairs
    (s, s + reach + s) for s in FAR_STEPS, as far as the block is long enough, at position `lead`, and the neighbours (5, 6) at the
    last base; none of these has another pair."""
    p0 = k // 2
    m = size - 2
    g_a = min(20, m)
    sizes = [g_a]
    for cap in (40, 40):
        sizes.append(min(cap, m - sum(sizes)))
    sizes.append(m - sum(sizes))
    far = [(s, s + reach + s) for s in FAR_STEPS if s + reach + s <= m - 1]
    assert all(g_a <= hi < g_a + sizes[1] for _, hi in far) and FAR_STEPS[-1] < 5
    fixed_a = {lo_: 20 + 2 * q for q, (lo_, _) in enumerate(far)}
    fixed_c = {hi - g_a: 20 + 2 * q for q, (_, hi) in enumerate(far)}
    keys = [_ranked_keys(sizes[0], fixed_a, twins=(6,)), _ranked_keys(sizes[1], fixed_c), _ranked_keys(sizes[2], {}), _ranked_keys(sizes[3], {})]
    head = head.copy()
    head[p0] = C
    specs = [(A, 0, "ends", {p0: A})]
    for g in (A, C, G, T):
        for r, key in enumerate(keys[g]):
            j = len(specs) - 1                                 # rank among the others
            q = [q for q, pr in enumerate(far) if j in pr]
            rid = ("far", q[0]) if q else "one" if j in (5, 6) else j
            specs.append((g, key, rid, {k - 1: C} if j == 6 else {}))
    specs.append((A, 0, "ends", {p0: T}))
    rows = _rows(rng, k, head[:lead], specs)
    return rows, far


@functools.lru_cache(maxsize=None)
def ladder_table(k, reach):
    """Window blocks of LADDER entries each (ladder_block).  The block of 65 has the prefix a..a and is the first of the table, the
    block of 66 has t..t and is the last; where the k-mer has bases enough behind position 64 (k = 85) every other block shares
    its bases in front of it, so that its far pairs differ in the third word.  A few hundred other k-mers.
    -> (Wide, {block size: (first entry, the far pairs as ranks among the block's inner entries, lead)})"""
    p0 = k // 2
    rng = np.random.default_rng([k, 78])
    rows, made = [], {}
    for q, size in enumerate(LADDER):
        lead = 64 if (k - 64 >= 6 and q % 2 == 1) else p0 + 1
        head = rng.integers(0, 4, max(lead, p0 + 1), dtype=np.uint8)
        head[0] = C + q % 2
        if size == 65:
            head[:p0] = A
        if size == 66:
            head[:p0] = T
        blk, far = ladder_block(rng, k, size, head, lead, reach)
        made[size] = (blk, far, lead)
        rows.append(blk)
    rows.append(fillers(rng, k, 150, [C], [A], p0))
    rows.append(fillers(rng, k, 150, [G], [A], p0))
    rows = np.concatenate(rows)
    packed, cnt = closed(rows, rng.integers(5, 60, len(rows)), k)
    t = analyse(packed, cnt, k)
    where = {}
    at = {tuple(w): i for i, w in enumerate(t.words.tolist())}
    for size, (blk, far, lead) in made.items():
        first = at[tuple(lo.packed_to_words(ktab.pack_bases(blk[:1]), k)[0].tolist())]
        where[size] = (first, far, lead)
    return t, where


# d. dense senders

@functools.lru_cache(maxsize=None)
def dense_table(k, tile):
    """About eight tiles.  800 x tile / 1024 quadruples z, z', z'', z''' -- z' differs from z behind the middle, z'' in front of
    it, z''' at both -- so that all four and their complements own a pair at p > k - 1 - p; single k-mers, a third of them with a
    partner (the middle position among them); and four k-mers that differ at their first base alone: their complements agree in
    the first two words.  -> Wide"""
    p0 = k // 2
    rng = np.random.default_rng([k, 79])
    nq = 800 * tile // 1024
    z = rng.integers(0, 4, (nq, k), dtype=np.uint8)
    p1 = rng.integers(p0 + 1, k - 1, nq)
    p2 = rng.integers(1, k - 1 - p0, nq)
    r = np.arange(nq)
    z1, z2 = z.copy(), z.copy()
    z1[r, p1] = (z[r, p1] + rng.integers(1, 4, nq)) & 3
    z2[r, p2] = (z[r, p2] + rng.integers(1, 4, nq)) & 3
    z3 = z1.copy()
    z3[r, p2] = z2[r, p2]
    fam = np.tile(rng.integers(0, 4, k, dtype=np.uint8), (4, 1))
    fam[:, 0] = (A, C, G, T)
    rows = np.concatenate([z, z1, z2, z3, fillers(rng, k, 880 * tile // 1024, [], [], p0), fam])
    packed, cnt = closed(rows, rng.integers(5, 60, len(rows)), k)
    return analyse(packed, cnt, k)


# e. flags

@functools.lru_cache(maxsize=None)
def flag_table(k):
    """just under 16 tiles of synth.adversarial_table: some 600 pairs that the prefix-side flag alone keeps out of the plot, and
    more than 6000 senders under the hash proof"""
    packed, cnt = synth.adversarial_table(k, 3900, 4, 300 + k, low_complexity=60, dense=1)
    return analyse(packed, cnt, k)
