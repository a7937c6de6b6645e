"""Tables on which the pair-sum limit decides degrees -- TEST INFRASTRUCTURE ONLY, held to independent code (oracle/brute.py,
tests/pass2_oracle.py, tests/lookup_oracle.py, tests/wide_oracle.py) and to its promises by tests/test_sum_limit_host.py.  Nothing
here knows a constant of the engine: the callers hand the thresholds in.

A pair is two k-mers one base apart whose counts sum to at most 1000 (PloidyPlot.c:533-537); a one-away neighbour beyond the limit
-- a DECOY -- is no pair and must not bump a degree.  A FAMILY is a random k-mer z and one-base variants of it whose counts are
chosen so that the limit decides what comes out (KINDS).  Counts that are not stated are random in 5 .. 59.

A ROUTE is where the kernels find the family, read off the sorted table (route_of): the window block -- the entries that share
their first k // 2 bases -- of the family's suffix-side image (a family at a position p < k // 2 is found on the suffix side as
its complement image, and on the prefix side as a request or a directory look-up):
  registers   the block has at most four entries: distances 1 .. 3;
  deferred    the block has 8 .. `mid` entries and the members stand at least four entries apart;
  long        the block has at least 120 entries: the members stand at its opposite ends.
"""
import functools
from typing import NamedTuple

import numpy as np

import pass2_oracle as po
from smudgeplot_amd import ktab

SMAX = 1000
A, C, G, T = 0, 1, 2, 3
HEAVY = (996, 1001, 20000, 32767)          # decoy counts of the kind "heavy", in turn
BEYOND_INT16 = (32768, 40000, 65535)       # ... of the tables that must never reach the reference binary
KINDS = ("triangle", "side", "boundary500", "boundary499", "four", "at_limit", "control", "heavy")
# degrees (pairs within the limit) of a family's members, in the order they are made
DEGREES = {"triangle": (1, 1, 0), "side": (1, 1, 0), "boundary500": (1, 1, 0), "boundary499": (1, 1, 0), "four": (2, 1, 1, 0),
           "at_limit": (2, 2, 2), "control": (2, 2, 2), "heavy": (1, 1, 0)}
DECIDED = tuple(kd for kd in KINDS if DEGREES[kd] == (1, 1, 0))      # members 0 and 1 are a pair of the plot, member 2 is the decoy
ROUTES = ("registers", "deferred", "long")
LONG_SIZES = (120, 130, 150, 180, 220, 300, 400, 600)
FILL_LEAD = 8                              # a filler begins and ends with this many a


class Family(NamedTuple):
    kind: str
    rows: np.ndarray                       # uint8[m, k] bases, member 0 first
    counts: np.ndarray                     # int64[m]
    pos: int                               # where members 0 and 1 differ


class Table(NamedTuple):
    k: int
    packed: np.ndarray
    cnt: np.ndarray                        # uint16
    fams: tuple                            # of Family
    rows: np.ndarray                       # the k-mers the table was closed from (without the fillers) ...
    row_counts: np.ndarray                 # ... and their counts
    nfill: int                             # leading fillers


def light(rng, n):
    return rng.integers(5, 60, n).astype(np.int64)


def make_family(rng, kind, z, p, q=None, heavy=None):
    """the family of `kind` around the k-mer z: variants at position p (side: the decoy at q != p)"""
    bases = [int(b) for b in rng.permutation(4)]                 # the members' bases at p: any order in the table
    if kind == "side":
        cz, cp = light(rng, 2)
        partner, decoy = z.copy(), z.copy()
        partner[p] = (z[p] + int(rng.integers(1, 4))) & 3
        decoy[q] = (z[q] + int(rng.integers(1, 4))) & 3
        return Family(kind, np.array([z, partner, decoy]), np.array([cz, cp, SMAX + 1 - cz]), p)
    a, b = light(rng, 2)
    counts = {"triangle": (a, b, SMAX + 1 - min(a, b)), "heavy": (a, b, heavy), "boundary500": (500, 500, 501),
              "boundary499": (499, 501, 502), "four": (10, 20, 985, 995), "at_limit": (a, b, SMAX - max(a, b)),
              "control": (a, b, int(light(rng, 1)[0]))}[kind]
    rows = np.tile(z, (len(counts), 1))
    rows[:, p] = bases[: len(counts)]
    return Family(kind, rows, np.array(counts, dtype=np.int64), p)


def close(rows, counts, k):
    packed, cnt = ktab.sort_unique_packed(ktab.pack_bases(rows), np.asarray(counts).astype(np.uint16))
    assert len(cnt) == len(rows), "two k-mers of the table are equal"
    packed, cnt = ktab.symmetrize(packed, cnt, k)
    return packed, cnt.astype(np.uint16)


def filler_rows(k, s):
    """s k-mers that begin and end with FILL_LEAD a (they sort in front of everything, their complements behind everything) and
    differ from one another in at least two bases: no neighbour"""
    assert k >= 2 * FILL_LEAD + 12 and s < 4 ** 6
    rows = np.zeros((s, k), np.uint8)
    for j in range(s):
        for d in range(6):
            rows[j, FILL_LEAD + 2 * d] = rows[j, FILL_LEAD + 2 * d + 1] = ((j + 1) >> (2 * d)) & 3
    return rows


def finish(k, fams, others, other_counts, nfill=0):
    keep = ~((others[:, :FILL_LEAD] == A).all(axis=1) | (others[:, k - FILL_LEAD:] == T).all(axis=1))      # (the fillers' place)
    others, other_counts = others[keep], other_counts[keep]
    rows = np.concatenate([f.rows for f in fams] + [others])
    counts = np.concatenate([f.counts for f in fams] + [other_counts])
    t = Table(k, None, None, tuple(fams), rows, counts, 0)
    return with_fillers(t, nfill)


def with_fillers(t, s):
    """the same table behind s leading fillers (count 30)"""
    k = t.k
    rows = np.concatenate([t.rows, filler_rows(k, s)])
    counts = np.concatenate([t.row_counts, np.full(s, 30, np.int64)])
    packed, cnt = close(rows, counts, k)
    lead = ktab.unpack_bases(packed, k)[:, :FILL_LEAD]
    head = (lead == A).all(axis=1)
    assert head[:s].all() and not head[s:].any(), "the fillers do not stand in front of everything"
    for a in (packed, cnt):
        a.setflags(write=False)
    return Table(k, packed, cnt, t.fams, t.rows, t.row_counts, s)


# ---- the three placements ------------------------------------------------------------------------------------------------

def register_families(rng, k, per_kind):
    """families around random k-mers: window blocks of three or four.  Positions over all of 0 .. k - 1, q anywhere else; for odd
    k the first two of every kind on the middle position"""
    fams = []
    for kind in KINDS:
        for j in range(per_kind):
            z = rng.integers(0, 4, k, dtype=np.uint8)
            p = k // 2 if (k & 1 and j < 2) else int(rng.integers(0, k))
            q = int((p + rng.integers(1, k)) % k)
            fams.append(make_family(rng, kind, z, p, q, HEAVY[j % len(HEAVY)]))          # (j = 0, 1, ..: every decoy count in turn)
    return fams


def _block(rng, k, size, kinds, j):
    """-> (families, the other rows) of one window block of `size` k-mers that share their first k // 2 + 1 bases and have random
    tails: one family of every kind in `kinds`, at the first free position (side: the decoy in the tail or in front of k // 2)"""
    share = k // 2 + 1
    head = rng.integers(0, 4, share, dtype=np.uint8)
    fams = []
    for kind in kinds:
        z = np.concatenate([head, rng.integers(0, 4, k - share, dtype=np.uint8)])
        q = int(rng.integers(share + 1, k)) if rng.random() < 0.5 else int(rng.integers(0, k // 2))
        fams.append(make_family(rng, kind, z, share, q, HEAVY[j % len(HEAVY)]))
    m = sum(int((f.rows[:, : k // 2] == head[: k // 2]).all(axis=1).sum()) for f in fams)          # (a decoy in front of k // 2 left)
    others = np.tile(np.concatenate([head, np.zeros(k - share, np.uint8)]), (size - m, 1))
    others[:, share:] = rng.integers(0, 4, (size - m, k - share), dtype=np.uint8)
    return fams, others


def order_in_block(fams, others):
    """rank of every family member among the rows of its block, by family"""
    rows = np.concatenate([f.rows for f in fams] + [others])
    v = ktab.pack_bases(rows)
    rank = np.argsort(np.argsort(v.view(np.dtype((np.void, v.shape[1]))).ravel(), kind="stable"))
    out, at = [], 0
    for f in fams:
        out.append(rank[at: at + len(f.rows)])
        at += len(f.rows)
    return out


def apart(fam, ranks, least):
    """the members that share the family's position stand at least `least` entries apart"""
    r = np.sort(ranks[:2] if fam.kind == "side" else ranks)
    return bool((np.diff(r) >= least).all())


def deferred_families(rng, k, per_kind, mid):
    """one family per window block of 8 .. mid entries, its members (side: z and its partner) four entries apart or more"""
    fams, others = [], []
    for kind in KINDS:
        for j in range(per_kind):
            for _ in range(10000):
                size = int(rng.integers(8, mid + 1))
                fs, oth = _block(rng, k, size, [kind], j + 1)
                if apart(fs[0], order_in_block(fs, oth)[0], 4):
                    break
            else:
                raise AssertionError(f"no deferred block for {kind}")
            fams += fs
            others.append(oth)
    return fams, np.concatenate(others)


def long_families(rng, k, per_kind, sizes=LONG_SIZES):
    """window blocks of LONG_SIZES entries in turn, one family of every kind in each"""
    fams, others = [], []
    for j in range(per_kind):
        fs, oth = _block(rng, k, sizes[j % len(sizes)], KINDS, j + 2)
        fams += fs
        others.append(oth)
    return fams, np.concatenate(others)


@functools.lru_cache(maxsize=None)
def decoy_table(k, route, seed, per_kind=8, mid=30, n_random=None, n_pairs=0):
    """route: one of ROUTES, or "mixed" (all three, per_kind families of every kind each).  n_random random k-mers; n_pairs plain
    disjoint pairs with light counts (they count: a background for the extract fixtures)"""
    rng = np.random.default_rng([k, seed, ROUTES.index(route) if route in ROUTES else 9])
    if n_random is None:
        n_random = 1200 if route == "registers" else 300
    fams, others = [], [rng.integers(0, 4, (n_random, k), dtype=np.uint8)]
    if route in ("registers", "mixed"):
        fams += register_families(rng, k, per_kind if route != "registers" else 2 * per_kind)
    if route in ("deferred", "mixed"):
        fs, oth = deferred_families(rng, k, per_kind, mid)
        fams += fs
        others.append(oth)
    if route in ("long", "mixed"):
        fs, oth = long_families(rng, k, per_kind)
        fams += fs
        others.append(oth)
    if n_pairs:
        x = rng.integers(0, 4, (n_pairs, k), dtype=np.uint8)
        y = x.copy()
        r, p = np.arange(n_pairs), rng.integers(0, k, n_pairs)
        y[r, p] = (x[r, p] + rng.integers(1, 4, n_pairs)) & 3
        others += [x, y]
    others = np.concatenate(others)
    return finish(k, fams, others, light(rng, len(others)))


@functools.lru_cache(maxsize=None)
def sparse_table(k, seed, n_heavy=8, n_light=150, n_random=1500):
    """The registers placement with few counts above 500: n_heavy triangles among n_light families of light counts (control) and
    random k-mers.  The heavy families begin with c and end with g, and so do their complement images: every count above 500 of
    the table stands among the k-mers c.., so that the tiles (and waves) of the other three quarters hold none."""
    rng = np.random.default_rng([k, seed, 7])
    fams = []
    for j in range(n_heavy + n_light):
        z = rng.integers(0, 4, k, dtype=np.uint8)
        p = int(rng.integers(1, k - 1))
        if j < n_heavy:
            z[0], z[k - 1] = C, G
            fams.append(make_family(rng, "triangle", z, p))
        else:
            fams.append(make_family(rng, "control", z, p))
    others = rng.integers(0, 4, (n_random, k), dtype=np.uint8)
    return finish(k, fams, others, light(rng, n_random))


# ---- where a family stands in the closed table ---------------------------------------------------------------------------------

class Placed(NamedTuple):
    fam: Family
    idx: np.ndarray                        # table index of every member ...
    rc: np.ndarray                         # ... and of its complement
    suffix: np.ndarray                     # those of the two whose pair (members 0, 1) differs at a position >= k // 2 (middle: idx)
    first: int                             # the window block of suffix[0]: its first entry ...
    size: int                              # ... and its length


def block_spans(packed, k):
    """per entry: first entry and length of its window block"""
    pre = ktab.unpack_bases(packed, k)[:, : k // 2]
    start = np.flatnonzero(np.r_[True, (pre[1:] != pre[:-1]).any(axis=1)])
    size = np.diff(np.r_[start, len(pre)])
    return np.repeat(start, size), np.repeat(size, size)


def place(t):
    """-> [Placed] of the table's families"""
    at = {bytes(r): i for i, r in enumerate(t.packed)}
    first, size = block_spans(t.packed, t.k)
    out = []
    for f in t.fams:
        pk = ktab.pack_bases(f.rows)
        idx = np.array([at[bytes(r)] for r in pk])
        rc = np.array([at[bytes(r)] for r in ktab.revcomp_packed(pk, t.k)])
        suffix = idx if f.pos >= t.k // 2 else rc
        out.append(Placed(f, idx, rc, suffix, int(first[suffix[0]]), int(size[suffix[0]])))
    return out


def route_of(pl, mid):
    """the route of a placed family, from the sorted table; None where it stands on none"""
    same = pl.suffix[:2] if pl.fam.kind == "side" else pl.suffix
    if not ((same >= pl.first) & (same < pl.first + pl.size)).all():
        return None
    gap = int(np.diff(np.sort(same)).min())
    if pl.size <= 4:
        return "registers"
    if 8 <= pl.size <= mid and gap >= 4:
        return "deferred"
    if pl.size >= LONG_SIZES[0]:
        return "long"
    return None


def degrees(packed, cnt, k):
    """pairs per entry within the limit, from tests/pass2_oracle.classify"""
    c = po.classify(packed, cnt, k)
    return c.s_all + c.pre


def senders(a, one_way):
    """bool per entry of an analysed table (wide_oracle.analyse), k <= 64: who sends a request from kf_pass1_d.  Two-way: the owner
    of a pair at p > k - 1 - p -- and, the relaxation smg_pass1d.hpp documents, every entry with two or more pairs at p >= k // 2,
    which the kernel does not look at one by one (for odd k they may all stand on the middle position; the request is harmless,
    its target has as many pairs and never counts).  One-way (odd k): the lower member of a complement class -- the high bit of its
    middle base is clear -- with any pair at p >= k // 2.  tests/lookup_oracle.py (owns_hi_pair, emitted_one_way) states the rules
    without the relaxation: the two differ exactly on the entries with two or more pairs that all stand on the middle position."""
    if one_way:
        lower = ktab.unpack_bases(a.packed, a.k)[:, a.k // 2] < 2
        return lower & (a.cls.s_all >= 1)
    return (a.s_hi > 0) | (a.cls.s_all >= 2)


def lightened(cnt):
    """every count above 400 replaced by 30: no decoy is left"""
    out = np.asarray(cnt).copy()
    out[out > 400] = 30
    return out


# ---- fillers that move a family onto a seam ----------------------------------------------------------------------------------------

def seam_shift(t, placed, seam, members, low, kinds):
    """the number of leading fillers (of a table that has none) that puts the first `low` members of a registers family of `members`
    entries in front of `seam` and the others behind it, and the family (of one of `kinds`) that then stands there
    -> (fillers, index into placed)"""
    assert t.nfill == 0
    best = None
    for n, pl in enumerate(placed):
        if len(pl.fam.rows) != members or pl.size != members or pl.fam.kind not in kinds or pl.fam.kind == "side":
            continue
        s = seam - (pl.first + low)
        if s >= 0 and (best is None or s < best[0]):
            best = (s, n)
    assert best is not None, "no family in front of the seam"
    return best


# ---- the uint8 wrap together with the limit (k > 85) ----------------------------------------------------------------------------

def hub(rng, k, heavy_in_triple, lone_heavy, prefix_side):
    """A k-mer x with 255 neighbours -- all three variants at 85 positions -- and the lone neighbour y (degree 1); built like
    make_golden.wrap_case.  heavy_in_triple: one of the 255 carries 996 (x has 256 neighbours and degree 255: its pair with y does
    not count; the degree would wrap to 0 were the limit ignored).  lone_heavy: one more lone neighbour that carries 996 (257
    neighbours, degree 256 = 0: the pair with y counts).  prefix_side: the heavy neighbour differs from x in front of k // 2.
    -> (rows, counts, (index of x, of y, of the heavy one))"""
    assert k >= 100
    x = rng.integers(0, 4, k, dtype=np.uint8)
    tri = list(range(15, 100)) if (lone_heavy and prefix_side) else list(range(85))
    free = [p for p in range(k) if p not in tri]
    rows, counts = [x], [int(light(rng, 1)[0])]
    hp = 20 if prefix_side else 60
    heavy_at = None
    for p in tri:
        for d in (1, 2, 3):
            v = x.copy(); v[p] = (v[p] + d) & 3
            if heavy_in_triple and p == hp and d == 2:
                heavy_at = len(rows)
                counts.append(996)
            else:
                counts.append(int(light(rng, 1)[0]))
            rows.append(v)
    y = x.copy(); y[free[-1]] = (y[free[-1]] + 1) & 3
    rows.append(y); counts.append(int(light(rng, 1)[0]))
    y_at = len(rows) - 1
    if lone_heavy:
        h = x.copy(); h[free[0]] = (h[free[0]] + 1) & 3
        heavy_at = len(rows)
        rows.append(h); counts.append(996)
    return np.array(rows), np.array(counts, dtype=np.int64), (0, y_at, heavy_at)


@functools.lru_cache(maxsize=None)
def wrap_table(k, seed, per_kind=2, mid=30, n_pairs=0):
    """a mixed decoy table with four hubs: 256 neighbours, one of them heavy, and 257 neighbours, one of them heavy -- the heavy one
    behind and in front of k // 2.  -> (Table, the hubs as (first row of the hub in Table.rows, (x, y, heavy) within the hub,
    the degree of x))"""
    base = decoy_table(k, "mixed", seed, per_kind=per_kind, mid=mid, n_random=300, n_pairs=n_pairs)
    rng = np.random.default_rng([k, seed, 11])
    rows, counts, hubs = [base.rows], [base.row_counts], []
    at = len(base.rows)
    for in_triple, lone, prefix in ((True, False, False), (True, False, True), (False, True, False), (False, True, True)):
        r, c, who = hub(rng, k, in_triple, lone, prefix)
        hubs.append((at, who, 255 if in_triple else 256))
        rows.append(r); counts.append(c)
        at += len(r)
    t = Table(k, None, None, base.fams, np.concatenate(rows), np.concatenate(counts), 0)
    return with_fillers(t, 0), tuple(hubs)


def index_of(t, row):
    """table index of a k-mer given as bases"""
    key = ktab.pack_bases(row[None, :])[0]
    lo, hi = 0, len(t.packed)
    kb = bytes(key)
    while lo < hi:
        m = (lo + hi) // 2
        if bytes(t.packed[m]) < kb:
            lo = m + 1
        else:
            hi = m
    assert bytes(t.packed[lo]) == kb
    return lo


# ---- counts the reference binary cannot take ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def beyond_int16_table(k, seed, per_kind=4, mid=30):
    """a mixed decoy table whose heavy decoys carry BEYOND_INT16 in turn -- for the engine and oracle/brute.py alone"""
    base = decoy_table(k, "mixed", seed, per_kind=per_kind, mid=mid, n_random=600)
    counts = base.row_counts.copy()
    fams, at, n = [], 0, 0
    for f in base.fams:
        c = f.counts.copy()
        if f.kind in ("heavy", "triangle", "side"):
            c[2] = BEYOND_INT16[n % len(BEYOND_INT16)]
            n += 1
        counts[at: at + len(c)] = c
        at += len(c)
        fams.append(f._replace(counts=c))
    t = Table(k, None, None, tuple(fams), base.rows, counts, 0)
    return with_fillers(t, 0)


# ---- the tables the tests run (tests/test_sum_limit_host.py says what they hold, tests/test_sum_limit_gpu.py runs them) --------------

KS_NARROW = (31, 30, 33, 51)               # kf_pass1_d: one word (odd, even), two words
KS_WIDE = (65, 85)                         # kf_pass1<3>
KS_COUNTED = (96, 100, 128)                # k_pass1
SPLITS = ((3, 1), (3, 2), (4, 1), (4, 2), (4, 3))      # (members of a family, those in front of the seam)
FIXTURES = {"k31_sumlimit": 31, "k32_sumlimit": 32, "k51_sumlimit": 51, "k65_sumlimit": 65, "k100_sumlimit": 100}


def mid_of(k, d_win, f_halo):
    """the longest block of the route "deferred": the partner window of kf_pass1_d; the halo of kf_pass1<3> for k = 65 .. 85 (one
    entry more and big_block_scan takes over).  The linear walk of k_pass1 (k > 85) has no export: blocks up to the partner window
    stand below it, blocks of 120 and more above it."""
    return f_halo if 64 < k <= 85 else d_win


def route_table(k, route, mid):
    return decoy_table(k, route, 100 + k, mid=mid)


def shifted(k, s, mid):
    return with_fillers(route_table(k, "registers", mid), s)


@functools.lru_cache(maxsize=None)
def seam_table(k, mid, tile, seam_no, members, low):
    """the registers table behind the fillers that put a family of `members` entries across the seam seam_no * tile, `low` of them
    in front of it -> (Table, index of that family in Table.fams)"""
    t0 = route_table(k, "registers", mid)
    s, n = seam_shift(t0, place(t0), seam_no * tile, members, low, DECIDED if members == 3 else ("four",))
    return with_fillers(t0, s), n


def fixture_table(name, mid):
    """the tables behind tests/golden/<name>.npz (tests/golden/make_golden_sum_limit.py): counts at or below 32767"""
    k = FIXTURES[name]
    if k == 100:
        return wrap_table(k, 5, per_kind=2, mid=mid, n_pairs=250)[0]
    return decoy_table(k, "mixed", 5, per_kind=4, mid=mid, n_random=300, n_pairs=250)
