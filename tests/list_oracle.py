"""Numpy oracle of the list route between pass 1 and pass 2 for one- and two-word k-mers (k <= 64: kf_compact, kf_fill_holes, the
sorts, kf_apply_sorted<1>, kf_sortkey with kf_apply_indexed<W>, kf_apply<W>, kf_filter<RW>, and sig_find under all of them), and
the generators of the tables that put known entries where those kernels change regime -- TEST INFRASTRUCTURE ONLY, held to
independent code (oracle/brute.py) and to its promises by tests/test_list_oracle_host.py.  Nothing here knows a constant of the
engine: the callers hand in engine.list_limits() and what engine.pass1_plan() says about the directory.

The semantics are those of tests/wide_oracle.py with W words per k-mer instead of three.  Per entry x of a closed table:
  s_all  pairs at p >= k // 2        pre  pairs at p < k // 2        mid  pairs at the middle position of an odd k
  s_hi   s_all - mid: x then tells rc(x), which owns the mirror image of such a pair on its prefix side, by a request row.
Three kinds of row name the target rc(x):
  key-only   W words; every row flags its target (only entries with s_hi > 0 send)
  meta       W + 1 words, the last one count | (s_hi > 0) << 16: only bit 16 flags, the count is compared under the exact proof
  one-way    W words, odd k, one row per complement class (tests/test_one_way_rule_host.py): the lower member x of a class sends
             rc(x) | f in bit 0 of the last word, f = [s_hi(x) > 0]; f flags the target y, and s_hi(y) > 0 flags the sender
"""
import functools
from typing import NamedTuple

import numpy as np

import brute
import lookup_oracle as lo
import pass2_oracle as po
import wide_oracle as wo
from smudgeplot_amd import ktab, synth

U = np.uint64
A, C, G, T = 0, 1, 2, 3
KS1 = (31, 32, 24)                        # one word; 32 has no pad bits
KS2 = (33, 51, 64)                        # two words; 64 has no pad bits
KS = KS1 + KS2
RUNS = (1, 2, 3, 64, 1000)                # lengths of the signature runs (the last one "about")
SIG_BITS = 16


class Table(NamedTuple):
    k: int
    packed: np.ndarray
    cnt: np.ndarray
    words: np.ndarray                     # uint64[n, W], left aligned
    cls: po.Classes
    mid: np.ndarray
    s_hi: np.ndarray
    rc: np.ndarray                        # index of the reverse complement
    plot: np.ndarray                      # brute.hetmers_plot


def words_per(k):
    return (k + 31) // 32


def find_words(words, q):
    """index in the sorted rows `words` (uint64[n, W]) of every row of q (uint64[m, W]), -1 where absent"""
    q = np.ascontiguousarray(q, dtype=U).reshape(-1, words.shape[1])
    if len(q) == 0 or len(words) == 0:
        return np.full(len(q), -1, np.int64)
    if words.shape[1] == 1:
        w = words[:, 0]
        j = np.minimum(np.searchsorted(w, q[:, 0]), len(w) - 1)
        return np.where(w[j] == q[:, 0], j, -1).astype(np.int64)
    uq, inv = np.unique(q, axis=0, return_inverse=True)
    at = {tuple(r): i for i, r in enumerate(words.tolist())}
    ju = np.array([at.get(tuple(r), -1) for r in uq.tolist()], np.int64)
    return ju[np.asarray(inv).ravel()]


def analyse(packed, cnt, k):
    cls = po.classify(packed, cnt, k)
    mid = wo.mid_pairs(packed, cnt, k)
    words = lo.packed_to_words(packed, k)
    rc = find_words(words, lo.packed_to_words(ktab.revcomp_packed(packed, k), k))
    assert (rc >= 0).all(), "the table is closed under reverse complement"
    t = Table(k, packed, cnt, words, cls, mid, cls.s_all - mid, rc, brute.hetmers_plot(packed, cnt, k))
    for a in (t.packed, t.cnt, t.words, t.mid, t.s_hi, t.rc, t.plot, *t.cls):
        a.setflags(write=False)
    return t


# ---- rows ---------------------------------------------------------------------------------------------------------------------

def key_rows(t):
    """the request list of the hash proof, sorted: rc(x) of every entry with s_hi > 0 (W words)"""
    return lo.sort_rows(t.words[t.rc[t.s_hi > 0]])


def meta_rows(t, exact):
    """rows with a meta word, sorted: every entry under the exact proof, the entries with s_hi > 0 otherwise"""
    send = np.ones(len(t.cnt), bool) if exact else t.s_hi > 0
    meta = t.cnt.astype(U) | ((t.s_hi > 0).astype(U) << U(16))
    return lo.sort_rows(np.concatenate([t.words[t.rc], meta[:, None]], axis=1)[send])


def lower_members(t):
    """odd k: the member of every class {x, rc x} whose middle base has its high bit clear"""
    assert t.k & 1
    return ktab.unpack_bases(t.packed, t.k)[:, t.k // 2] < 2


def one_way_rows(t):
    """the one-way request list, sorted: the lower member x sends rc(x) | [s_hi(x) > 0] when s_hi(x) > 0 or s_all(x) == 1"""
    send = np.flatnonzero(lower_members(t) & ((t.s_hi > 0) | (t.cls.s_all == 1)))
    rows = t.words[t.rc[send]].copy()
    assert (rows[:, -1] & U(1) == 0).all(), "odd k: bit 0 of the last word is a pad bit"
    rows[:, -1] |= (t.s_hi[send] > 0).astype(U)
    return lo.sort_rows(rows)


def index_of_rows(t, rows):
    """table index of the k-mer of every row (-1: absent); a meta word behind the k-mer is ignored"""
    return find_words(t.words, np.ascontiguousarray(rows)[:, : t.words.shape[1]])


def flagged_by(t, rows):
    """the entries that carry the prefix-side flag after these rows were applied: the targets of key-only rows, the targets of the
    meta rows with bit 16 set"""
    w = t.words.shape[1]
    rows = np.ascontiguousarray(rows, dtype=U).reshape(-1, rows.shape[1])
    f = np.zeros(len(t.cnt), bool)
    j = index_of_rows(t, rows)
    sets = np.ones(len(rows), bool) if rows.shape[1] == w else (rows[:, w] >> U(16)) & U(1) == 1
    f[j[(j >= 0) & sets]] = True
    return f


def flagged_by_one_way(t, rows):
    w = t.words.shape[1]
    rows = np.ascontiguousarray(rows, dtype=U).reshape(-1, w)
    f = np.zeros(len(t.cnt), bool)
    flag = rows[:, -1] & U(1) == 1
    y = rows.copy()
    y[:, -1] &= ~U(1)
    j = find_words(t.words, y)
    f[j[(j >= 0) & flag]] = True
    back = j[(j >= 0)]
    f[t.rc[back[t.s_hi[back] > 0]]] = True
    return f


def missing_of(t, rows, exact):
    """how many rows the look-ups must report: a k-mer the table lacks, or -- exact proof, rows with a meta word -- another count"""
    w = t.words.shape[1]
    j = index_of_rows(t, rows)
    bad = j < 0
    if exact and rows.shape[1] > w:
        bad |= t.cnt[np.maximum(j, 0)].astype(U) != (rows[:, w] & U(0xFFFF))
    return int(bad.sum())


mutual_pairs = wo.mutual_pairs
flag_plot = wo.flag_plot
held_by_flag_alone = wo.held_by_flag_alone


def deciding(t):
    """the entries whose flag alone keeps a pair out of the plot: members of a mutual pair whose other member has no pair in front"""
    i, j, _ = mutual_pairs(t)
    return np.concatenate([i[(t.cls.pre[i] > 0) & (t.cls.pre[j] == 0)], j[(t.cls.pre[j] > 0) & (t.cls.pre[i] == 0)]])


def apply_list(t, rows, m):
    """the distinct `rows` reordered so that row m - 1 and the last row each decide a pair alone"""
    dec = np.isin(index_of_rows(t, rows), deciding(t))
    d, rest = rows[dec], rows[~dec]
    assert len(d) >= 2 and len(rest) >= m - 1
    return np.concatenate([rest[: m - 1], d[:1], rest[m - 1:], d[1:]])


def repeated_list(t, rows, cuts, seed):
    """a list of cuts[-1] rows for the cuts c0 < c1 < c2: the distinct rows but two deciding ones, repeated in a shuffled order;
    one deciding row at position c1 - 1 and nowhere in front of it, the other one last and nowhere else -- so the first c0
    rows, the first c1 and all of them flag three different sets"""
    c0, c1, c2 = cuts
    assert c0 == c1 - 1 < c2 - 1
    dec = np.isin(index_of_rows(t, rows), deciding(t))
    d, rest = rows[dec], rows[~dec]
    assert len(d) >= 2
    rest = np.concatenate([rest, d[2:]])[:c0]           # (every distinct row, or as many as the shortest cut holds)
    rng = np.random.default_rng(seed)
    front = rng.permutation(np.concatenate([np.arange(len(rest)), rng.integers(0, len(rest), c0 - len(rest))]))
    body = rest[np.concatenate([front, rng.integers(0, len(rest), c2 - 2 - c0)])]
    return np.concatenate([body[:c0], d[:1], body[c0:], d[1:2]])


# ---- tables -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def flag_table(k, senders):
    """synth.adversarial_table grown until at least `senders` entries send under the hash proof; at least two pairs that a single
    row decides alone"""
    m = 2000
    while True:
        packed, cnt = synth.adversarial_table(k, m, 4, 300 + k, low_complexity=60, dense=1)
        if int((wo.mid_pairs(packed, cnt, k) < po.classify(packed, cnt, k).s_all).sum()) >= senders:
            return analyse(packed, cnt, k)
        m *= 2


@functools.lru_cache(maxsize=None)
def adversarial(k, m, seed):
    packed, cnt = synth.adversarial_table(k, m, 4, seed, low_complexity=60, dense=1)
    return analyse(packed, cnt, k)


def fillers(rng, k, m):
    """m random k-mers; every third one is a one-base variant of the one in front of it, at the middle position, the base behind
    it, the last base but two or the third base in turn"""
    rows = rng.integers(0, 4, (m, k), dtype=np.uint8)
    where = (k // 2, k // 2 + 1, k - 3, 2)
    for j in range(2, m, 3):
        p = where[(j // 3) % 4]
        rows[j] = rows[j - 1]
        rows[j, p] = (rows[j - 1, p] + 1 + (j // 12) % 3) & 3
    return rows


def poly_rows(k):
    """T x k with a one-base variant at position k - 12, and such a variant of A x k (A x k itself is the complement of T x k): each
    of the two homopolymers owns a pair at p >= k // 2 whose partner has no other pair, so each sends the other one as a request"""
    x = np.full(k, T, np.uint8)
    y, y2 = x.copy(), np.full(k, A, np.uint8)
    y[k - 12], y2[k - 12] = G, C
    return np.array([x, y, y2])


def flagged_trios(rng, k, m):
    """m random k-mers z, each with a variant behind the middle and one in front of it: z has one pair at p >= k // 2 and the
    flag (its complement owns the mirror image of the other pair), so the pair is one that only the flag keeps out of the plot"""
    z = rng.integers(0, 4, (m, k), dtype=np.uint8)
    r = np.arange(m)
    z1, z2 = z.copy(), z.copy()
    p1, p2 = rng.integers(k // 2 + 1, k - 1, m), rng.integers(1, k // 2 - 1, m)
    z1[r, p1] = (z[r, p1] + rng.integers(1, 4, m)) & 3
    z2[r, p2] = (z[r, p2] + rng.integers(1, 4, m)) & 3
    return np.concatenate([z, z1, z2])


def holes_of(nreq, chunk):
    """slots that stay empty when nreq records fill chunks of `chunk` to the brim"""
    return -(-nreq // chunk) * chunk - nreq


@functools.lru_cache(maxsize=None)
def brim_full_table(k, one_way, chunk, least, poly=False):
    """A diploid table (synth.diploid_table_u64, k <= 32) whose request list -- one-way or two-way -- has `least` records at
    least, leaves less than a sixteenth of its last chunk of `chunk` records empty, and holds no window block of more than four
    entries (no entry sends twice: the list is exactly the oracle's); 400 flagged_trios among them.  poly: with poly_rows(k).
    -> Table"""
    n0 = 36000
    while True:
        keys, cnt = synth.diploid_table_u64(n0, k=k, seed=40 + k, het_frac=0.35, cov=30, L=6)
        more = flagged_trios(np.random.default_rng([k, n0]), k, 400)
        if poly:
            more = np.concatenate([more, poly_rows(k)])
        packed = np.concatenate([ktab.u64_to_packed(keys, k), ktab.pack_bases(more)])
        packed, cnt = ktab.sort_unique_packed(packed, np.concatenate([cnt, (20 + np.arange(len(more)) % 17).astype(np.uint16)]))
        packed, cnt = ktab.symmetrize(packed, cnt, k)
        keys, cnt = ktab.packed_to_u64(packed), cnt.astype(np.uint16)
        nreq = len(lo.emitted_one_way(keys, cnt, k)[0]) if one_way else int(lo.owns_hi_pair(keys, cnt, k).sum())
        if nreq >= least and 16 * holes_of(nreq, chunk) < nreq and not lo.may_send_twice(keys, k).any():
            return analyse(packed, cnt, k)
        n0 += 300


# signatures: the directory bucket of an entry is named by the bits of its first word from `sigsh` + 16 up, its signature is the 16
# bits from `sigsh` up, and entries that agree in both are told apart by their k-mers

def own_directory_shift(n, first_hi32, last_hi32, per):
    """the shift of a directory over the leading 32 k-mer bits with `per` .. 2 `per` entries per bucket: the smallest that leaves
    the table's span inside 2^bits buckets, 2^bits the largest power of two <= n / per (16 at least)"""
    bits = 4
    while bits < 30 and (1 << (bits + 1)) <= n // per:
        bits += 1
    dsh = 0
    while dsh < 31 and ((last_hi32 >> dsh) - (first_hi32 >> dsh)) >= (1 << bits):
        dsh += 1
    return dsh


def sig_shift(t, per, index_bytes):
    """bit of the first word at which the signature of table t begins: below the 8 * index_bytes bits of a prefix index, or below
    the bucket bits of a directory of `per` entries per bucket (index_bytes = 0)"""
    if index_bytes:
        return 64 - 8 * index_bytes - SIG_BITS
    return SIG_BITS + own_directory_shift(len(t.cnt), int(t.words[0, 0] >> U(32)), int(t.words[-1, 0] >> U(32)), per)


class Family(NamedTuple):
    length: int                           # the run it was built for
    members: np.ndarray                   # bases [length, k]
    target: np.ndarray                    # bool per member: it has a pair in front of k // 2, so its complement sends it
    candidate: np.ndarray                 # bool per member: it was given exactly one pair at p >= k // 2
    absent: np.ndarray                    # bases [k]: a k-mer the table lacks, with the members' bucket and signature


def _family(rng, k, sigsh, length, lone_target):
    """`length` k-mers that share the first word's bits from sigsh up.  Members come in pairs that differ at position pp, the first
    base at p >= k // 2 below the shared bits (a, then c: the two halves of the run); their bases behind pp differ from pair to
    pair in two places at least, so a member has that one pair.  Of three pairs in turn the a-member, none and the c-member have a
    pair in front of k // 2 as well (with a k-mer outside the run).  An odd member has its pair outside the run, at a position in
    the shared bits, where k // 2 lies in front of their end -- else it has none and is no candidate."""
    hb = 64 - sigsh                                   # shared bits
    nh = (hb + 1) // 2                                # bases that hold them
    pp = max(nh, k // 2)
    t = k - 1 - pp                                    # bases behind pp
    assert t >= 1 and nh >= 2
    head = rng.integers(0, 4, k, dtype=np.uint8)
    head[0] = C + int(rng.integers(0, 2))
    npairs = length // 2
    rests = np.zeros((0, t), np.uint8)
    if npairs:
        cap = 4 ** (t - 1)
        npairs = min(npairs, cap - 1 if cap > 1 else 1)
        if t == 1:
            body = np.zeros((1, 0), np.uint8)
        elif cap <= 4 * npairs:
            body = np.array(np.unravel_index(rng.permutation(cap)[:npairs], (4,) * (t - 1))).T.astype(np.uint8).reshape(npairs, t - 1)
        else:
            body = np.unique(rng.integers(0, 4, (4 * npairs, t - 1), dtype=np.uint8), axis=0)
            body = body[rng.permutation(len(body))[:npairs]]
        rests = np.concatenate([body, ((-body.astype(np.int64).sum(axis=1)) & 3).astype(np.uint8)[:, None]], axis=1)
        rests = rests[np.lexsort(rests.T[::-1])]
    members, target, cand, extra = [], [], [], []
    for half, base in enumerate((A, C)):
        for i, r in enumerate(rests):
            x = head.copy()
            x[pp] = base
            x[pp + 1:] = r
            members.append(x)
            target.append(i % 3 == (0, 2)[half])
            cand.append(True)
    if length % 2:
        x = head.copy()
        x[pp] = G
        x[pp + 1:] = rng.integers(0, 4, t, dtype=np.uint8)
        if len(rests) and t >= 2:                       # (two bases away from the pair it shares the run with)
            x[pp + 1:] = rests[0]
            x[k - 2:] = (x[k - 2:] + 1) & 3
        p_out = k // 2
        feasible = p_out <= (hb - 1) // 2
        if feasible:
            y = x.copy()
            y[p_out] ^= 2
            extra.append(y)
        members.append(x)
        target.append(lone_target)
        cand.append(feasible)
    members = np.array(members, np.uint8)
    target = np.array(target, bool)
    for x in members[target]:
        z = x.copy()
        z[1] = (z[1] + 1 + int(rng.integers(0, 3))) & 3
        extra.append(z)
    # (one base from a member, so no member itself: behind the first one, or in front of the first one of the second half)
    if len(rests) == 0 or members[0][k - 1] < 3:
        absent = members[0].copy()
        absent[k - 1] = (absent[k - 1] + 1) & 3
    else:
        absent = members[len(rests)].copy()
        absent[k - 1] = 2
    return Family(len(members), members, target, np.array(cand, bool), absent), extra


def _signature_rows(k, sigsh, seed):
    rng = np.random.default_rng([k, sigsh, seed])
    fams, rows = [], []
    for length, lone_target in [(1, True), (1, False)] + [(n, bool(n & 2)) for n in RUNS[1:]]:
        f, extra = _family(rng, k, sigsh, length, lone_target)
        fams.append(f)
        rows += [f.members, np.array(extra, np.uint8).reshape(-1, k)]
    # the directory spans all leading bits: a k-mer that begins with sixteen a, one that begins with sixteen t
    ends = rng.integers(0, 4, (2, k), dtype=np.uint8)
    ends[0, :16], ends[1, :16] = A, T
    ends[:, -1] = C
    rows += [ends, fillers(rng, k, 900)]
    rows = np.concatenate(rows)
    return fams, rows, rng.integers(5, 60, len(rows))


@functools.lru_cache(maxsize=None)
def signature_table(k, per, index_bytes):
    """Families of entries that agree in every bit of the first word down to and including the 16 signature bits, and differ below
    them: runs of 1 (twice: a target, and not), 2, 3, 64 and about 1000 (as many as the bits below the signature hold pairs that
    differ in two bases), for a table with a prefix index of `index_bytes` bytes or (0) for pass 1's own directory of `per`
    entries per bucket.  -> (Table, sigsh, families)"""
    sigsh = 64 - 8 * index_bytes - SIG_BITS if index_bytes else 40
    for _ in range(4):
        fams, rows, counts = _signature_rows(k, sigsh, 5)
        packed, cnt = wo.closed(rows, counts, k)
        t = analyse(packed, cnt, k)
        got = sig_shift(t, per, index_bytes)
        if got == sigsh:
            return t, sigsh, fams
        sigsh = got
    raise AssertionError("the signature shift did not settle")


def runs_of(t, sigsh):
    """per entry: the number of entries that share its directory bucket and its signature"""
    key = t.words[:, 0] >> U(sigsh)
    _, inv, count = np.unique(key, return_inverse=True, return_counts=True)
    return count[np.asarray(inv).ravel()]


def family_rows(t, fam):
    """(words of the members, their table indices, words of the absent k-mer)"""
    w = lo.packed_to_words(ktab.pack_bases(fam.members), t.k)
    j = find_words(t.words, w)
    assert (j >= 0).all()
    return w, j, lo.packed_to_words(ktab.pack_bases(fam.absent[None, :]), t.k)
