"""What the look-up chain between pass 1 and pass 2 (smudgeplot_amd/csrc/smg_lookup.hpp) has to do, in plain numpy on uint64 --
TEST INFRASTRUCTURE ONLY.  Nothing here is imported from the library: the geometry, the map layouts and the hash are
restated from the comments of smg_lookup.hpp and smg_fast.hpp, so that a change of the code has to be made twice.

  geometry   a map of fb id bits (bit id = rec0 >> (64 - fb)) is folded 4:1 into cb = fb - 2 coarse bits; the requests are
             bucketed on their leading nb = cb - 20 bits, 1 <= nb <= 10; a bucket's slice of the coarse map has cb - nb bits;
  one bit    map word id >> 5 (32 bits), bit id & 31;
  two bits   map word id >> 5 is 64 bits wide: the low half holds bit id & 31, the high half a bit at the position hashed from
             the low 32 bits of the record's first word; a two-way record passes when both are set;
  emitted    the request list of a two-way hash proof: rc(x) of every entry x that owns a pair at a position p > k-1-p whose
             counts sum to <= 1000 (tests/fake_engine.py: NumpyEngine.pass1);
  tables     the ones tests/test_lookup_regimes_gpu.py runs, with what they promise (tests/test_lookup_oracle_host.py).
"""
import functools

import numpy as np

from smudgeplot_amd import ktab, synth

U = np.uint64
NB_MAX, SLICE_LG = 10, 20
GOLDEN32 = 0x9E3779B1
SMAX = 1000

# smg_engine_lookup_limits, restated; the host and the GPU tests assert that the library says the same
LIMITS = {"F_CH": 4096, "PT_BATCH_RW1": 16384, "PT_BATCH_RW2": 8192, "PB_TRIP": 8192, "PB_WQ": 192, "PX_PART": 2048,
          "PX_TRIP": 2048, "L_NB_MAX": 10, "L_SLICE_LG": 20, "BF_MAXGRID": 512, "LW_SL": 64, "LW_UNR": 8}
PB_WAVES = 16


def wave_shares(size, trip=LIMITS["PB_TRIP"]):
    """records of a bucket per wave of a kl_probe workgroup: wave v takes 512 of every 8192"""
    per = trip // PB_WAVES
    full, rest = divmod(size, trip)
    return [full * per + min(max(rest - v * per, 0), per) for v in range(PB_WAVES)]


# ---- geometry ----------------------------------------------------------------------------------------------------------

def lookup_geo(fb):
    """-> (coarse bits, bucket bits, coarse bits of one bucket's slice)"""
    cb = fb - 2
    nb = min(max(cb - SLICE_LG, 1), NB_MAX)
    return cb, nb, cb - nb


def bucket_of(rec0, nb):
    return (np.asarray(rec0, dtype=U) >> U(64 - nb)).astype(np.int64)


def ids_of(rec0, fb):
    return np.asarray(rec0, dtype=U) >> U(64 - fb)


def hash_pos(rec0):
    """position of the second bit: the low 32 bits of the first word, times the 32-bit golden ratio, the top five bits"""
    lo = np.asarray(rec0, dtype=U) & U(0xFFFFFFFF)
    return ((lo * U(GOLDEN32)) & U(0xFFFFFFFF)) >> U(27)


# ---- the filter --------------------------------------------------------------------------------------------------------

def keep_one_bit(rec0, fb, map_fn):
    """map_fn: the map's 32-bit words (anything that can be indexed with an int64 array), or a formula ids -> bool"""
    ids = ids_of(rec0, fb)
    if callable(map_fn):
        return np.asarray(map_fn(ids), dtype=bool) & np.ones(len(ids), bool)
    w = np.asarray(map_fn[(ids >> U(5)).astype(np.int64)]).astype(U)
    return ((w >> (ids & U(31))) & U(1)).astype(bool)


def keep_two_bit(rec0, fb, map_fn):
    """map_fn: the map's 32-bit words, low and high halves alternating, or a formula (ids, positions) -> bool.  The two-way
    rule: the phase API never sends one-way records."""
    ids, pos = ids_of(rec0, fb), hash_pos(rec0)
    if callable(map_fn):
        return np.asarray(map_fn(ids, pos), dtype=bool) & np.ones(len(ids), bool)
    wi = (ids >> U(5)).astype(np.int64)
    lo = np.asarray(map_fn[2 * wi]).astype(U)
    hi = np.asarray(map_fn[2 * wi + 1]).astype(U)
    return (((lo >> (ids & U(31))) & (hi >> pos)) & U(1)).astype(bool)


def keep(rec0, fb, two, map_fn):
    return keep_two_bit(rec0, fb, map_fn) if two else keep_one_bit(rec0, fb, map_fn)


# ---- maps: the formula (ids -> bool) of the low halves, a position or None for the high halves ------------------------------

def low_formula(kind, fb):
    _, nb, _ = lookup_geo(fb)
    last = U((1 << (fb - nb)) - 1)                           # a bucket's slice of the map: fb - nb id bits
    return {"ones": lambda ids: np.ones(len(ids), bool),
            "zero": lambda ids: np.zeros(len(ids), bool),
            "one_in_four": lambda ids: (ids & U(3)) == U(3),
            "slice_edges": lambda ids: ((ids & last) == U(0)) | ((ids & last) == last)}[kind]


def formula(kind, fb, two, hi_pos=None):
    """the map `kind` as a formula for keep_one_bit / keep_two_bit; two-bit: high halves all ones, or bit hi_pos only"""
    low = low_formula(kind, fb)
    if not two:
        return low
    if hi_pos is None:
        return lambda ids, pos: low(ids)
    return lambda ids, pos: low(ids) & (pos == U(hi_pos))


def map_words(kind, fb, two, hi_pos=None):
    """the same map as the array the engine reads: uint32[2^fb / 32], twice that for the two-bit layout"""
    _, nb, _ = lookup_geo(fb)
    nw, sw = 1 << (fb - 5), 1 << (fb - nb - 5)               # words of the map, of one bucket's slice
    low = np.zeros(nw, np.uint32)
    if kind == "ones":
        low[:] = 0xFFFFFFFF
    elif kind == "one_in_four":
        low[:] = 0x88888888
    elif kind == "slice_edges":
        low[0::sw] |= np.uint32(1)
        low[sw - 1::sw] |= np.uint32(0x80000000)
    elif kind != "zero":
        raise ValueError(kind)
    if not two:
        return low
    out = np.empty(2 * nw, np.uint32)
    out[0::2] = low
    out[1::2] = 0xFFFFFFFF if hi_pos is None else (1 << hi_pos)
    return out


def device_map(kind, fb, two, hi_pos=None, device="cuda:0"):
    """the tensor Engine.filter takes (keep it alive while the engine reads it)"""
    import torch
    if kind in ("ones", "zero", "one_in_four"):              # every word alike: filled on the device (512 MB at fb = 32)
        as_i32 = lambda v: v - (1 << 32) if v >> 31 else v
        low = as_i32({"ones": 0xFFFFFFFF, "zero": 0, "one_in_four": 0x88888888}[kind])
        nw = 1 << (fb - 5)
        if not two:
            return torch.full((nw,), low, dtype=torch.int32, device=device)
        m = torch.empty((nw, 2), dtype=torch.int32, device=device)
        m[:, 0] = low
        m[:, 1] = as_i32(0xFFFFFFFF if hi_pos is None else 1 << hi_pos)
        return m.reshape(-1)
    return torch.from_numpy(map_words(kind, fb, two, hi_pos).view(np.int32)).to(device)


class DeviceWords:
    """a map that stays on the device (the engine's own, read with blockmap_copy): indexing gathers there.  A gather, not
    code under test."""

    def __init__(self, tensor):
        self.t = tensor

    def __getitem__(self, idx):
        import torch
        i = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(self.t.device)
        return self.t[i].cpu().numpy().view(np.uint32)


# ---- the request list ----------------------------------------------------------------------------------------------------

def hi_positions(k):
    return [p for p in range(k // 2, k) if p > k - 1 - p]


def owns_hi_pair(keys, cnt, k):
    """bool per entry (k <= 32, keys sorted, left aligned): a partner that differs in one base at a position p > k-1-p, the two
    counts summing to <= SMAX.  One stable sort per position; the members of a group (<= 4) stand next to each other."""
    keys = np.asarray(keys, dtype=U)
    c = np.asarray(cnt).astype(np.int64)
    own = np.zeros(len(keys), bool)
    for p in hi_positions(k):
        masked = keys & ~(U(3) << U(62 - 2 * p))
        order = np.argsort(masked, kind="stable")
        m, cc = masked[order], c[order]
        for d in (1, 2, 3):
            hit = (m[d:] == m[:-d]) & (cc[d:] + cc[:-d] <= SMAX)
            own[order[d:][hit]] = True
            own[order[:-d][hit]] = True
    return own


def emitted(keys, cnt, k):
    """sorted uint64 array: rc(x) of every entry that owns a hi-side pair"""
    keys = np.asarray(keys, dtype=U)
    return np.sort(ktab.revcomp_u64(keys[owns_hi_pair(keys, cnt, k)], k))


def pair_counts(keys, cnt, k, positions):
    """pairs per entry at the given positions (sum of the counts <= SMAX)"""
    keys = np.asarray(keys, dtype=U)
    c = np.asarray(cnt).astype(np.int64)
    n = np.zeros(len(keys), np.int64)
    for p in positions:
        masked = keys & ~(U(3) << U(62 - 2 * p))
        order = np.argsort(masked, kind="stable")
        m, cc = masked[order], c[order]
        for d in (1, 2, 3):
            hit = (m[d:] == m[:-d]) & (cc[d:] + cc[:-d] <= SMAX)
            np.add.at(n, order[d:][hit], 1)
            np.add.at(n, order[:-d][hit], 1)
    return n


def emitted_one_way(keys, cnt, k):
    """odd k <= 31, one request per complement class (smg_fast.hpp, ONE-WAY REQUESTS): with A = pairs at p >= (k-1)/2 and H = pairs
    at p > (k-1)/2, the LOWER member of a class (high bit of its middle base clear) sends rc(x) when H > 0 or A = 1, with the flag
    [H > 0] in bit 0.  -> (records sorted, the senders' indices in the same order)"""
    assert k & 1 and k <= 31
    keys = np.asarray(keys, dtype=U)
    a = pair_counts(keys, cnt, k, range(k // 2, k))
    h = pair_counts(keys, cnt, k, hi_positions(k))
    lower = ((keys >> U(64 - k)) & U(1)) == U(0)
    send = np.flatnonzero(lower & ((h > 0) | (a == 1)))
    rec = ktab.revcomp_u64(keys[send], k) | (h[send] > 0).astype(U)
    order = np.argsort(rec, kind="stable")
    return rec[order], send[order]


def keep_one_way(rec0, fb, two, map_fn):
    """one-way records against the engine's own map (an array of words): one-bit map -- the id bit; two-bit map -- the id bit and, in
    the high half, plane H (bits 16 .. 31) or, with the flag set, plane C (bits 0 .. 15) as well, at the position hashed from
    the low 32 bits with the flag bit cleared: (lo * golden mod 2^32) >> 28"""
    rec0 = np.asarray(rec0, dtype=U)
    if not two:
        return keep_one_bit(rec0, fb, map_fn)
    ids = ids_of(rec0, fb)
    f = rec0 & U(1)
    lo = rec0 & U(0xFFFFFFFE)
    pos = ((lo * U(GOLDEN32)) & U(0xFFFFFFFF)) >> U(28)
    wi = (ids >> U(5)).astype(np.int64)
    low = np.asarray(map_fn[2 * wi]).astype(U)
    hw = np.asarray(map_fn[2 * wi + 1]).astype(U)
    planes = (hw >> U(16)) | np.where(f == U(1), hw, U(0))
    return (((low >> (ids & U(31))) & (planes >> pos)) & U(1)).astype(bool)


def may_send_twice(keys, k):
    """bool per entry: the entry stands in a window block -- the entries that share their leading k // 2 bases -- of more than
    four.  Pass 1 tests distances 1 .. 3 from registers and hands an entry whose block goes on to the exact redo, which sends the
    request of an entry with a hi-side pair AGAIN (smg_pass1d.hpp, "sends again from kf_bigfix": a request only ORs a flag
    into its target).  An entry of a shorter block has nothing at distance 4 and is never redone."""
    pre = np.asarray(keys, dtype=U) >> U(64 - 2 * (k // 2))
    start = np.flatnonzero(np.r_[True, pre[1:] != pre[:-1]])
    size = np.diff(np.r_[start, len(pre)])
    return np.repeat(size, size) > 4


# ---- rows of records -------------------------------------------------------------------------------------------------------

def sort_rows(rec):
    """records uint64[n, rw] -> the same rows in lexicographic order"""
    rec = np.ascontiguousarray(rec, dtype=U)
    if rec.ndim == 1:
        rec = rec.reshape(-1, 1)
    if len(rec) == 0:
        return rec
    if rec.shape[1] == 1:
        return np.sort(rec, axis=0)
    return rec[np.lexsort(rec.T[::-1])]


def multiset_diff(a, b):
    """rows of sorted `a` that sorted `b` lacks, and the other way round (with multiplicity)"""
    from collections import Counter
    ca, cb = Counter(map(tuple, a.tolist())), Counter(map(tuple, b.tolist()))
    return sorted((ca - cb).elements()), sorted((cb - ca).elements())


# ---- tables ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def diploid(n0):
    """n0 = 150000: 405 038 entries, 101 608 requests; n0 = 400000: 1 079 704 entries, 270 612 requests (k = 31)"""
    keys, cnt = synth.diploid_table_u64(n0, k=31, seed=9, het_frac=0.35, cov=30, L=6)
    for a in (keys, cnt):
        a.setflags(write=False)
    return keys, cnt


@functools.lru_cache(maxsize=None)
def clustered(n=70000, seed=5):
    """k = 31: random k-mers that begin with AAAAA and end with TTTTT (a class closed under reverse complement), and as many
    that begin with TTTTT and end with AAAAA; a third of them with a partner at a position 16 .. 25.  Every request -- the
    complement of an entry -- falls into the first or the last of 2^10 buckets."""
    k = 31
    rng = np.random.default_rng(seed)
    rows = []
    for head, tail in ((0, 3), (3, 0)):
        b = rng.integers(0, 4, (n, k), dtype=np.uint8)
        b[:, :5], b[:, k - 5:] = head, tail
        het = b[rng.random(n) < 0.35].copy()
        pos = rng.integers(16, 26, len(het))
        het[np.arange(len(het)), pos] = (het[np.arange(len(het)), pos] + rng.integers(1, 4, len(het))) & 3
        # ... and a third of those with a partner at a position 5 .. 14 as well: the complement of such a k-mer sends a request
        # that names a candidate -- the requests that survive the engine's own map and set a flag
        pre = het[rng.random(len(het)) < 0.35].copy()
        pos = rng.integers(5, 15, len(pre))
        pre[np.arange(len(pre)), pos] = (pre[np.arange(len(pre)), pos] + rng.integers(1, 4, len(pre))) & 3
        rows += [b, het, pre]
    packed = ktab.pack_bases(np.concatenate(rows))
    cnt = rng.integers(6, 60, len(packed)).astype(np.uint16)
    packed, cnt = ktab.sort_unique_packed(packed, cnt)
    packed, cnt = ktab.symmetrize(packed, cnt, k)
    keys, cnt = ktab.packed_to_u64(packed), cnt.astype(np.uint16)
    for a in (keys, cnt):
        a.setflags(write=False)
    return keys, cnt


@functools.lru_cache(maxsize=None)
def edges(fb=25, m=300, seed=3):
    """k = 31: requests at the first and the last id of every bucket's slice of an fb-bit map, among random ones.  A request y is
    the complement of an entry x with a partner at a position p > 15; here y is made first -- its leading fb bits an id at a
    slice's end -- and y' differs from it at base 13 or 14 (behind the id bits, fb <= 26): rc(y) and rc(y') are partners at
    p = 17 or 16 and send y and y'.  The background: random k-mers, a third with a partner at a position 16 .. 25."""
    k = 31
    assert fb <= 26
    _, nb, _ = lookup_geo(fb)
    rng = np.random.default_rng(seed)
    ids = [(b << (fb - nb)) | e for b in range(1 << nb) for e in (0, (1 << (fb - nb)) - 1)]
    rows = []
    for i in ids:
        y = rng.integers(0, 4, (m, k), dtype=np.uint8)
        lead = (i << (26 - fb)) | (0 if i & 1 == 0 else (1 << (26 - fb)) - 1)            # 13 bases
        for q in range(13):
            y[:, q] = (lead >> (24 - 2 * q)) & 3
        y2 = y.copy()
        pos = rng.integers(13, 15, m)
        y2[np.arange(m), pos] = (y2[np.arange(m), pos] + rng.integers(1, 4, m)) & 3
        rows += [y, y2]
    b = rng.integers(0, 4, (20000, k), dtype=np.uint8)
    het = b[:7000].copy()
    pos = rng.integers(16, 26, len(het))
    het[np.arange(len(het)), pos] = (het[np.arange(len(het)), pos] + rng.integers(1, 4, len(het))) & 3
    packed = ktab.pack_bases(np.concatenate(rows + [b, het]))
    cnt = rng.integers(6, 60, len(packed)).astype(np.uint16)
    packed, cnt = ktab.sort_unique_packed(packed, cnt)
    packed, cnt = ktab.symmetrize(packed, cnt, k)
    keys, cnt = ktab.packed_to_u64(packed), cnt.astype(np.uint16)
    for a in (keys, cnt):
        a.setflags(write=False)
    return keys, cnt


def long_block_families(k, seed):
    """families of 120 .. 2600 k-mers that share their first k/2 + 1 bases (one window block each, in buckets of their
    own): dense ones (a k-mer, all its single mutants behind the shared part, double mutants) and sparse ones (random
    tails, a few hundred of them with exactly one partner -- often far away in the block), some counts beyond the
    sum limit, a random background"""
    rng = np.random.default_rng(seed)
    share = k // 2 + 1
    rows = []
    for f, size in enumerate([120, 400, 1000, 1800, 2600, 150, 700, 1500, 2000, 2300]):
        base = rng.integers(0, 4, k, dtype=np.uint8)
        base[0], base[1] = f & 3, f >> 2                       # (a leading 2-mer of its own: never two families in a bucket)
        fam = np.tile(base, (size, 1))
        if f < 5:                                              # dense
            j = 1
            for p in range(share, k):
                for d in (1, 2, 3):
                    if j < size:
                        fam[j, p] = (base[p] + d) & 3; j += 1
            while j < size:
                p, q = rng.integers(share, k, 2)
                fam[j, p] = (base[p] + rng.integers(1, 4)) & 3
                fam[j, q] = (base[q] + rng.integers(1, 4)) & 3
                j += 1
        else:                                                  # sparse
            fam[:, share:] = rng.integers(0, 4, (size, k - share), dtype=np.uint8)
            for j in range(0, min(size - 1, 600), 2):
                fam[j + 1] = fam[j]
                p = rng.integers(share, k)
                fam[j + 1, p] = (fam[j, p] + rng.integers(1, 4)) & 3
        rows.append(fam)
    rows.append(rng.integers(0, 4, (3000, k), dtype=np.uint8))
    packed = ktab.pack_bases(np.concatenate(rows))
    cnt = rng.integers(5, 60, size=len(packed)).astype(np.uint16)
    cnt[rng.random(len(cnt)) < 0.04] = 700                     # (pairs of two such counts exceed the sum limit)
    packed, cnt = ktab.sort_unique_packed(packed, cnt)
    return ktab.symmetrize(packed, cnt, k)


@functools.lru_cache(maxsize=None)
def families(k=31):
    packed, cnt = long_block_families(k, 300 + k)
    keys, cnt = ktab.packed_to_u64(packed), cnt.astype(np.uint16)
    for a in (keys, cnt):
        a.setflags(write=False)
    return keys, cnt


@functools.lru_cache(maxsize=None)
def wide(k, m=250000):
    """two-word k-mers: (packed, counts) of synth.adversarial_table -- 972 842 entries at k = 51"""
    packed, cnt = synth.adversarial_table(k, m, 4, 300 + k, low_complexity=60, dense=1)
    for a in (packed, cnt):
        a.setflags(write=False)
    return packed, cnt


def packed_to_words(packed, k):
    """packed k-mers -> uint64[n, W], left aligned words as the engine holds them"""
    words = (k + 31) // 32
    buf = np.zeros((len(packed), 8 * words), np.uint8)
    buf[:, : packed.shape[1]] = packed
    return buf.view(">u8").astype(U)


# ---- what a table does to the kernels (preconditions of the GPU tests, from the table and engine.lookup_limits alone) --------

def bucket_sizes(rec0, fb):
    _, nb, _ = lookup_geo(fb)
    return np.bincount(bucket_of(rec0, nb), minlength=1 << nb)


def tickets(sizes, part):
    """kl_probe_x: tickets per bucket"""
    return (np.asarray(sizes) + part - 1) // part
