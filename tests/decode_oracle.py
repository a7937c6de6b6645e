"""Numpy reference of the FastK record decoder (smg_decode.hpp: k_decode) and the generators of the tables the decoder
tests run on -- TEST INFRASTRUCTURE ONLY, held to independent code by tests/test_decode_oracle_host.py.  No engine in here.

A format-F table is a prefix index (index[p] = number of entries whose first ibyte bytes are <= p) and one record per entry:
the kbyte - ibyte bytes behind the prefix, then the count as a little-endian uint16.  Decoding entry i of the table: its
prefix is the smallest p with index[p] > i, its k-mer the prefix bytes followed by the record's suffix bytes, most significant
byte first, left aligned in W = ceil(k / 32) words of 64 bits, every byte behind the kbyte-th zero.  The bytes are taken as they
are: where k is no multiple of 4 the unused low bits of the last byte are part of the word (a FastK table has zeros there;
the generated tables below do NOT, so that a decoder which loses or invents bits there is seen).

The generated tables take the prefix of every entry from the caller and every suffix byte from a seeded generator, so a byte
that leaks in from a neighbouring record shows; they are not ordered inside a bucket, which no decoder looks at.
"""
import numpy as np

EDGE_COUNTS = (0xFFFF, 0x8000, 0x7FFF, 1, 0)


def kbyte_of(k):
    return (k + 3) // 4


def nwords(k):
    return (k + 31) // 32


# ---- the format ------------------------------------------------------------------------------------------------------------

def prefixes_of(packed, ibyte):
    """the first ibyte bytes of every row of packed[n, kbyte] as one number, most significant byte first"""
    packed = np.asarray(packed, dtype=np.uint8)
    pre = np.zeros(len(packed), dtype=np.int64)
    for j in range(ibyte):
        pre = pre * 256 + packed[:, j]
    return pre


def index_of(prefix, ibyte):
    """the prefix index of entries with these prefixes: int64[2^(8 ibyte)], cumulative ends"""
    prefix = np.asarray(prefix, dtype=np.int64)
    assert (np.diff(prefix) >= 0).all(), "entries are in prefix order"
    return np.cumsum(np.bincount(prefix, minlength=1 << (8 * ibyte))).astype(np.int64)


def records_of(packed, counts, ibyte):
    """table bytes packed[n, kbyte] and counts[n] -> (records uint8[n, kbyte - ibyte + 2], index int64[2^(8 ibyte)])"""
    packed = np.asarray(packed, dtype=np.uint8)
    n, kb = packed.shape
    assert kb > ibyte and len(counts) == n
    c = np.asarray(counts).astype(np.int64)
    rec = np.empty((n, kb - ibyte + 2), dtype=np.uint8)
    rec[:, : kb - ibyte] = packed[:, ibyte:]
    rec[:, kb - ibyte] = c & 0xFF
    rec[:, kb - ibyte + 1] = (c >> 8) & 0xFF
    return rec, index_of(prefixes_of(packed, ibyte), ibyte)


def decode(records, index, k, ibyte, first_entry=0):
    """records uint8[n, pbyte] of the entries first_entry .. first_entry + n - 1 of the table `index` belongs to
    -> (k-mers uint64[n, W], counts uint16[n])"""
    records = np.asarray(records, dtype=np.uint8)
    kb, W = kbyte_of(k), nwords(k)
    n, pb = records.shape
    assert pb == kb - ibyte + 2 and len(index) == 1 << (8 * ibyte)
    pre = np.searchsorted(np.asarray(index, dtype=np.int64), first_entry + np.arange(n, dtype=np.int64), side="right")
    assert n == 0 or pre.max() < len(index), "an entry behind the table's last"
    buf = np.zeros((n, 8 * W), dtype=np.uint8)
    for j in range(ibyte):
        buf[:, j] = (pre >> (8 * (ibyte - 1 - j))) & 0xFF
    buf[:, ibyte:kb] = records[:, : kb - ibyte]
    keys = buf.view(">u8").astype(np.uint64).reshape(n, W)
    counts = records[:, kb - ibyte].astype(np.uint16) | (records[:, kb - ibyte + 1].astype(np.uint16) << np.uint16(8))
    return keys, counts


def words_of_packed(packed, k):
    """packed[n, kbyte] -> uint64[n, W]: the bytes, left aligned (what decode() must give for the table they came from)"""
    packed = np.asarray(packed, dtype=np.uint8)
    buf = np.zeros((len(packed), 8 * nwords(k)), dtype=np.uint8)
    buf[:, : packed.shape[1]] = packed
    return buf.view(">u8").astype(np.uint64).reshape(len(packed), nwords(k))


# ---- where k_decode changes regime, from the index alone ---------------------------------------------------------------------

def tile_spans(index, n, tile, first_entry=0):
    """per tile of `tile` entries of the n records decoded from entry first_entry on: hi - lo as k_decode defines them (lo, hi:
    the prefixes of the tile's first and last entry).  A tile with hi - lo < DEC_IX stages its slice of the index."""
    i0 = np.arange(0, n, tile, dtype=np.int64)
    i1 = np.minimum(i0 + tile, n)
    index = np.asarray(index, dtype=np.int64)
    lo = np.searchsorted(index, first_entry + i0, side="right")
    hi = np.searchsorted(index, first_entry + i1 - 1, side="right")
    return hi - lo


def first_difference(got, want, tile, ept, first_entry=0):
    """None, or a sentence naming the first entry where (keys, counts) differ: its number, tile, thread and slot"""
    (gk, gc), (wk, wc) = got, want
    if gk.shape != wk.shape or gc.shape != wc.shape:
        return f"shapes differ: keys {gk.shape} counts {gc.shape}, expected {wk.shape} and {wc.shape}"
    bad = (gk != wk).any(axis=1) | (gc != wc)
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    t = i % tile
    return (f"{int(bad.sum())} of {len(bad)} entries differ, the first is entry {i} (entry {first_entry + i} of the table): tile {i // tile}, "
            f"thread {t // ept}, slot {t % ept}: k-mer {[hex(int(x)) for x in gk[i]]} count {int(gc[i]):#x}, expected "
            f"{[hex(int(x)) for x in wk[i]]} count {int(wc[i]):#x}")


# ---- tables ----------------------------------------------------------------------------------------------------------------

def counts_for(n, rng):
    """random counts that hold 0xFFFF, 0x8000, 0x7FFF, 1 and 0 (as many of them as fit, in this order of preference)"""
    c = rng.integers(0, 1 << 16, size=n).astype(np.uint16)
    at = rng.permutation(n)[: len(EDGE_COUNTS)]
    c[at] = EDGE_COUNTS[: len(at)]
    return c


def table_of(prefix, k, ibyte, rng):
    """-> (packed uint8[n, kbyte], counts uint16[n]): entry i has prefix[i] (non-decreasing), random suffix bytes and random
    counts with the edge values; the first record's suffix bytes are 0xFF, the last one's 0x00"""
    prefix = np.asarray(prefix, dtype=np.int64)
    n, kb = len(prefix), kbyte_of(k)
    assert kb > ibyte and (np.diff(prefix) >= 0).all() and (n == 0 or (prefix[0] >= 0 and prefix[-1] < 1 << (8 * ibyte)))
    packed = rng.integers(0, 256, size=(n, kb), dtype=np.uint8)
    for j in range(ibyte):
        packed[:, j] = (prefix >> (8 * (ibyte - 1 - j))) & 0xFF
    if n:
        packed[-1, ibyte:] = 0x00
        packed[0, ibyte:] = 0xFF
    return packed, counts_for(n, rng)


def random_prefixes(n, ibyte, rng, span=None):
    """n sorted prefixes drawn from `span` values (all of them by default) that start at a random place"""
    P = 1 << (8 * ibyte)
    span = P if span is None else min(span, P)
    base = int(rng.integers(0, P - span + 1))
    return np.sort(rng.integers(0, span, size=n)) + base


# the index regimes: every builder returns the prefix of every entry

def one_bucket(ntiles, tile, prefix):
    """ntiles full tiles in one bucket: hi == lo in every tile"""
    return np.full(ntiles * tile, prefix, dtype=np.int64)


def staged_beside_bisecting(tile, ix, base=3):
    """tile 0 spans ix - 1 buckets (staged), tile 1 spans ix (bisects), three entries more in the bucket behind"""
    i = np.arange(tile, dtype=np.int64)
    a = base + i * (ix - 1) // (tile - 1)
    b = a[-1] + 1 + i * ix // (tile - 1)
    return np.concatenate([a, b, np.full(3, b[-1] + 1)])


def one_per_bucket(tile, ix, rng, base=5):
    """2 tiles + 3 entries, one entry per bucket, 0 .. 6 empty buckets between neighbours, and: a run of ix + 5 empty buckets
    inside tile 0, a run of 40 that ends at the first entry of tile 1, of 17 at the last entry of tile 0, of 33 at the last entry
    of tile 1, of 9 and 5 inside the last tile"""
    n = 2 * tile + 3
    gap = rng.integers(1, 8, size=n)                 # prefix[i] - prefix[i - 1]
    gap[0] = 0
    gap[tile // 3] = ix + 6
    gap[tile - 1], gap[tile], gap[2 * tile - 1], gap[2 * tile + 1], gap[2 * tile + 2] = 18, 41, 34, 10, 6
    return base + np.cumsum(gap)


def small_buckets(tile, base=1000):
    """2 tiles + 3 entries in buckets of 1, 2, 3, 4, 5, 1, 2, ... entries without a gap: since 15 is odd, bucket edges fall on
    every slot of a thread's entries"""
    n = 2 * tile + 3
    sizes = np.resize(np.arange(1, 6), n)
    return (base + np.repeat(np.arange(n), sizes))[:n].astype(np.int64)


def alternating(tile, base=77):
    """4 tiles + 3 entries: tiles 0 and 2 in buckets of four entries (staged), tiles 1 and 3 one entry per bucket (they bisect
    as long as tile - 1 >= DEC_IX), the last three entries in one bucket"""
    out, p = [], base
    for t in range(4):
        q = p + (np.arange(tile) // 4 if t % 2 == 0 else np.arange(tile))
        out.append(q)
        p = int(q[-1]) + 1
    out.append(np.full(3, p))
    return np.concatenate(out).astype(np.int64)
