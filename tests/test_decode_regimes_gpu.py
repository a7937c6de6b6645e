"""The FastK record decoder (smg_decode.hpp: k_decode) and the piece-wise ingest in front of it (smg_ingest.hpp) entry by entry,
against tests/decode_oracle.py, where the kernel changes regime: words per k-mer, kbyte mod 4 (the mask behind the k-mer's last
byte), bytes of the index prefix, record width, byte skew of the record pointer, a tile that walks its slice of the index in
LDS or bisects the whole index, the vector or the scalar store, a shard (first_entry != 0), and parts and pieces that take turns
in the pinned and the device ring.

Every comparison is exact.  All shapes come from engine.decode_limits(); what a table does to the kernel is asserted from its
index and its part sizes before the engine is looked at.  Records lie in torch uint8 tensors with GUARD spare bytes on both
sides and are handed over at data_ptr() + GUARD + skew, never at the edge of an allocation."""
import functools

import numpy as np
import pytest
import torch

import decode_oracle as do
from smudgeplot_amd import engine, ktab

pytestmark = pytest.mark.gpu

LIM = engine.decode_limits()
T, EPT, IX, READERS = LIM["DEC_TILE"], LIM["DEC_EPT"], LIM["DEC_IX"], LIM["READERS"]
CHUNK = LIM["ING_CHUNK_KIB"] * 1024
DEV = torch.device("cuda:0")
GUARD = 16


@functools.lru_cache(maxsize=None)
def the_engine():
    return engine.Engine(0)


def device_records(rec, skew):
    """the records at byte GUARD + skew of a tensor with 0xA5 in every spare byte -> (tensor, pointer)"""
    buf = np.full(rec.size + 2 * GUARD + 4, 0xA5, dtype=np.uint8)
    buf[GUARD + skew: GUARD + skew + rec.size] = rec.reshape(-1)
    t = torch.from_numpy(buf).to(DEV)
    return t, t.data_ptr() + GUARD + skew


@functools.lru_cache(maxsize=4)
def device_index(key, ibyte):
    """the index on the device, built there from the prefixes as tools/decode_time.py builds it; key: prefixes as bytes"""
    prefix = torch.from_numpy(np.frombuffer(key, dtype=np.int64).copy()).to(DEV)
    ix = torch.cumsum(torch.bincount(prefix, minlength=1 << (8 * ibyte)), 0).to(torch.int64)
    assert ix.numel() == 1 << (8 * ibyte)
    return ix


class Table:
    """a table, its records and index, what the oracle decodes them to, and its index on the device"""

    def __init__(self, packed, counts, k, ibyte):
        self.k, self.ibyte = k, ibyte
        self.rec, self.index = do.records_of(packed, counts, ibyte)
        self.want = do.decode(self.rec, self.index, k, ibyte)
        assert np.array_equal(self.want[0], do.words_of_packed(packed, k)) and np.array_equal(self.want[1], counts)
        self.d_index = device_index(do.prefixes_of(packed, ibyte).tobytes(), ibyte)


def check(tab, skews=(0, 1, 2, 3), lo=0, hi=None, what=""):
    """decode the records [lo, hi) of the table at every skew; each result must be the oracle's"""
    k, ibyte, rec, d_index = tab.k, tab.ibyte, tab.rec, tab.d_index
    hi = len(rec) if hi is None else hi
    want = (tab.want[0][lo:hi], tab.want[1][lo:hi])
    if lo or hi < len(rec):                            # (a shard: the oracle's own first_entry says the same)
        part = do.decode(rec[lo:hi], tab.index, k, ibyte, first_entry=lo)
        assert np.array_equal(part[0], want[0]) and np.array_equal(part[1], want[1])
    e = the_engine()
    for skew in skews:
        t, ptr = device_records(rec[lo:hi], skew)
        e.decode(k, ibyte, hi - lo, ptr, d_index.data_ptr(), first_entry=lo)
        got = e.table_host()
        assert e.table()[0] == hi - lo
        diff = do.first_difference(got, want, T, EPT, first_entry=lo)
        assert diff is None, f"{what} k={k} ibyte={ibyte} pbyte={rec.shape[1]} skew={skew} entries [{lo}, {hi}): {diff}"
        del t


# ---- a. geometry: every ibyte, every record width, every skew -------------------------------------------------------------------

GEOMETRY = [(ibyte, kbyte) for ibyte in (1, 2, 3) for kbyte in range(ibyte + 1, 33)]


def k_of(ibyte, kbyte):
    return 4 * kbyte - (kbyte + kbyte // 4 + ibyte) % 4


def test_the_sweep_meets_every_word_count_and_mask_under_every_ibyte():
    for ibyte in (1, 2, 3):
        seen = {(do.nwords(k_of(i, kb)), kb % 4) for i, kb in GEOMETRY if i == ibyte and kb > 4}
        assert seen == {(w, m) for w in (1, 2, 3, 4) for m in range(4)}
        assert {kb - i + 2 for i, kb in GEOMETRY if i == ibyte} == set(range(3, 35 - ibyte))
        assert {4 * kb - k_of(i, kb) for i, kb in GEOMETRY if i == ibyte} == {0, 1, 2, 3}
    assert all(do.kbyte_of(k_of(i, kb)) == kb and 1 <= k_of(i, kb) <= 128 for i, kb in GEOMETRY)


@pytest.mark.parametrize("ibyte, kbyte", GEOMETRY)
def test_geometry(ibyte, kbyte):
    k = k_of(ibyte, kbyte)
    rng = np.random.default_rng(1000 * ibyte + kbyte)
    n = 2 * T + 3
    packed, counts = do.table_of(do.random_prefixes(n, ibyte, rng, span=n // 3), k, ibyte, rng)
    check(Table(packed, counts, k, ibyte), what="geometry")


# ---- b. tails ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k, ibyte", [(31, 3), (70, 2)])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, T - 1, T, T + 1, T + 3, 2 * T - 1, 2 * T + 1])
def test_tails(n, k, ibyte):
    rng = np.random.default_rng(n + k)
    packed, counts = do.table_of(do.random_prefixes(n, ibyte, rng, span=max(n // 2, 1)), k, ibyte, rng)
    check(Table(packed, counts, k, ibyte), skews=(n % 4, (n + 1) % 4), what="tail")
    if n == 0:
        keys, cnt = the_engine().table_host()
        assert keys.shape == (0, do.nwords(k)) and cnt.shape == (0,)


# ---- c. index regimes ----------------------------------------------------------------------------------------------------------

def regime_table(name, ibyte):
    """(prefixes, the check of hi - lo per tile that the case stands for)"""
    P = 1 << (8 * ibyte)
    if name == "one_bucket_first":
        return do.one_bucket(3, T, 0), lambda s: s == [0, 0, 0]
    if name == "one_bucket_last":
        return do.one_bucket(3, T, P - 1), lambda s: s == [0, 0, 0]
    if name == "staged_beside_bisecting":
        return do.staged_beside_bisecting(T, IX, base=P - 2 * IX - 7), lambda s: s == [IX - 1, IX, 0]
    if name == "one_per_bucket":
        return do.one_per_bucket(T, IX, np.random.default_rng(ibyte)), lambda s: s[0] > IX and s[1] >= IX and 0 < s[2] < IX
    if name == "small_buckets":
        return do.small_buckets(T), lambda s: len(s) == 3 and all(0 < v < IX for v in s)
    if name == "alternating":
        return do.alternating(T), lambda s: [v < IX for v in s] == [True, False, True, False, True]
    raise KeyError(name)


@pytest.mark.parametrize("k", [31, 40])
@pytest.mark.parametrize("ibyte", [2, 3])
@pytest.mark.parametrize("name", ["one_bucket_first", "one_bucket_last", "staged_beside_bisecting", "one_per_bucket", "small_buckets",
                                  "alternating"])
def test_index_regimes(name, ibyte, k):
    prefix, stands_for = regime_table(name, ibyte)
    spans = do.tile_spans(do.index_of(prefix, ibyte), len(prefix), T).tolist()
    assert stands_for(spans), (name, spans)
    rng = np.random.default_rng(len(name) + ibyte + k)
    packed, counts = do.table_of(prefix, k, ibyte, rng)
    check(Table(packed, counts, k, ibyte), skews=(0, 3), what=name)


# ---- d. shards -----------------------------------------------------------------------------------------------------------------

def shard_prefixes(kind, ibyte, rng):
    n = 4 * T + 5
    if kind == "dense":                                # about three entries a bucket: every tile walks its slice
        return do.random_prefixes(n, ibyte, rng, span=n // 3)
    P = 1 << (8 * ibyte)                               # pairs of entries spread over all prefixes: every tile bisects
    p = np.sort(rng.choice(P, size=n // 2 + 1, replace=False))
    return np.repeat(p, 2)[:n]


@pytest.mark.parametrize("kind", ["dense", "spread"])
@pytest.mark.parametrize("k, ibyte", [(31, 2), (31, 3), (70, 2), (70, 3)])
def test_shards(k, ibyte, kind):
    rng = np.random.default_rng(k + ibyte + len(kind))
    prefix = shard_prefixes(kind, ibyte, rng)
    n = len(prefix)
    same = np.flatnonzero(prefix[1:] == prefix[:-1]) + 1          # entries that are not the first of their bucket
    lo_mid = int(same[same > 2 * T + 1][0])
    hi_mid = int(same[same > 3 * T + 1][0])
    index = do.index_of(prefix, ibyte)
    tab = Table(*do.table_of(prefix, k, ibyte, rng), k, ibyte)
    for lo in (1, 3, T - 1, T + 2, lo_mid):
        for hi in (n, hi_mid):
            assert prefix[hi_mid - 1] == prefix[hi_mid] and prefix[lo_mid - 1] == prefix[lo_mid] and lo < hi
            spans = do.tile_spans(index, hi - lo, T, first_entry=lo)
            assert (spans < IX).all() if kind == "dense" else (spans[:-1] >= IX).all(), (kind, lo, hi, spans)
            check(tab, skews=((lo + hi) % 4,), lo=lo, hi=hi, what=f"shard of a {kind} table")


def test_decode_refuses_a_negative_first_entry():
    t, ptr = device_records(np.zeros((4, 7), np.uint8), 0)
    ix = torch.full((1 << 8,), 4, dtype=torch.int64, device=DEV)
    with pytest.raises(engine.EngineError):
        engine.Engine(0).decode(21, 1, 4, ptr, ix.data_ptr(), first_entry=-1)


# ---- e. the ingest: host table -> pinned ring -> device ring -> a decode per piece -> table ---------------------------------

def piece_entries(pbyte):
    """entries per piece of the ingest: whole tiles"""
    return CHUNK // pbyte // 1024 * 1024


def pieces_of(part_nels, pbyte):
    """(first entry, entries) of every piece, in the order the ingest takes them"""
    out, base, per = [], 0, piece_entries(pbyte)
    for pn in part_nels:
        out += [(base + a, min(per, pn - a)) for a in range(0, pn, per)]
        base += pn
    return out


def store_regimes(pieces):
    """threads of all pieces that take the vector store, and that take the scalar store although their four entries are there
    (the piece does not start on a multiple of 4 entries of the table), and that take it for a tail"""
    full = sum(nent // EPT for first, nent in pieces if first % EPT == 0)
    odd = sum(nent // EPT for first, nent in pieces if first % EPT != 0)
    tail = sum(1 for first, nent in pieces if nent % EPT)
    return full, odd, tail


def slots_used(npieces):
    """how often every slot of the pinned / device ring is used"""
    nslots = min(READERS, npieces) + 2
    return [len(range(s, npieces, nslots)) for s in range(nslots)]


def ingested(packed, counts, k, ibyte, part_nels, what):
    index = do.index_of(do.prefixes_of(packed, ibyte), ibyte)
    table = ktab.KTable(k, ibyte, len(part_nels), 1, packed, counts, index, np.array(part_nels, dtype=np.int64))
    got = engine.condition_table(table, condition=0)
    want = do.decode(*do.records_of(packed, counts, ibyte), k, ibyte)
    diff = do.first_difference(got, want, T, EPT)
    if diff is not None and got[1].shape == want[1].shape:
        pbyte = do.kbyte_of(k) - ibyte + 2
        i = int(np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[1] != want[1]))[0])
        c, (first, nent) = [(c, p) for c, p in enumerate(pieces_of(part_nels, pbyte)) if p[0] <= i][-1]
        diff += f"; piece {c} (entries {first} .. {first + nent - 1}), its entry {i - first}"
    assert diff is None, f"{what} k={k} ibyte={ibyte}: {diff}"


PART_SIZES = [0, 1, 2, 3, 5, T - 1, T, T + 1, 0, 7, 2 * T + 1, 4, 1, 3 * T - 1, 6, 9, T + 2, 2, 11, 13, 0, 2 * T, 4 * T + 3,
              T - 3, 8, 15, 3]


@pytest.mark.parametrize("k, ibyte", [(31, 3), (31, 1), (40, 2), (70, 2), (100, 1)])
def test_ingest_many_small_parts(k, ibyte):
    """Every part is one piece; the 24 pieces take each of the READERS + 2 pinned and device slots four times, begin on every
    residue mod 4 of the table's entries (first = where own_keys / own_cnt are written: both stores), and end in tails."""
    pbyte = do.kbyte_of(k) - ibyte + 2
    pieces = pieces_of(PART_SIZES, pbyte)
    assert len(PART_SIZES) >= 2 * (READERS + 2) + 1 and {0, 1, 2, 3, 5, T - 1, T, T + 1} <= set(PART_SIZES)
    assert len(pieces) == sum(1 for v in PART_SIZES if v) and min(slots_used(len(pieces))) >= 3
    assert {first % EPT for first, nent in pieces if nent >= 2 * EPT} == set(range(EPT))
    full, odd, tail = store_regimes(pieces)
    assert full >= T // EPT and odd >= T // EPT and tail >= 4
    rng = np.random.default_rng(k + ibyte)
    n = sum(PART_SIZES)
    packed, counts = do.table_of(do.random_prefixes(n, ibyte, rng, span=n // 3), k, ibyte, rng)
    ingested(packed, counts, k, ibyte, PART_SIZES, "many small parts")


def test_ingest_one_part_of_many_full_pieces():
    """The widest record (k = 128, ibyte 1: 33 bytes), one part of full pieces, as many that every slot of both rings is used
    twice, and a last piece of DEC_TILE + 3 entries: copies, decodes and the reuse of slots overlap on pieces of ING_CHUNK bytes.
    A hand-over between the copy stream and the decode stream that was not ordered would show here as a piece of wrong entries;
    the test can observe such a failure, it cannot force one."""
    k, ibyte = 128, 1
    pbyte = do.kbyte_of(k) - ibyte + 2
    per = piece_entries(pbyte)
    nfull = max(READERS + 4, 2 * (READERS + 2) - 1)
    n = nfull * per + T + 3
    pieces = pieces_of([n], pbyte)
    assert pbyte == 33 and len(pieces) == nfull + 1 and pieces[-1][1] == T + 3 and all(p[1] == per for p in pieces[:-1])
    assert (per + 1024) * pbyte > CHUNK >= per * pbyte and min(slots_used(len(pieces))) >= 2
    rng = np.random.default_rng(128)
    words = rng.integers(0, np.iinfo(np.uint64).max, size=(n, 4), dtype=np.uint64, endpoint=True)
    words[:, 0] = np.sort(words[:, 0])                 # (in table order by the first word, random behind it)
    packed = words.astype(">u8").view(np.uint8).reshape(n, 32)
    packed[0, ibyte:], packed[-1, ibyte:] = 0xFF, 0x00
    counts = do.counts_for(n, rng)
    ingested(packed, counts, k, ibyte, [n], "one part of full pieces")
