"""tests/decode_oracle.py held to independent code (no GPU): condition_oracle.words_of on bases, the table bytes, the record
layout of engine._table_view and conftest.make_table, ktab.write_ktab / read_ktab; and the guarantees of its table builders,
with the tile sizes the library exports (engine.decode_limits)."""
import functools

import numpy as np
import pytest

import condition_oracle as co
import decode_oracle as do
from conftest import golden_names, load_golden, make_table
from smudgeplot_amd import engine, ktab

LIM = engine.decode_limits()
T, EPT, IX = LIM["DEC_TILE"], LIM["DEC_EPT"], LIM["DEC_IX"]


def test_limits_are_what_the_builders_assume():
    assert T % EPT == 0 and T - 1 >= IX > 16 and EPT == 4
    assert LIM["ING_CHUNK_KIB"] * 1024 // 34 >= 4 * T           # (a piece holds several tiles of the widest record)
    assert 1 <= LIM["READERS"] <= 64


@functools.lru_cache(maxsize=None)
def golden(name):
    return load_golden(name)


@pytest.mark.parametrize("ibyte", [1, 2, 3])
@pytest.mark.parametrize("name", golden_names())
def test_decode_gives_back_every_golden_table(name, ibyte):
    g = golden(name)
    k, packed, counts = g["k"], g["packed"], g["counts"]
    rec, index = do.records_of(packed, counts, ibyte)
    assert rec.shape == (len(counts), do.kbyte_of(k) - ibyte + 2) and index[-1] == len(counts)
    keys, cnt = do.decode(rec, index, k, ibyte)
    assert keys.dtype == np.uint64 and cnt.dtype == np.uint16
    assert np.array_equal(keys, co.words_of(ktab.unpack_bases(packed, k), k))
    assert np.array_equal(co.packed_of(keys, k), packed) and np.array_equal(keys, do.words_of_packed(packed, k))
    assert np.array_equal(cnt, counts)
    # the records and the index are the ones the engine is handed
    table = make_table(dict(g, ibyte=ibyte, nparts=3))
    assert np.array_equal(table.index, index)
    tv, keep = engine._table_view(table)
    assert np.array_equal(np.concatenate(keep[0]), rec) and tv.nparts == 3
    # a shard of it
    lo, hi = len(cnt) // 3 + 1, len(cnt) - 2
    sk, sc = do.decode(rec[lo:hi], index, k, ibyte, first_entry=lo)
    assert np.array_equal(sk, keys[lo:hi]) and np.array_equal(sc, counts[lo:hi])


@pytest.mark.parametrize("ibyte", [1, 2, 3])
@pytest.mark.parametrize("name", golden_names())
def test_decode_gives_back_a_table_written_and_read(name, ibyte, tmp_path):
    g = golden(name)
    k = g["k"]
    ktab.write_ktab(str(tmp_path / "t"), k, g["packed"], g["counts"], ibyte=ibyte, nparts=g["nparts"])
    t = ktab.read_ktab(str(tmp_path / "t"))
    assert np.array_equal(t.packed, g["packed"]) and np.array_equal(t.counts, g["counts"]) and t.ibyte == ibyte
    # the records as they lie in the part files, the index as it lies in the stub
    pb = do.kbyte_of(k) - ibyte + 2
    raw = [np.fromfile(tmp_path / f".t.ktab.{p + 1}", dtype=np.uint8)[12:].reshape(-1, pb) for p in range(t.nparts)]
    assert [len(r) for r in raw] == [int(v) for v in t.part_nels]
    rec, index = do.records_of(t.packed, t.counts, ibyte)
    assert np.array_equal(np.concatenate(raw), rec)
    assert np.array_equal(np.fromfile(tmp_path / "t.ktab", dtype="<i8", offset=16), index)
    keys, cnt = do.decode(np.concatenate(raw), t.index, k, ibyte)
    assert np.array_equal(co.packed_of(keys, k), g["packed"]) and np.array_equal(cnt, g["counts"])


@pytest.mark.parametrize("k, ibyte", [(5, 1), (12, 2), (13, 3), (31, 3), (40, 2), (70, 2), (100, 1), (128, 1), (125, 3)])
def test_generated_tables_decode_to_their_own_bytes(k, ibyte):
    rng = np.random.default_rng(k * 4 + ibyte)
    n = 2 * T + 3
    packed, counts = do.table_of(do.random_prefixes(n, ibyte, rng), k, ibyte, rng)
    assert packed.shape == (n, do.kbyte_of(k))
    assert (packed[0, ibyte:] == 0xFF).all() and (packed[-1, ibyte:] == 0).all()
    assert set(do.EDGE_COUNTS) <= set(counts.tolist()) and len(set(counts.tolist())) > n // 2
    rec, index = do.records_of(packed, counts, ibyte)
    keys, cnt = do.decode(rec, index, k, ibyte)
    assert np.array_equal(keys, do.words_of_packed(packed, k)) and np.array_equal(cnt, counts)
    # byte by byte, with Python integers
    for i in (0, 1, T - 1, T, n - 1):
        v = int.from_bytes(packed[i].tobytes(), "big") << (8 * (8 * do.nwords(k) - do.kbyte_of(k)))
        assert [int(x) for x in keys[i]] == [(v >> (64 * (do.nwords(k) - 1 - w))) & (2 ** 64 - 1) for w in range(do.nwords(k))]
        assert int(cnt[i]) == int(rec[i, -2]) + 256 * int(rec[i, -1])


def test_counts_for_short_tables_take_the_edge_values_first():
    for n in range(0, 7):
        c = do.counts_for(n, np.random.default_rng(n))
        assert len(c) == n and set(do.EDGE_COUNTS[:n]) <= set(c.tolist())


def test_first_difference_names_entry_tile_thread_and_slot():
    keys = np.arange(3 * T, dtype=np.uint64).reshape(-1, 1)
    cnt = np.zeros(3 * T, dtype=np.uint16)
    assert do.first_difference((keys, cnt), (keys, cnt), T, EPT) is None
    bad = cnt.copy()
    bad[T + 4 * 7 + 2] = 1
    bad[2 * T] = 1
    msg = do.first_difference((keys, bad), (keys, cnt), T, EPT, first_entry=10)
    assert f"entry {T + 30} (entry {T + 40} of the table): tile 1, thread 7, slot 2" in msg and msg.startswith("2 of")
    assert "shapes differ" in do.first_difference((keys[:5], cnt[:5]), (keys, cnt), T, EPT)


# ---- the index regimes: what every builder promises, from the index alone ----------------------------------------------------

def spans_of(prefix, ibyte):
    index = do.index_of(prefix, ibyte)
    got = do.tile_spans(index, len(prefix), T)
    # (the same from the prefixes themselves)
    want = [int(prefix[min(i + T, len(prefix)) - 1] - prefix[i]) for i in range(0, len(prefix), T)]
    assert got.tolist() == want
    return got.tolist(), index


@pytest.mark.parametrize("ibyte", [2, 3])
def test_one_bucket(ibyte):
    for p in (0, (1 << (8 * ibyte)) - 1):
        prefix = do.one_bucket(3, T, p)
        spans, index = spans_of(prefix, ibyte)
        assert spans == [0, 0, 0] and len(prefix) == 3 * T
        assert index[p] == 3 * T and (p == 0 or index[p - 1] == 0)


@pytest.mark.parametrize("ibyte", [2, 3])
def test_staged_beside_bisecting(ibyte):
    spans, _ = spans_of(do.staged_beside_bisecting(T, IX), ibyte)
    assert spans == [IX - 1, IX, 0]


@pytest.mark.parametrize("ibyte", [2, 3])
def test_one_per_bucket(ibyte):
    prefix = do.one_per_bucket(T, IX, np.random.default_rng(1))
    spans, index = spans_of(prefix, ibyte)
    gap = np.diff(prefix)
    assert len(prefix) == 2 * T + 3 and (gap >= 1).all() and prefix[-1] < 1 << 16
    assert spans[0] >= IX and spans[1] >= IX and 0 < spans[2] < IX
    inside = gap[: T - 1]                                      # gap[i] = prefix[i + 1] - prefix[i]
    assert inside.max() - 1 > IX and 0 < int(np.argmax(inside)) < T - 2, "a run of more than DEC_IX empty buckets inside tile 0"
    assert gap[T - 2] - 1 == 17 and gap[T - 1] - 1 == 40 and gap[2 * T - 2] - 1 == 33, "runs that end at a tile's last / first entry"
    assert set(np.unique(gap - 1).tolist()) >= set(range(7)), "runs of 0 .. 6 empty buckets"
    assert np.array_equal(np.diff(np.concatenate([[0], index])).nonzero()[0], prefix)


@pytest.mark.parametrize("ibyte", [2, 3])
def test_small_buckets(ibyte):
    prefix = do.small_buckets(T)
    spans, index = spans_of(prefix, ibyte)
    assert len(prefix) == 2 * T + 3 and all(0 < s < IX for s in spans)
    sizes = np.diff(np.concatenate([[0], index]))
    sizes = sizes[sizes > 0]
    assert sizes[:-1].tolist() == np.resize(np.arange(1, 6), len(sizes) - 1).tolist() and (np.diff(np.unique(prefix)) == 1).all()
    edges = np.flatnonzero(np.diff(prefix)) + 1                  # first entries of buckets
    for size in range(1, 6):                                     # every bucket size begins on every slot of a thread
        assert set((edges[:-1][np.diff(edges) == size] % EPT).tolist()) == set(range(EPT))


@pytest.mark.parametrize("ibyte", [2, 3])
def test_alternating(ibyte):
    spans, _ = spans_of(do.alternating(T), ibyte)
    assert spans == [T // 4 - 1, T - 1, T // 4 - 1, T - 1, 0] and T // 4 - 1 < IX <= T - 1


def test_random_prefixes_stay_in_range():
    rng = np.random.default_rng(3)
    for ibyte in (1, 2, 3):
        for span in (None, 7, 1 << 30):
            p = do.random_prefixes(500, ibyte, rng, span)
            assert (np.diff(p) >= 0).all() and p[0] >= 0 and p[-1] < 1 << (8 * ibyte)
            assert span != 7 or p[-1] - p[0] < 7
