"""tests/wide_oracle.py held to independent code (oracle/brute.py, tests/pass2_oracle.py) and to what its tables promise, on the
CPU: a table that does not put its case where tests/test_wide_fast_path_gpu.py needs it fails here, before any GPU runs.  The
sizes come from the library (engine.wide_limits, which needs no device); none is typed here."""
import functools

import numpy as np
import pytest

import brute
import wide_oracle as wo
from smudgeplot_amd import engine

KS = wo.KS
U = np.uint64


@functools.lru_cache(maxsize=None)
def lim():
    return engine.wide_limits()


def seam(k):
    L = lim()
    return wo.seam_table(k, L["F_TILE"], L["F_HALO"], L["CODE_REACH"])


def ladder(k):
    return wo.ladder_table(k, lim()["CODE_REACH"])


def dense(k):
    return wo.dense_table(k, lim()["F_TILE"])


def in_plot(t):
    pa, pb, _ = brute.unique_pairs(t.packed, t.cnt, t.k)
    return set(zip(pa.tolist(), pb.tolist()))


def neighbours(t, i):
    """entries of i's window block in front of it and behind it"""
    start, size = wo.blocks(t)
    b = np.searchsorted(start, i, side="right") - 1
    return i - start[b], start[b] + size[b] - 1 - i


def test_limits_are_what_the_generators_take_for_granted():
    L = lim()
    assert set(L) == set(engine.WIDE_LIMITS) and all(v > 0 for v in L.values())
    assert L["CODE_REACH"] + 1 < L["F_HALO"] < wo.BLOCK < L["F_TILE"] and L["F_CH"] % L["F_TILE"] == 0
    assert L["BB_LIN"] < min(wo.LADDER) and L["F_HALO"] < L["BB_STEP"] < max(wo.LADDER) and L["F_FSTAGE"] < L["F_CH"] <= L["SORT_MIN"]
    assert L["CODE_REACH"] == wo.po.REACH


# ---- the oracle against independent code ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_classes_and_partial_flag_plot_against_brute(k):
    """with every prefix-side flag set the partial-flag plot is the plot; an entry has a pair in front of k // 2 exactly when its
    complement has one behind it that is not its own mirror image (the rows of the hash proof are the entries with pre > 0)"""
    for t in (seam(k)[0], ladder(k)[0], dense(k), wo.flag_table(k), wo.cut(k, lim()["F_TILE"] + 1)):
        assert np.array_equal(wo.flag_plot(t, t.cls.pre > 0), t.plot)
        assert t.plot.sum() > 0 and (t.s_hi >= 0).all()
        E = wo.emitted_rows(t, False)
        assert np.array_equal(E[:, :3], wo.lo.sort_rows(t.words[t.cls.pre > 0]))
        assert (E[:, 3] >> U(16) == 1).all()
        X = wo.emitted_rows(t, True)
        assert np.array_equal(X[:, :3], t.words) and len(np.unique(X[:, :3], axis=0)) == len(X)
        # the flag of the exact proof's rows: set in exactly the rows of the hash proof
        assert np.array_equal(X[X[:, 3] >> U(16) == 1], E)
        j = wo.index_of_rows(t, X)
        assert np.array_equal(j, np.arange(len(j))) and np.array_equal(X[:, 3] & U(0xFFFF), t.cnt.astype(U))
        if k % 2:
            assert ((t.mid > 0) & (t.s_hi == 0)).sum() > 0         # senders of the exact proof alone that own a pair
        else:
            assert not t.mid.any()


def test_chunk_replay_on_small_cases():
    f = 100
    assert wo.chunk_replay(np.array([40, 60, 1, 0, 99]), 1, f) == [100, 100]
    assert wo.chunk_replay(np.array([40, 61, 0, 0, 99]), 1, f) == [40, 61, 99]
    assert wo.chunk_replay(np.array([40, 61, 0, 0, 99]), 2, f) == [40, 99, 61] and wo.chunk_replay(np.array([0, 0]), 1, f) == []
    assert wo.chunk_replay(np.array([40, 61, 7, 0, 99]), 8, f) == [40, 61, 7, 99]


def test_ranks_and_map_on_small_cases():
    rows = np.array([[5, 5, 1, 0], [5, 5, 2, 0], [5, 5, 3, 0], [4, 9, 9, 0], [6, 0, 0, 0]], U)
    sp = np.array([[5, 5, 2], [5, 5, 3]], U)
    assert wo.ranks_of(rows, sp).tolist() == [0, 1, 2, 0, 2]
    t = wo.cut(65, 40)
    w, val = wo.map_bits(t, 12)
    ids = sorted({int(x) >> 52 for x, s in zip(t.words[:, 0].tolist(), t.cls.s_all.tolist()) if s == 1})
    assert sorted(int(a) * 32 + b for a, v in zip(w.tolist(), val.tolist()) for b in range(32) if v >> b & 1) == ids and ids


# ---- a. sizes ------------------------------------------------------------------------------------------------------------------

def test_tables_that_end_next_to_a_seam():
    tile = lim()["F_TILE"]
    rest = set()
    for k in KS:
        seen = set()
        for n in wo.size_list(tile):
            t = wo.cut(k, n)
            assert n <= len(t.cnt) <= n + (k % 2) and t.plot.sum() > 0
            seen.add(len(t.cnt))
            rest.add(len(t.cnt) % 4)
        for s in (tile, 2 * tile):
            assert seen & {s - 2, s - 1} and seen & {s, s + 1} and seen & {s + 2, s + 3}
        assert max(seen) > 4 * tile and -(-max(seen) // tile) <= 16
    assert rest == {0, 1, 2, 3}                                  # the scalar tail of the count loads, at every length


# ---- b. seams ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_seam_table_puts_its_pairs_across_both_inner_seams(k):
    L = lim()
    halo, reach, tile = L["F_HALO"], L["CODE_REACH"], L["F_TILE"]
    t, seams, mid = seam(k)
    n = len(t.cnt)
    assert 3 * tile - 2 * wo.BLOCK <= n <= 3 * tile + 2 * wo.BLOCK and seams == (tile, 2 * tile)
    start, size = wo.blocks(t)
    plotted = in_plot(t)
    i, j, _ = wo.mutual_pairs(t)
    for s in seams:
        b = np.searchsorted(start, s, side="right") - 1
        assert start[b] == s - mid and size[b] == wo.BLOCK, (k, s, start[b], size[b])
        cross = [(a, c) for a, c in zip(i.tolist(), j.tolist()) if a < s <= c]
        assert sorted(c - a for a, c in cross) == [1, reach, reach + 1]
        for a, c in cross:
            assert (a, c) in plotted and t.cls.pre[a] == 0 and t.cls.pre[c] == 0       # a miss shows in the plot
            fa, fc = neighbours(t, a), neighbours(t, c)
            if c - a == reach + 1:                                  # found by the linear scan of its lower member, coded far
                assert max(fa) < halo and fc[0] >= halo
            if c - a == reach:                                      # the last near code: by the walk from below, by the scan from above
                assert fa[1] >= halo and max(fc) < halo
            if c - a == 1:
                assert max(fa) < halo and max(fc) < halo and t.cls.pos[a] >= 64
        assert {int(t.cls.pos[a]) < 64 for a, _ in cross} == {True, False}             # positions in the second and in the third word


# ---- c. block ladder -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_ladder_table_holds_every_block_length_with_its_pairs(k):
    L = lim()
    reach = L["CODE_REACH"]
    t, where = ladder(k)
    n = len(t.cnt)
    start, size = wo.blocks(t)
    plotted = in_plot(t)
    assert -(-n // L["F_TILE"]) <= 16
    seen_far, words = set(), set()
    for sz in wo.LADDER:
        first, far, lead = where[sz]
        b = np.searchsorted(start, first, side="right") - 1
        assert start[b] == first and size[b] == sz, (k, sz)
        last = first + sz - 1
        assert t.cls.partner[first] == last and t.cls.partner[last] == first and t.cls.pos[first] == k // 2
        assert (first, last) in plotted
        seen_far.add(sz - 1)
        for lo_, hi in far:
            a, c = first + 1 + lo_, first + 1 + hi
            assert t.cls.partner[a] == c and t.cls.partner[c] == a and (a, c) in plotted and t.cls.pos[a] == lead
            seen_far.add(c - a)
            words.add(lead >= 64)
        a = first + 1 + 5
        assert t.cls.partner[a] == a + 1 and (a, a + 1) in plotted and t.cls.pos[a] == k - 1
        if sz > reach + 2 * max(wo.FAR_STEPS) + 2:
            assert [hi - lo_ for lo_, hi in far] == [reach + s for s in wo.FAR_STEPS]
    assert {reach, reach + 1, reach + 2} <= seen_far
    assert words == ({False, True} if k - 64 >= 6 else {False})
    # the gallop's two ends: a block of BB_LIN < length that the first step leaves at once, at entry 0 and at entry n - 1
    assert where[65][0] == 0 and where[66][0] + 66 == n
    assert L["F_HALO"] < 65 <= L["BB_STEP"] + 1 and L["F_HALO"] < 66


# ---- d. dense senders ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_dense_table_fills_and_rolls_chunks(k):
    L = lim()
    tile, f_ch = L["F_TILE"], L["F_CH"]
    t = dense(k)
    n = len(t.cnt)
    ntiles = -(-n // tile)
    assert 7 <= ntiles <= 9 and (t.s_hi > 0).mean() >= 0.70
    hash_tiles, exact_tiles = wo.senders_per_tile(t, False, tile), wo.senders_per_tile(t, True, tile)
    fills = wo.chunk_replay(hash_tiles, 1, f_ch)
    assert len(fills) >= 2 and sum(fills) == (t.s_hi > 0).sum() > f_ch
    assert 0 < fills[0] < f_ch                                     # a chunk that is closed partly full: used + qn > F_CH
    assert (hash_tiles[: ntiles - 1] < tile).all() and hash_tiles.min() > 0        # .. after appends to a chunk partly full
    fills = wo.chunk_replay(exact_tiles, 1, f_ch)
    assert fills[0] == f_ch and len(fills) >= 2 and (exact_tiles[: f_ch // tile] == tile).all()     # equality: no roll-over
    assert len(wo.chunk_replay(exact_tiles, 3, f_ch)) == 3 and len(wo.chunk_replay(exact_tiles, ntiles, f_ch)) == ntiles
    # kf_filter, one workgroup, a map of ones: more than one input chunk, more survivors than a chunk holds, several flushes
    assert (t.s_hi > 0).sum() > f_ch + L["F_FSTAGE"]
    # four k-mers whose complements agree in their first two words
    a, b = wo.two_word_family(t)
    assert b - a == 4 and len(np.unique(t.words[a:b, 2])) == 4


# ---- e. flags ------------------------------------------------------------------------------------------------------------------

def kept_rows(t, bits):
    """the rows of the hash proof that name a block with a candidate: what the engine's own map of `bits` id bits keeps"""
    E = wo.emitted_rows(t, False)
    w, val = wo.map_bits(t, bits)
    ids = wo.ids_of(E, bits)
    at = np.searchsorted(w, ids >> 5)
    hit = (at < len(w)) & (w[np.minimum(at, len(w) - 1)] == ids >> 5)
    return E[hit & ((val[np.minimum(at, len(w) - 1)] >> (ids & 31)) & 1 == 1)]


@pytest.mark.parametrize("k", KS)
def test_flag_table_has_pairs_that_the_flag_alone_holds_back(k):
    L = lim()
    t = wo.flag_table(k)
    assert wo.held_by_flag_alone(t) >= 100
    assert -(-len(t.cnt) // L["F_TILE"]) <= 16
    # (the rows that survive the engine's own map are fewer than SORT_MIN in a table of sixteen tiles: the lists of the GPU test
    #  are rows of E, the rows of K among them; a row that names no candidate sets a flag nobody reads)
    E = wo.emitted_rows(t, False)
    K = kept_rows(t, 30)
    assert len(E) > L["SORT_MIN"] > len(K) > 0
    assert np.array_equal(wo.flag_plot(t, wo.flagged_by(t, K)), t.plot)
    E = wo.apply_list(t, E, L["SORT_MIN"])
    plots = [wo.flag_plot(t, wo.flagged_by(t, E[:m])) for m in (L["SORT_MIN"] - 1, L["SORT_MIN"], len(E))]
    assert not np.array_equal(plots[0], plots[1]) and not np.array_equal(plots[1], plots[2]) and not np.array_equal(plots[0], plots[2])
    assert np.array_equal(plots[2], t.plot)
