"""The seams between the tiles of kf_pass1_d (smg_pass1d.hpp).  A tile owns D_OWN consecutive entries and stages D_LEAD in front
of them -- one thread, whose tests against its right neighbour hand the pairs at distances 1 .. 3 across the seam; pairs at
distances >= 4 are found from their lower entry alone, looking forward past the end of its tile.  The sizes come from the library
(engine.pass1_limits), no constant is typed here.

Plots against oracle/brute.py, request counts against tests/lookup_oracle.py (k <= 32) and between the forms, through both hot
forms (one-way and SMG_TWO_WAY=1; even k has one) for k = 31, k = 30 (even) and k = 33 (two words).

The seam tables are built so that what lies on a seam is known, and say so from the sorted table before the GPU runs: a table that
does not put its cases on the seams fails."""
import functools

import numpy as np
import pytest

import brute
import lookup_oracle as lo
from smudgeplot_amd import engine, ktab
from test_pass1_forms_gpu import Bound, clear, run_once, words_of, TWO_WAY_HOT

pytestmark = pytest.mark.gpu

KS = (31, 30, 33)
BLOCK = 40                 # entries of a seam block: a window block longer than the partner window + 1
A, C, G, T = 0, 1, 2, 3


def limits():
    lim = engine.pass1_limits()
    assert lim["D_LEAD"] == 4 and lim["D_SLOTS"] == lim["D_OWN"] + 8, "a tile stages one thread in front of and one behind what it owns"
    assert BLOCK > lim["D_WIN"] + 1
    return lim


def forms(k):
    """(name, environment, VAR) of the hot forms a table of this k can run"""
    if k & 1:
        return (("one-way", {}, 2), ("two-way", {"TWO_WAY": 1}, TWO_WAY_HOT))
    return (("two-way", {}, 2), ("two-way, hook set", {"TWO_WAY": 1}, 2))


# ---- what a table must send ----------------------------------------------------------------------------------------------

def emitted_bounds(packed, cnt, k, one_way):
    """-> (lo, hi) for the requests pass 1 and kf_bigfix emit together (k <= 32): the senders of the final state at least; an entry
    of a window block of more than four may have sent from its provisional state as well (smg_pass1d.hpp: a superset), once"""
    keys = ktab.packed_to_u64(packed)
    again = lo.may_send_twice(keys, k)
    if one_way:
        rec, _ = lo.emitted_one_way(keys, cnt, k)
        lower = ((keys >> np.uint64(64 - k)) & np.uint64(1)) == 0
        return len(rec), len(rec) + int((again & lower).sum())
    return int(lo.owns_hi_pair(keys, cnt, k).sum()), int(lo.owns_hi_pair(keys, cnt, k).sum()) + int(again.sum())


def check_run(packed, cnt, want, k, env, var, what):
    plot, st, form = run_once(packed, cnt, k)
    assert form == {"var": var, "w": words_of(k), "rw": words_of(k), "inner_only": 0}, (what, form)
    assert st["path"] == 1, (what, st)
    assert np.array_equal(plot, want), what
    if k <= 32:
        low, high = emitted_bounds(packed, cnt, k, one_way=bool(k & 1) and "TWO_WAY" not in env)
        print(f"{what}: emitted {st['nemitted']} in [{low}, {high}], kept {st['nrequests']}")
        assert low <= st["nemitted"] <= high, what
    return st["nemitted"], st["nrequests"]


# ---- 1. tables that end on, before and behind a seam ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def units(k):
    """random k-mers, every other one followed by a one-base variant of itself (so that the table has pairs)"""
    rng = np.random.default_rng(9100 + k)
    rows = []
    for j in range(1500):
        z = rng.integers(0, 4, k, dtype=np.uint8)
        rows.append(z)
        if j % 2 == 0:
            y = z.copy()
            p = int(rng.integers(0, k))
            y[p] = (y[p] + int(rng.integers(1, 4))) & 3
            rows.append(y)
    return np.array(rows, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def cut(k, n):
    """the closed table of the fewest leading rows of units(k) that has at least n entries -> (packed, counts, the oracle's plot)"""
    rows = units(k)
    counts = np.random.default_rng(k).integers(20, 60, len(rows)).astype(np.uint16)
    for m in range((n + 1) // 2, len(rows) + 1):
        packed, cnt = ktab.sort_unique_packed(ktab.pack_bases(rows[:m]), counts[:m])
        packed, cnt = ktab.symmetrize(packed, cnt, k)
        if len(cnt) >= n:
            cnt = cnt.astype(np.uint16)
            return packed, cnt, brute.hetmers_plot(packed, cnt, k)
    raise AssertionError("units(k) is too short")


def seam_sizes(own, where):
    return {"one tile": [own + d for d in range(-3, 6)], "two tiles": [2 * own + d for d in range(-3, 4)],
            "four tiles": [4 * own + 1, 4 * own + 5]}[where]


@pytest.mark.parametrize("where", ["one tile", "two tiles", "four tiles"])
@pytest.mark.parametrize("k", KS)
def test_tables_that_end_next_to_a_seam(k, where, monkeypatch):
    own = limits()["D_OWN"]
    seen = set()
    for n in seam_sizes(own, where):
        packed, cnt, want = cut(k, n)
        assert n <= len(cnt) <= n + 1
        if len(cnt) in seen:                      # (a closed table of odd k has an even number of entries)
            continue
        seen.add(len(cnt))
        assert want.sum() > 0
        for name, env, var in forms(k):
            clear(monkeypatch, **env)
            check_run(packed, cnt, want, k, env, var, f"k={k} n={len(cnt)} {name}")
    # a table that ends in front of, one that ends on (or one entry behind) and one that ends behind the seam
    s = {"one tile": own, "two tiles": 2 * own}.get(where)
    if s is not None:
        assert seen & {s - 2, s - 1} and seen & {s, s + 1} and seen & {s + 2, s + 3}, sorted(seen)
    else:
        assert min(seen) > 4 * own


# ---- 2. tables with known entries on their two inner seams ---------------------------------------------------------------

def one_away(suf):
    """bool[n, n]: the rows differ in exactly one base"""
    return (suf[:, None, :] != suf[None, :, :]).sum(axis=2) == 1


def cases(pair, first, last, seam, win):
    """-> (the cases the entries around `seam` put on it, the crossing pairs as (i, j)); pair = one_away of the suffixes of the window
    block first .. last that the seam cuts"""
    got, pairs = set(), []
    for i in range(max(first, seam - win), seam):
        for j in range(seam, min(last + 1, i + win + 1)):
            if pair[i - first, j - first]:
                d = j - i
                pairs.append((i, j))
                got.add(f"d{d}" if d <= 3 else "batch" if d <= 9 else "far")       # (4 .. 9: the batch of d_detect)
                if d >= 4 and j < seam + 4:
                    got.add("upper among the first four")
    if last - first + 1 > win + 1:
        got.add("big")
    return got, pairs


def crossing(bases, k, seam, win):
    """the same from the sorted table alone: a pair has the same first k // 2 bases and one other base that differs"""
    p0 = k // 2
    pre = bases[:, :p0]
    if not (pre[seam - 1] == pre[seam]).all():
        return set(), []
    first, last = seam - 1, seam
    while first > 0 and (pre[first - 1] == pre[seam]).all():
        first -= 1
    while last + 1 < len(bases) and (pre[last + 1] == pre[seam]).all():
        last += 1
    return cases(one_away(bases[first: last + 1, p0:]), first, last, seam, win)


FAR = {"batch", "far", "big", "upper among the first four"}


def family(rng, size, k):
    """suffixes of a window block: random ones, each with up to two one-away partners on the top suffix base and up to three on
    the base below it, as the families of tests/lookup_oracle.py (partners on the base below stand a few entries apart, those on
    the top base a quarter of the block and more); the last base is a, so that every complement starts with t.
    -> uint8[<= size, k - k // 2], sorted as the table sorts them"""
    m = k - k // 2
    suf = np.empty((size, m), np.uint8)
    j = 0
    while j < size:
        root = rng.integers(0, 4, m, dtype=np.uint8)
        root[-1] = A
        suf[j] = root
        j += 1
        for p, most in ((0, 2), (1, 3)):
            for step in rng.permutation(3)[: int(rng.integers(0, most + 1))] + 1:
                if j < size:
                    suf[j] = root
                    suf[j, p] = (root[p] + step) & 3
                    j += 1
    return np.unique(suf, axis=0)


@functools.lru_cache(maxsize=None)
def seam_block(k, near, tag, win):
    """A family of BLOCK entries and the offset at which a seam has to cut it.  near = the distances among 1 .. 3 at which pairs
    have to cross the seam (and at no other of them); with one distance alone that pair must be the only one of both its entries,
    so that the plot shows whether it was found; so must one pair at a distance >= 4 always.  -> (suffixes, offset)"""
    rng = np.random.default_rng([k, tag, int(near)])
    for _ in range(20000):
        suf = family(rng, BLOCK, k)
        if len(suf) != BLOCK:
            continue
        pair = one_away(suf)
        deg = pair.sum(axis=1)
        for off in range(8, BLOCK - 7):
            got, pairs = cases(pair, 0, BLOCK - 1, off, win)
            if got != FAR | {f"d{d}" for d in near}:
                continue
            alone = [(i, j) for i, j in pairs if deg[i] == 1 and deg[j] == 1]
            if len(near) == 1 and not any(j - i == int(near) for i, j in alone):
                continue
            if not any(j - i >= 4 for i, j in alone):      # a far pair that enters the plot
                continue
            return suf, off
    raise AssertionError(f"no seam block for k={k} near={near}")


@functools.lru_cache(maxsize=None)
def seam_table(k, near):
    """About three tiles of entries whose two inner seams each cut a seam_block at its offset.  In table order: k-mers a.. (their
    complements behind the first block or at the end), block one (ca..), k-mers cc.., block two (ga..), families as the blocks
    (gc.. to gt..), and, starting with t, the complements of everything that ends with a.
    -> (packed, counts, the oracle's plot, (seam, seam))"""
    lim = limits()
    own, win = lim["D_OWN"], lim["D_WIN"]
    p0 = k // 2
    rng = np.random.default_rng([k, 77, int(near)])
    (suf1, off1), (suf2, off2) = seam_block(k, near, 1, win), seam_block(k, near, 2, win)
    between = own - off2 + off1 - BLOCK                   # entries between the blocks
    n_front = own - off1                                  # ... in front of the first one
    n_mid = min(n_front, between)                         # k-mers a..ag: their complements ct.. stand between the blocks

    def singles(m, head, tail):
        rows = rng.integers(0, 4, (m, k), dtype=np.uint8)
        rows[:, : len(head)] = head
        rows[:, k - len(tail):] = tail
        return rows

    def block(head, suf):
        rows = np.empty((len(suf), k), np.uint8)
        rows[:, :p0] = rng.integers(0, 4, p0, dtype=np.uint8)
        rows[:, : len(head)] = head
        rows[:, p0:] = suf
        return rows

    rows = [singles(n_mid, [A], [A, G]), singles(n_front - n_mid, [A], [A]), block([C, A], suf1),
            singles(between - n_mid, [C, C], [A]), block([G, A], suf2)]
    have = 2 * sum(len(r) for r in rows)
    while have < 3 * own - BLOCK:                         # families behind the second block, 5 .. 40 entries each
        suf = family(rng, int(rng.integers(5, BLOCK + 1)), k)
        rows.append(block([G, int(rng.integers(1, 4))], suf))
        have += 2 * len(suf)
    packed = ktab.pack_bases(np.concatenate(rows))
    cnt = rng.integers(5, 60, len(packed)).astype(np.uint16)
    packed, cnt = ktab.sort_unique_packed(packed, cnt)
    packed, cnt = ktab.symmetrize(packed, cnt, k)
    cnt = cnt.astype(np.uint16)
    assert len(cnt) == have, "two k-mers of the table are equal"
    for a in (packed, cnt):
        a.setflags(write=False)
    return packed, cnt, brute.hetmers_plot(packed, cnt, k), (own, 2 * own)


def assert_seams(packed, cnt, k, near, seams):
    """from the sorted table itself: what the issue of this test wants on each inner seam"""
    win = limits()["D_WIN"]
    bases = ktab.unpack_bases(packed, k)
    assert 3 * seams[0] - BLOCK <= len(cnt) <= 3 * seams[0] + 2 * BLOCK
    pa, pb, _ = brute.unique_pairs(packed, cnt, k)
    in_plot = set(zip(pa.tolist(), pb.tolist()))
    for s in seams:
        got, pairs = crossing(bases, k, s, win)
        assert got == FAR | {f"d{d}" for d in near}, (k, near, s, got)
        for i, j in pairs:
            if j - i <= 3:
                assert i >= s - 3                          # the lower entry is among the last three of its tile
        if len(near) == 1:                                 # the one near pair enters the plot: a miss shows
            assert any(j - i == int(near) and (i, j) in in_plot for i, j in pairs), (k, near, s)
        assert any(j - i >= 4 and (i, j) in in_plot for i, j in pairs), (k, near, s)


@pytest.mark.parametrize("near", ["123", "1", "2", "3"])
@pytest.mark.parametrize("k", KS)
def test_pairs_and_long_blocks_across_both_inner_seams(k, near, monkeypatch):
    packed, cnt, want, seams = seam_table(k, near)
    assert_seams(packed, cnt, k, near, seams)
    got = {}
    for name, env, var in forms(k) + (("general", {"NO_INDEX_DIR": 1}, 1), ("general two-way", {"NO_INDEX_DIR": 1, "TWO_WAY": 1}, 1)):
        clear(monkeypatch, **env)
        got[name] = check_run(packed, cnt, want, k, env, var, f"k={k} near={near} {name}")
    # the hot forms send what the general form sends under the same protocol
    assert got[forms(k)[0][0]] == got["general"], got
    assert got[forms(k)[1][0]] == got["general two-way"], got


@pytest.mark.parametrize("k", KS)
def test_every_grid_of_pass1_across_the_seams(k, monkeypatch):
    packed, cnt, want, seams = seam_table(k, "123")
    assert_seams(packed, cnt, k, "123", seams)
    got = {}
    for grid in (1, 2, None):
        for name, env, var in forms(k):
            if grid is not None:
                env = dict(env, P1_GRID=grid)
            clear(monkeypatch, **env)
            b = Bound(packed, cnt, k)
            try:
                plot, st, form = b.run()
                ls = b.e.lookup_state()
            finally:
                b.close()
            assert form["var"] == var and st["path"] == 1, (name, grid, form, st)
            if grid is not None:
                assert ls["p1_grid"] == grid, ls
            assert np.array_equal(plot, want), (name, grid)
            got.setdefault(name, set()).add((st["nemitted"], st["nrequests"]))
    # the requests are a function of the table, not of the grid
    assert all(len(v) == 1 for v in got.values()), got
