"""What the tables of tests/sum_limit_oracle.py hold, asserted on the CPU: tests/test_sum_limit_gpu.py relies on every line of it.
A table that does not put its families where its docstring says, or whose plot does not hang on the sum limit, fails here and
not on the device.  Every threshold comes from the library (engine.pass1_limits, wide_limits, pass2_limits: no device needed)."""
import collections
import functools

import numpy as np
import pytest

import brute
import lookup_oracle as lo
import pass2_oracle as po
import sum_limit_oracle as so
import wide_oracle as wo
from conftest import load_golden
from smudgeplot_amd import engine, ktab

U = np.uint64


@functools.lru_cache(maxsize=None)
def limits():
    p1, wide = engine.pass1_limits(), engine.wide_limits()
    assert wide["CODE_REACH"] == po.REACH and p1["D_WIN"] < so.LONG_SIZES[0] and wide["F_HALO"] < so.LONG_SIZES[0]
    assert wide["BB_LIN"] < p1["D_WIN"], "blocks of the deferred route on both sides of the walk's linear reads"
    return p1, wide


def mid(k):
    p1, wide = limits()
    return so.mid_of(k, p1["D_WIN"], wide["F_HALO"])


def tile_of(k):
    p1, wide = limits()
    return p1["D_OWN"] if k <= 64 else wide["F_TILE"]


@functools.lru_cache(maxsize=None)
def analysed(k, route):
    t = so.route_table(k, route, mid(k))
    return t, wo.analyse(t.packed, t.cnt, k)


ALL_KS = so.KS_NARROW + so.KS_WIDE + so.KS_COUNTED


def check_families(t, a):
    """every family has the degrees of its kind on both images; -> {(kind, route): families}"""
    deg = a.cls.s_all + a.cls.pre
    seen = collections.Counter()
    for pl in so.place(t):
        want = so.DEGREES[pl.fam.kind]
        assert tuple(deg[pl.idx]) == want and tuple(deg[pl.rc]) == want, (pl.fam.kind, pl.idx, deg[pl.idx], deg[pl.rc])
        assert (t.cnt[pl.idx] == pl.fam.counts).all() and (t.cnt[pl.rc] == pl.fam.counts).all()
        if pl.fam.kind in so.DECIDED:                                  # the two light members name each other, nobody names the decoy
            both = a.cls.s_all + a.cls.pre
            assert both[pl.suffix[2]] == 0 and a.cls.partner[pl.suffix[0]] == pl.suffix[1] and a.cls.partner[pl.suffix[1]] == pl.suffix[0]
            assert a.cls.pos[pl.suffix[0]] >= t.k // 2
        seen[(pl.fam.kind, so.route_of(pl, mid(t.k)))] += 1
    return seen


@pytest.mark.parametrize("route", so.ROUTES)
@pytest.mark.parametrize("k", ALL_KS)
def test_every_kind_stands_on_its_route_eight_times(k, route):
    t, a = analysed(k, route)
    seen = check_families(t, a)
    assert set(seen) == {(kind, route) for kind in so.KINDS}, seen
    assert min(seen.values()) >= 8, seen
    ntiles = len(t.cnt) / tile_of(k)
    assert 3 <= ntiles <= 5, (len(t.cnt), ntiles)
    assert int(t.cnt.max()) == 32767


@pytest.mark.parametrize("route", so.ROUTES)
@pytest.mark.parametrize("k", ALL_KS)
def test_the_plot_exists_only_because_decoys_are_ignored(k, route):
    t, a = analysed(k, route)
    decided = sum(1 for f in t.fams if f.kind in so.DECIDED)
    assert a.plot.sum() == 2 * decided > 0                              # a pair and its mirror image
    assert a.plot[1000, 500] >= 16 and a.plot[1000, 499] >= 16          # (the boundary families: the first is never printed)
    assert brute.hetmers_plot(t.packed, so.lightened(t.cnt), k).sum() == 0


@pytest.mark.parametrize("route", so.ROUTES)
@pytest.mark.parametrize("k", ALL_KS)
def test_the_oracles_agree_on_degrees_and_senders(k, route):
    """oracle/brute.py, pass2_oracle.classify, wide_oracle.analyse and (k <= 32) lookup_oracle restate the limit independently"""
    t, a = analysed(k, route)
    deg = a.cls.s_all + a.cls.pre
    pa, pb, pp = brute.unique_pairs(t.packed, t.cnt, k)
    assert (deg[pa] == 1).all() and (deg[pb] == 1).all() and len(pa) == a.plot.sum()
    mine = np.flatnonzero((deg == 1) & (a.cls.s_all == 1) & (a.cls.partner > np.arange(len(deg))))
    mine = mine[deg[a.cls.partner[mine]] == 1]
    keep = pp >= k // 2
    assert sorted(zip(pa[keep].tolist(), pb[keep].tolist())) == sorted(zip(mine.tolist(), a.cls.partner[mine].tolist()))
    assert np.array_equal(wo.flag_plot(a, a.cls.pre > 0), a.plot)
    if k <= 32:
        keys = ktab.packed_to_u64(t.packed)
        assert np.array_equal(lo.owns_hi_pair(keys, t.cnt, k), a.s_hi > 0)
        assert np.array_equal(lo.pair_counts(keys, t.cnt, k, range(k // 2, k)), a.cls.s_all)
        # the senders of kf_pass1_d: lookup_oracle's rules and, where two or more pairs all stand on the middle position, one more
        relaxed = (a.cls.s_all >= 2) & (a.s_hi == 0)
        assert np.array_equal(so.senders(a, False), lo.owns_hi_pair(keys, t.cnt, k) | relaxed)
        assert relaxed.any() == (route == "registers" and k & 1 == 1)
        if k & 1:
            rec, send = lo.emitted_one_way(keys, t.cnt, k)
            lower = ((keys >> U(64 - k)) & U(1)) == U(0)
            assert np.array_equal(np.sort(send), np.flatnonzero(lower & ((a.s_hi > 0) | (a.cls.s_all == 1))))
            assert np.array_equal(rec & U(1), (a.s_hi[send] > 0).astype(U))
            assert np.array_equal(np.flatnonzero(so.senders(a, True)), np.sort(np.r_[send, np.flatnonzero(lower & relaxed)]))


@pytest.mark.parametrize("k", so.KS_NARROW)
def test_long_blocks_hold_far_pairs_and_the_decoy_on_either_side_of_the_partner(k):
    t, a = analysed(k, "long")
    order = collections.Counter()
    far = 0
    for pl in so.place(t):
        if pl.fam.kind in so.DECIDED and pl.fam.kind != "side":
            low, high, decoy = min(pl.suffix[:2]), max(pl.suffix[:2]), pl.suffix[2]
            order["front" if decoy < low else "between" if decoy < high else "behind"] += 1
            far += high - low > po.REACH
    assert min(order[w] for w in ("front", "between", "behind")) >= 4, order
    assert far >= 8
    assert po.far(a.cls).sum() >= 8


@pytest.mark.parametrize("k", so.KS_NARROW)
def test_deferred_blocks_stand_on_both_sides_of_the_linear_reads(k):
    """big_block_walk reads a block of at most BB_LIN entries eight at a time and bisects a longer one first"""
    t, _ = analysed(k, "deferred")
    lin = limits()[1]["BB_LIN"]
    sizes = [pl.size for pl in so.place(t)]
    assert sum(s <= lin for s in sizes) >= 8 and sum(s > lin for s in sizes) >= 8


@pytest.mark.parametrize("k", so.KS_NARROW)
def test_shifted_tables_put_families_on_every_entry_of_a_thread(k):
    t0 = so.route_table(k, "registers", mid(k))
    at0 = [pl.suffix for pl in so.place(t0)]
    firsts = set()
    for s in range(4):
        t = so.shifted(k, s, mid(k))
        assert t.nfill == s and len(t.cnt) == len(t0.cnt) + 2 * s
        deg = so.degrees(t.packed, t.cnt, k)
        assert (deg[:s] == 0).all() and (deg[len(deg) - s:] == 0).all()          # the fillers and their complements: no neighbour
        for was, pl in zip(at0, so.place(t)):
            assert np.array_equal(pl.suffix, was + s)
        assert np.array_equal(brute.hetmers_plot(t.packed, t.cnt, k), brute.hetmers_plot(t0.packed, t0.cnt, k))
        firsts |= {(int(min(pl.suffix)) % 4, len(pl.fam.rows)) for pl in so.place(t) if pl.size == len(pl.fam.rows)}
    assert firsts == {(e, m) for e in range(4) for m in (3, 4)}


@pytest.mark.parametrize("members,low", so.SPLITS)
@pytest.mark.parametrize("seam_no", [1, 2])
@pytest.mark.parametrize("k", so.KS_NARROW)
def test_seam_tables_split_a_family_as_they_say(k, seam_no, members, low):
    own = limits()[0]["D_OWN"]
    t, n = so.seam_table(k, mid(k), own, seam_no, members, low)
    pl = so.place(t)[n]
    assert len(t.cnt) > seam_no * own + members
    assert sorted(pl.suffix.tolist()) == list(range(seam_no * own - low, seam_no * own - low + members))
    assert pl.fam.kind in (so.DECIDED if members == 3 else ("four",))
    t0 = so.route_table(k, "registers", mid(k))
    assert np.array_equal(brute.hetmers_plot(t.packed, t.cnt, k), brute.hetmers_plot(t0.packed, t0.cnt, k))


@pytest.mark.parametrize("k", so.KS_NARROW)
def test_the_sparse_table_has_tiles_with_and_without_a_heavy_count(k):
    own = limits()[0]["D_OWN"]
    t = so.sparse_table(k, 100 + k)
    assert 3 <= len(t.cnt) / own <= 5
    heavy = np.bincount(np.flatnonzero(t.cnt > 500) // own, minlength=-(-len(t.cnt) // own))
    assert (heavy > 0).any() and (heavy == 0).sum() >= 2, heavy
    quarter = np.bincount(np.flatnonzero(t.cnt > 500) // (own // 4), minlength=-(-len(t.cnt) // (own // 4)))
    assert (quarter > 0).sum() >= 2 and (quarter == 0).sum() > (quarter > 0).sum()
    plot = brute.hetmers_plot(t.packed, t.cnt, k)
    assert plot.sum() == 16 and brute.hetmers_plot(t.packed, so.lightened(t.cnt), k).sum() == 0


# ---- the wrap of a uint8 degree together with the limit -------------------------------------------------------------------------------

def test_wrap_cases_count_or_not_because_of_the_limit():
    k = 100
    t, hubs = so.wrap_table(k, 5, per_kind=2, mid=mid(k), n_pairs=250)
    deg = so.degrees(t.packed, t.cnt, k)
    pa, pb, _ = brute.unique_pairs(t.packed, t.cnt, k)
    pairs = set(zip(pa.tolist(), pb.tolist()))
    la, lb, _ = brute.unique_pairs(t.packed, so.lightened(t.cnt), k)
    light = set(zip(la.tolist(), lb.tolist()))
    sides = set()
    for at, (x, y, h), want in hubs:
        ix, iy, ih = (so.index_of(t, t.rows[at + j]) for j in (x, y, h))
        assert deg[ix] == want and deg[iy] == 1 and t.cnt[ih] == 996
        pair = (min(ix, iy), max(ix, iy))
        # 255: too many; 256 wraps to 0 and the pair counts.  Without the limit: 256 (counts), 257 = 1 (counts, and so does the decoy)
        assert (pair in pairs) == (want == 256) and pair in light
        sides.add((want, bool((t.rows[at + h] != t.rows[at + x]).argmax() < k // 2)))
    assert sides == {(255, False), (255, True), (256, False), (256, True)}
    assert not np.array_equal(brute.hetmers_plot(t.packed, t.cnt, k), brute.hetmers_plot(t.packed, so.lightened(t.cnt), k))


# ---- fixtures --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(so.FIXTURES))
def test_fixtures_are_the_generators_tables_and_hang_on_the_limit(name):
    g = load_golden(name)
    k = g["k"]
    t = so.fixture_table(name, mid(k))
    assert k == so.FIXTURES[name] and np.array_equal(g["packed"], t.packed) and np.array_equal(g["counts"], t.cnt)
    assert int(t.cnt.max()) == 32767 and int(t.cnt.min()) >= g["L"]
    a = wo.analyse(t.packed, t.cnt, k)
    seen = check_families(t, a)
    assert set(seen) == {(kind, route) for kind in so.KINDS for route in so.ROUTES} and min(seen.values()) >= 2, seen
    assert brute.smu_text(a.plot) == g["smu"]
    assert "499\t501\t" in g["smu"] and "500\t500\t" not in g["smu"] and a.plot[1000, 500] > 0
    assert brute.smu_text(brute.hetmers_plot(t.packed, so.lightened(t.cnt), k)) != g["smu"]


# ---- counts beyond int16 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 51, 70, 100])
def test_tables_beyond_int16_hold_every_route_and_every_count(k):
    t = so.beyond_int16_table(k, 100 + k, mid=mid(k))
    a = wo.analyse(t.packed, t.cnt, k)
    seen = check_families(t, a)
    assert {r for _, r in seen} == set(so.ROUTES)
    assert set(so.BEYOND_INT16) <= set(t.cnt.tolist())
    assert a.plot.sum() > 0 and brute.hetmers_plot(t.packed, so.lightened(t.cnt), k).sum() == 0
