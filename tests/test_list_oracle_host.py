"""What tests/list_oracle.py promises to tests/test_list_lookups_gpu.py, asserted without a GPU: its semantics against independent code
(oracle/brute.py: flag_plot of all senders' rows is the plot), and that every generated table puts its entries where the list route
changes regime.  The thresholds come from engine.list_limits, the directory of a table from engine.pass1_plan."""
import functools

import numpy as np
import pytest

import list_oracle as lz
import lookup_oracle as lo
from smudgeplot_amd import engine

U = np.uint64


@functools.lru_cache(maxsize=None)
def lim():
    return engine.list_limits()


def form(k, proof, have_index):
    """(entries per directory bucket, bytes of the prefix index that serves as directory or 0, signatures) of a phase-API pass 1"""
    p = engine.pass1_plan(k, 5000, proof, own_lookups=False, have_index=have_index, bm_cap=30)
    return p["dir_per"], 3 if p["dir_preset"] else 0, bool(p["use_sig"])


def all_rows_give_the_plot(t):
    assert np.array_equal(lz.flag_plot(t, lz.flagged_by(t, lz.key_rows(t))), t.plot)
    for exact in (False, True):
        rows = lz.meta_rows(t, exact)
        assert rows.shape[1] == t.words.shape[1] + 1 and lz.missing_of(t, rows, True) == 0
        assert np.array_equal(lz.flag_plot(t, lz.flagged_by(t, rows)), t.plot)
    assert len(lz.meta_rows(t, True)) == len(t.cnt)
    if t.k & 1:
        rows = lz.one_way_rows(t)
        assert np.array_equal(lz.flag_plot(t, lz.flagged_by_one_way(t, rows)), t.plot)
    # no flag at all: the pairs that only a flag keeps out come in
    none = lz.flag_plot(t, np.zeros(len(t.cnt), bool))
    assert int(none.sum() - t.plot.sum()) >= lz.held_by_flag_alone(t) > 0


def test_the_limits_are_ordered_as_the_tests_assume():
    L = lim()
    assert L["SORT_MIN"] < L["APPLY_SORT_MIN"] < L["FILTER_SORT_MIN"] and L["F_CH"] <= L["SORT_MIN"]
    assert L["SORT_MIN"] == engine.wide_limits()["SORT_MIN"] and L["F_CH"] == engine.lookup_limits()["F_CH"]


@pytest.mark.parametrize("k", lz.KS)
def test_flag_table(k):
    L = lim()
    t = lz.flag_table(k, L["SORT_MIN"] + 2)
    assert t.words.shape[1] == lz.words_per(k)
    all_rows_give_the_plot(t)
    rows = lz.key_rows(t)
    assert len(rows) >= L["SORT_MIN"] + 2 and len(np.unique(rows, axis=0)) == len(rows) and len(lz.deciding(t)) >= 2
    assert len(t.cnt) >= L["SORT_MIN"]                                 # (the exact proof sends every entry)
    # a meta row with bit 16 clear does not flag: the rows of the entries that do not send change nothing
    meta = lz.meta_rows(t, True)
    quiet = (meta[:, -1] >> U(16)) & U(1) == 0
    assert quiet.sum() > 100 and not lz.flagged_by(t, meta[quiet]).any()
    # the ordered list: the cut in front of a deciding row, the cut behind it and the whole list give three plots
    for m, lst in ((L["SORT_MIN"], lz.apply_list(t, rows, L["SORT_MIN"])), (L["SORT_MIN"], lz.apply_list(t, meta, L["SORT_MIN"]))):
        plots = [lz.flag_plot(t, lz.flagged_by(t, lst[:c])) for c in (m - 1, m, len(lst))]
        assert not np.array_equal(plots[0], plots[1]) and not np.array_equal(plots[1], plots[2]) and np.array_equal(plots[2], t.plot)


@pytest.mark.parametrize("k", lz.KS1)
def test_repeated_list(k):
    """the list of the real threshold in small: every distinct row (or as many as the shortest cut holds) in front of the first
    cut, a deciding row at the second cut and one at the end"""
    L = lim()
    t = lz.flag_table(k, L["SORT_MIN"] + 2)
    rows = lz.key_rows(t)
    for m in (L["SORT_MIN"], 3 * L["SORT_MIN"]):
        cuts = (m - 1, m, 2 * m + 3)
        lst = lz.repeated_list(t, rows, cuts, k)
        assert len(lst) == cuts[2] and (lz.index_of_rows(t, lst) >= 0).all()
        distinct = len(np.unique(lst[: cuts[0]]))
        assert distinct == min(cuts[0], len(rows) - 2) and (m == L["SORT_MIN"] or distinct >= L["SORT_MIN"])
        assert not np.array_equal(lst[: cuts[0]], np.sort(lst[: cuts[0]], axis=0))          # (shuffled)
        plots = [lz.flag_plot(t, lz.flagged_by(t, lst[:c])) for c in cuts]
        assert not np.array_equal(plots[0], plots[1]) and not np.array_equal(plots[1], plots[2]) and not np.array_equal(plots[0], plots[2])
        if distinct == len(rows) - 2:
            assert np.array_equal(plots[2], t.plot)


@pytest.mark.parametrize("have_index", [True, False], ids=["prefix index", "own directory"])
@pytest.mark.parametrize("proof", ["hash", "exact"])
@pytest.mark.parametrize("k", lz.KS)
def test_signature_table(k, proof, have_index):
    per, ib, sig = form(k, proof, have_index)
    assert sig and (ib == 3) == (have_index and proof == "hash")
    t, sigsh, fams = lz.signature_table(k, per, ib)
    assert sigsh == lz.sig_shift(t, per, ib) and (not ib or sigsh == 64 - 24 - 16)
    all_rows_give_the_plot(t)
    runs = lz.runs_of(t, sigsh)
    lengths = []
    for f in fams:
        w, j, absent = lz.family_rows(t, f)
        lengths.append(f.length)
        # the run, read from the sorted table: the members and nobody else, next to each other
        assert (runs[j] == f.length).all() and np.array_equal(np.sort(j), np.arange(j.min(), j.min() + f.length))
        assert (w[:, 0] >> U(sigsh) == w[0, 0] >> U(sigsh)).all() and len(np.unique(w, axis=0)) == f.length
        # ... the absent k-mer has their bucket and signature, and stands inside a run of two or more
        assert lz.find_words(t.words, absent)[0] == -1 and absent[0, 0] >> U(sigsh) == w[0, 0] >> U(sigsh)
        if f.length >= 2:
            both = lo.sort_rows(np.concatenate([w, absent]))
            at = int(np.flatnonzero((both == absent[0]).all(axis=1))[0])
            assert 0 < at < f.length
        # targets are the members with a pair in front of k // 2: their complements send them
        assert np.array_equal(t.cls.pre[j] > 0, f.target) and np.array_equal(t.s_hi[t.rc[j]] > 0, f.target)
        if f.length >= 2:
            assert f.target.any() and not f.target.all()
        # candidates whose pair only the flag removes: one pair at p >= k // 2, the partner without a pair in front
        assert np.array_equal(t.cls.s_all[j] == 1, f.candidate)
        c = j[f.candidate]
        partner = t.cls.partner[c]
        assert (t.cls.s_all[partner] == 1).all() and (t.cls.partner[partner] == c).all()
        assert np.isin(c[f.target[f.candidate]], lz.deciding(t)).all()
        # (an odd member is a candidate only where a position p >= k // 2 lies in the bits the run shares)
        assert f.candidate[: f.length - f.length % 2].all()
        if f.length % 2:
            assert f.candidate[-1] == (k // 2 <= (64 - sigsh - 1) // 2)
    assert lengths[:4] == [1, 1, 2, 3] and [f.target[0] for f in fams[:2]] == [True, False]
    room = 4 ** max(k - 2 - max((64 - sigsh + 1) // 2, k // 2), 0)               # pairs the bits below the signature hold, two bases apart
    assert lengths[4] == min(64, 2 * (room - 1)) and lengths[5] == min(1000, 2 * (room - 1)) and lengths[5] >= 30
    # the flags of exactly the targets' rows: every non-target pair of a run is in the plot, none of a target
    rows = np.concatenate([lz.family_rows(t, f)[0][f.target] for f in fams])
    plot = lz.flag_plot(t, lz.flagged_by(t, rows))
    i, jj, wgt = lz.mutual_pairs(t)
    members = np.concatenate([lz.family_rows(t, f)[1] for f in fams])
    targets = np.concatenate([lz.family_rows(t, f)[1][f.target] for f in fams])
    inside = np.isin(i, members) & np.isin(jj, members)
    shown = inside & ~np.isin(i, targets) & ~np.isin(jj, targets)
    assert shown.sum() > len(members) // 8 and (inside & ~shown).sum() > len(members) // 8
    assert plot.sum() >= int(wgt[shown].sum())


def test_poly_t_table():
    L = lim()
    t = lz.brim_full_table(32, False, L["F_CH"], 3 * L["SORT_MIN"], True)
    all_rows_give_the_plot(t)
    last = len(t.cnt) - 1
    assert t.words[last, 0] == ~U(0) and t.words[0, 0] == U(0) and t.rc[last] == 0
    rows = lz.key_rows(t)
    assert rows[-1, 0] == ~U(0) and rows[0, 0] == U(0)                  # each of the two is sent by the other one
    assert last in lz.deciding(t).tolist() and 0 in lz.deciding(t).tolist()
    without = lz.flag_plot(t, lz.flagged_by(t, rows[:-1]))
    assert int(np.abs(without - t.plot).sum()) >= 1                      # the flag of T x 32 decides a cell
    assert 16 * lz.holes_of(len(rows), L["F_CH"]) < len(rows) >= 3 * L["SORT_MIN"]


@pytest.mark.parametrize("k,one_way", [(31, True), (24, False)])
def test_brim_full_tables(k, one_way):
    L = lim()
    t = lz.brim_full_table(k, one_way, L["F_CH"], 3 * L["SORT_MIN"])
    all_rows_give_the_plot(t)
    keys = t.words[:, 0]
    assert not lo.may_send_twice(keys, k).any()
    rows = lz.one_way_rows(t) if one_way else lz.key_rows(t)
    want = lo.emitted_one_way(keys, t.cnt, k)[0] if one_way else lo.emitted(keys, t.cnt, k)
    assert np.array_equal(rows[:, 0], want)                              # (the oracle of the look-up chain says the same)
    assert len(rows) >= 3 * L["SORT_MIN"] and 16 * lz.holes_of(len(rows), L["F_CH"]) < len(rows)


def test_small_tables_of_the_engines_own_lists():
    L = lim()
    t = lz.adversarial(10, 3000, 7)
    all_rows_give_the_plot(t)
    assert int((t.s_hi > 0).sum()) > L["F_CH"]                           # more than one chunk for the filter
    assert engine.pass1_plan(10, len(t.cnt), "hash", own_lookups=False, have_index=False, bm_cap=30)["nb"] == 0
    small, large = lz.adversarial(51, 500, 11), lz.adversarial(51, 8000, 11)
    for t in (small, large):
        all_rows_give_the_plot(t)
    assert len(small.cnt) < L["SORT_MIN"] <= len(lz.one_way_rows(large)) and 0 < len(lz.one_way_rows(small))
