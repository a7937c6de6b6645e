"""Key ranges finer than a 12-bit bin, host side, no GPU: the flat planner (`smg_count_plan_fine`) over whole bins and the 4096
sub-bins of every split bin -- budget, cover, fewest ranges, ranges that leave a split bin, the refusal of a sub-bin -- and
`smg_count_plan`, which must give what it gave before the flat planner existed (tests/golden/count_plan.json)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from smudgeplot_amd import count
from test_count_parts_host import HISTS

BINS, FINE = 4096, 1 << 24
GOLDEN = os.path.join(ROOT, "tests", "golden", "count_plan.json")


def lead(v, bases):
    return "".join("acgt"[(v >> (2 * (bases - 1 - j))) & 3] for j in range(bases))


def cases():
    """name -> (windows[4096], {split bin: sub-bin windows[4096]})"""
    rng = np.random.default_rng(24)
    c = {}

    def sub_of(total, occupied, top):
        s = np.zeros(BINS, np.uint64)
        at = rng.choice(BINS, occupied, replace=False)
        s[at] = rng.integers(1, top, occupied).astype(np.uint64)
        s[at[0]] += np.uint64(total - int(s.sum())) if total > int(s.sum()) else np.uint64(0)
        return s

    w = rng.integers(0, 300, BINS).astype(np.uint64)
    split = {0: sub_of(40_000, 2100, 30), 1365: sub_of(15_000, 900, 30)}
    for b, s in split.items():
        w[b] = s.sum()
    c["two_hot_bins"] = (w, split)

    w = rng.integers(0, 300, BINS).astype(np.uint64)                        # neighbours, and the last bin of all
    split = {7: sub_of(9000, 4096, 5), 8: sub_of(12_000, 10, 2000), 4095: sub_of(20_000, 333, 100)}
    for b, s in split.items():
        w[b] = s.sum()
    c["neighbours_and_last"] = (w, split)

    w = np.zeros(BINS, np.uint64)                                           # everything in one bin, spread evenly
    s = np.full(BINS, 3, np.uint64)
    w[2000] = s.sum()
    c["one_bin_only"] = (w, {2000: s})

    w = rng.integers(0, 300, BINS).astype(np.uint64)                        # a split bin that would have fitted
    s = sub_of(200, 50, 5)
    w[99] = s.sum()
    c["split_without_need"] = (w, {99: s})
    return c


CASES = cases()


def units_of(w, split):
    """the flat sequence the planner cuts: (24-bit start, windows) per whole bin and per sub-bin of a split bin"""
    u = []
    for b in range(BINS):
        if b in split:
            u += [((b << 12) + j, int(split[b][j])) for j in range(BINS)]
        else:
            u.append((b << 12, int(w[b])))
    return u


def greedy(units, budget):
    """a range takes units while its windows stay within the budget"""
    cuts, run = [0], 0
    for at, n in units:
        assert n <= budget
        if run + n > budget:
            cuts.append(at)
            run = 0
        run += n
    return cuts + [FINE]


def fewest(units, budget):
    """fewest contiguous ranges, by a programme over prefixes that does not know the greedy rule"""
    cum = [0]
    for _, n in units:
        cum.append(cum[-1] + n)
    best, j = [0] * (len(units) + 1), 0
    for i in range(1, len(units) + 1):
        while cum[i] - cum[j] > budget:
            j += 1
        best[i] = best[j] + 1
    return best[-1]


def plan_fine(w, split, budget):
    bins = sorted(split)
    return count.plan_fine(w, bins, np.stack([split[b] for b in bins]) if bins else np.zeros((0, BINS), np.uint64), budget)


def windows_between(units, lo, hi):
    return sum(n for at, n in units if lo <= at < hi)


@pytest.mark.parametrize("name", sorted(CASES))
def test_flat_cuts_cover_fit_and_are_the_fewest(name):
    w, split = CASES[name]
    units = units_of(w, split)
    top = max(n for _, n in units)
    total = sum(n for _, n in units)
    assert total == int(w.astype(object).sum())
    for budget in sorted({top, top + 1, 2 * top, max(total // 50, top), max(total // 7, top), total, 10 * total}):
        cuts = plan_fine(w, split, budget)
        assert cuts[0] == 0 and cuts[-1] == FINE
        assert np.all(np.diff(cuts.astype(np.int64)) > 0)                   # ascending: every unit in exactly one range
        for c in cuts:
            assert c % BINS == 0 or (c >> 12) in split, c                   # a whole bin is never cut
        sums = [windows_between(units, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        assert max(sums) <= budget and sum(sums) == total, (name, budget)
        assert list(cuts) == greedy(units, budget), (name, budget)
        assert len(cuts) - 1 == fewest(units, budget), (name, budget)


def test_a_range_leaves_a_split_bin_and_takes_the_whole_bins_behind_it():
    w = np.zeros(BINS, np.uint64)
    s = np.zeros(BINS, np.uint64)
    s[10], s[20], s[4000] = 60, 60, 30                                      # bin 5: 150 windows, budget 100
    w[5], w[6], w[7], w[9] = 150, 40, 20, 90
    cuts = count.plan_fine(w, [5], s[None, :], 100)
    # [0, 5:20) holds 60; [5:20, 6:0) holds 60 + 30, and the 40 of bin 6 would be above 100; [6:0, 9:0) holds 40 + 20
    assert list(cuts) == [0, (5 << 12) + 20, 6 << 12, 9 << 12, FINE]
    s[4000] = 5                                                             # 60 + 5 + 20 + 10 fits: from inside bin 5 to bin 9
    w[5], w[6], w[7] = 125, 20, 10
    cuts = count.plan_fine(w, [5], s[None, :], 100)
    assert list(cuts) == [0, (5 << 12) + 20, 9 << 12, FINE]
    lo, hi = int(cuts[1]), int(cuts[2])
    assert lo % BINS != 0 and lo >> 12 == 5 and hi % BINS == 0 and (hi >> 12) > 6
    # and into a split bin from the whole bins in front of it
    w2 = np.zeros(BINS, np.uint64)
    w2[3], w2[5] = 70, 125
    cuts = count.plan_fine(w2, [5], s[None, :], 100)
    assert list(cuts) == [0, (5 << 12) + 10, (5 << 12) + 20, FINE]         # 70 | 60 | 60 + 5: 70 + 60 is above 100 ...
    w2[3] = 40
    cuts = count.plan_fine(w2, [5], s[None, :], 100)
    assert list(cuts) == [0, (5 << 12) + 20, FINE]                          # ... 40 + 60 is not


def test_a_sub_bin_above_the_budget_is_refused_with_both_names():
    w, split = CASES["neighbours_and_last"]
    b = 8
    j = int(np.argmax(split[b]))
    n = int(split[b][j])
    with pytest.raises(count.CountError) as e:
        plan_fine(w, split, n - 1)
    assert e.value.code == -3
    msg = str(e.value)
    head = (f"bin {b} (canonical k-mers that begin with {lead(b, 6)}) holds {int(w[b])} windows, one merge holds {n - 1} entries")
    assert head in msg and msg.index(head) == len("smg_count error -3: ")
    assert f"sub-bin {j} " in msg and f"begin with {lead((b << 12) + j, 12)}" in msg and f"holds {n} windows" in msg
    assert "cannot be split" in msg
    plan_fine(w, split, n)
    # a whole bin above the budget that was not split cannot be planned: the caller has to hand its sub-bins over
    with pytest.raises(count.CountError) as e:
        count.plan_fine(w, [7], split[7][None, :], n)
    assert e.value.code == -2 and "bin 8 " in str(e.value)


def test_bad_arguments_of_the_flat_planner():
    w, split = CASES["two_hot_bins"]
    sub = np.stack([split[0], split[1365]])
    for bins in ([1365, 0], [0, 0], [0, 4096], [-1, 0]):
        with pytest.raises(count.CountError) as e:
            count.plan_fine(w, bins, sub, 10 ** 6)
        assert e.value.code == -2, bins
    wrong = sub.copy()
    wrong[1, 17] += np.uint64(1)                                            # sub-bins that do not add up to their bin
    with pytest.raises(count.CountError) as e:
        count.plan_fine(w, [0, 1365], wrong, 10 ** 6)
    assert e.value.code == -2 and "bin 1365 " in str(e.value)
    with pytest.raises(count.CountError) as e:
        count.plan_fine(w, [0, 1365], sub, 0)
    assert e.value.code == -2
    with pytest.raises(ValueError):
        count.plan_fine(w, [0], sub, 10 ** 6)


@pytest.mark.parametrize("name", sorted(HISTS))
def test_without_split_bins_the_flat_planner_is_the_coarse_one(name):
    w = HISTS[name]
    top, total = max(int(w.max()), 1), max(int(w.astype(object).sum()), 1)
    for budget in (top, max(total // 7, top), total):
        fine = count.plan_fine(w, [], np.zeros((0, BINS), np.uint64), budget)
        assert np.array_equal(fine.astype(np.int64), count.plan(w, budget).astype(np.int64) << 12)


def test_smg_count_plan_gives_what_it_gave():
    """cuts and refusal text recorded from the build before the flat planner (tests/golden/make_count_plan_golden.py)"""
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert len(gold["cuts"]) >= 80
    for g in gold["cuts"]:
        cuts = count.plan(HISTS[g["hist"]], g["budget"], partitions=g["partitions"])
        assert cuts.dtype == np.int32 and len(cuts) - 1 == g["ranges"], g
        assert hashlib.sha256(cuts.astype("<i4").tobytes()).hexdigest() == g["sha256"], g
    assert len(gold["refused"]) >= 2
    for g in gold["refused"]:
        with pytest.raises(count.CountError) as e:
            count.plan(HISTS[g["hist"]], g["budget"])
        assert e.value.code == -3 and str(e.value) == g["message"]
