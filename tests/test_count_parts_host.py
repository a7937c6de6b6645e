"""Key-range partitioned counting, host side, no GPU: the cut chooser (`smg_count_plan`) against its contract and against a
dynamic programme for the fewest contiguous ranges, and the `-p` argument errors of the `smg_count` executable."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from smudgeplot_amd import count

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
BINS = 4096


def histograms():
    rng = np.random.default_rng(42)
    h = {}
    h["random"] = rng.integers(0, 1000, BINS).astype(np.uint64)
    h["random_wide"] = (rng.integers(0, 1 << 20, BINS) ** 2).astype(np.uint64)          # up to 2^40 per bin
    hot = rng.integers(0, 50, BINS).astype(np.uint64)
    hot[1234] = 90_000
    h["one_hot_bin"] = hot
    gaps = rng.integers(1, 500, BINS).astype(np.uint64)
    gaps[100:900] = 0
    gaps[2000:2001] = 0
    gaps[3000:] = 0
    h["empty_stretches"] = gaps
    last = np.zeros(BINS, np.uint64)
    last[BINS - 1] = 77_777
    h["all_in_the_last_bin"] = last
    first = np.zeros(BINS, np.uint64)
    first[0] = 5
    h["all_in_the_first_bin"] = first
    h["empty"] = np.zeros(BINS, np.uint64)
    return h


HISTS = histograms()


def fewest_ranges(w, budget):
    """fewest contiguous ranges of bins with at most `budget` windows each: best[i] over prefixes, two pointers
    (the leftmost feasible start of a range that ends at i gives the minimum because best[] does not decrease)"""
    cum = np.concatenate([[0], np.cumsum(w.astype(object))])
    best = [0] * (BINS + 1)
    j = 0
    for i in range(1, BINS + 1):
        while cum[i] - cum[j] > budget:
            j += 1
        assert j < i
        best[i] = best[j] + 1
    return best[BINS]


@pytest.mark.parametrize("name", sorted(HISTS))
def test_greedy_cuts_cover_fit_and_are_minimal(name):
    w = HISTS[name]
    top, total = int(w.max()), int(w.astype(object).sum())
    for budget in sorted({max(top, 1), max(top, 1) + 1, 2 * max(top, 1), max(total // 7, top, 1), max(total // 2, top, 1),
                          max(total, 1), 10 * max(total, 1)}):
        cuts = count.plan(w, budget)
        assert cuts[0] == 0 and cuts[-1] == BINS
        assert np.all(np.diff(cuts) > 0)                                   # ascending: every bin in exactly one range
        sums = [int(w[a:b].astype(object).sum()) for a, b in zip(cuts[:-1], cuts[1:])]
        assert max(sums) <= budget, (name, budget)
        assert sum(sums) == total
        assert len(cuts) - 1 == fewest_ranges(w, budget), (name, budget)
    if total <= 10:
        assert len(count.plan(w, 10)) == 2                                  # one range


@pytest.mark.parametrize("name", sorted(HISTS))
@pytest.mark.parametrize("parts", [1, 2, 3, 7, 64, 4096])
def test_requested_number_of_ranges(name, parts):
    w = HISTS[name]
    cuts = count.plan(w, 0, partitions=parts)
    assert len(cuts) == parts + 1 and cuts[0] == 0 and cuts[-1] == BINS
    assert np.all(np.diff(cuts) > 0)
    if name == "random" and parts in (2, 3, 7, 64):                         # an equal share, as close as whole bins allow
        total = int(w.sum())
        sums = np.array([int(w[a:b].sum()) for a, b in zip(cuts[:-1], cuts[1:])])
        assert np.all(np.abs(sums - total / parts) <= 2 * int(w.max()))


def test_a_bin_above_the_budget_is_refused_and_named():
    w = HISTS["one_hot_bin"]
    with pytest.raises(count.CountError) as e:
        count.plan(w, 89_999)
    assert e.value.code == -3
    msg = str(e.value)
    assert "bin 1234 " in msg and "90000 windows" in msg and "89999" in msg
    assert "begin with " + "".join("acgt"[(1234 >> s) & 3] for s in (10, 8, 6, 4, 2, 0)) in msg
    count.plan(w, 90_000)
    with pytest.raises(count.CountError) as e:
        count.plan(HISTS["all_in_the_last_bin"], 77_776)
    assert "bin 4095 " in str(e.value) and "tttttt" in str(e.value)
    for bad in (-1, 4097):
        with pytest.raises(count.CountError) as e:
            count.plan(w, 100_000, partitions=bad)
        assert e.value.code == -2 and "out of range 0 .. 4096" in str(e.value)
    with pytest.raises(count.CountError) as e:
        count.plan(w, 0)
    assert e.value.code == -2


def test_smg_count_partition_argument_errors_write_nothing(tmp_path):
    (tmp_path / "r.fa").write_bytes(b">a\nACGTACGTACGTACGTACGT\n")
    for args, msg in ((["-p4097", "r.fa"], "Number of key ranges must be 0 .. 4096 (4097)"),
                      (["-p-1", "r.fa"], "Number of key ranges must be 0 .. 4096 (-1)"),
                      (["-px", "r.fa"], "argument is not an integer"),
                      (["-p", "r.fa"], "argument is not an integer"),
                      (["-p4x", "-k21", "r.fa"], "argument is not an integer")):
        r = subprocess.run([COUNT_BIN, *args], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 1, (args, r.stderr)
        assert msg in r.stderr, (args, r.stderr)
        assert sorted(os.listdir(tmp_path)) == ["r.fa"], args
    r = subprocess.run([COUNT_BIN], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "[-p<int(0)>]" in r.stderr and "-p: count in this many ranges" in r.stderr
