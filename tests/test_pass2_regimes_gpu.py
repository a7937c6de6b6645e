"""Pass 2 (kf_pass2, kf_pass2_far, kf_pass2_farscan) and the extract leg (kf_extract) where their LDS structures fill: a
candidate queue that overflows in aligned tiles, on both parities of a workgroup's iteration; more far cells than the cache
has slots, and one hot cell among them; every cell of the LDS plot tile; far entries on both sides of the look-ups' flag;
an extract staging buffer that is flushed in the middle of a run; an output buffer smaller than the record count.

The tables come from tests/pass2_oracle.py (what they promise is asserted without a device by test_pass2_oracle_host.py),
the thresholds from the library (engine.pass2_limits), the expected plots and lines from oracle/brute.py.  SMG_P2_GRID and
SMG_EXTRACT_GRID cut the grids down so that a table of 1e5 entries takes a workgroup through several tiles or rounds."""
import functools

import numpy as np
import pytest

import brute
import pass2_oracle as po
from conftest import make_table
from smudgeplot_amd import engine, ktab
from test_pass2_oracle_host import KS, LIMITS, far_table, hot_table, ragged_table, star_table

pytestmark = pytest.mark.gpu

NAMES = ("1A1B", "3A1B", "2A2B")


def table_from(packed, cnt, k):
    return make_table(dict(packed=packed, counts=cnt, k=k, ibyte=1, nparts=1))


@functools.lru_cache(maxsize=None)
def case(make, k):
    """(packed, counts, the oracle's plot) of one generated table: made once, shared, never written to"""
    packed, cnt = make(k)[:2]
    want = brute.hetmers_plot(packed, cnt, k)
    for a in (packed, cnt, want):
        a.setflags(write=False)
    return packed, cnt, want


@functools.lru_cache(maxsize=None)
def every_cell(k):
    return po.every_cell_table(k, 7, 215)


def set_grid(monkeypatch, name, grid):
    if grid is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(grid))


def check_plot(packed, cnt, k, want, proofs=("hash", "exact")):
    for mode in proofs:
        plot, st = engine.hetmers_run(table_from(packed, cnt, k), symcheck=mode)
        assert st["path"] == 1, st
        assert np.array_equal(plot, want), (k, mode)
    return st


def labels_of(want, every=False):
    """three names, a quarter of the pixels unlabelled (as test_extract_fresh_tables_vs_oracle has it) -- or every pixel"""
    s, m = np.nonzero(want[:, :500])
    return {(int(mm), int(ss - mm)): NAMES[(ss + mm) % 3]
            for ss, mm in zip(s.tolist(), m.tolist()) if every or (ss * 7 + mm) % 4}


@functools.lru_cache(maxsize=None)
def lines_case(make, k, every=False):
    packed, cnt, want = case(make, k)
    labels = labels_of(want, every)
    return labels, brute.extract_lines(packed, cnt, k, labels)


def test_the_library_says_what_the_host_tests_assume():
    assert engine.pass2_limits() == LIMITS


# ---- a. queue overflow and the far cache ---------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [None, 1, 3])
@pytest.mark.parametrize("k", KS)
def test_queue_overflow_and_far_cache(k, grid, monkeypatch):
    """three aligned tiles with ~12200 candidates for a queue of P2_QCAP (the rest is finished in place), ~9700 far cells on
    all P2_FAR slots.  One workgroup walks all eight tiles: overflow on both parities of `it`, after a reset of the idle
    counter, with the prefetch of the next tile in flight; three workgroups: the last iteration is partly idle."""
    packed, cnt, want = case(star_table, k)
    assert len(cnt) > 7 * LIMITS["P2_TILE"] and want.sum() > 20000
    set_grid(monkeypatch, "SMG_P2_GRID", grid)
    check_plot(packed, cnt, k, want)


@pytest.mark.parametrize("grid", [None, 1, 3])
def test_queue_overflow_with_a_ragged_last_tile(grid, monkeypatch):
    """six full tiles and four entries: n % 16 != 0, and the last tile is all but empty"""
    k = 31
    packed, cnt, want = case(ragged_table, k)
    assert len(cnt) % 16 != 0 and 0 < len(cnt) % LIMITS["P2_TILE"] < 16
    set_grid(monkeypatch, "SMG_P2_GRID", grid)
    check_plot(packed, cnt, k, want)


@pytest.mark.parametrize("grid", [99999, 0, -3])
def test_a_grid_out_of_range_leaves_the_plot_alone(grid, monkeypatch):
    """(the hook takes 1 .. P2_GRID; what it does with anything else cannot be seen from outside, only that nothing breaks)"""
    packed, cnt, want = case(star_table, 31)
    set_grid(monkeypatch, "SMG_P2_GRID", grid)
    check_plot(packed, cnt, 31, want, proofs=("hash",))


# ---- b. a hot far cell --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [None, 1])
@pytest.mark.parametrize("k", KS)
def test_hot_far_cell_among_colliding_ones(k, grid, monkeypatch):
    """11000 pairs on the cell (300, 150), 3000 on ~2000 random cells beyond the LDS tile: the slot of the hot cell is hit,
    about four cells contend for every other slot (the first one is cached, the others go to the plot directly), and
    the cache is flushed at the end"""
    packed, cnt, want = case(hot_table, k)
    assert want[300, 150] >= 20000
    set_grid(monkeypatch, "SMG_P2_GRID", grid)
    check_plot(packed, cnt, k, want)


# ---- c. every cell of the LDS tile --------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [None, 1])
@pytest.mark.parametrize("k", [31, 51])
def test_every_cell_of_the_plot_tile(k, grid, monkeypatch):
    """1 .. 3 pairs on every cell two counts can reach below sum 216: the decode of a triangular cell index back into
    (sum, min) is exercised for all of them, with neighbours that hold other values; and the corners of the plot"""
    packed, cnt, want = case(every_cell, k)
    assert want[1001:].size == 0 and want[1000, 500] > 0           # the oracle itself is where it is expected
    assert want[1000, 499] > 0 and want[999, 499] > 0 and want[1000, 1] > 0
    planted = every_cell(k)[2]
    expect = np.zeros_like(want)
    expect[planted[:, 0], planted[:, 1]] = 2 * planted[:, 2]       # a pair and its mirror image
    assert np.array_equal(want, expect)
    inside = {(s, m) for s in range(2, LIMITS["P2_SMAX"]) for m in range(1, s // 2 + 1)}
    assert all(want[s, m] > 0 for s, m in inside)
    set_grid(monkeypatch, "SMG_P2_GRID", grid)
    check_plot(packed, cnt, k, want)


# ---- d. far entries with the P flag -------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 51, 66, 70, 85])
def test_far_entries_with_the_flag(k):
    """~540 entries whose only partner stands hundreds of entries away, in every lane of the 16-byte code scan; a third of
    them own a pair in front of k // 2 as well, a third of their partners do, a third count.  k <= 64: the listed form
    (kf_pass2_far), above: the scan (kf_pass2_farscan); then the extract leg's far branch on every pixel of the plot.
    The look-ups store the flag as the whole byte 0x80, whose low six bits no longer say "far": a flagged entry is skipped by
    the code test alone and a flagged partner reads as "no pair", so the flag tests of the far kernels are redundant as long
    as SET_P stores that byte (dropping them changes no result).  What this test holds the far kernels to is the partner
    they find, that only the lower member counts a pair, the partner's code and the counts."""
    packed, cnt, want = case(far_table, k)
    assert want.sum() > 300
    st = check_plot(packed, cnt, k, want)
    assert st["key_words"] == (k + 31) // 32 and (k > 64 or st["nbig"] > 3000), st
    labels, lines = lines_case(far_table, k, True)
    plot, got = engine.hetmers_extract(table_from(packed, cnt, k), labels)
    assert np.array_equal(plot, want)
    assert {lab: sorted(v) for lab, v in got.items()} == lines
    assert sum(len(v) for v in lines.values()) > 300


# ---- e. extract staging -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [1, 2, 5, None])
@pytest.mark.parametrize("k", KS)
def test_extract_staging_flushes_mid_run(k, grid, monkeypatch):
    """~16000 records from the first half of the table: with 1, 2 or 5 workgroups each of them fills more than half of its
    EX_STAGE records again and again before its last round"""
    packed, cnt, want = case(star_table, k)
    labels, lines = lines_case(star_table, k)
    if grid is not None:
        lab = np.zeros(want.shape, dtype=bool)
        for (mn, mx) in labels:
            lab[mn + mx, mn] = True
        nrec = po.records_of(packed, cnt, k, po.classify(packed, cnt, k), lab)
        assert int(nrec.sum()) == sum(len(v) for v in lines.values())
        early, most = po.staged_flushes(nrec, grid, LIMITS["F_TPB"], LIMITS["EX_STAGE"])
        assert early >= 3 and LIMITS["EX_STAGE"] // 2 < most <= LIMITS["EX_STAGE"], (early, most)
    set_grid(monkeypatch, "SMG_EXTRACT_GRID", grid)
    plot, got = engine.hetmers_extract(table_from(packed, cnt, k), labels)
    assert np.array_equal(plot, want)
    assert {lab: sorted(v) for lab, v in got.items()} == lines
    assert sum(len(v) for v in lines.values()) > 10000


# ---- f. extract capacity ------------------------------------------------------------------------------------------

def test_extract_capacity_and_count_only():
    """Engine.run, then Engine.extract: count only, into a buffer of a third of the records, into one that holds them all.
    (Run alone it takes ~11 s, all of it `import torch` in a process whose HIP runtime the engine has initialised: once per
    process, whichever test imports torch first.)"""
    import torch
    k, words = 31, 2
    packed, cnt, want = case(star_table, k)
    labels, lines = lines_case(star_table, k)
    names = sorted(set(labels.values()))
    lab = np.zeros(engine.PLOT_CELLS, dtype=np.uint16)
    for (mn, mx), name in labels.items():
        lab[(mn + mx) * engine.PLOT_COLS + mn] = names.index(name) + 1
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(ktab.packed_to_u64(packed).view(np.int64)).to(dev)
    tc = torch.from_numpy(cnt.copy().view(np.int16)).to(dev)
    tl = torch.from_numpy(lab.view(np.int16)).to(dev)
    plot = torch.zeros(engine.PLOT_CELLS, dtype=torch.int64, device=dev)
    e = engine.Engine(0)
    e.bind(k, len(cnt), tk.data_ptr(), tc.data_ptr())
    st = e.run(plot.data_ptr(), "hash")
    torch.cuda.synchronize()
    assert st["path"] == 1 and np.array_equal(plot.cpu().numpy().reshape(want.shape), want)

    count = e.extract(tl.data_ptr(), 0, 0)
    assert count == int(want.ravel()[lab > 0].sum()) == sum(len(v) for v in lines.values()) > 10000

    SENT, guard = -0x0123456789ABCDEF, 4096
    cap = count // 3
    small = torch.full((cap * words + guard,), SENT, dtype=torch.int64, device=dev)
    assert e.extract(tl.data_ptr(), small.data_ptr(), cap) == count            # what there is, not what was written
    torch.cuda.synchronize()
    small = small.cpu().numpy()
    assert (small[cap * words:] == SENT).all()

    full = torch.full((count * words + guard,), SENT, dtype=torch.int64, device=dev)
    assert e.extract(tl.data_ptr(), full.data_ptr(), count) == count
    torch.cuda.synchronize()
    full = full.cpu().numpy()
    assert (full[count * words:] == SENT).all()
    rec = full[: count * words].view(np.uint64).reshape(count, words)
    got = engine.record_lines(rec, k, names)
    assert {name: sorted(v) for name, v in got.items()} == lines

    # every record of the short call is a record of the full call, and none more often than there
    some = small[: cap * words].view(np.uint64).reshape(cap, words)
    u, c_full = np.unique(rec, axis=0, return_counts=True)
    v, c_some = np.unique(some, axis=0, return_counts=True)
    at = {tuple(r): n for r, n in zip(u.tolist(), c_full.tolist())}
    assert all(at.get(tuple(r), 0) >= n for r, n in zip(v.tolist(), c_some.tolist()))
    e.close()
