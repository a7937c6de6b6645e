"""The forms of kf_pass1_d (smg_pass1d.hpp, VAR): the hot form with the one-way rule compiled in (VAR = 2, odd k through
smg_engine_run), the hot form that stays two-way although k is odd (VAR = 6: the phase API with a 32-bit two-bit map, or the test
hook SMG_TWO_WAY=1) and the general form with its run-time switch (VAR = 1).  Which one a run launched is read from
smg_engine_pass1_form; plots against oracle/brute.py, request counts of the hot forms against the general form's under the
same protocol.  A tile owns 960 entries: the small tables end in front of, on and behind a tile's last entry."""
import functools

import numpy as np
import pytest
import torch

import brute
import lookup_oracle as lo
from smudgeplot_amd import engine, ktab, synth
from test_one_way_gpu import hand_built_table

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
M = 4000                  # base k-mers of the generator's tables, as tests/test_one_way_gpu.py
TWO_WAY_HOT = 6           # VAR of "hot form, two-way although k is odd"
D_OWN = 960               # entries a tile owns (smg_pass1d.hpp)
HOOKS = ("SMG_TWO_WAY", "SMG_NO_INDEX_DIR", "SMG_P1_GRID", "SMG_BM_BITS", "SMG_ONE_BIT_MAP", "SMG_NO_FILTER", "SMG_SIG")


@functools.lru_cache(maxsize=None)
def big(k):
    """-> (packed, counts, the oracle's plot): the generator's table of tests/test_one_way_gpu.py, made once per k"""
    packed, cnt = synth.adversarial_table(k, M, 4, 300 + k, low_complexity=60, dense=1)
    return packed, cnt, brute.hetmers_plot(packed, cnt, k)


@functools.lru_cache(maxsize=None)
def units(k):
    """base k-mers, every other one followed by a one-base variant of itself (so that the table has pairs): one row each"""
    rng = np.random.default_rng(7700 + k)
    rows = []
    for j in range(1200):
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
    """the closed table of the fewest leading rows of units(k) that has at least n entries (odd k: a row and its complement are
    two entries, so it has n or n + 1) -> (packed, counts, the oracle's plot)"""
    rows = units(k)
    rng = np.random.default_rng(n)
    for m in range((n + 1) // 2, len(rows) + 1):
        packed = ktab.pack_bases(rows[:m])
        packed, cnt = ktab.sort_unique_packed(packed, rng.integers(20, 60, m).astype(np.uint16))
        packed, cnt = ktab.symmetrize(packed, cnt, k)
        if len(cnt) >= n:
            cnt = cnt.astype(np.uint16)
            return packed, cnt, brute.hetmers_plot(packed, cnt, k)
    raise AssertionError("units(k) is too short")


def clear(monkeypatch, **env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv("SMG_" + name, str(val))


class Bound:
    """a table on the device with its prefix index, and an engine bound to it"""

    def __init__(self, packed, cnt, k, ibyte=3):
        words = lo.packed_to_words(packed, k)
        self.k, self.n = k, len(cnt)
        self.keys = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1).copy()).to(DEV)
        self.cnt = torch.from_numpy(np.ascontiguousarray(cnt).view(np.int16).copy()).to(DEV)
        lead = torch.from_numpy((words[:, 0] >> np.uint64(64 - 8 * ibyte)).astype(np.int64)).to(DEV)
        self.index = torch.cumsum(torch.bincount(lead, minlength=1 << (8 * ibyte)), 0)
        self.plot = torch.zeros(engine.PLOT_CELLS, dtype=torch.int64, device=DEV)
        self.e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
        self.e.bind(k, self.n, self.keys.data_ptr(), self.cnt.data_ptr())
        self.e.set_prefix_index(self.index.data_ptr(), ibyte, 0)        # (reads SMG_NO_INDEX_DIR)

    def run(self, symcheck="hash"):
        """-> (plot, stats, pass-1 form) of one smg_engine_run"""
        st = self.e.run(self.plot.data_ptr(), symcheck)
        torch.cuda.synchronize()
        plot = self.plot.cpu().numpy().reshape(engine.PLOT_ROWS, engine.PLOT_COLS)
        return plot, st, self.e.pass1_form()

    def close(self):
        self.e.close()


def run_once(packed, cnt, k, ibyte=3, symcheck="hash"):
    b = Bound(packed, cnt, k, ibyte)
    try:
        return b.run(symcheck)
    finally:
        b.close()


def words_of(k):
    return (k + 31) // 32


# ---- 1. which form a run launches --------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [25, 31, 33, 63])
def test_odd_k_with_its_index_launches_the_one_way_hot_form(k, monkeypatch):
    packed, cnt, want = big(k)
    clear(monkeypatch)
    plot, st, form = run_once(packed, cnt, k)
    assert form == {"var": 2, "w": words_of(k), "rw": words_of(k), "inner_only": 0}, form
    assert st["path"] == 1 and np.array_equal(plot, want)
    clear(monkeypatch, TWO_WAY=1)
    plot, st, form = run_once(packed, cnt, k)
    assert form == {"var": TWO_WAY_HOT, "w": words_of(k), "rw": words_of(k), "inner_only": 0}, form
    assert st["path"] == 1 and np.array_equal(plot, want)


@pytest.mark.parametrize("k", [25, 31, 33, 63])
def test_the_phase_api_launches_the_two_way_hot_form(k, monkeypatch):
    """requests of the phase API leave the engine: two-way, and with a 32-bit two-bit map and the table's index the hot form"""
    packed, cnt, want = big(k)
    clear(monkeypatch)
    b = Bound(packed, cnt, k)
    try:
        b.e.set_blockmap_bits(32)
        b.e.pass1("hash")
        st = b.e.lookup_state()
        assert st["one_way"] == 0 and st["bm2"] == 1 and st["fb"] == 32
        assert b.e.pass1_form() == {"var": TWO_WAY_HOT, "w": words_of(k), "rw": words_of(k), "inner_only": 0}
        n_phase = b.e.nreq()
        # the default map of the phase API (30 id bits, to be exchanged) comes with signatures: the general form
        b.e.set_blockmap_bits(0)
        b.e.pass1("hash")
        assert b.e.pass1_form()["var"] == 1
        assert b.e.nreq() == n_phase, "the two forms emit the same two-way requests"
    finally:
        b.close()
    clear(monkeypatch, TWO_WAY=1)
    _, st2, _ = run_once(packed, cnt, k)
    assert st2["nemitted"] == n_phase, "phase API and SMG_TWO_WAY=1 run the same form on the same table"


@pytest.mark.parametrize("k", [24, 32, 64])
def test_even_k_has_one_hot_form(k, monkeypatch):
    packed, cnt, want = big(k)
    for env in ({}, {"TWO_WAY": 1}):
        clear(monkeypatch, **env)
        plot, st, form = run_once(packed, cnt, k)
        assert form == {"var": 2, "w": words_of(k), "rw": words_of(k), "inner_only": 0}, (env, form)
        assert np.array_equal(plot, want)


@pytest.mark.parametrize("what", ["ibyte1", "k17", "k23", "exact", "no_index_hook"])
def test_what_keeps_the_general_form(what, monkeypatch):
    k = {"k17": 17, "k23": 23}.get(what, 31)
    packed, cnt, want = big(k)
    clear(monkeypatch, **({"NO_INDEX_DIR": 1} if what == "no_index_hook" else {}))
    plot, st, form = run_once(packed, cnt, k, ibyte=1 if what == "ibyte1" else 3, symcheck="exact" if what == "exact" else "hash")
    assert form["var"] == 1 and form["w"] == 1 and form["rw"] == (2 if what == "exact" else 1), form
    assert st["path"] == 1 and np.array_equal(plot, want)


# ---- 2. plots and counts of the three forms ----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [25, 31, 33, 51, 63])
def test_the_three_forms_agree(k, monkeypatch):
    packed, cnt, want = big(k)
    got = {}
    for name, env, var in (("hot one-way", {}, 2), ("hot two-way", {"TWO_WAY": 1}, TWO_WAY_HOT),
                           ("general one-way", {"NO_INDEX_DIR": 1}, 1), ("general two-way", {"NO_INDEX_DIR": 1, "TWO_WAY": 1}, 1)):
        clear(monkeypatch, **env)
        plot, st, form = run_once(packed, cnt, k)
        assert form["var"] == var, (name, form)
        assert st["path"] == 1 and np.array_equal(plot, want), name
        got[name] = (st["nemitted"], st["nrequests"])
    print(f"k={k}: (emitted, kept) {got}")
    assert got["hot one-way"] == got["general one-way"]
    assert got["hot two-way"] == got["general two-way"]
    assert 0 < got["hot one-way"][0] < got["hot two-way"][0]
    # the general form without the index (ibyte = 1: no hook) is the same launch
    clear(monkeypatch)
    plot, st, form = run_once(packed, cnt, k, ibyte=1)
    assert form["var"] == 1 and np.array_equal(plot, want)
    assert (st["nemitted"], st["nrequests"]) == got["general one-way"]


# ---- 3. tile edges --------------------------------------------------------------------------------------------------

# (957: one entry short of a tile as well; a closed table of odd k has an even number of entries, so 1 -> 2, 959 -> 960, ..)
@pytest.mark.parametrize("n", [1, 5, 957, 959, 960, 961, 1919, 1921])
@pytest.mark.parametrize("k", [31, 33])
def test_tables_that_end_at_a_tile_edge(k, n, monkeypatch):
    packed, cnt, want = cut(k, n)
    assert n <= len(cnt) <= n + 1
    if n == 960:
        assert len(cnt) == D_OWN
    got = {}
    for name, env, var in (("one-way", {}, 2), ("two-way", {"TWO_WAY": 1}, TWO_WAY_HOT)):
        clear(monkeypatch, **env)
        plot, st, form = run_once(packed, cnt, k)
        assert form["var"] == var, (name, form)
        assert st["path"] == 1, (name, st)
        assert np.array_equal(plot, want), (name, len(cnt))
        got[name] = plot
    assert np.array_equal(got["one-way"], got["two-way"])
    if len(cnt) >= 6:
        assert want.sum() > 0


@pytest.mark.parametrize("grid", [1, 2, 8, None])
@pytest.mark.parametrize("k", [31, 33])
def test_every_grid_of_pass1(k, grid, monkeypatch):
    packed, cnt, want = big(k)
    assert len(cnt) > 8 * D_OWN            # (more tiles than workgroups: every workgroup draws tickets)
    got = {}
    for name, env, var in (("one-way", {}, 2), ("two-way", {"TWO_WAY": 1}, TWO_WAY_HOT)):
        if grid is not None:
            env = dict(env, P1_GRID=grid)
        clear(monkeypatch, **env)
        b = Bound(packed, cnt, k)
        try:
            plot, st, form = b.run()
            ls = b.e.lookup_state()
        finally:
            b.close()
        assert form["var"] == var, (name, form)
        if grid is not None:
            assert ls["p1_grid"] == grid
        assert st["path"] == 1 and np.array_equal(plot, want), (name, grid)
        got[name] = (st["nemitted"], st["nrequests"])
    # the requests are a function of the table, not of the grid
    clear(monkeypatch)
    _, st0, _ = run_once(packed, cnt, k)
    assert got["one-way"] == (st0["nemitted"], st0["nrequests"])
    assert got["one-way"][0] < got["two-way"][0]


# ---- 4. the hand-built classes of tests/test_one_way_gpu.py ------------------------------------------------------------

def test_hand_built_classes_through_both_hot_forms(monkeypatch):
    k = 31
    packed, cnt = hand_built_table()
    want = brute.hetmers_plot(packed, cnt, k)
    assert want.sum() >= 24
    got = {}
    for name, env, var in (("hot one-way", {}, 2), ("hot two-way", {"TWO_WAY": 1}, TWO_WAY_HOT),
                           ("general one-way", {"NO_INDEX_DIR": 1}, 1), ("general two-way", {"NO_INDEX_DIR": 1, "TWO_WAY": 1}, 1)):
        clear(monkeypatch, **env)
        plot, st, form = run_once(packed, cnt, k)
        assert form["var"] == var, (name, form)
        assert st["path"] == 1 and st["nbig"] >= 24, (name, st)          # (kind e went through the exact redo)
        assert np.array_equal(plot, want), name
        got[name] = (st["nemitted"], st["nrequests"])
    print(f"hand-built: (emitted, kept) {got}")
    assert got["hot one-way"] == got["general one-way"]
    assert got["hot two-way"] == got["general two-way"]
