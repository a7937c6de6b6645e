"""The fast path of three-word k-mers (k = 65 .. 85) record by record at its seams: kf_pass1<3>, kf_filter<4>, kf_compact, kf_sortkey
with kf_apply_indexed<3> or kf_apply<3>, the routing kernels with four-word records, kf_pass2_farscan<3> and kf_extract<3>
(smg_fast.hpp; drivers in smg_hetmers.hip).

The phase API hands out the emitted list E (pass1, route) and the kept list K (pass1, filter(map), route), takes a flat list the test
owns (apply) and gives the engine's own candidate map (blockmap, blockmap_copy).  All of it is compared, integer for integer, with
tests/wide_oracle.py; the plots with oracle/brute.py.  What a table puts where is asserted on the CPU by
tests/test_wide_oracle_host.py; every size comes from engine.wide_limits, which regime ran from engine.lookup_state."""
import functools

import numpy as np
import pytest
import torch

import brute
import lookup_oracle as lo
import wide_oracle as wo
from smudgeplot_amd import engine

pytestmark = pytest.mark.gpu

U = np.uint64
KS = wo.KS
DEV = torch.device("cuda:0")
SENT = -0x0123456789ABCDEF
GUARD = 1024
HOOKS = ("SMG_P1_GRID", "SMG_BM_BITS", "SMG_FILTER_GRID", "SMG_NO_FILTER", "SMG_P2_GRID", "SMG_EXTRACT_GRID")
GRIDS = (None, 1, 3)
NAMES = ("1A1B", "3A1B", "2A2B")


@functools.lru_cache(maxsize=None)
def lim():
    return engine.wide_limits()


def seam(k):
    L = lim()
    return wo.seam_table(k, L["F_TILE"], L["F_HALO"], L["CODE_REACH"])[0]


def ladder(k):
    return wo.ladder_table(k, lim()["CODE_REACH"])[0]


def dense(k):
    return wo.dense_table(k, lim()["F_TILE"])


def hooks(monkeypatch, **env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        if val is not None:
            monkeypatch.setenv("SMG_" + name, str(val))


_ON_DEVICE = {}


def bound(t):
    """an engine on the table (the table goes to the device once)"""
    if id(t) not in _ON_DEVICE:
        tk = torch.from_numpy(np.ascontiguousarray(t.words).view(np.int64).reshape(-1).copy()).to(DEV)
        tc = torch.from_numpy(np.ascontiguousarray(t.cnt).view(np.int16).copy()).to(DEV)
        _ON_DEVICE[id(t)] = (t, tk, tc)
    _, tk, tc = _ON_DEVICE[id(t)]
    e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
    e.bind(t.k, len(t.cnt), tk.data_ptr(), tc.data_ptr())
    return e


def to_device(rows):
    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int64).reshape(-1).copy()).to(DEV)


def routed(e, n, splitters=None, nranks=1):
    """the engine's current request list as it was routed -> (rows in buffer order, per-rank counts); the buffer behind the records
    must stay untouched"""
    rw = e.record_words()
    assert rw == 4
    buf = torch.full((n * rw + GUARD,), SENT, dtype=torch.int64, device=DEV)
    counts = e.route(np.zeros(0, U) if splitters is None else splitters, nranks, buf.data_ptr(), n)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert sum(counts) == n, (counts, n)
    assert (host[n * rw:] == SENT).all(), "route wrote behind the records it reported"
    return host[: n * rw].view(U).reshape(n, rw), counts


def same_rows(got, want, what):
    got = lo.sort_rows(got)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    extra, lost = lo.multiset_diff(got, want)
    show = lambda rows: [tuple(hex(x) for x in r) for r in rows[:4]]
    raise AssertionError(f"{what}: {len(got)} rows for {len(want)}; {len(extra)} not expected {show(extra)}, {len(lost)} missing {show(lost)}")


def expected_map(t, bits, nw):
    w, val = wo.map_bits(t, bits)
    m = torch.zeros(nw, dtype=torch.int32, device=DEV)
    m[torch.from_numpy(w).to(DEV)] = torch.from_numpy(val.astype(np.uint32).view(np.int32)).to(DEV)
    return m


def own_map(e):
    bits, nw = e.blockmap()
    m = torch.empty(nw, dtype=torch.int32, device=DEV)
    e.blockmap_copy(0, nw, m.data_ptr())
    torch.cuda.synchronize()
    return bits, m


def plot_of(e):
    plot = torch.zeros(engine.PLOT_CELLS, dtype=torch.int64, device=DEV)
    e.pass2(plot.data_ptr())
    torch.cuda.synchronize()
    return plot.cpu().numpy().reshape(engine.PLOT_ROWS, engine.PLOT_COLS)


def run_of(e, proof):
    plot = torch.zeros(engine.PLOT_CELLS, dtype=torch.int64, device=DEV)
    st = e.run(plot.data_ptr(), proof)
    torch.cuda.synchronize()
    return plot.cpu().numpy().reshape(engine.PLOT_ROWS, engine.PLOT_COLS), st


def test_the_library_says_what_the_tables_were_built_for():
    L = lim()
    assert L["CODE_REACH"] == wo.po.REACH and L["F_CH"] == engine.lookup_limits()["F_CH"]
    assert L["F_FSTAGE"] == 4 * engine.pass2_limits()["F_TPB"]


# ---- A. pass 1, record by record ----------------------------------------------------------------------------------------------

def pass1_record_by_record(t, monkeypatch):
    """one table through both proofs and every grid of pass 1 -> the (proof, grid, chunks) it ran"""
    L = lim()
    tile, f_ch = L["F_TILE"], L["F_CH"]
    n = len(t.cnt)
    ntiles = -(-n // tile)
    e = bound(t)
    ran = []
    for proof in ("hash", "exact"):
        want = wo.emitted_rows(t, proof == "exact")
        assert len(np.unique(want[:, :3], axis=0)) == len(want)
        per_tile = wo.senders_per_tile(t, proof == "exact", tile)
        for grid in GRIDS:
            bits = None if grid is None else 20                        # the default map once, a coarse one otherwise
            hooks(monkeypatch, P1_GRID=grid, BM_BITS=bits)
            what = f"k={t.k} n={n} {proof} grid={grid}"
            e.pass1(proof)
            n0 = e.nreq()
            E, _ = routed(e, n0)
            same_rows(E, want, what)                                    # the oracle's rows, none twice
            ls = e.lookup_state()
            g = min(grid or ntiles, ntiles)
            chunks = wo.chunk_replay(per_tile, g, f_ch)
            assert (ls["rw"], ls["nb"], ls["one_way"], ls["p1_grid"], ls["p1_chunks"]) == (4, 0, 0, g, len(chunks)), (what, ls)
            assert e.stats()["nemitted"] == len(want) == sum(chunks), what
            if proof == "hash":
                got_bits, m = own_map(e)
                assert got_bits == (bits or 30) == ls["fb"], (what, got_bits)
                assert torch.equal(m, expected_map(t, got_bits, m.numel())), what
            else:
                assert e.blockmap() == (0, 0)
            assert e.apply_own() == 0, what
            assert np.array_equal(plot_of(e), t.plot), what
            plot, st = run_of(e, proof)
            assert st["path"] == 1 and st["nemitted"] == len(want) and np.array_equal(plot, t.plot), what
            ran.append((proof, g, len(chunks)))
    e.close()
    return ran


@pytest.mark.parametrize("where", [0, 1, 2], ids=["one tile", "two tiles", "four tiles"])
@pytest.mark.parametrize("k", KS)
def test_pass1_on_tables_that_end_next_to_a_seam(k, where, monkeypatch):
    sizes = wo.size_list(lim()["F_TILE"])
    seen = set()
    for n in (sizes[:9], sizes[9:16], sizes[16:])[where]:
        t = wo.cut(k, n)
        if len(t.cnt) in seen:                                          # (a closed table of odd k has an even number of entries)
            continue
        seen.add(len(t.cnt))
        pass1_record_by_record(t, monkeypatch)


@pytest.mark.parametrize("make", [seam, ladder, dense], ids=["seams", "ladder", "dense"])
@pytest.mark.parametrize("k", KS)
def test_pass1_on_blocks_across_seams_block_lengths_and_dense_senders(k, make, monkeypatch):
    """seams: pairs at distance 1, reach and reach + 1 across two tile seams, the hand-over to the block walk; ladder: blocks of
    31 .. 130 entries, at both ends of the table; dense: chunks that roll over partly full (hash) and that four full tiles fill
    exactly (exact) in the only workgroup of grid 1"""
    ran = pass1_record_by_record(make(k), monkeypatch)
    if make is dense:
        assert all(c >= 2 for p, g, c in ran if g == 1) and len(ran) == 2 * len(GRIDS)


# ---- B. filter --------------------------------------------------------------------------------------------------------------

FB = 20


def map_of(kind, t, nw):
    if kind == "own":
        return expected_map(t, FB, nw)
    word = {"ones": -1, "zero": 0, "every other id": 0x55555555}[kind]
    return torch.full((nw,), word, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("kind", ["ones", "zero", "every other id", "own"])
@pytest.mark.parametrize("k", KS)
def test_kept_list_is_the_emitted_list_under_the_map(k, kind, monkeypatch):
    """kf_filter<4> with one, two and all its workgroups: with one, it takes every chunk of pass 1, flushes its stage several times
    per chunk and splits the survivors of a flush across two output chunks"""
    L = lim()
    t = dense(k)
    want = wo.emitted_rows(t, False)
    e = bound(t)
    e.set_blockmap_bits(FB)
    kept_at = {}
    for fgrid in (None, 1, 2):
        hooks(monkeypatch, FILTER_GRID=fgrid)
        e.pass1("hash")
        E, _ = routed(e, e.nreq())
        same_rows(E, want, f"k={k} emitted")
        ls = e.lookup_state()
        assert ls["fb"] == FB and ls["p1_chunks"] >= 2 and len(E) > L["F_CH"] + L["F_FSTAGE"]
        bits, nw = e.blockmap()
        m = map_of(kind, t, nw)
        kept = e.filter(m.data_ptr())
        assert kept == e.nreq()
        K, _ = routed(e, kept)
        mw = m.cpu().numpy().view(np.uint32).astype(np.int64)
        ids = wo.ids_of(want, FB)
        keep = (mw[ids >> 5] >> (ids & 31)) & 1 == 1
        same_rows(K, want[keep], f"k={k} map={kind} filter grid={fgrid}")
        kept_at[fgrid] = kept
        if kind == "ones":
            assert kept == len(want) > L["F_CH"]                        # more than one output chunk from one workgroup
        if kind == "zero":
            assert kept == 0
        if kind == "every other id":
            assert 0.3 * len(want) < kept < 0.7 * len(want)
        # the look-ups of the kept list and pass 2: a map of ones or the table's own keeps every request that matters
        if kind in ("ones", "own"):
            assert e.apply_own() == 0
            assert np.array_equal(plot_of(e), t.plot)
    assert len(set(kept_at.values())) == 1, kept_at                  # a function of table and map, not of the grid
    e.close()


# ---- C. route ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nranks", [3, 16])
@pytest.mark.parametrize("k", KS)
def test_route_tells_splitters_apart_by_their_third_word(k, nranks, monkeypatch):
    """exact proof: every entry sends, the rows are the table itself.  Two splitters are members of the family whose k-mers agree
    in their first two words"""
    hooks(monkeypatch)
    t = dense(k)
    n = len(t.cnt)
    a, b = wo.two_word_family(t)
    pick = {a + 1, a + 3}
    others = [int(x) for x in np.linspace(n // 40, n - n // 40, nranks).astype(np.int64) if not a - 1 <= x <= b]
    pick = sorted(pick | set(others[: nranks - 3]))
    assert len(pick) == nranks - 1
    sp = np.ascontiguousarray(t.words[pick])
    assert sp[pick.index(a + 1), :2].tolist() == sp[pick.index(a + 3), :2].tolist() and sp[pick.index(a + 1), 2] != sp[pick.index(a + 3), 2]
    want = wo.emitted_rows(t, True)
    rank = wo.ranks_of(want, sp)
    assert np.array_equal(rank, np.searchsorted(np.array(pick), np.arange(n), side="right"))     # (the rows are the table, in order)
    e = bound(t)
    e.pass1("exact")
    assert e.nreq() == n
    rows, counts = routed(e, n, sp.reshape(-1), nranks)
    assert counts == np.bincount(rank, minlength=nranks).tolist(), (counts, np.bincount(rank, minlength=nranks))
    at = 0
    for r, c in enumerate(counts):
        same_rows(rows[at: at + c], want[rank == r], f"k={k} rank {r} of {nranks}")
        at += c
    assert all(counts[r] > 0 for r in (pick.index(a + 1), pick.index(a + 1) + 1, pick.index(a + 3) + 1))
    e.close()


# ---- D. apply, record by record ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_flags_of_a_list_the_test_chose(k, monkeypatch):
    """hash proof: SORT_MIN - 1 rows (kf_apply), SORT_MIN rows and all rows (kf_sortkey, the sort, kf_apply_indexed); the plot
    is the oracle's for the flags of exactly those rows.  The rows come from E: the rows that survive the engine's own map are
    fewer than SORT_MIN in a table of sixteen tiles (asserted on the CPU), and all of them are among the rows applied last."""
    hooks(monkeypatch)
    L = lim()
    t = wo.flag_table(k)
    want = wo.emitted_rows(t, False)
    e = bound(t)
    e.pass1("hash")
    E, _ = routed(e, e.nreq())
    same_rows(E, want, f"k={k} emitted")
    bits, m = own_map(e)
    assert torch.equal(m, expected_map(t, bits, m.numel()))
    kept = e.filter(None)
    K, _ = routed(e, kept)
    mw = wo.map_bits(t, bits)
    ids = wo.ids_of(want, bits)
    at = np.minimum(np.searchsorted(mw[0], ids >> 5), len(mw[0]) - 1)
    keep = (mw[0][at] == ids >> 5) & ((mw[1][at] >> (ids & 31)) & 1 == 1)
    same_rows(K, want[keep], f"k={k} kept by the engine's own map")
    assert 0 < kept < L["SORT_MIN"] < len(want)
    rows = wo.apply_list(t, want, L["SORT_MIN"])
    buf = to_device(rows)
    plots = []
    for cut in (L["SORT_MIN"] - 1, L["SORT_MIN"], len(rows)):
        e.pass1("hash")
        assert e.apply(buf.data_ptr(), cut) == 0
        got = plot_of(e)
        expect = wo.flag_plot(t, wo.flagged_by(t, rows[:cut]))
        assert np.array_equal(got, expect), (k, cut, int(np.abs(got - expect).sum()))
        plots.append(expect)
    assert not np.array_equal(plots[0], plots[1]) and not np.array_equal(plots[1], plots[2]) and np.array_equal(plots[2], t.plot)
    e.close()


@pytest.mark.parametrize("short", [True, False], ids=["kf_apply", "kf_apply_indexed"])
@pytest.mark.parametrize("k", KS)
def test_exact_proof_counts_what_is_missing(k, short, monkeypatch):
    hooks(monkeypatch)
    L = lim()
    t = wo.flag_table(k)
    rows = wo.emitted_rows(t, True)
    m = L["SORT_MIN"] - 1 if short else len(rows)
    assert len(rows) >= L["SORT_MIN"]
    rows = rows[:m]
    e = bound(t)
    off = rows.copy()
    off[m // 2, 3] += U(1)                                              # a count that is off by one
    absent = rows.copy()
    absent[m // 3, 2] ^= U(1) << U(63)                                  # another base behind position 63: a k-mer the table lacks
    assert wo.index_of_rows(t, absent[m // 3: m // 3 + 1])[0] == -1
    for what, lst, ok in (("unchanged", rows, True), ("count", off, False), ("absent", absent, False)):
        e.pass1("exact")
        missing = e.apply(to_device(lst).data_ptr(), m)
        assert (missing == 0) if ok else (missing >= 1), (k, what, missing)
    e.close()


# ---- E. extract -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [seam, ladder], ids=["seams", "ladder"])
@pytest.mark.parametrize("k", KS)
def test_extract_lines_with_every_pixel_labelled(k, make, monkeypatch):
    """the near and the far branch of kf_extract<3>: pairs at distance reach (near), reach + 1 and beyond (the block walk again)"""
    hooks(monkeypatch)
    t = make(k)
    s, m = np.nonzero(t.plot)
    labels = {(int(mm), int(ss - mm)): NAMES[(ss + mm) % 3] for ss, mm in zip(s.tolist(), m.tolist())}
    lines = brute.extract_lines(t.packed, t.cnt, k, labels)
    names = sorted(set(labels.values()))
    lab = np.zeros(engine.PLOT_CELLS, dtype=np.uint16)
    for (mn, mx), name in labels.items():
        lab[(mn + mx) * engine.PLOT_COLS + mn] = names.index(name) + 1
    tl = torch.from_numpy(lab.view(np.int16)).to(DEV)
    e = bound(t)
    plot, st = run_of(e, "hash")
    assert st["path"] == 1 and np.array_equal(plot, t.plot)
    count = e.extract(tl.data_ptr(), 0, 0)
    assert count == int(t.plot.sum()) == sum(len(v) for v in lines.values())
    out = torch.full((count * 4 + GUARD,), SENT, dtype=torch.int64, device=DEV)
    assert e.extract(tl.data_ptr(), out.data_ptr(), count) == count
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[count * 4:] == SENT).all()
    got = engine.record_lines(host[: count * 4].view(U).reshape(count, 4), k, names)
    assert {name: sorted(v) for name, v in got.items()} == lines
    e.close()


# ---- F. one engine, several runs -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [seam, dense], ids=["seams", "dense"])
@pytest.mark.parametrize("k", KS)
def test_one_engine_hash_exact_then_hash_on_one_workgroup(k, make, monkeypatch):
    """the request list of the exact run (every entry) is the larger one and stays: the hash runs behind it run in its chunks"""
    t = make(k)
    e = bound(t)
    emitted = []
    for proof, grid in (("hash", None), ("exact", None), ("hash", 1)):
        hooks(monkeypatch, P1_GRID=grid)
        plot, st = run_of(e, proof)
        assert st["path"] == 1 and np.array_equal(plot, t.plot), (k, proof, grid)
        emitted.append(st["nemitted"])
        if grid:
            assert e.lookup_state()["p1_grid"] == grid
    assert emitted == [int((t.s_hi > 0).sum()), len(t.cnt), int((t.s_hi > 0).sum())]
    e.close()
