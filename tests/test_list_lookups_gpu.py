"""The list route between pass 1 and pass 2 for one- and two-word k-mers, record by record: kf_compact on ragged chunks,
kf_fill_holes and the sentinel words it writes, the forced-Onesweep sorts, kf_apply_sorted<1>, kf_sortkey with
kf_apply_indexed<W>, kf_apply<W>, kf_filter<1>, and sig_find under all of them (smg_fast.hpp; drivers in smg_hetmers.hip).  It is
the route of every sharded run for the requests a rank receives, of the exact proof, of SMG_NO_FILTER and of k-mers too short for
a 12-bit map.

A, B, C hand the engine flat lists the test owns (pass1, apply, pass2): the plot must be tests/list_oracle.py's for the flags of
exactly those rows, `missing` the oracle's.  D runs the engine's own list through the route.  Which branch ran is asserted from
engine.Engine.apply_state and lookup_state, every size comes from engine.list_limits, the directory of a table from
engine.pass1_plan; what a table puts where is asserted on the CPU by tests/test_list_oracle_host.py.  Every device buffer handed
to the engine is followed by a guard of sentinel words that must come back untouched."""
import functools

import numpy as np
import pytest
import torch

import list_oracle as lz
import lookup_oracle as lo
import wide_oracle as wo
from smudgeplot_amd import engine
from test_pass1_tile_seam_gpu import emitted_bounds

pytestmark = pytest.mark.gpu

U = np.uint64
DEV = torch.device("cuda:0")
GUARD = 1024
SENT = {torch.int64: -0x0123456789ABCDEF, torch.int16: -0x1235, torch.int32: -0x01234567}
HOOKS = ("SMG_P1_GRID", "SMG_BM_BITS", "SMG_FILTER_GRID", "SMG_NO_FILTER", "SMG_TWO_WAY", "SMG_SIG", "SMG_ONE_BIT_MAP", "SMG_DIR_PER",
         "SMG_NO_INDEX_DIR", "SMG_APPLY_SORT_MIN", "SMG_FILTER_SORT_MIN", "SMG_VERIFY_SORT")


@functools.lru_cache(maxsize=None)
def lim():
    return engine.list_limits()


def hooks(monkeypatch, **env):
    """the hooks of this test and no others (monkeypatch puts the environment back when the test ends)"""
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        if val is not None:
            monkeypatch.setenv("SMG_" + name, str(val))


class Guarded:
    """device buffers, each followed by GUARD sentinel words"""

    def __init__(self):
        self.bufs = []

    def put(self, host, dtype=torch.int64):
        host = np.ascontiguousarray(host).reshape(-1)
        buf = torch.full((len(host) + GUARD,), SENT[dtype], dtype=dtype, device=DEV)
        if len(host):
            buf[: len(host)] = torch.from_numpy(host.copy()).to(DEV)
        self.bufs.append((buf, len(host)))
        return buf

    def adopt(self, dev, dtype):
        buf = torch.full((len(dev) + GUARD,), SENT[dtype], dtype=dtype, device=DEV)
        buf[: len(dev)] = dev
        self.bufs.append((buf, len(dev)))
        return buf

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool((buf[n:] == SENT[buf.dtype]).all()), f"the guard behind a buffer of {n} words was written"


class Bound(Guarded):
    """a table on the device, with its 3-byte prefix index where asked for, and an engine bound to it"""

    def __init__(self, t, index=False):
        super().__init__()
        self.t = t
        self.keys = self.put(t.words.view(np.int64))
        self.cnt = self.put(t.cnt.view(np.int16), torch.int16)
        self.plot = self.put(np.zeros(engine.PLOT_CELLS, np.int64))
        self.e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
        self.e.bind(t.k, len(t.cnt), self.keys.data_ptr(), self.cnt.data_ptr())
        if index:
            lead = torch.from_numpy((t.words[:, 0] >> U(40)).astype(np.int64)).to(DEV)
            self.index = self.adopt(torch.cumsum(torch.bincount(lead, minlength=1 << 24), 0), torch.int64)
            self.e.set_prefix_index(self.index.data_ptr(), 3, 0)

    def host_plot(self):
        torch.cuda.synchronize()
        return self.plot[: engine.PLOT_CELLS].cpu().numpy().reshape(engine.PLOT_ROWS, engine.PLOT_COLS)

    def pass2(self):
        self.e.pass2(self.plot.data_ptr())
        return self.host_plot()

    def run(self, proof):
        st = self.e.run(self.plot.data_ptr(), proof)
        return self.host_plot(), st

    def routed(self, n):
        rw = self.e.record_words()
        buf = self.put(np.zeros(n * rw, np.int64))
        counts = self.e.route(np.zeros(0, U), 1, buf.data_ptr(), n)
        torch.cuda.synchronize()
        assert counts == [n], (counts, n)
        return lo.sort_rows(buf[: n * rw].cpu().numpy().view(U).reshape(n, rw))

    def close(self):
        self.check()
        self.e.close()


def same_plot(got, want, what):
    assert np.array_equal(got, want), (what, int(np.abs(got - want).sum()), int(got.sum()), int(want.sum()))


def state(e, kernel, sorted_, holes, covered, sig, what):
    ap = e.apply_state()
    assert (ap["kernel"], ap["sorted"], ap["holes"], ap["sig"]) == (kernel, sorted_, holes, sig), (what, ap)
    assert covered is None or ap["covered"] == covered, (what, ap)
    return ap


def signatures_planned(t, on, proof="hash"):
    """the default map of the phase API (30 id bits) comes with signatures; SMG_SIG=0 (set by the caller) takes them away"""
    plan = engine.pass1_plan(t.k, len(t.cnt), proof, own_lookups=False, have_index=False, bm_cap=30)
    assert bool(plan["use_sig"]) == on, plan


def test_the_library_says_what_the_tables_were_built_for():
    L = lim()
    assert L["SORT_MIN"] == engine.wide_limits()["SORT_MIN"] and L["F_CH"] == engine.lookup_limits()["F_CH"]
    assert L["SORT_MIN"] < L["APPLY_SORT_MIN"] < L["FILTER_SORT_MIN"]


# ---- A. flat lists of one-word k-mers: kf_apply_sorted, as they come and sorted -----------------------------------------------

@pytest.mark.parametrize("sig", [True, False], ids=["signatures", "k-mers"])
@pytest.mark.parametrize("hook", [False, True], ids=["real threshold", "hook at its floor"])
@pytest.mark.parametrize("k", lz.KS1)
def test_key_only_list_on_both_sides_of_the_sort(k, hook, sig, monkeypatch):
    """cuts at APPLY_SORT_MIN - 1 (looked up as it comes), APPLY_SORT_MIN and 2 APPLY_SORT_MIN + 3 (sorted first, every sort
    self-checked): the flag table's rows repeated in a shuffled order, one deciding row at the second cut and one at the end, so
    that the three plots differ.  With the hook the same at a few thousand rows."""
    L = lim()
    hooks(monkeypatch, VERIFY_SORT=1, APPLY_SORT_MIN=L["SORT_MIN"] if hook else None, SIG=None if sig else 0)
    m = L["SORT_MIN"] if hook else L["APPLY_SORT_MIN"]
    cuts = (m - 1, m, 2 * m + 3)
    t = lz.flag_table(k, L["SORT_MIN"] + 2)
    lst = lz.repeated_list(t, lz.key_rows(t), cuts, k)
    assert hook or len(np.unique(lst[: cuts[0]])) >= L["SORT_MIN"]
    signatures_planned(t, sig)
    b = Bound(t)
    buf = b.put(lst.view(np.int64))
    plots = []
    for cut in cuts:
        what = f"k={k} cut={cut} sig={sig}"
        b.e.pass1("hash")
        assert b.e.record_words() == 1 and b.e.lookup_state()["one_way"] == 0
        assert b.e.apply(buf.data_ptr(), cut) == 0, what
        state(b.e, "kf_apply_sorted", cut >= m, None, cut, sig, what)
        want = lz.flag_plot(t, lz.flagged_by(t, lst[:cut]))
        same_plot(b.pass2(), want, what)
        plots.append(want)
    assert not any(np.array_equal(plots[i], plots[j]) for i, j in ((0, 1), (1, 2), (0, 2)))
    b.close()


# ---- B. two-word k-mers, and lists with a meta word: kf_apply, kf_sortkey + kf_apply_indexed ----------------------------------

def cuts_of_a_list(b, proof, lst, sig, what):
    """SORT_MIN - 1 rows (kf_apply), SORT_MIN rows and all of them (kf_sortkey, the pair sort, kf_apply_indexed)"""
    L, t = lim(), b.t
    w = t.words.shape[1]
    buf = b.put(lst.view(np.int64))
    plots = []
    for cut in (L["SORT_MIN"] - 1, L["SORT_MIN"], len(lst)):
        b.e.pass1(proof)
        assert b.e.record_words() == lst.shape[1] == w + (proof == "exact")
        assert b.e.apply(buf.data_ptr(), cut) == 0 == lz.missing_of(t, lst[:cut], proof == "exact"), (what, cut)
        long = cut >= L["SORT_MIN"]
        state(b.e, "kf_apply_indexed" if long else "kf_apply", long, None, cut, sig, (what, cut))
        want = lz.flag_plot(t, lz.flagged_by(t, lst[:cut]))
        same_plot(b.pass2(), want, (what, cut))
        plots.append(want)
    assert not np.array_equal(plots[0], plots[1]) and not np.array_equal(plots[1], plots[2]) and np.array_equal(plots[2], t.plot)


@pytest.mark.parametrize("sig", [True, False], ids=["signatures", "k-mers"])
@pytest.mark.parametrize("k", lz.KS2)
def test_key_only_list_of_two_word_kmers(k, sig, monkeypatch):
    hooks(monkeypatch, SIG=None if sig else 0)
    L = lim()
    t = lz.flag_table(k, L["SORT_MIN"] + 2)
    signatures_planned(t, sig)
    b = Bound(t)
    cuts_of_a_list(b, "hash", lz.apply_list(t, lz.key_rows(t), L["SORT_MIN"]), sig, f"k={k} hash sig={sig}")
    b.close()


@pytest.mark.parametrize("k", lz.KS)
def test_list_with_a_meta_word(k, monkeypatch):
    """exact proof: a row per entry, count | flag << 16.  The rows with bit 16 clear -- two thirds of them -- must not flag: the
    plot is the oracle's for the rows with the bit, cut by cut"""
    hooks(monkeypatch)
    L = lim()
    t = lz.flag_table(k, L["SORT_MIN"] + 2)
    lst = lz.apply_list(t, lz.meta_rows(t, True), L["SORT_MIN"])
    quiet = (lst[:, -1] >> U(16)) & U(1) == 0
    assert quiet[: L["SORT_MIN"] - 1].sum() > 100
    b = Bound(t)
    cuts_of_a_list(b, "exact", lst, True, f"k={k} exact")
    b.close()


@pytest.mark.parametrize("short", [True, False], ids=["kf_apply", "kf_apply_indexed"])
@pytest.mark.parametrize("k", lz.KS)
def test_exact_proof_reports_what_is_missing(k, short, monkeypatch):
    """a count off by one, a k-mer the table lacks inside a run of 64 equal signatures, one with the signature of a lone entry:
    each reports missing; the unchanged list reports 0"""
    hooks(monkeypatch)
    L = lim()
    plan = engine.pass1_plan(k, 5000, "exact", own_lookups=False, have_index=False, bm_cap=30)
    assert plan["use_sig"] == 1 and plan["dir_preset"] == 0
    t, sigsh, fams = lz.signature_table(k, plan["dir_per"], 0)
    assert lz.runs_of(t, sigsh)[lz.family_rows(t, fams[0])[1][0]] == 1 and fams[4].length >= 30
    rows = lz.meta_rows(t, True)
    m = L["SORT_MIN"] - 1 if short else len(rows)
    assert len(rows) >= L["SORT_MIN"]
    w = t.words.shape[1]
    lists = {"unchanged": rows[:m]}
    off = rows[:m].copy()
    off[m // 2, w] += U(1)
    lists["count"] = off
    for name, fam in (("absent in a run", fams[4]), ("absent beside a lone entry", fams[0])):
        lst = rows[:m].copy()
        lst[m // 3, :w] = lz.family_rows(t, fam)[2][0]
        lists[name] = lst
    b = Bound(t)
    for what, lst in lists.items():
        want = lz.missing_of(t, lst, True)
        assert want == (0 if what == "unchanged" else 1)
        b.e.pass1("exact")
        got = b.e.apply(b.put(lst.view(np.int64)).data_ptr(), m)
        assert (got > 0) == (want > 0), (k, what, got)
        state(b.e, "kf_apply" if short else "kf_apply_indexed", not short, None, m, True, (k, what))
    b.close()


# ---- C. sig_find on runs of equal signatures ----------------------------------------------------------------------------------

def signature_bound(k, proof, index):
    plan = engine.pass1_plan(k, 5000, proof, own_lookups=False, have_index=index, bm_cap=30)
    assert plan["use_sig"] == 1 and bool(plan["dir_preset"]) == (index and proof == "hash")
    t, sigsh, fams = lz.signature_table(k, plan["dir_per"], 3 if plan["dir_preset"] else 0)
    return Bound(t, index), sigsh, fams


@pytest.mark.parametrize("index", [True, False], ids=["prefix index", "own directory"])
@pytest.mark.parametrize("k", lz.KS)
def test_runs_of_equal_signatures(k, index, monkeypatch):
    """runs of 1, 2, 3, 64 and about 1000 entries that share bucket and signature, in the directory of a 3-byte prefix index and
    in pass 1's own.  Hash proof: the rows of exactly the targets; every member is a candidate whose pair only its flag (a
    target) or nobody's (the others) removes, so the plot shows a flag on any other member; a k-mer the table lacks inside a run
    of two or more is missing, because there the k-mers are compared.  Exact proof: a row per member, and the absent k-mer of
    every run is missing.  (With signatures on, a hash-proof list otherwise holds table k-mers only: the design lets a lone
    signature stand for its k-mer -- the fingerprint proves the closure --, which is not asserted either way.)"""
    hooks(monkeypatch)
    b, sigsh, fams = signature_bound(k, "hash", index)
    t = b.t
    w = t.words.shape[1]
    members = [lz.family_rows(t, f) for f in fams]
    rows = lo.sort_rows(np.concatenate([mw[f.target] for (mw, _, _), f in zip(members, fams)]))
    kernel = "kf_apply_sorted" if w == 1 else "kf_apply"
    b.e.pass1("hash")
    assert b.e.apply(b.put(rows.view(np.int64)).data_ptr(), len(rows)) == 0
    state(b.e, kernel, False, None, len(rows), True, (k, index))
    flagged = lz.flagged_by(t, rows)
    assert np.array_equal(np.flatnonzero(flagged), np.sort(np.concatenate([j[f.target] for (_, j, _), f in zip(members, fams)])))
    same_plot(b.pass2(), lz.flag_plot(t, flagged), (k, index, "targets"))
    for f, (_, _, absent) in zip(fams, members):
        if f.length >= 2:
            lst = np.concatenate([rows, absent])
            assert lz.missing_of(t, lst, False) == 1
            b.e.pass1("hash")
            assert b.e.apply(b.put(lst.view(np.int64)).data_ptr(), len(lst)) > 0, (k, index, f.length)
    b.close()
    # exact proof: pass 1 writes its own directory, eight entries per bucket
    b, sigsh, fams = signature_bound(k, "exact", index)
    t = b.t
    members = [lz.family_rows(t, f) for f in fams]
    at = np.concatenate([j for _, j, _ in members])
    every = lz.meta_rows(t, True)
    rows = every[np.isin(lz.index_of_rows(t, every), at)]
    assert len(rows) == len(at)
    b.e.pass1("exact")
    assert b.e.apply(b.put(rows.view(np.int64)).data_ptr(), len(rows)) == 0
    state(b.e, "kf_apply", False, None, len(rows), True, (k, index, "exact"))
    same_plot(b.pass2(), lz.flag_plot(t, lz.flagged_by(t, rows)), (k, index, "exact"))
    for f, (_, _, absent) in zip(fams, members):
        lst = rows.copy()
        lst[len(lst) // 2, :w] = absent[0]
        b.e.pass1("exact")
        assert b.e.apply(b.put(lst.view(np.int64)).data_ptr(), len(lst)) > 0, (k, index, f.length, "exact")
    b.close()


# ---- D. the engine's own list through the list route ---------------------------------------------------------------------------

@pytest.mark.parametrize("floor", [False, True], ids=["as it comes", "sorted"])
@pytest.mark.parametrize("k,two_way", [(31, False), (24, True)], ids=["k=31 one-way", "k=24 two-way"])
def test_unfiltered_run_through_sentinels_and_through_compaction(k, two_way, floor, monkeypatch):
    """one workgroup of pass 1 fills its chunks to the brim: the holes of the last one become sentinel words (kf_fill_holes), which
    are skipped before the flag bit of a one-way record is read -- and, with the sort at its floor, sorted to the end of the
    list; the default grid leaves ragged chunks, which are squeezed (kf_compact)"""
    L = lim()
    t = lz.brim_full_table(k, not two_way, L["F_CH"], 3 * L["SORT_MIN"])
    nreq = len(lz.key_rows(t) if two_way else lz.one_way_rows(t))
    low, high = emitted_bounds(t.packed, t.cnt, k, not two_way)
    assert low == high == nreq
    b = Bound(t)
    for grid, holes in ((1, "sentinels"), (None, "compacted")):
        what = f"k={k} grid={grid} floor={floor}"
        hooks(monkeypatch, NO_FILTER=1, VERIFY_SORT=1, TWO_WAY=1 if two_way else None, P1_GRID=grid,
              APPLY_SORT_MIN=L["SORT_MIN"] if floor else None)
        plot, st = b.run("hash")
        ls = b.e.lookup_state()
        assert st["path"] == 1 and ls["nb"] == 0 and ls["fb"] == 0 and ls["one_way"] == (not two_way) and ls["rw"] == 1, (what, ls)
        assert (grid is None and ls["p1_grid"] > 1) or ls["p1_grid"] == grid, (what, ls)
        assert low <= st["nemitted"] <= high and st["nrequests"] == st["nemitted"], (what, st)
        slots = ls["p1_chunks"] * L["F_CH"]
        ap = state(b.e, "kf_apply_sorted", floor, holes, slots if holes == "sentinels" else nreq, True, what)
        assert holes == "compacted" or nreq < ap["covered"] < nreq + nreq // 16, (what, ap)
        same_plot(plot, t.plot, what)
    b.close()


def test_k32_compacts_because_the_all_t_kmer_is_the_sentinel(monkeypatch):
    """T x 32 is a request (A x 32 sends it) and all ones: even with brim-full chunks the engine squeezes the list instead of
    filling its holes, and the flag of T x 32, which decides a plot cell, is set"""
    L = lim()
    t = lz.brim_full_table(32, False, L["F_CH"], 3 * L["SORT_MIN"], True)
    rows = lz.key_rows(t)
    assert rows[-1, 0] == ~U(0)
    b = Bound(t)
    for floor in (False, True):
        hooks(monkeypatch, NO_FILTER=1, VERIFY_SORT=1, P1_GRID=1, APPLY_SORT_MIN=L["SORT_MIN"] if floor else None)
        plot, st = b.run("hash")
        ls = b.e.lookup_state()
        assert st["path"] == 1 and ls["p1_grid"] == 1 and ls["nb"] == 0 and st["nemitted"] == len(rows)
        assert ls["p1_chunks"] * L["F_CH"] < len(rows) + len(rows) // 16          # (brim-full: k < 32 would take the sentinels)
        state(b.e, "kf_apply_sorted", floor, "compacted", len(rows), True, floor)
        same_plot(plot, t.plot, floor)
    assert not np.array_equal(lz.flag_plot(t, lz.flagged_by(t, rows[:-1])), t.plot)
    b.close()


@pytest.mark.parametrize("proof", ["hash", "exact"])
def test_two_word_run_compacts_and_looks_up_through_the_index_sort(proof, monkeypatch):
    """k = 51 without the filter, and under the exact proof: kf_compact, then kf_apply<2> below SORT_MIN records and kf_sortkey,
    the pair sort and kf_apply_indexed<2> from there on (two tables)"""
    L = lim()
    hooks(monkeypatch, NO_FILTER=1)
    for t in (lz.adversarial(51, 500, 11), lz.adversarial(51, 8000, 11)):
        least = len(t.cnt) if proof == "exact" else len(lz.one_way_rows(t))
        again = int(lo.may_send_twice(t.words[:, 0], t.k).sum())           # (k // 2 bases lie in the first word)
        b = Bound(t)
        plot, st = b.run(proof)
        ls = b.e.lookup_state()
        assert st["path"] == 1 and ls["nb"] == 0 and ls["rw"] == (3 if proof == "exact" else 2) and ls["one_way"] == (proof == "hash")
        assert least <= st["nemitted"] <= least + again, (st, least, again)
        long = st["nemitted"] >= L["SORT_MIN"]
        assert long == (least >= L["SORT_MIN"])
        state(b.e, "kf_apply_indexed" if long else "kf_apply", long, "compacted", st["nemitted"], True, (proof, len(t.cnt)))
        same_plot(plot, t.plot, (proof, len(t.cnt)))
        b.close()


@pytest.mark.parametrize("bucketed", [False, True], ids=["chunk list", "bucketed first"])
def test_short_kmers_filter_their_chunk_list_with_a_one_bit_map(bucketed, monkeypatch):
    """k = 10 has no 12 id bits: the plan gives no look-up chain, kf_filter<1> reads the chunk list -- or, with
    SMG_FILTER_SORT_MIN at its floor, the list bucketed on its leading 8 bits, sentinel words among it -- under a one-bit map.
    The kept list is the emitted list under the engine's own map as a multiset; the look-ups of the kept list give the plot"""
    L = lim()
    hooks(monkeypatch, FILTER_SORT_MIN=L["SORT_MIN"] if bucketed else None)
    k = 10
    t = lz.adversarial(k, 3000, 7)
    plan = engine.pass1_plan(k, len(t.cnt), "hash", own_lookups=False, have_index=False, bm_cap=30)
    assert plan["nb"] == 0 and plan["bm2"] == 0 and 0 < plan["bm_bits"] < 12
    want = lz.key_rows(t)
    b = Bound(t)
    b.e.pass1("hash")
    E = b.routed(b.e.nreq())
    assert np.array_equal(np.unique(E[:, 0]), want[:, 0]) and len(E) <= len(want) + int(lo.may_send_twice(t.words[:, 0], k).sum())
    bits, nw = b.e.blockmap()
    assert bits == plan["bm_bits"]
    m = b.put(np.zeros(nw, np.int32), torch.int32)
    b.e.blockmap_copy(0, nw, m.data_ptr())
    torch.cuda.synchronize()
    mw = m[:nw].cpu().numpy().view(np.uint32).astype(np.int64)
    ew, ev = wo.map_bits(t, bits)                                        # (a set bit means "maybe": the candidates' at least)
    full = np.zeros(nw, np.int64)
    full[ew] = ev
    assert np.array_equal(mw & full, full) and 0 < int((mw != 0).sum())
    kept = b.e.filter(None)
    ap = b.e.apply_state()
    assert ap["presorted"] == ("bucketed" if bucketed else "as it is") and b.e.lookup_state()["nb"] == 0, ap
    K = b.routed(kept)
    ids = wo.ids_of(E, bits)
    keep = (mw[ids >> 5] >> (ids & 31)) & 1 == 1
    assert 0 < keep.sum() < len(E)
    extra, lost = lo.multiset_diff(K, E[keep])
    assert not extra and not lost, (len(K), int(keep.sum()), extra[:4], lost[:4])
    assert b.e.apply_own() == 0
    ap = b.e.apply_state()
    assert ap["kernel"] == "kf_apply_sorted" and ap["holes"] in ("sentinels", "compacted") and ap["sig"], ap
    same_plot(b.pass2(), t.plot, bucketed)
    b.close()
