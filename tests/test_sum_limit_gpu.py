"""The pair-sum limit where it decides a degree, at every site that applies it: d_tests<.., CHECK> of kf_pass1_d (smg_pass1d.hpp),
both halves of big_block_walk behind kf_bigfix and big_block_scan, kf_pass1<3>, the far scan of pass 2, kf_extract (smg_fast.hpp),
k_pass1 with its linear, bisection and look-up branches, k_pass2 and the extract kernels of k > 85 (smg_counted.hpp).

The tables are those of tests/sum_limit_oracle.py: families with a DECOY, a one-away neighbour beyond the limit that must not bump a
degree, on the routes "registers", "deferred" and "long".  Every pair of their plots exists only because a decoy was ignored, and
tests/test_sum_limit_host.py asserts on the CPU what each table holds.  Expected values: oracle/brute.py for plots and extract
lines, tests/lookup_oracle.py and tests/wide_oracle.py for request records and candidate maps, the reference binary's fixtures
(tests/golden/k*_sumlimit.*) for the tables that went through it."""
import functools

import numpy as np
import pytest
import torch

import brute
import lookup_oracle as lo
import sum_limit_oracle as so
import test_lookup_regimes_gpu as lr
import test_wide_fast_path_gpu as wf
import wide_oracle as wo
from conftest import load_golden, make_table
from smudgeplot_amd import engine, ktab, sharded
from test_extract import load_extract
from test_extract_general import all_labels, check, is_closed
from test_gpu_parity import _manual_sharded, table_from
from test_pass1_forms_gpu import TWO_WAY_HOT, Bound, clear, run_once, words_of
from test_sum_limit_host import analysed, limits, mid

pytestmark = pytest.mark.gpu

U = np.uint64
DEV = torch.device("cuda:0")
SENT = -0x0123456789ABCDEF

# name: (k, hooks, ibyte of the index handed over, proof, the smg_engine_pass1_form it must launch as (var, words per record))
FORMS = {
    "k31 one-way hot": (31, {}, 3, "hash", (2, 1)),
    "k31 two-way hot": (31, {"TWO_WAY": 1}, 3, "hash", (TWO_WAY_HOT, 1)),
    "k30": (30, {}, 3, "hash", (2, 1)),
    "k33": (33, {}, 3, "hash", (2, 2)),
    "k51": (51, {}, 3, "hash", (2, 2)),
    "k31 general": (31, {}, 1, "hash", (1, 1)),
    "k31 exact": (31, {}, 3, "exact", (1, 2)),
}
HOT = ("k31 one-way hot", "k31 two-way hot", "k30", "k33", "k51")


def long_blocks(t):
    """bool per entry: its window block has more than four entries, so that the exact redo may send its request again (what
    lookup_oracle.may_send_twice says for k <= 32)"""
    return so.block_spans(t.packed, t.k)[1] > 4


def run_form(form, t, want, what, big=False, a=None):
    """one table through one form: the form, the path, the plot and (k <= 32, hash proof) how many requests it may send"""
    k, env, ibyte, proof, (var, rw) = FORMS[form]
    assert k == t.k
    plot, st, got = run_once(t.packed, t.cnt, k, ibyte=ibyte, symcheck=proof)
    assert got == {"var": var, "w": words_of(k), "rw": rw, "inner_only": 0}, (what, got)
    assert st["path"] == 1 and st["nels"] == len(t.cnt), (what, st)
    if not np.array_equal(plot, want):
        s, m = np.nonzero(plot != want)
        raise AssertionError(f"{what}: {len(s)} pixels differ, the first (sum {s[0]}, min {m[0]}): {plot[s[0], m[0]]} for {want[s[0], m[0]]}")
    if big:
        assert st["nbig"] > 0, (what, st)
    if proof == "hash":                      # the senders of the final state, and once more those an exact redo may send again
        a = a or wo.analyse(t.packed, t.cnt, k)
        send = so.senders(a, one_way=bool(k & 1) and "TWO_WAY" not in env)
        low, high = int(send.sum()), int(send.sum()) + int((send & long_blocks(t)).sum())
        print(f"{what}: emitted {st['nemitted']} in [{low}, {high}], kept {st['nrequests']}")
        assert low <= st["nemitted"] <= high, what
    return st


# ---- 1. the three routes through every form of kf_pass1_d --------------------------------------------------------------------------

@pytest.mark.parametrize("route", so.ROUTES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_route_through_every_form(form, route, monkeypatch):
    k, env = FORMS[form][:2]
    t, a = analysed(k, route)
    clear(monkeypatch, **env)
    run_form(form, t, a.plot, f"{form} {route}", big=route != "registers", a=a)


@pytest.mark.parametrize("route", so.ROUTES)
def test_hash_and_exact_proofs_give_the_same_plot(route, monkeypatch):
    clear(monkeypatch)
    for k in so.KS_NARROW:
        t, a = analysed(k, route)
        got = {proof: run_once(t.packed, t.cnt, k, symcheck=proof) for proof in ("hash", "exact")}
        assert got["exact"][2]["var"] == 1 and got["exact"][2]["rw"] == words_of(k) + 1
        assert np.array_equal(got["hash"][0], got["exact"][0]) and np.array_equal(got["hash"][0], a.plot), (k, route)
        assert got["exact"][1]["nemitted"] >= len(t.cnt)                # every entry sends count | hi << 16


# ---- 2. registers: every entry of a thread, lane boundaries, tile seams, waves with and without a heavy count --------------------------

@pytest.mark.parametrize("form", HOT + ("k31 general",))
def test_families_on_every_entry_of_a_thread(form, monkeypatch):
    """the same closed table behind 0 .. 3 leading fillers: a family's members fall on every one of a thread's four entries and
    across a lane boundary"""
    k, env = FORMS[form][:2]
    clear(monkeypatch, **env)
    want = analysed(k, "registers")[1].plot
    sent = set()
    for s in range(4):
        t = so.shifted(k, s, mid(k))
        st = run_form(form, t, want, f"{form} shift {s}", big=False)
        sent.add((st["nemitted"], st["nrequests"]))
    assert len(sent) == 1, sent                                          # the fillers send nothing


@pytest.mark.parametrize("members,low", so.SPLITS)
@pytest.mark.parametrize("form", HOT)
def test_a_family_across_an_inner_tile_seam(form, members, low, monkeypatch):
    """1|2 and 2|1 of a triple, 1|3, 2|2 and 3|1 of a four, on the first and on the second inner seam"""
    k, env = FORMS[form][:2]
    clear(monkeypatch, **env)
    want = analysed(k, "registers")[1].plot
    for seam_no in (1, 2):
        t, _ = so.seam_table(k, mid(k), limits()[0]["D_OWN"], seam_no, members, low)
        run_form(form, t, want, f"{form} seam {seam_no} split {low}|{members - low}", big=False)


@pytest.mark.parametrize("form", HOT)
def test_waves_with_and_without_a_heavy_count_in_one_launch(form, monkeypatch):
    k, env = FORMS[form][:2]
    clear(monkeypatch, **env)
    t = so.sparse_table(k, 100 + k)
    run_form(form, t, brute.hetmers_plot(t.packed, t.cnt, k), f"{form} sparse", big=False)


# ---- 3. request records and the candidate map of the phase API (two-way: hot form 6 for odd k, 2 for even k) -------------------------

def phase_pass1(t, a, what):
    """pass 1 of the phase API with a 32-bit map and the table's index: the emitted list against the oracle's, record by record,
    and the low halves of the engine's own candidate map against the entries with exactly one suffix-side pair"""
    k = t.k
    b = Bound(t.packed, t.cnt, k)
    try:
        b.e.set_blockmap_bits(32)
        b.e.pass1("hash")
        form, ls, n0 = b.e.pass1_form(), b.e.lookup_state(), b.e.nreq()
        assert form == {"var": TWO_WAY_HOT if k & 1 else 2, "w": words_of(k), "rw": words_of(k), "inner_only": 0}, (what, form)
        assert (ls["one_way"], ls["bm2"], ls["fb"]) == (0, 1, 32), (what, ls)
        E, _ = lr.routed(b.e, n0)
        rc = lo.packed_to_words(ktab.revcomp_packed(t.packed, k), k)
        send = so.senders(a, one_way=False)
        want = lo.sort_rows(rc[send])
        again = lo.sort_rows(rc[send & long_blocks(t)])
        uniq, mult = np.unique(E, axis=0, return_counts=True)
        lr.same_rows(uniq, want, 10, f"{what}: emitted records")
        assert mult.max() <= 2 and not lo.multiset_diff(uniq[mult > 1], again)[0], what
        if k <= 32:
            assert np.array_equal(long_blocks(t), lo.may_send_twice(ktab.packed_to_u64(t.packed), k))
        bits, nw = b.e.blockmap()
        m = torch.empty(nw, dtype=torch.int32, device=DEV)
        b.e.blockmap_copy(0, nw, m.data_ptr())
        torch.cuda.synchronize()
        low = m[0::2]
        at = torch.nonzero(low).flatten()
        got_w, got_v = at.cpu().numpy(), low[at].cpu().numpy().view(np.uint32).astype(np.int64)
        w, v = wo.map_bits(a, bits)
        have = dict(zip(got_w.tolist(), got_v.tolist()))
        assert all(have.get(wi, 0) & vi == vi for wi, vi in zip(w.tolist(), v.tolist())), f"{what}: a candidate without its bit"
        if not long_blocks(t).any():                                     # (the provisional bits of a redone entry are a superset)
            assert np.array_equal(got_w, w) and np.array_equal(got_v, v), f"{what}: the map is not the oracle's"
        return len(E)
    finally:
        b.close()


@pytest.mark.parametrize("k", so.KS_NARROW)
def test_requests_and_candidate_map_record_by_record(k, monkeypatch):
    """no decoy is named: a heavy neighbour on a position p > k - 1 - p sends no request and sets no bit; shifted, on the seams and
    on every route"""
    clear(monkeypatch)
    own = limits()[0]["D_OWN"]
    for route in so.ROUTES:
        t, a = analysed(k, route)
        phase_pass1(t, a, f"k={k} {route}")
    for s in (1, 2, 3):
        t = so.shifted(k, s, mid(k))
        phase_pass1(t, wo.analyse(t.packed, t.cnt, k), f"k={k} shift {s}")
    for members, low in so.SPLITS:
        t, _ = so.seam_table(k, mid(k), own, 1, members, low)
        phase_pass1(t, wo.analyse(t.packed, t.cnt, k), f"k={k} split {low}|{members - low}")
    t = so.sparse_table(k, 100 + k)
    phase_pass1(t, wo.analyse(t.packed, t.cnt, k), f"k={k} sparse")


# ---- 4. k = 65 .. 85: kf_pass1<3> and big_block_scan ------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", so.ROUTES)
@pytest.mark.parametrize("k", so.KS_WIDE)
def test_three_word_kmers_record_by_record(k, route, monkeypatch):
    """blocks of at most four, blocks up to the halo of kf_pass1<3> and blocks far beyond it (big_block_scan): the emitted rows with
    their S_hi flag, the candidate map, the plot after the engine's own look-ups, one run -- under both proofs"""
    wf.hooks(monkeypatch)
    t, a = analysed(k, route)
    e = wf.bound(a)
    try:
        for proof in ("hash", "exact"):
            what = f"k={k} {route} {proof}"
            want = wo.emitted_rows(a, proof == "exact")
            e.pass1(proof)
            E, _ = wf.routed(e, e.nreq())
            wf.same_rows(E, want, what)
            if proof == "hash":
                bits, m = wf.own_map(e)
                assert torch.equal(m, wf.expected_map(a, bits, m.numel())), what
            assert e.apply_own() == 0, what
            assert np.array_equal(wf.plot_of(e), a.plot), what
            plot, st = wf.run_of(e, proof)
            assert st["path"] == 1 and st["nemitted"] == len(want) and np.array_equal(plot, a.plot), what
    finally:
        e.close()


# ---- 5. k > 85: k_pass1, k_pass2 ------------------------------------------------------------------------------------------------------

def counted_rows(t, a, exact):
    """the request list of k_pass1 (symmetric path): rc(x), count | S_hi << 16, for S_hi > 0 (exact proof: for every entry)"""
    send = np.ones(len(t.cnt), bool) if exact else a.s_hi > 0
    rc = lo.packed_to_words(ktab.revcomp_packed(t.packed, t.k), t.k)
    meta = t.cnt.astype(U) | ((a.s_hi & 0xFF).astype(U) << U(16))
    return lo.sort_rows(np.concatenate([rc, meta[:, None]], axis=1)[send])


def routed_to(e, n, splitters, nranks):
    """the engine's request list as routed -> (rows in buffer order, per-rank counts)"""
    rw = e.record_words()
    buf = torch.full((n * rw + 1024,), SENT, dtype=torch.int64, device=DEV)
    counts = e.route(np.zeros(0, U) if splitters is None else splitters, nranks, buf.data_ptr(), n)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert sum(counts) == n and (host[n * rw:] == SENT).all(), "route wrote behind the records it reported"
    return host[: n * rw].view(U).reshape(n, rw), counts


def engine_on(words, cnt, k):
    tk = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1).copy()).to(DEV)
    tc = torch.from_numpy(np.ascontiguousarray(cnt).view(np.int16).copy()).to(DEV)
    e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
    e.bind(k, len(cnt), tk.data_ptr(), tc.data_ptr())
    return e, (tk, tc)


@pytest.mark.parametrize("route", so.ROUTES)
@pytest.mark.parametrize("k", so.KS_COUNTED)
def test_counted_kernels_on_both_sides_of_the_linear_walk(k, route):
    """blocks of at most four, blocks up to the partner window (the linear branch of k_pass1) and blocks of 120 .. 600 (its
    bisection branch): the requests carry S_hi, the number of pairs within the limit at p > k - 1 - p; plots under every proof"""
    t, a = analysed(k, route)
    e, keep = engine_on(a.words, t.cnt, k)
    try:
        for proof in ("hash", "exact"):
            e.pass1(proof)
            E, _ = routed_to(e, e.nreq(), None, 1)
            wf.same_rows(E, counted_rows(t, a, proof == "exact"), f"k={k} {route} {proof}")
    finally:
        e.close()
    for proof in ("hash", "exact", "none"):
        plot, st = engine.hetmers_run(table_from(t.packed, t.cnt, k), symcheck=proof)
        assert st["path"] == (2 if proof == "none" else 1) and np.array_equal(plot, a.plot), (k, route, proof)


@pytest.mark.parametrize("shards", [0, 2], ids=["in core", "two shards out of core"])
def test_the_wrap_of_a_degree_meets_the_limit(shards, monkeypatch):
    """k100_sumlimit, through the reference binary: a k-mer with 256 neighbours, one of them heavy, has degree 255 and its pair does
    not count (it would with the limit ignored: 256 wraps to 0); one with 257, one of them heavy, has degree 0 and its pair counts"""
    g = load_golden("k100_sumlimit")
    if shards:
        monkeypatch.setenv("SMG_SEQUENTIAL_SHARDS", str(shards))
    for proof in ("hash", "exact"):
        plot, st = engine.hetmers_run(make_table(g), symcheck=proof)
        assert st["path"] == 1 and engine.smu_text(plot) == g["smu"], (shards, proof)
        assert np.array_equal(plot, brute.hetmers_plot(g["packed"], g["counts"], g["k"])), (shards, proof)


# ---- 6. the general path: prefix-side decoys are resolved by look-ups --------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def unclosed(name):
    """the fixture without the complement of one bystander (a k-mer without a neighbour): the proof fails
    -> (packed, counts, k, plot, labels, lines)"""
    k = so.FIXTURES[name]
    t = so.fixture_table(name, mid(k))
    deg = so.degrees(t.packed, t.cnt, k)
    rc = ktab.revcomp_packed(t.packed, k)
    at = {bytes(r): i for i, r in enumerate(t.packed)}
    x = next(i for i in range(len(deg) // 3, len(deg)) if deg[i] == 0 and t.cnt[i] < 60 and at[bytes(rc[i])] != i)
    keep = np.ones(len(deg), bool)
    keep[at[bytes(rc[x])]] = False
    packed, cnt = t.packed[keep], t.cnt[keep]
    assert not is_closed(packed, cnt, k)
    plot = brute.hetmers_plot(packed, cnt, k)
    assert np.array_equal(plot, brute.hetmers_plot(t.packed, t.cnt, k))            # (a bystander: the same plot)
    labels = all_labels(plot)
    return packed, cnt, k, plot, labels, brute.extract_lines(packed, cnt, k, labels)


@pytest.mark.parametrize("shards", [0, 2, 3])
@pytest.mark.parametrize("name", ["k31_sumlimit", "k100_sumlimit"])
def test_general_path_and_its_extract_lines(name, shards, monkeypatch):
    """k_pass1<W, false>: the decoys in front of k // 2 are found by directory look-ups (in another shard of the device where the
    table is cut into virtual shards) and must not count; the extract lines come from the same run"""
    packed, cnt, k, want_plot, labels, want = unclosed(name)
    assert sum(len(v) for v in want.values()) > 300
    if shards:
        monkeypatch.setenv("SMG_SHARD_LIMIT", str(len(cnt) // shards + 1))
    tab = lambda: make_table(dict(packed=packed, counts=cnt, k=k, ibyte=1, nparts=1))
    for proof in ("hash", "exact"):
        plot, st = engine.hetmers_run(tab(), symcheck=proof)
        assert st["path"] == 2 and np.array_equal(plot, want_plot), (name, shards, proof)
        check(tab(), labels, want_plot, want, symcheck=proof)


# ---- 7. extract lines of the symmetric path ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", so.ROUTES)
@pytest.mark.parametrize("k", [31, 30, 51, 65, 100])
def test_extract_lines_of_decoy_decided_pairs(k, route):
    """every pixel labelled: the lines name the light partner, never the decoy (kf_extract and its far branch, k_extract)"""
    t, a = analysed(k, route)
    labels = all_labels(a.plot)
    want = brute.extract_lines(t.packed, t.cnt, k, labels)
    assert sum(len(v) for v in want.values()) == a.plot[:, :500].sum() > 0
    for proof in ("hash", "exact"):
        check(table_from(t.packed, t.cnt, k), labels, a.plot, want, symcheck=proof)


@pytest.mark.parametrize("name", ["k31_sumlimit", "k100_sumlimit"])
def test_extract_goldens_label_decoy_decided_pixels(name):
    g, labels, lines, _ = load_extract(name)
    assert (499, 501) in labels                                          # the boundary family (499, 501, 502)
    plot, got = engine.hetmers_extract(make_table(g), labels)
    assert engine.smu_text(plot) == g["smu"] and {lab: sorted(v) for lab, v in got.items()} == lines


# ---- 8. the phase API over two prefix shards, the exchange done by hand ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["k31_sumlimit", "k100_sumlimit"])
def test_two_shards_exchange_requests_with_the_right_s_hi(name):
    """a cut in the middle of the table: most families stand on one shard and their complement images on the other, so that the
    degree of an image's prefix side arrives as a request.  Every shard's routed list against the oracle, rank by rank (k = 100: the
    record carries S_hi itself; k = 31: the record is sent exactly when S_hi > 0); then the whole protocol against the plot"""
    k = so.FIXTURES[name]
    t = so.fixture_table(name, mid(k))
    a = wo.analyse(t.packed, t.cnt, k)
    W = words_of(k)
    flat = np.ascontiguousarray(a.words).reshape(-1)
    n = len(t.cnt)
    cut = sharded.fix_cut(flat, W, k, n // 2)
    apart = sum(1 for pl in so.place(t) if ((pl.idx < cut).all() and (pl.rc >= cut).all()) or ((pl.rc < cut).all() and (pl.idx >= cut).all()))
    assert apart >= 24, apart
    split = a.words[cut].copy()
    rc = lo.packed_to_words(ktab.revcomp_packed(t.packed, k), k)
    behind = np.array([tuple(r) >= tuple(split.tolist()) for r in rc.tolist()])           # the rank that owns rc(x)
    for r, (first, last) in enumerate(((0, cut), (cut, n))):
        e, keep = engine_on(a.words[first:last], t.cnt[first:last], k)
        try:
            e.pass1("hash")
            E, counts = routed_to(e, e.nreq(), split, 2)
        finally:
            e.close()
        mine = np.zeros(n, bool)
        mine[first:last] = True
        for dst in (0, 1):
            got = lo.sort_rows(E[sum(counts[:dst]): sum(counts[: dst + 1])])
            send = mine & (a.s_hi > 0 if k > 85 else so.senders(a, one_way=False)) & (behind == bool(dst))
            what = f"{name}: shard {r} to shard {dst}"
            if k > 85:
                meta = t.cnt.astype(U) | ((a.s_hi & 0xFF).astype(U) << U(16))
                wf.same_rows(got, lo.sort_rows(np.concatenate([rc, meta[:, None]], axis=1)[send]), what)
            else:
                uniq, mult = np.unique(got, axis=0, return_counts=True)
                wf.same_rows(uniq, lo.sort_rows(rc[send]), what)
                assert not lo.multiset_diff(uniq[mult > 1], lo.sort_rows(rc[send & long_blocks(t)]))[0], what
    tk = torch.from_numpy(flat.view(np.int64).copy()).to(DEV)
    tc = torch.from_numpy(np.ascontiguousarray(t.cnt).view(np.int16).copy()).to(DEV)
    for proof in ("hash", "exact"):
        total, _ = _manual_sharded(k, tk, tc, [0, cut, n], DEV, symcheck=proof)
        assert np.array_equal(total.cpu().numpy().reshape(engine.PLOT_ROWS, engine.PLOT_COLS), a.plot), (name, proof)


# ---- 9. counts the reference binary cannot take ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 51, 70, 100])
def test_decoys_beyond_int16(k, monkeypatch):
    """decoys of 32768, 40000 and 65535: a count is an unsigned 16-bit number and a sum must not be taken in 16 bits.  Bound with
    Engine.bind (no probe on that door) and compared with oracle/brute.py alone: the reference reads such a count as negative."""
    clear(monkeypatch)
    t = so.beyond_int16_table(k, 100 + k, mid=mid(k))
    want = brute.hetmers_plot(t.packed, t.cnt, k)
    words = lo.packed_to_words(t.packed, k)
    for proof in ("hash", "exact", "none"):
        if k <= 64:
            plot, st, _ = run_once(t.packed, t.cnt, k, symcheck=proof)
        else:
            e, keep = engine_on(words, t.cnt, k)
            try:
                plot, st = wf.run_of(e, proof)
            finally:
                e.close()
        assert st["path"] == (2 if proof == "none" else 1), (k, proof, st)
        if not np.array_equal(plot, want):
            s, m = np.nonzero(plot != want)
            raise AssertionError(f"k={k} {proof}: {len(s)} pixels differ, the first (sum {s[0]}, min {m[0]}): {plot[s[0], m[0]]} for {want[s[0], m[0]]}")
