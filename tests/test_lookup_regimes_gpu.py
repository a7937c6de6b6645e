"""The look-up chain between pass 1 and pass 2 (smg_lookup.hpp: kl_tot, kl_scan, kl_woff, kl_part, kl_probe, kl_probe_x) record
by record, at the sizes where its kernels change regime.

A. The phase API hands out the emitted list E (pass1, route) and the kept list K (pass1, filter(map), route): K must be, as
   a multiset, the records of E whose bits are set in the map -- a map the test owns, or the engine's own read back
   (tests/lookup_oracle.py).  Every record that goes through kl_tot / kl_scan / kl_woff / kl_part / kl_probe<LIST> is checked.
B. The fused forms (kl_probe<false>, kl_probe_x) set P flags: the plot against the C oracle (k = 31) or the engine's general
   path (two-word k-mers, where no oracle finishes in time), and the kept count, which is a function of table and map and
   not of the kernel.

What a table does to the kernels is asserted from the oracle and engine.lookup_limits (tests/test_lookup_oracle_host.py), which
regime ran from engine.lookup_state; SMG_P1_GRID gives one or two owners all the requests of a 4e5-entry table."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import lookup_oracle as lo
from conftest import ORACLE_BIN
from smudgeplot_amd import engine, ktab, synth

pytestmark = pytest.mark.gpu

U = np.uint64
LIMITS, wave_shares = lo.LIMITS, lo.wave_shares
DEV = torch.device("cuda:0")
SENT = -0x0123456789ABCDEF
HOOKS = ("SMG_P1_GRID", "SMG_BM_BITS", "SMG_ONE_BIT_MAP", "SMG_PROBE_X", "SMG_PX_ONE_XCC", "SMG_TWO_WAY", "SMG_NO_FILTER", "SMG_SIG")


# ---- tables: (k, words uint64[n, W], counts), made once, on the device once ---------------------------------------------

@functools.lru_cache(maxsize=None)
def table(name):
    if name in ("d405k", "d1080k", "d1133k"):
        keys, cnt = lo.diploid({"d405k": 150000, "d1080k": 400000, "d1133k": 420000}[name])
        return 31, keys.reshape(-1, 1), cnt
    if name == "clustered":
        keys, cnt = lo.clustered()
        return 31, keys.reshape(-1, 1), cnt
    if name == "edges":
        keys, cnt = lo.edges(25)
        return 31, keys.reshape(-1, 1), cnt
    if name == "families":
        keys, cnt = lo.families(31)
        return 31, keys.reshape(-1, 1), cnt
    k = {"wide51": 51, "wide64": 64}[name]
    packed, cnt = lo.wide(k)
    words = lo.packed_to_words(packed, k)
    words.setflags(write=False)
    return k, words, cnt


@functools.lru_cache(maxsize=None)
def on_device(name):
    k, words, cnt = table(name)
    tk = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1).copy()).to(DEV)
    tc = torch.from_numpy(np.ascontiguousarray(cnt).view(np.int16).copy()).to(DEV)
    return tk, tc


@functools.lru_cache(maxsize=None)
def emitted_of(name):
    """the oracle's request list (k <= 32), and the records an exact redo may send a second time"""
    k, words, cnt = table(name)
    keys = words[:, 0]
    own = lo.owns_hi_pair(keys, cnt, k)
    e = np.sort(ktab.revcomp_u64(keys[own], k))
    again = np.sort(ktab.revcomp_u64(keys[own & lo.may_send_twice(keys, k)], k))
    for a in (e, again):
        a.setflags(write=False)
    return e, again


@functools.lru_cache(maxsize=None)
def one_way_of(name):
    k, words, cnt = table(name)
    rec, send = lo.emitted_one_way(words[:, 0], cnt, k)
    for a in (rec, send):
        a.setflags(write=False)
    return rec, send


def bound(name):
    k, words, cnt = table(name)
    tk, tc = on_device(name)
    e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
    e.bind(k, len(cnt), tk.data_ptr(), tc.data_ptr())
    return e


def hooks(monkeypatch, **env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        if val is not None:
            monkeypatch.setenv("SMG_" + name, str(val))


def routed(e, n):
    """the engine's current request list as sorted rows; the buffer behind the records must stay untouched"""
    rw, guard = e.record_words(), 1024
    buf = torch.full((n * rw + guard,), SENT, dtype=torch.int64, device=DEV)
    counts = e.route(np.zeros(0, np.uint64), 1, buf.data_ptr(), n)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert counts == [n], (counts, n)
    assert (host[n * rw:] == SENT).all(), "route wrote behind the records it reported"
    return lo.sort_rows(host[: n * rw].view(np.uint64).reshape(n, rw)), host


def own_map(e):
    bits, nw = e.blockmap()
    m = torch.empty(nw, dtype=torch.int32, device=DEV)
    e.blockmap_copy(0, nw, m.data_ptr())
    torch.cuda.synchronize()
    return m


def same_rows(got, want, nb, what):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    extra, lost = lo.multiset_diff(got, want)
    show = lambda rows: [(hex(r[0]), int(r[0]) >> (64 - nb)) for r in rows[:8]]
    raise AssertionError(f"{what}: {len(got)} rows for {len(want)}; {len(extra)} not expected {show(extra)}, "
                         f"{len(lost)} missing {show(lost)} (first word, bucket)")


def check_emitted(name, E):
    """E against the oracle: the same records, and none twice but those an exact redo may send again"""
    want, again = emitted_of(name)
    uniq, mult = np.unique(E[:, 0], return_counts=True)
    same_rows(uniq.reshape(-1, 1), want.reshape(-1, 1), 10, "emitted records")
    assert mult.max() <= 2 and np.isin(uniq[mult > 1], again).all()
    if len(again) == 0:
        assert np.array_equal(E[:, 0], want)


def exact_filter(name, fb, mapkind, monkeypatch, one_bit=False, grid=None, hi_pos=None, E_ref=None):
    """one (table, map bits, map, pass-1 grid): E and K through the phase API -> (E, K, state, kept)"""
    hooks(monkeypatch, P1_GRID=grid, ONE_BIT_MAP=1 if one_bit else None)
    k = table(name)[0]
    e = bound(name)
    e.set_blockmap_bits(fb)
    e.pass1("hash")
    n0 = e.nreq()
    E, _ = routed(e, n0)
    if k <= 32:
        check_emitted(name, E)
    if E_ref is not None:
        same_rows(E, E_ref, 10, "emitted records at another pass-1 grid")
    e.pass1("hash")
    assert e.nreq() == n0 == len(E)
    st = e.lookup_state()
    two = bool(st["bm2"])
    assert two == (not one_bit) and st["fb"] == fb and st["one_way"] == 0 and st["rw"] == E.shape[1] == (k + 31) // 32
    assert st["nb"] == lo.lookup_geo(fb)[1] and st["probe"] == 0
    if mapkind == "own":
        m = own_map(e)
        assert m.numel() == (1 << (fb - 5)) << two
        kept = e.filter(None)
        keep = lo.keep(E[:, 0], fb, two, lo.DeviceWords(m))
    else:
        m = lo.device_map(mapkind, fb, two, hi_pos)
        kept = e.filter(m.data_ptr())
        keep = lo.keep(E[:, 0], fb, two, lo.formula(mapkind, fb, two, hi_pos))
    assert kept == e.nreq()
    K, host = routed(e, kept)
    print(f"{name} fb={fb} map={mapkind} two={two} grid={grid}: emitted {n0}, kept {kept}, oracle {int(keep.sum())}")
    assert len(K) == kept
    same_rows(K, E[keep], st["nb"], "kept records")
    st = e.lookup_state()
    assert st["probe"] == 3 and st["nb"] == lo.lookup_geo(fb)[1] and st["ticket"] == 0
    e.close()
    return E, K, st, host


def test_the_library_says_what_the_host_tests_assume():
    assert engine.lookup_limits() == LIMITS


# ---- A. record-exact filter ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("one_bit", [False, True], ids=["two_bit", "one_bit"])
@pytest.mark.parametrize("mapkind", ["own", "one_in_four"])
@pytest.mark.parametrize("fb", [12, 23, 24, 25, 30])
def test_kept_list_is_the_emitted_list_under_the_map(fb, mapkind, one_bit, monkeypatch):
    """fb = 12: a slice of 16 coarse words for 1024 threads, nb = 1; 23: the largest slice at two buckets of ~5e4 records (six
    trips of a kl_probe workgroup, the last one partial); 24, 25, 30: nb = 2, 3, 8.  "One id in four" sets every coarse bit and
    a quarter of the ids: every record passes the folded test, pb_fold must OR all four bits of a group."""
    E, K, st, _ = exact_filter("d405k", fb, mapkind, monkeypatch, one_bit=one_bit)
    sizes = lo.bucket_sizes(E[:, 0], fb)
    if fb <= 25:
        assert sizes.min() > LIMITS["PB_TRIP"] and (sizes % 64 != 0).all()       # a second stripe, a ragged end
    if mapkind == "one_in_four":
        assert 0.2 * len(E) < len(K) < 0.3 * len(E)
        # a wave keeps a quarter of two wave instructions: less than one queue drain per pair -- and with a map of ones
        # (test_every_chunk_rolls_over) two per pair


@pytest.mark.parametrize("fb,hi_pos", [(24, 11), (25, None)])
def test_second_bit_at_one_fixed_position(fb, hi_pos, monkeypatch):
    """two-bit layout, low halves all ones: high halves with one position only (one record in 32 passes), and all ones"""
    E, K, _, _ = exact_filter("d405k", fb, "ones", monkeypatch, hi_pos=hi_pos)
    if hi_pos is None:
        assert len(K) == len(E)
    else:
        assert len(E) / 64 < len(K) < len(E) / 16


@pytest.mark.parametrize("name", ["d405k", "clustered"])
def test_32_bit_map_of_the_engine_itself(name, monkeypatch):
    """nb = 10: a few dozen records per bucket -- or two buckets with 4.9e4 each and 1022 without a record"""
    E, K, st, _ = exact_filter(name, 32, "own", monkeypatch)
    sizes = lo.bucket_sizes(E[:, 0], 32)
    if name == "clustered":
        assert np.flatnonzero(sizes).tolist() == [0, 1023] and sizes[[0, 1023]].min() > 5 * LIMITS["PB_TRIP"]
        assert 0 < len(K) < len(E)            # (k-mers with a partner on either side: requests that name a candidate)
    else:
        assert sizes.min() >= 1 and sizes.max() < 256 and len(K) < len(E)


@pytest.mark.parametrize("name,one_bit", [("d1080k", False), ("d1080k", True), ("d1133k", False)])
def test_every_chunk_rolls_over(name, one_bit, monkeypatch):
    """a map of ones at fb = 23: K = E, two queue drains per pair of wave instructions, the worst case of fast_filter's list size.
    On the 1.08e6-entry table every wave of the two working workgroups keeps 8192 records or more: two chunks to the brim --
    seven waves of sixteen stop exactly there, a full chunk is not rolled over before the next record comes -- and nine roll
    over into a third.  On the 1.13e6-entry table every wave keeps more than two chunks and rolls over twice."""
    E, K, st, _ = exact_filter(name, 23, "ones", monkeypatch, one_bit=one_bit)
    sizes = lo.bucket_sizes(E[:, 0], 23)
    for size in sizes.tolist():
        w = wave_shares(size)
        if name == "d1080k":
            assert min(w) == 2 * LIMITS["F_CH"] and sum(x > 2 * LIMITS["F_CH"] for x in w) == 9
        else:
            assert min(w) > 2 * LIMITS["F_CH"]
    assert len(K) == len(E) == (270612 if name == "d1080k" else 283826)
    # default grid, ~1000 owners: the whole list is less than a batch per owner; test_one_or_two_owners has the batches


def test_a_wave_takes_its_open_chunk_from_bucket_to_bucket(monkeypatch):
    """fb = 32, one id in four: 1024 buckets of ~100 records, ~25 of them kept in each, for at most one workgroup per CU -- a
    workgroup takes several buckets that keep records, and a wave that kept some writes on into the chunk it opened in an
    earlier bucket (its queue is drained at the end of every bucket: what is carried over is the chunk and its fill)"""
    E, K, st, _ = exact_filter("d405k", 32, "one_in_four", monkeypatch, one_bit=True)
    keep = lo.keep(E[:, 0], 32, False, lo.formula("one_in_four", 32, False))
    with_kept = np.count_nonzero(np.bincount(lo.bucket_of(E[keep, 0], 10), minlength=1024))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert with_kept == 1024 > 2 * cus >= 2
    # every wave of a workgroup strides through each of its buckets from the bucket's start: wave 0 keeps records in all of them
    per_bucket = np.bincount(lo.bucket_of(E[:, 0], 10), minlength=1024)
    assert per_bucket.min() >= 1 and 0.2 * len(E) < len(K) < 0.3 * len(E)


def test_a_map_of_zeros_keeps_nothing(monkeypatch):
    E, K, st, host = exact_filter("d405k", 23, "zero", monkeypatch)
    assert len(K) == 0 and (host == SENT).all()


@pytest.mark.parametrize("one_bit", [False, True], ids=["two_bit", "one_bit"])
def test_first_and_last_id_of_every_slice(one_bit, monkeypatch):
    """fb = 25: only the two ids at the ends of each bucket's slice of the map are set, and the table sends 600 requests to
    each of the sixteen among 1.4e4 others: the first and the last word of the slice a workgroup folds into LDS"""
    E, K, st, _ = exact_filter("edges", 25, "slice_edges", monkeypatch, one_bit=one_bit)
    ids = lo.ids_of(K[:, 0], 25)
    span = 1 << 22
    assert sorted(set(ids.tolist())) == sorted(b * span + x for b in range(8) for x in (0, span - 1))
    assert 16 * 500 <= len(K) < len(E) - 10000


@pytest.mark.parametrize("grid,nown", [(1, 513), (2, 514), (61, 573), (None, None)])
def test_one_or_two_owners_hold_all_the_requests(grid, nown, monkeypatch):
    """SMG_P1_GRID: grid 1 -- one owner with 25 chunks, i.e. seven batches of kl_part, the last one partial; grid 2 -- two owners;
    grid 61 -- 573 owners, nine rows per slice of kl_tot / kl_woff: their eight-row unroll ends inside a slice"""
    E, K, st, _ = exact_filter("d405k", 23, "one_in_four", monkeypatch, grid=grid)
    if grid is None:
        assert st["p1_grid"] > 61 and st["nown"] == st["p1_grid"] + LIMITS["BF_MAXGRID"]
        return
    assert st["p1_grid"] == grid and st["nown"] == nown
    chunks_of_owner0 = (st["p1_chunks"] - 1) // st["nown"] + 1
    per_batch = LIMITS["PT_BATCH_RW1"] // LIMITS["F_CH"]
    if grid <= 2:
        assert chunks_of_owner0 >= 3 * per_batch and len(E) // grid > 3 * LIMITS["PT_BATCH_RW1"]
    else:
        rows = -(-st["nown"] // LIMITS["LW_SL"])
        assert rows == 9 and rows % LIMITS["LW_UNR"] == 1


@pytest.mark.parametrize("grid", [1, None])
def test_owners_of_the_exact_redo_hold_records(grid, monkeypatch):
    """long window blocks: most requests come from kf_bigfix, whose owners follow those of pass 1"""
    hooks(monkeypatch, P1_GRID=grid)
    e = bound("families")
    e.set_blockmap_bits(23)
    e.pass1("hash")
    nbig = e.stats()["nbig"]
    e.close()
    assert nbig > 5000
    E, K, st, _ = exact_filter("families", 23, "own", monkeypatch, grid=grid)
    assert st["nown"] == st["p1_grid"] + LIMITS["BF_MAXGRID"] and (grid is None or st["p1_grid"] == 1)
    # only the exact redo sends a request a second time: records that E holds twice were written by a kf_bigfix owner, thousands of
    # them, and they are in the kept list of a map of ones below, so kl_part read those owners' chunks
    uniq, mult = np.unique(E[:, 0], return_counts=True)
    assert len(uniq) == len(emitted_of("families")[0]) and int((mult == 2).sum()) > 1000
    exact_filter("families", 23, "ones", monkeypatch, grid=grid)
    exact_filter("families", 23, "one_in_four", monkeypatch, grid=grid)


# two-word records: a batch of kl_part is two chunks

_WIDE = {}


def wide_reference(name, monkeypatch):
    """E at the default grid, and the request count of a plain two-way run, once per table"""
    if name not in _WIDE:
        hooks(monkeypatch, TWO_WAY=1)
        k, words, cnt = table(name)
        plot = torch.zeros(engine.PLOT_CELLS, dtype=torch.int64, device=DEV)
        e = bound(name)
        st = e.run(plot.data_ptr(), "hash")
        assert st["path"] == 1
        hooks(monkeypatch)
        e.set_blockmap_bits(30)
        e.pass1("hash")
        E, _ = routed(e, e.nreq())
        e.close()
        assert len(E) == st["nemitted"]
        E.setflags(write=False)
        _WIDE[name] = E
    return _WIDE[name]


@pytest.mark.parametrize("name,fb,mapkind,grid", [("wide51", 23, "own", 1), ("wide51", 30, "ones", None), ("wide51", 23, "ones", None),
                                                  ("wide51", 30, "own", 1), ("wide64", 23, "ones", 1), ("wide64", 30, "own", None),
                                                  ("wide64", 23, "own", None), ("wide64", 30, "ones", 1)])
def test_two_word_records(name, fb, mapkind, grid, monkeypatch):
    E_ref = wide_reference(name, monkeypatch)
    E, K, st, _ = exact_filter(name, fb, mapkind, monkeypatch, grid=grid, E_ref=E_ref)
    assert st["rw"] == 2
    if grid == 1:
        assert st["nown"] == 513 and len(E) > 3 * LIMITS["PT_BATCH_RW2"]
        assert (st["p1_chunks"] - 1) // st["nown"] + 1 >= 3 * (LIMITS["PT_BATCH_RW2"] // LIMITS["F_CH"])
    if mapkind == "ones":
        assert len(K) == len(E)
    sizes = lo.bucket_sizes(E[:, 0], fb)
    if fb == 23:
        assert sizes.min() > 2 * LIMITS["PB_TRIP"]


# ---- B. fused forms -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def expected_smu(tmp_path_factory):
    """the C oracle's .smu of a k = 31 table, computed once per table"""
    done = {}

    def get(name):
        if name not in done:
            k, words, cnt = table(name)
            d = tmp_path_factory.mktemp(name)
            synth.write_u64_table(str(d / "t"), words[:, 0], cnt, k)
            subprocess.run([ORACLE_BIN, f"-o{d}/orc", str(d / "t")], check=True)
            done[name] = (d / "orc.smu").read_text()
        return done[name]
    return get


_GENERAL = {}


def general_plot(name):
    """two-word k-mers: the engine's general path, which shares no look-up code"""
    if name not in _GENERAL:
        plot = torch.zeros(engine.PLOT_CELLS, dtype=torch.int64, device=DEV)
        e = bound(name)
        st = e.run(plot.data_ptr(), "none")
        torch.cuda.synchronize()
        assert st["path"] == 2
        e.close()
        _GENERAL[name] = plot.cpu().numpy().reshape(engine.PLOT_ROWS, engine.PLOT_COLS)
    return _GENERAL[name]


_PHASE_E = {}


def phase_emitted(name, monkeypatch):
    """the two-way request list of a table through the phase API (checked against the oracle by the tests of part A)"""
    if name not in _PHASE_E:
        hooks(monkeypatch)
        e = bound(name)
        e.set_blockmap_bits(30)
        e.pass1("hash")
        E, _ = routed(e, e.nreq())
        e.close()
        if table(name)[0] <= 32:
            check_emitted(name, E)
        _PHASE_E[name] = E
    return _PHASE_E[name]


PROBES = [dict(PROBE_X=0), dict(PROBE_X=1), dict(PROBE_X=1, PX_ONE_XCC=1)]
#         fb, one-bit map, two-way forced, pass-1 grid
GROUPS = [(23, False, True, None), (23, True, False, 1), (25, False, True, None), (25, True, False, None),
          (32, False, False, None), (32, True, True, 1), (32, False, True, None)]


def fused_group(name, fb, one_bit, two_way, grid, want_plot, monkeypatch):
    k, words, cnt = table(name)
    n = len(cnt)
    E = phase_emitted(name, monkeypatch)
    nb = lo.lookup_geo(fb)[1]
    seen = []
    for probe in PROBES:
        hooks(monkeypatch, BM_BITS=fb, ONE_BIT_MAP=1 if one_bit else None, TWO_WAY=1 if two_way else None, P1_GRID=grid, **probe)
        plot = torch.zeros(engine.PLOT_CELLS, dtype=torch.int64, device=DEV)
        e = bound(name)
        st = e.run(plot.data_ptr(), "hash")
        torch.cuda.synchronize()
        ls = e.lookup_state()
        got = plot.cpu().numpy().reshape(engine.PLOT_ROWS, engine.PLOT_COLS)
        assert st["path"] == 1, (probe, st)
        if isinstance(want_plot, str):
            assert engine.smu_text(got) == want_plot, (name, fb, probe)
        else:
            assert np.array_equal(got, want_plot), (name, fb, probe)
        one_way = int((k & 1) and not two_way)
        assert (ls["fb"], ls["nb"], ls["bm2"], ls["one_way"]) == (fb, nb, int(not one_bit), one_way), ls
        assert grid is None or (ls["p1_grid"], ls["nown"]) == (grid, grid + LIMITS["BF_MAXGRID"])
        if probe["PROBE_X"] and nb >= 3:
            part = LIMITS["PX_PART"] if st["nemitted"] * 100 > n * (14 if one_way else 28) else 2 * LIMITS["PX_PART"]
            assert (ls["probe"], ls["ticket"]) == (2, part), ls
        else:
            assert (ls["probe"], ls["ticket"]) == (1, 0), ls             # kl_probe_x needs eight buckets
        if not one_way:
            assert st["nemitted"] == len(E)
            two = not one_bit
            keep = lo.keep(E[:, 0], fb, two, lo.DeviceWords(own_map(e)))
            assert st["nrequests"] == int(keep.sum()), (probe, st["nrequests"], int(keep.sum()))
        else:
            assert 0 < st["nemitted"] < len(E)
            if k <= 31:
                # the one-way list and its filter, restated: exact where no entry can be redone, else between the list with every
                # redone sender's flag clear and that list plus a second copy of those senders with the flag set
                rec, send = one_way_of(name)
                again = lo.may_send_twice(words[:, 0], k)[send]
                m = lo.DeviceWords(own_map(e))
                sure = lo.keep_one_way(np.where(again, rec & ~U(1), rec), fb, not one_bit, m)
                most = lo.keep_one_way(rec | again.astype(U), fb, not one_bit, m)
                lo_n, hi_n = int(sure.sum()), int(most.sum()) + int(most[again].sum())
                assert len(rec) <= st["nemitted"] <= len(rec) + int(again.sum()), (probe, st["nemitted"], len(rec))
                assert lo_n <= st["nrequests"] <= hi_n, (probe, st["nrequests"], lo_n, hi_n)
                if not again.any():
                    assert st["nemitted"] == len(rec) and st["nrequests"] == lo_n == hi_n
        seen.append((st["nemitted"], st["nrequests"]))
        e.close()
    print(f"{name} fb={fb} one_bit={one_bit} two_way={two_way} grid={grid}: (emitted, kept) per probe form {seen}")
    assert seen[0] == seen[1] == seen[2], "the kept count is a function of table and map, not of the kernel"
    return E, seen


@pytest.mark.parametrize("fb,one_bit,two_way,grid", GROUPS)
@pytest.mark.parametrize("name", ["d405k", "clustered", "families"])
def test_fused_forms_at_k_31(name, fb, one_bit, two_way, grid, expected_smu, monkeypatch):
    """kl_probe, kl_probe_x and kl_probe_x on one XCC id against the C oracle's plot.  d405k at fb = 25: three to seven tickets per
    bucket, the last one partial; at fb = 32 128 buckets per XCD class (two rounds of the ticket scan); clustered at fb = 32:
    every ticket belongs to the classes 0 and 7, a workgroup of another class steals from the start, and with one XCC id all of
    class 7 is stolen; families: most requests come from the owners of the exact redo."""
    E, seen = fused_group(name, fb, one_bit, two_way, grid, expected_smu(name), monkeypatch)
    sizes = lo.bucket_sizes(E[:, 0], fb)
    if name == "d405k" and fb == 25:
        for part in (LIMITS["PX_PART"], 2 * LIMITS["PX_PART"]):
            t = lo.tickets(sizes, part)
            assert 3 < t.min() and t.max() <= 7 and (sizes % part != 0).all()
    if name == "clustered" and fb == 32:
        assert {b % 8 for b in np.flatnonzero(sizes).tolist()} == {0, 7}
        assert lo.tickets(sizes, 2 * LIMITS["PX_PART"])[[0, 1023]].min() > 10


@pytest.mark.parametrize("fb,one_bit,two_way,grid", [GROUPS[0], GROUPS[3], GROUPS[4], GROUPS[5]])
@pytest.mark.parametrize("name", ["wide51", "wide64"])
def test_fused_forms_with_two_word_records(name, fb, one_bit, two_way, grid, monkeypatch):
    """the expected plot is the engine's general path (symcheck none)"""
    if table(name)[0] % 2 == 0:
        two_way = True                                                   # (even k: there is no one-way protocol)
    fused_group(name, fb, one_bit, two_way, grid, general_plot(name), monkeypatch)
