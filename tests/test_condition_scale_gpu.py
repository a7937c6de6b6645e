"""Table conditioning (trim at -e, close under reverse complement) where its sorts and grids change regime, and on the inputs
that the small conditioning tests of test_gpu_parity.py cannot see: against the numpy oracle of tests/condition_oracle.py
(held to ktab.symmetrize and to fake_engine.NumpyEngine by tests/test_condition_oracle_host.py), ENTRY FOR ENTRY -- k-mers and
counts of the table the engine holds afterwards (Engine.table_host), not only the plot it gives.  Every case asserts, from the
oracle's numbers, that it reached the regime it is there for.

Size thresholds the assertions rely on, and where each comes from (retune one, move the assertion named with it):
  ONE_SWEEP = 2^20    rocPRIM's default radix_sort_config (rocprim/device/device_radix_sort.hpp): one block sorts up to 1024
                      items, a merge sort up to merge_sort_limit = 1024 * 1024, the one-sweep radix sort above.
                      sort_permutation (smg_keysort.hpp) sorts 2 x kept items (entries and complements) once per key word.
  HIST_GRID = 2048 * 256   smg_engine_symm_hist launches kc_symm_hist with at most 2048 workgroups of TPB = 256: its grid-stride
                      loop takes a second trip above that many entries.
  F_CH = 4096         records per chunk of route_records (smg_fast.hpp): smg_engine_symm_route presents its 2 n records as
                      ceil(2 n / F_CH) chunks, the last one partly filled.

The inputs (condition_oracle.raw_table) hold what random k-mers do not: families that share their first / last 32 j bases for
every j < W, so that adjacent entries of the closed table tie in words 0 .. j-1 and the passes over the low words and the
comparison of all W words decide; and, for even k, self-complementary k-mers, which the closed table holds twice before
de-duplication -- among them the smallest and the largest one, at its two ends.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import condition_oracle as co
from conftest import ORACLE_BIN, REF_BIN, ROOT
from smudgeplot_amd import engine, ktab
from test_gpu_parity import table_from

pytestmark = pytest.mark.gpu

ONE_SWEEP = 1 << 20
HIST_GRID = 2048 * 256
F_CH = 4096
L = 6
N_RAW = 700_000
CONDITION_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_condition")
BOTH = engine.COND_TRIM | engine.COND_SYMM


# (the caches hold what the next few tests share, not every key width's 7e5 x k bases for the whole session)
@functools.lru_cache(maxsize=3)
def raw(k, n=N_RAW):
    """(bases, counts): one raw table per key width"""
    return co.raw_table(k, n, 1000 + k, L=L)


@functools.lru_cache(maxsize=4)
def want(k, trim=True, symm=True, n=N_RAW):
    return co.condition(*raw(k, n), k, L, trim=trim, symm=symm)


def kept_of(k, n=N_RAW):
    return int((raw(k, n)[1] >= L).sum())


def on_device(keys, counts):
    import torch
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64).reshape(-1).copy()).to(dev)
    tc = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint16).view(np.int16).copy()).to(dev)
    return tk, tc


def conditioned(k, bases, counts, trim, symm, ethresh=L):
    """Engine.bind on torch tensors, condition, table_host"""
    import torch
    tk, tc = on_device(co.words_of(bases, k), counts)
    e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
    try:
        e.bind(k, len(counts), tk.data_ptr(), tc.data_ptr())
        n = e.condition(ethresh, trim, symm)
        keys, cnt = e.table_host()
        assert n == len(cnt) == e.table()[0]
        return keys, cnt
    finally:
        e.close()


def same_table(got, exp):
    assert got[0].shape == exp[0].shape and got[1].shape == exp[1].shape, (got[0].shape, exp[0].shape)
    bad = np.flatnonzero((got[0] != exp[0]).any(axis=1) | (got[1] != exp[1]))
    assert len(bad) == 0, f"{len(bad)} of {len(exp[1])} entries differ, the first at {bad[:5]}"


# ---- a. one engine, every key width -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 32, 33, 64, 65, 96, 97, 128])
def test_one_engine_every_key_width(k):
    bases, counts = raw(k)
    exp = want(k)
    kept = kept_of(k)
    assert 2 * kept > ONE_SWEEP and len(counts) > ONE_SWEEP // 2         # one-sweep regime of every word pass; trim above 2^19
    if k % 2 == 0:
        assert 2 * kept - len(exp[1]) > 100                              # duplicates dropped: flag == 0 of kc_flag_first / kc_compact
    else:
        assert 2 * kept == len(exp[1])
    ties = co.leading_ties(exp[0])
    assert len(ties) == co.nwords(k) - 1 and all(t > 0 for t in ties)    # words 1..W-1 decide the order, every one of them
    same_table(conditioned(k, bases, counts, True, True), exp)


@pytest.mark.parametrize("k", [64, 97])
def test_trim_only_and_symmetrise_only(k):
    bases, counts = raw(k)
    keep = counts >= L
    assert int(keep.sum()) > HIST_GRID
    same_table(conditioned(k, bases, counts, True, False), want(k, True, False))
    same_table(conditioned(k, bases[keep], counts[keep], False, True), want(k))
    same_table(conditioned(k, bases, counts, True, False, ethresh=40000), (np.zeros((0, co.nwords(k)), np.uint64), np.zeros(0, np.uint16)))


# ---- b. around the sort's other boundaries ----------------------------------------------------------------------------

def truncated(k, kept):
    """the head of raw(k) that holds `kept` entries at or above L"""
    bases, counts = raw(k)
    n = int(np.searchsorted(np.cumsum(counts >= L), kept)) + 1
    assert int((counts[:n] >= L).sum()) == kept
    return bases[:n], counts[:n]


@pytest.mark.parametrize("k", [31, 32, 33, 64, 65, 96, 97, 128])
def test_around_one_block_of_the_sort(k):
    """2 x kept is even: Engine.condition sorts 1022, 1024 and 1026 items, and smg_engine_symm_finish is handed the first 1023,
    1024 and 1025 records of the 1026 (entries, then complements) -- one block of rocPRIM's sort against its merge sort"""
    import torch
    W = co.nwords(k)
    for kept in (511, 512, 513):
        bases, counts = truncated(k, kept)
        same_table(conditioned(k, bases, counts, True, True), co.condition(bases, counts, k, L))
    keep = counts >= L
    tb, tcnt = bases[keep], counts[keep]
    rec = np.zeros((2 * kept, W + 1), dtype=np.uint64)
    rec[:, :W] = co.words_of(np.concatenate([tb, co.revcomp(tb)]), k)
    rec[:kept, W] = tcnt
    rec[kept:, W] = tcnt.astype(np.uint64) | np.uint64(1 << 16)
    for nrecv in (1023, 1024, 1025):
        # what is left of the closed table: all entries, the complements of the first nrecv - 513
        part = np.concatenate([tb, co.revcomp(tb[: nrecv - kept])])
        keys = co.words_of(part, k)
        o = co.order_of(keys)
        first = np.ones(nrecv, dtype=bool)
        first[1:] = (keys[o][1:] != keys[o][:-1]).any(axis=1)
        exp = keys[o][first], np.concatenate([tcnt, tcnt[: nrecv - kept]])[o][first]
        buf = torch.from_numpy(rec[:nrecv].view(np.int64).reshape(-1).copy()).to("cuda:0")
        tk, tc = on_device(co.words_of(tb[:1], k), tcnt[:1])
        e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
        try:
            e.bind(k, 1, tk.data_ptr(), tc.data_ptr())
            assert e.symm_finish(buf.data_ptr(), nrecv) == len(exp[1])
            same_table(e.table_host(), exp)
        finally:
            e.close()


@pytest.mark.parametrize("n2", [ONE_SWEEP - 2, ONE_SWEEP, ONE_SWEEP + 2])
def test_around_the_merge_sort_limit(n2):
    k = 64
    bases, counts = truncated(k, n2 // 2)
    exp = co.condition(bases, counts, k, L)
    assert 2 * int((counts >= L).sum()) == n2 and n2 - len(exp[1]) > 0 and co.leading_ties(exp[0])[0] > 0
    same_table(conditioned(k, bases, counts, True, True), exp)


# ---- c. the sharded primitives, one rank, at size ---------------------------------------------------------------------

def leading_bits(bases, bits):
    nb = (bits + 1) // 2
    v = np.zeros(len(bases), dtype=np.int64)
    for i in range(nb):
        v = (v << 2) | bases[:, i]
    return v >> (2 * nb - bits)


@pytest.mark.parametrize("k", [31, 64, 100])
def test_sharded_primitives_one_rank(k):
    import torch
    from smudgeplot_amd import sharded
    bases, counts = raw(k)
    keep = counts >= L
    tk, tc = on_device(co.words_of(bases, k), counts)
    eng = sharded.TorchEngine(torch.device("cuda:0"))
    eng.bind(k, tk, tc)
    n = eng.trim(L)
    assert n == int(keep.sum()) > HIST_GRID                              # a second trip of kc_symm_hist's grid-stride loop
    assert (2 * n) % F_CH != 0 and 2 * n > 256 * F_CH                    # many route chunks, the last one partly filled
    driver_bits = max(2, min(12, 2 * (k // 2)))                          # (sharded.condition_sharded)
    for bits in sorted({12, driver_bits, 7}):
        h = eng.symm_hist(bits)
        own = np.bincount(leading_bits(bases[keep], bits), minlength=1 << bits)
        rcs = np.bincount(leading_bits(co.revcomp(bases[keep]), bits), minlength=1 << bits)
        assert np.array_equal(h[: 1 << bits], own) and np.array_equal(h[1 << bits:], rcs), bits
    eng2, split = sharded.condition_sharded(k, tk, tc, ethresh=L, trim=True, symm=True)
    assert len(split) == 0 and 2 * n > ONE_SWEEP                         # nrecv of symm_finish
    assert eng2.nels() == len(want(k)[1])
    same_table(eng2.e.table_host(), want(k))


# ---- d. two shards by hand, at size -----------------------------------------------------------------------------------

def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def test_two_shards_by_hand():
    """two engines, the exchange by hand, every shard's sort in the one-sweep regime.  The receive order differs between the
    destinations, but on canonical input that cannot decide a count: the only k-mers that arrive twice are self-complementary,
    and their entry and complement come from one source with one count.  The count-choosing branch of kc_compact_pref is
    test_both_strands_with_different_counts' to check (complements_first), not this test's."""
    import torch
    from smudgeplot_amd import sharded
    k, n, W = 64, 1_500_000, 2
    bases, counts = co.raw_table(k, n, 1000 + k, L=L)                    # (not cached: nobody else needs it)
    exp = co.condition(bases, counts, k, L)
    dev = torch.device("cuda:0")
    cut = n // 2 + 12_345
    engs, kept_of_shard = [], []
    for lo, hi in ((0, cut), (cut, n)):
        tk, tc = on_device(co.words_of(bases[lo:hi], k), counts[lo:hi])
        en = sharded.TorchEngine(dev)
        en.bind(k, tk, tc)
        kept_of_shard.append(en.trim(L))
        engs.append(en)
    assert kept_of_shard == [int((counts[:cut] >= L).sum()), int((counts[cut:] >= L).sum())]
    bits = 12
    hist = engs[0].symm_hist(bits) + engs[1].symm_hist(bits)
    split = sharded.symm_splitters(hist, bits, 2, W)
    assert split.shape == (W,) and split[0] != 0 and split[1] == 0
    sends, sent = [], []
    for en, m in zip(engs, kept_of_shard):
        buf = torch.empty(2 * m * (W + 1), dtype=torch.int64, device=dev)
        sent.append(en.symm_route(split, 2, buf))
        sends.append(buf)
    # the records a shard sends: per destination the multiset of (k-mer, count | is-a-complement << 16) the oracle expects
    for src, (lo, hi) in enumerate(((0, cut), (cut, n))):
        keep = counts[lo:hi] >= L
        b, c = bases[lo:hi][keep], counts[lo:hi][keep].astype(np.uint64)
        rec = np.zeros((2 * len(c), W + 1), dtype=np.uint64)
        rec[:, :W] = co.words_of(np.concatenate([b, co.revcomp(b)]), k)
        rec[:, W] = np.concatenate([c, c | np.uint64(1 << 16)])
        dest = rec[:, 0] >= split[0]                                      # (the splitter's other words are 0)
        got = sends[src].cpu().numpy().view(np.uint64).reshape(-1, W + 1)
        assert sent[src] == [int((~dest).sum()), int(dest.sum())]
        assert np.array_equal(sorted_rows(got[: sent[src][0]]), sorted_rows(rec[~dest]))
        assert np.array_equal(sorted_rows(got[sent[src][0]:]), sorted_rows(rec[dest]))
    nrecv = [sent[0][d] + sent[1][d] for d in range(2)]
    assert min(nrecv) > ONE_SWEEP
    tables = []
    for dst, order in ((0, (1, 0)), (1, (0, 1))):                         # destination 0 receives source 1's records in front
        parts = []
        for src in order:
            off = sum(sent[src][:dst]) * (W + 1)
            parts.append(sends[src][off: off + sent[src][dst] * (W + 1)])
        recv = torch.cat(parts)
        engs[dst].symm_finish(recv, nrecv[dst])
        tables.append(engs[dst].e.table_host())
    assert len(tables[0][1]) > 0 and len(tables[1][1]) > 0
    assert tables[0][0][-1, 0] < split[0] <= tables[1][0][0, 0]          # the halves meet at the splitter
    same_table((np.concatenate([t[0] for t in tables]), np.concatenate([t[1] for t in tables])), exp)


# ---- e. the drivers, at size ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_smu(k):
    """the C oracle's .smu of the numpy-conditioned table, once per k; where the reference binary was built it must write
    the same bytes"""
    import tempfile
    keys, cnt = want(k)
    with tempfile.TemporaryDirectory() as d:
        ktab.write_ktab(os.path.join(d, "cond"), k, co.packed_of(keys, k), cnt, ibyte=3, nparts=1, minval=L)
        subprocess.run([ORACLE_BIN, f"-e{L}", f"-o{d}/orc", os.path.join(d, "cond")], check=True)
        smu = open(os.path.join(d, "orc.smu")).read()
        if os.path.exists(REF_BIN):
            q = subprocess.run([REF_BIN, f"-e{L}", "-T4", "-oref", "cond"], cwd=d, capture_output=True, text=True)
            assert q.returncode == 0, q.stderr
            assert open(os.path.join(d, "ref.smu")).read() == smu
        return smu


@pytest.mark.parametrize("env", [{"SMG_VIRTUAL_SHARDS": "3"}, {"SMG_SEQUENTIAL_SHARDS": "3"}, {}], ids=["virtual3", "sequential3", "one"])
@pytest.mark.parametrize("k", [64, 31])
def test_drivers_condition_a_raw_table(k, env, monkeypatch):
    """hetmers_run on the raw table through the virtual shards of host_run_multi, the out-of-core shards of
    host_condition_sequential and one engine: plot and entry count against the C oracle (and the reference binary) on the
    numpy-conditioned table.  Only the single engine sorts above 2^20 items here; each of three shards sorts about a third of the
    closed table, the merge-sort side, on W-word k-mers with ties in the leading words."""
    bases, counts = raw(k)
    smu = oracle_smu(k)
    assert sum(int(line.split()[2]) for line in smu.splitlines()) >= 1000
    if env:
        assert 1024 < 2 * kept_of(k) // 3 < ONE_SWEEP // 2               # a shard's share, balanced or not far from it
    else:
        assert 2 * kept_of(k) > ONE_SWEEP
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    table = table_from(ktab.pack_bases(bases), counts, k)
    plot, st = engine.hetmers_run(table, symcheck="hash", condition=BOTH, ethresh=L)
    assert st["path"] == 1 and st["nels"] == len(want(k)[1])
    assert engine.smu_text(plot) == smu


# ---- f. the smg_condition executable, at size -------------------------------------------------------------------------

def test_condition_executable(tmp_path):
    k = 64
    bases, counts = raw(k)
    keys, cnt = want(k)
    ktab.write_ktab(str(tmp_path / "raw"), k, ktab.pack_bases(bases), counts, ibyte=2, nparts=3)
    r = subprocess.run([CONDITION_BIN, f"-e{L}", "raw.ktab", "cond"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = ktab.read_ktab(str(tmp_path / "cond"))
    assert t.k == k and t.ibyte == 2 and t.nparts == 3
    assert 2 * kept_of(k) > ONE_SWEEP
    assert np.array_equal(t.packed, co.packed_of(keys, k)) and np.array_equal(t.counts, cnt)


# ---- g. the documented rule for input that is neither canonical nor closed --------------------------------------------

@pytest.mark.parametrize("k", [32, 65])
def test_both_strands_with_different_counts(k):
    """smg_condition.hpp, "table conditioning on device" and "symmetrising a table that is cut into prefix shards": every input
    entry keeps its own count, and a complement is added (with its entry's count) only where the table does not hold it"""
    import torch
    from smudgeplot_amd import sharded
    rng = np.random.default_rng(k)
    x = rng.integers(0, 4, size=(3000, k), dtype=np.uint8)
    if k % 2 == 0:
        x[:50, k // 2:] = 3 - x[:50, : k // 2][:, ::-1]                   # self-complementary ones
    rows = {bytes(r): int(c) for r, c in zip(x, rng.integers(1, 200, size=len(x)))}
    for r in x[100:1100]:                                                 # both strands in the input, with counts of their own
        rows.setdefault(bytes(3 - r[::-1]), int(rng.integers(200, 400)))
    table = sorted(rows.items())
    expect = dict(rows)
    added = 0
    for r, c in table:
        rc = bytes(3 - np.frombuffer(r, np.uint8)[::-1])
        if rc not in rows:
            expect[rc] = c
            added += 1
    assert added >= 1900 and len(rows) >= 3990 and len(expect) == len(rows) + added
    both = sum(1 for r, c in table if rows.get(bytes(3 - np.frombuffer(r, np.uint8)[::-1]), c) != c)
    assert both >= 1990                                                   # entries whose complement is an entry with another count
    bases = np.array([np.frombuffer(r, np.uint8) for r, _ in table])
    counts = np.array([c for _, c in table], dtype=np.uint16)
    exp_rows = sorted(expect.items())
    exp = (co.words_of(np.array([np.frombuffer(r, np.uint8) for r, _ in exp_rows]), k), np.array([c for _, c in exp_rows], dtype=np.uint16))
    same_table(conditioned(k, bases, counts, False, True), exp)
    W, n = co.nwords(k), len(counts)
    tk, tc = on_device(co.words_of(bases, k), counts)
    for complements_first in (False, True):
        eng = sharded.TorchEngine(torch.device("cuda:0"))
        eng.bind(k, tk, tc)
        send = torch.empty(2 * n * (W + 1), dtype=torch.int64, device="cuda:0")
        assert eng.symm_route(np.zeros(0, np.uint64), 1, send) == [2 * n]
        rec = send.view(2 * n, W + 1)
        is_copy = (rec[:, W] >> 16) == 1
        assert int(is_copy.sum()) == n
        if complements_first:
            send = torch.cat([rec[is_copy], rec[~is_copy]]).reshape(-1).contiguous()
        assert eng.symm_finish(send, 2 * n) == len(exp[1])
        same_table(eng.e.table_host(), exp)
