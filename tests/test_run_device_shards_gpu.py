"""A table on the device beyond one engine, or beyond the memory: the closure of a canonical table one key range at a time
(smg_engine_close_canonical_range) and the run in prefix shards of the closed table one after the other that
smg_hetmers_run_device takes where it refused (count.reads_to_plot, `smg_count -e`).

The range closure against ktab.symmetrize entry for entry: the key space cut into 2, 3 and 5 ranges at boundaries of the
leading 12 bits, and the ranges that can go wrong by themselves -- no entry at all, no entry of the table but complements,
self-complementary k-mers only, one entry below, at and above a tile of the merge, too little room for the complements.
The run in shards (SMG_DEVICE_SHARDS, SMG_DEVICE_SHARD_LIMIT: the plan's test hooks) against the same call without hooks
and against the oracles, and the executable byte for byte against itself in core.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import brute
import count_oracle
from conftest import ORACLE_BIN, ROOT, load_golden
from smudgeplot_amd import count, engine, ktab

pytestmark = pytest.mark.gpu

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
_TEXT = np.frombuffer(b"ACGTN", np.uint8)
TRIM, SYMM = engine.COND_TRIM, engine.COND_SYMM
HOOKS = ("SMG_DEVICE_SHARDS", "SMG_DEVICE_SHARD_LIMIT", "SMG_HBM_LIMIT")


# ---- inputs (the generator style of test_count_device_gpu.py) ---------------------------------------------------------------

def sample_reads(rng, genomes, n_each, L, err=0.005):
    """n_each reads of L bases from every genome: uniform starts, substitutions, half of them reverse-complemented"""
    out = []
    for g in genomes:
        st = rng.integers(0, len(g) - L, n_each)
        R = g[st[:, None] + np.arange(L)]
        m = rng.random(R.shape) < err
        R = np.where(m, (R + rng.integers(1, 4, R.shape)) & 3, R).astype(np.uint8)
        flip = rng.random(n_each) < 0.5
        R[flip] = (3 - R[flip])[:, ::-1]
        out.append(R)
    return np.concatenate(out)


def stream_of(R):
    return np.concatenate([_TEXT[R], np.full((len(R), 1), ord("\n"), np.uint8)], axis=1).reshape(-1)


def fastq_bytes(text):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(r), b"I" * len(r)) for i, r in enumerate(text))


def words_of_packed(packed, k):
    W = (k + 31) // 32
    pad = np.zeros((len(packed), 8 * W), dtype=np.uint8)
    pad[:, : packed.shape[1]] = packed
    return np.ascontiguousarray(pad).view(">u8").astype(np.uint64).reshape(len(packed), W)


PALINDROMES = 3            # reverse-palindromic 22-mers that the k = 22 read set carries


@functools.lru_cache(maxsize=None)
def palindromes():
    """s + rc(s) for three 11-mers s: 22-mers that are their own reverse complement"""
    rng = np.random.default_rng(22)
    s = rng.integers(0, 4, (PALINDROMES, 11)).astype(np.uint8)
    return np.concatenate([s, (3 - s)[:, ::-1]], axis=1)


@functools.lru_cache(maxsize=None)
def small_reads(k):
    """about 2e5 bases: 150-base reads of a 20 kb genome at 10x, both strands, with errors; k = 22: and one read around each
    of the palindromes"""
    rng = np.random.default_rng(4242)
    genome = rng.integers(0, 4, 20_000).astype(np.uint8)
    R = sample_reads(rng, [genome], 1330, 150)
    if k == 22:
        extra = rng.integers(0, 4, (PALINDROMES, 150)).astype(np.uint8)
        extra[:, 60:82] = palindromes()
        R = np.concatenate([R, extra])
    return R


@functools.lru_cache(maxsize=None)
def closed_oracle(k):
    """the counted table of small_reads(k) as the numpy oracle counts it, (words [n, W], counts), and its closure by
    ktab.symmetrize in the same form"""
    keys, cnt, _ = count_oracle.kmer_counts(small_reads(k), k)
    packed, counts, _ = count_oracle.table(keys, cnt, k, 1)
    cp, cc = ktab.symmetrize(packed, counts, k)
    for a in (keys, counts, cp, cc):
        a.setflags(write=False)
    return words_of_packed(packed, k), counts, words_of_packed(cp, k), np.asarray(cc, dtype=np.uint16)


class Counted:
    """the counted table of small_reads(k) on the device, one engine to close ranges of it in, and the oracle beside it"""

    def __init__(self, k):
        self.k, self.W = k, (k + 31) // 32
        self.table, _, _ = count.count_bases_device(stream_of(small_reads(k)), k, t=1, partitions=1)
        self.cw, self.cc, self.tw, self.tc = closed_oracle(k)
        assert self.table.nels == len(self.cc) > 15_000
        self.e = engine.Engine(0)

    def shard(self, lo, hi, capacity=None):
        t = self.table
        n = self.e.close_canonical_range(self.k, t.nels, t.keys_ptr, t.counts_ptr, lo, hi, capacity)
        keys, counts = self.e.table_host()
        assert keys.shape == (n, self.W) and counts.shape == (n,)
        return keys, counts

    def oracle(self, lo, hi):
        """the entries of the oracle's closed table in [lo, hi)"""
        t = [tuple(int(x) for x in row) for row in self.tw]
        sel = np.array([(lo is None or tuple(int(x) for x in lo) <= x) and (hi is None or x < tuple(int(x) for x in hi)) for x in t], dtype=bool)
        return self.tw[sel], self.tc[sel]

    def close(self):
        self.e.close()
        self.table.close()


@pytest.fixture(scope="module", params=[21, 22, 31, 33, 65, 100])
def counted(request):
    c = Counted(request.param)
    yield c
    c.close()


def bin_key(b, W):
    """the first k-mer of bin b of the leading 12 bits"""
    key = np.zeros(W, dtype=np.uint64)
    key[0] = np.uint64(b) << np.uint64(52)
    return key


def above(key):
    """the smallest key above a k-mer whose last word has pad bits (k no multiple of 32): no k-mer lies between"""
    up = np.array(key, dtype=np.uint64)
    up[-1] += np.uint64(1)
    return up


# ---- the range closure ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", [2, 3, 5])
def test_ranges_that_tile_the_key_space_give_the_closed_table(counted, q):
    c = counted
    cuts = [None] + [bin_key(int(c.tw[len(c.tw) * i // q, 0] >> np.uint64(52)), c.W) for i in range(1, q)] + [None]
    keys, counts, sizes = [], [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sk, sc = c.shard(lo, hi)
        keys.append(sk); counts.append(sc); sizes.append(len(sc))
    assert min(sizes) > 0 and sum(sizes) == len(c.tc)
    assert np.array_equal(np.concatenate(keys), c.tw)
    assert np.array_equal(np.concatenate(counts), c.tc)


def test_the_borrowed_table_is_not_changed_and_open_ends_give_everything(counted):
    c = counted
    keys, counts = c.shard(None, None)
    assert np.array_equal(keys, c.tw) and np.array_equal(counts, c.tc)
    e2 = engine.Engine(0)
    e2.bind(c.k, c.table.nels, c.table.keys_ptr, c.table.counts_ptr)
    hk, hc = e2.table_host()
    e2.close()
    assert np.array_equal(hk, c.cw) and np.array_equal(hc, c.cc)


def test_a_range_with_no_entry_at_all(counted):
    c = counted
    i = len(c.tw) // 2
    keys, counts = c.shard(above(c.tw[i]), c.tw[i + 1])           # between two neighbours of the closed table
    assert len(counts) == 0
    keys, counts = c.shard(c.tw[i], c.tw[i])                      # an empty range
    assert len(counts) == 0
    keys, counts = c.shard(c.tw[i + 1], c.tw[i])                  # ... and one that ends in front of its start
    assert len(counts) == 0


def test_a_range_above_the_table_holds_complements_only(counted):
    c = counted
    lo = above(c.cw[-1])                                          # behind the last canonical entry: a canonical table crowds the low end
    wk, wc = c.oracle(lo, None)
    assert len(wc) > 0
    keys, counts = c.shard(lo, None)
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc)


def test_a_range_that_no_complement_falls_into_is_a_copy_of_the_slice(counted):
    c = counted
    inv = {tuple(int(x) for x in row) for row in c.cw}
    own = np.array([tuple(int(x) for x in row) in inv for row in c.tw], dtype=bool)
    run = next(i for i in range(len(own) - 3) if own[i:i + 3].all())      # three entries of the table next to each other in its closure
    keys, counts = c.shard(c.tw[run], above(c.tw[run + 2]))
    assert np.array_equal(keys, c.tw[run:run + 3]) and np.array_equal(counts, c.tc[run:run + 3])


def test_a_range_of_self_complementary_kmers_only():
    c = Counted(22)
    try:
        pal = count_oracle.window_keys(palindromes(), 22)[0].reshape(PALINDROMES, 1).astype(np.uint64)
        for p in pal:
            at = int(np.searchsorted(c.tw[:, 0], p[0]))
            assert c.tw[at, 0] == p[0]                              # in the table, and once in its closure
            keys, counts = c.shard(p, above(p))
            assert np.array_equal(keys, c.tw[at:at + 1]) and np.array_equal(counts, c.tc[at:at + 1])
            keys, counts = c.shard(c.tw[at - 1], above(c.tw[at + 1]))      # ... and with a neighbour on either side
            assert np.array_equal(keys, c.tw[at - 1:at + 2]) and np.array_equal(counts, c.tc[at - 1:at + 2])
        assert len(c.tc) == 2 * len(c.cc) - PALINDROMES
    finally:
        c.close()


@pytest.mark.parametrize("k", [31, 65])
def test_shards_of_one_tile_of_the_merge_less_and_more(k):
    c = Counted(k)
    try:
        T = engine.merge_tile(c.W)
        assert T > 0 and len(c.tc) > 3 * T + 1000
        for first in (0, 777):
            for size in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
                keys, counts = c.shard(c.tw[first] if first else None, c.tw[first + size])
                assert np.array_equal(keys, c.tw[first:first + size]), (first, size)
                assert np.array_equal(counts, c.tc[first:first + size]), (first, size)
    finally:
        c.close()


@pytest.mark.parametrize("k", [31, 65])
def test_too_little_room_for_the_complements_is_an_error(k):
    """through smg_engine_close_canonical_range_cap, the door the shard driver uses: room for exactly the complements of the
    range is enough, one less is an error that names both figures and leaves the engine's table as it was.  That nothing is
    written behind the room is the kernel's bound check (slot < cap); no test can see the bytes behind a device buffer"""
    c = Counted(k)
    try:
        lo, hi = c.tw[len(c.tw) // 4], c.tw[3 * len(c.tw) // 4]
        wk, wc = c.oracle(lo, hi)
        inv = {tuple(int(x) for x in row) for row in c.cw}
        m = sum(tuple(int(x) for x in row) not in inv for row in wk)           # the complements among them
        assert 0 < m < len(wc)
        keys, counts = c.shard(lo, hi, capacity=m)
        assert np.array_equal(keys, wk) and np.array_equal(counts, wc)
        before = c.e.table()
        with pytest.raises(engine.EngineError) as err:
            c.shard(lo, hi, capacity=m - 1)
        assert err.value.code == -2 and f"room was made for {m - 1}" in str(err.value) and str(m) in str(err.value)
        assert c.e.table() == before                                            # the engine's table is the shard of before
        keys, counts = c.e.table_host()
        assert np.array_equal(keys, wk) and np.array_equal(counts, wc)
    finally:
        c.close()


def test_a_closed_table_is_refused_as_not_canonical():
    import torch
    g = load_golden("k31_i1")
    k, n = g["k"], len(g["counts"])
    keys = words_of_packed(g["packed"], k)
    tk = torch.from_numpy(keys.view(np.int64).reshape(-1).copy()).to("cuda:0")
    tc = torch.from_numpy(np.ascontiguousarray(g["counts"], dtype=np.uint16).view(np.int16).copy()).to("cuda:0")
    e = engine.Engine(0)
    e.bind(k, n, tk.data_ptr(), tc.data_ptr())
    before = e.table()
    for lo, hi in ((None, None), (None, bin_key(2048, 1)), (bin_key(5, 1), bin_key(5, 1))):
        with pytest.raises(engine.EngineError) as err:
            e.close_canonical_range(k, n, tk.data_ptr(), tc.data_ptr(), lo, hi)
        assert err.value.code == -2 and "table is not canonical" in str(err.value)
        assert e.table() == before
    hk, hc = e.table_host()
    assert np.array_equal(hk, keys) and np.array_equal(hc, g["counts"])
    e.close()


# ---- reads to plot in shards ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def diploid_reads(L):
    """about 2e5 bases: a 10 kb diploid genome, 1 % heterozygous SNPs, reads of L bases of both strands at 10x per haplotype
    with 0.2 % substitution errors"""
    rng = np.random.default_rng(31 + L)
    G, cov = 10_000, 10
    h1 = rng.integers(0, 4, G).astype(np.uint8)
    h2 = h1.copy()
    snp = rng.random(G) < 0.01
    h2[snp] = (h2[snp] + rng.integers(1, 4, snp.sum())) & 3
    return sample_reads(rng, [h1, h2], G * cov // L, L, err=0.002)


@functools.lru_cache(maxsize=None)
def oracle_plot(k, L, e, tmp):
    """(closed entries, plot of the oracle) of the numpy oracle's table of the read set trimmed at e and closed:
    brute.hetmers_plot at k = 21, the C oracle (its .smu text) above"""
    keys, cnt, _ = count_oracle.kmer_counts(diploid_reads(L), k)
    packed, counts, _ = count_oracle.table(keys, cnt, k, 1)
    keep = counts >= e
    cp, cc = ktab.symmetrize(packed[keep], counts[keep], k)
    if k == 21:
        return len(cc), engine.smu_text(brute.hetmers_plot(cp, cc, k))
    ktab.write_ktab(os.path.join(tmp, f"cond{k}_{e}"), k, cp, cc, ibyte=3, nparts=1, minval=e)
    subprocess.run([ORACLE_BIN, f"-e{e}", f"-o{tmp}/orc{k}_{e}", os.path.join(tmp, f"cond{k}_{e}")], check=True)
    return len(cc), open(os.path.join(tmp, f"orc{k}_{e}.smu")).read()


def set_hooks(monkeypatch, **env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv("SMG_" + name, str(val))


@pytest.mark.parametrize("hook", ["shards2", "shards3", "shards5", "limit"])
@pytest.mark.parametrize("k,L", [(21, 150), (51, 250), (100, 400)])
def test_reads_to_plot_in_shards(monkeypatch, tmp_path_factory, k, L, hook):
    tmp = str(tmp_path_factory.getbasetemp())
    stream = stream_of(diploid_reads(L))
    for t, e in ((1, 6), (4, 4)):                                   # e > t: the table is trimmed first; e = t: nothing to trim
        nclosed, smu = oracle_plot(k, L, e, tmp)
        assert sum(int(line.split()[2]) for line in smu.splitlines()) >= 20
        for proof in ("hash", "exact"):
            set_hooks(monkeypatch)
            plain, hist, st = count.reads_to_plot(stream, k, t, e, symcheck=proof)
            n = st["kept"]
            assert engine.run_device_mode(k, n, 2.5e11, proof, TRIM | SYMM)["mode"] == "core"
            if hook == "limit":
                set_hooks(monkeypatch, DEVICE_SHARD_LIMIT=2 * n - 1)          # just below the 2 n that the closure is planned with
                want = {"mode": "sequential", "count": 2, "cut_by_limit": 2}
            else:
                set_hooks(monkeypatch, DEVICE_SHARDS=int(hook[-1]))
                want = {"mode": "sequential", "count": int(hook[-1]), "cut_by_limit": 0}
            assert engine.run_device_mode(k, n, 2.5e11, proof, TRIM | SYMM) == want
            plot, hist2, st2 = count.reads_to_plot(stream, k, t, e, symcheck=proof)
            assert np.array_equal(plot, plain) and np.array_equal(hist2, hist), (t, e, proof)
            assert engine.smu_text(plot) == smu, (t, e, proof)
            assert st2["hetmers"]["nels"] == nclosed == st["hetmers"]["nels"] and st2["hetmers"]["path"] == 1
            assert st2["hetmers"]["key_words"] == (k + 31) // 32


def test_the_run_says_how_many_shards_it_takes(monkeypatch, capfd):
    k, t, e = 21, 1, 6
    table, _, st = count.count_bases_device(stream_of(diploid_reads(150)), k, t=t, partitions=1)
    with table:
        set_hooks(monkeypatch, DEVICE_SHARDS=3)
        capfd.readouterr()
        plot, est = engine.hetmers_run_device(k, table.nels, table.keys_ptr, table.counts_ptr, verbose=1, condition=TRIM | SYMM, ethresh=e)
        err = capfd.readouterr().err
        assert "3 prefix shards one after the other" in err, err
        set_hooks(monkeypatch)
        plain, pst = engine.hetmers_run_device(k, table.nels, table.keys_ptr, table.counts_ptr, verbose=1, condition=TRIM | SYMM, ethresh=e)
        assert "prefix shards" not in capfd.readouterr().err
    assert np.array_equal(plot, plain) and est["nels"] == pst["nels"] and int(plot.sum()) > 0


# ---- the executable ---------------------------------------------------------------------------------------------------------

def test_smg_count_e_in_shards_writes_the_same_smu(monkeypatch, tmp_path):
    k, e = 21, 6
    text = _TEXT[diploid_reads(150)]
    half = len(text) // 2
    (tmp_path / "reads_1.fq").write_bytes(fastq_bytes(text[:half]))
    (tmp_path / "reads_2.fq").write_bytes(fastq_bytes(text[half:]))
    base = {name: val for name, val in os.environ.items() if name not in HOOKS}

    def run(out, **env):
        r = subprocess.run([COUNT_BIN, f"-k{k}", "-t1", f"-e{e}", "-n", "-v", f"-o{out}", "reads_1.fq", "reads_2.fq"], cwd=tmp_path,
                           capture_output=True, text=True, env=dict(base, **env))
        assert r.returncode == 0, r.stderr
        return r.stderr, (tmp_path / f"{out}.smu").read_bytes()

    err, smu = run("Core")
    assert "het-mers at -e6" in err and "prefix shards" not in err and len(smu.splitlines()) > 20
    err3, smu3 = run("Three", SMG_DEVICE_SHARDS="3")
    assert smu3 == smu
    assert "in 3 prefix shards one after the other" in err3 and "; 3 prefix shards one after the other" in err3, err3

    # a memory limit under which in core does not fit and some number of shards does, found through the plan
    n = int(next(line for line in err.splitlines() if "with count >= 1" in line).split("distinct, ")[1].split()[0])
    found = None
    for bits in range(12, 31):
        set_hooks(monkeypatch, HBM_LIMIT=1 << bits)
        try:
            m = engine.run_device_mode(k, n, 1.0, "hash", TRIM | SYMM)
        except engine.EngineError as refusal:
            assert refusal.code == -3 and "does not fit the device in core" in str(refusal)
            continue
        found = (1 << bits, m)
        break
    set_hooks(monkeypatch)
    assert found and found[1]["mode"] == "sequential" and 2 <= found[1]["count"] <= 16 and found[1]["cut_by_limit"] == 0
    errm, smum = run("Limit", SMG_HBM_LIMIT=str(found[0]))
    assert smum == smu
    assert f"in {found[1]['count']} prefix shards one after the other" in errm, errm


@pytest.mark.parametrize("name", ["k31_i1", "k65_i1"])
def test_a_closed_table_ignores_the_hook_and_runs_in_core(monkeypatch, name):
    """a golden table is closed, hence not canonical: the shards are not for it, the generic closure runs in core as ever"""
    import torch
    g = load_golden(name)
    k, n = g["k"], len(g["counts"])
    keys = words_of_packed(g["packed"], k)
    tk = torch.from_numpy(keys.view(np.int64).reshape(-1).copy()).to("cuda:0")
    tc = torch.from_numpy(np.ascontiguousarray(g["counts"], dtype=np.uint16).view(np.int16).copy()).to("cuda:0")
    set_hooks(monkeypatch, DEVICE_SHARDS=2)
    plot, st = engine.hetmers_run_device(k, n, tk.data_ptr(), tc.data_ptr(), condition=SYMM)
    assert engine.smu_text(plot) == g["smu"]
    assert st["nels"] == n and st["path"] == 1
