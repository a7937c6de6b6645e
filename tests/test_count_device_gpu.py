"""The counted table left in device memory (count_*_device), and reads to the het-mer plot in one process from there
(count.reads_to_plot, smg_hetmers_run_device, `smg_count -e`).

The device entries against the host entries on the same input -- k-mers, counts, histogram, distinct, kept -- in one pass, in
three ranges and in automatic ranges under a max_entries limit.  The fused route against brute.hetmers_plot (k = 21) and the C
oracle (k = 51) on the numpy oracle's table trimmed and closed, and against `smg_count` followed by `hetmers` byte for byte.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import brute
import count_oracle
from conftest import HETMERS_BIN, ORACLE_BIN, ROOT, load_golden
from smudgeplot_amd import count, engine, ktab

pytestmark = pytest.mark.gpu

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
_TEXT = np.frombuffer(b"ACGTN", np.uint8)


# ---- inputs ---------------------------------------------------------------------------------------------------------

def sample_reads(rng, genomes, n_each, L, err=0.005, p_n=0.0):
    """n_each reads of L bases from every genome: uniform starts, substitutions, Ns, half of them reverse-complemented"""
    out = []
    for g in genomes:
        st = rng.integers(0, len(g) - L, n_each)
        R = g[st[:, None] + np.arange(L)]
        m = rng.random(R.shape) < err
        R = np.where(m, (R + rng.integers(1, 4, R.shape)) & 3, R).astype(np.uint8)
        R[rng.random(R.shape) < p_n] = 4
        flip = rng.random(n_each) < 0.5
        R[flip] = np.where(R[flip] > 3, 4, 3 - np.minimum(R[flip], 3))[:, ::-1]
        out.append(R)
    return np.concatenate(out)


def stream_of(R):
    """reads as the byte stream count_bases takes: one newline behind every read"""
    return np.concatenate([_TEXT[R], np.full((len(R), 1), ord("\n"), np.uint8)], axis=1).reshape(-1)


def fastq_bytes(text):
    q = b"@>I#"
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(r), bytes([q[(i + j) % 4] for j in range(len(r))])) for i, r in enumerate(text))


@functools.lru_cache(maxsize=None)
def small_stream():
    """about 2e5 bases: 150-base reads of a 20 kb genome at 10x, both strands, with errors and Ns"""
    rng = np.random.default_rng(4242)
    genome = rng.integers(0, 4, 20_000).astype(np.uint8)
    return stream_of(sample_reads(rng, [genome], 1330, 150, p_n=5e-4))


@functools.lru_cache(maxsize=None)
def host_count(k, t):
    return count.count_bases(small_stream(), k, t=t, partitions=1)


def same_as_host(got, want, k, t):
    """a device result (DeviceTable, hist, stats) against a host result (KTable, hist, stats)"""
    table, hist, st = got
    wt, whist, wst = want
    with table:
        assert (table.k, table.t, table.nels, table.words) == (k, t, wt.nels, (k + 31) // 32)
        assert table.keys_ptr and table.counts_ptr                          # whole allocations, also when empty
        assert table.keys_ptr % 16 == 0 and table.counts_ptr % 8 == 0       # what smg_engine_bind asks for
        keys, counts = table.to_host()
    assert table.keys_ptr is None and table.counts_ptr is None
    assert np.array_equal(count.keys_to_packed(keys, k), wt.packed)
    assert np.array_equal(counts, wt.counts)
    assert np.array_equal(hist, whist)
    for f in ("bases", "windows", "distinct", "kept"):
        assert st[f] == wst[f], f


# ---- the table on the device ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["one_pass", "three_ranges", "automatic"])
@pytest.mark.parametrize("t", [1, 4])
@pytest.mark.parametrize("k", [21, 31, 33, 65])
def test_device_table_equals_host_table(k, t, mode):
    want = host_count(k, t)
    assert want[2]["distinct"] > 15_000 and 0 < want[2]["kept"] and (t == 1 or want[2]["kept"] < want[2]["distinct"])
    if mode == "one_pass":
        got = count.count_bases_device(small_stream(), k, t=t, partitions=1)
        assert got[2]["used"] == 1 and got[2]["store_bytes"] == 0
    elif mode == "three_ranges":
        got = count.count_bases_device(small_stream(), k, t=t, partitions=3)
        assert got[2]["used"] == 3 and got[2]["store_bytes"] > 0
    else:
        limit = want[2]["distinct"] // 3
        with pytest.raises(count.CountError) as e:
            count.count_bases_device(small_stream(), k, t=t, partitions=1, max_entries=limit)
        assert e.value.code == -3
        got = count.count_bases_device(small_stream(), k, t=t, partitions=0, max_entries=limit)
        assert got[2]["used"] > 1                                           # ranges appended to the device table, which grew
    same_as_host(got, want, k, t)


def test_device_table_from_files(tmp_path):
    rng = np.random.default_rng(77)
    genome = rng.integers(0, 4, 5000).astype(np.uint8)
    text = _TEXT[sample_reads(rng, [genome], 600, 150, p_n=1e-3)]
    (tmp_path / "a.fq").write_bytes(fastq_bytes(text[:300]))
    (tmp_path / "b.fq").write_bytes(fastq_bytes(text[300:]).replace(b"\n", b"\r\n"))
    paths = [tmp_path / "a.fq", tmp_path / "b.fq"]
    for k, t, parts in ((31, 4, 0), (65, 2, 3)):
        want = count.count_files(paths, k, t=t, threads=2, partitions=parts)
        got = count.count_files_device(paths, k, t=t, threads=2, partitions=parts)
        assert got[2]["used"] == want[2]["used"] == (parts or 1)
        same_as_host(got, want, k, t)


def test_input_without_any_window_gives_an_empty_device_table():
    seq = b"ACGTACGTAC\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\nACGTNACGTNACGTNACGTNACGT\n"
    for parts in (1, 3):
        table, hist, st = count.count_bases_device(seq, 21, t=1, partitions=parts)
        with table:
            assert table.nels == 0 and table.keys_ptr and table.counts_ptr
            keys, counts = table.to_host()
        assert keys.shape == (0, 1) and counts.shape == (0,)
        assert hist.sum() == 0 and st["windows"] == 0 and st["kept"] == 0


# ---- reads to plot --------------------------------------------------------------------------------------------------

def diploid_reads(seed, L):
    """100 kb diploid genome, 1 % heterozygous SNPs, reads of L bases of both strands at ~20x per haplotype with 0.5 %
    substitution errors (the read set of test_count_gpu.py::test_reads_to_smu_end_to_end and of its k = 51 repeat)"""
    rng = np.random.default_rng(seed)
    G, cov = 100_000, 20
    h1 = rng.integers(0, 4, G).astype(np.uint8)
    h2 = h1.copy()
    snp = rng.random(G) < 0.01
    h2[snp] = (h2[snp] + rng.integers(1, 4, snp.sum())) & 3
    return sample_reads(rng, [h1, h2], G * cov // L, L)


@functools.lru_cache(maxsize=None)
def closed_oracle_table(seed, L, k, e):
    """(packed, counts) of the numpy oracle's table of the read set, trimmed at e and closed; the oracle's histogram"""
    keys, cnt, _ = count_oracle.kmer_counts(diploid_reads(seed, L), k)
    packed, counts, hist = count_oracle.table(keys, cnt, k, 1)
    keep = counts >= e
    cp, cc = ktab.symmetrize(packed[keep], counts[keep], k)
    return cp, cc, hist


def test_reads_to_plot_k21():
    k, t, e = 21, 1, 6
    R = diploid_reads(11, 150)
    cp, cc, whist = closed_oracle_table(11, 150, k, e)
    want = brute.hetmers_plot(cp, cc, k)
    assert int(want.sum()) >= 1000
    plot, hist, st = count.reads_to_plot(stream_of(R), k, t, e)
    assert plot.shape == (engine.PLOT_ROWS, engine.PLOT_COLS) and plot.dtype == np.int64
    assert np.array_equal(plot, want)
    assert np.array_equal(hist, whist)
    assert st["hetmers"]["nels"] == len(cc) and st["hetmers"]["path"] == 1 and st["kept"] == int(whist.sum())
    # e = t: nothing to trim, the counted table is closed as it is
    cp4, cc4, _ = closed_oracle_table(11, 150, k, 4)
    plot4, _, st4 = count.reads_to_plot(stream_of(R), k, 4, 4, partitions=3)
    assert st4["used"] == 3 and st4["hetmers"]["nels"] == len(cc4)
    assert np.array_equal(plot4, brute.hetmers_plot(cp4, cc4, k))


def test_reads_to_plot_k51_from_files(tmp_path):
    k, t, e = 51, 1, 6
    text = _TEXT[diploid_reads(12, 400)]
    half = len(text) // 2
    (tmp_path / "reads_1.fq").write_bytes(fastq_bytes(text[:half]))
    (tmp_path / "reads_2.fq").write_bytes(fastq_bytes(text[half:]))
    cp, cc, whist = closed_oracle_table(12, 400, k, e)
    ktab.write_ktab(str(tmp_path / "cond"), k, cp, cc, ibyte=3, nparts=1, minval=e)
    subprocess.run([ORACLE_BIN, f"-e{e}", f"-o{tmp_path}/orc", str(tmp_path / "cond")], check=True)
    smu = (tmp_path / "orc.smu").read_text()
    assert sum(int(line.split()[2]) for line in smu.splitlines()) >= 1000
    plot, hist, st = count.reads_to_plot([tmp_path / "reads_1.fq", tmp_path / "reads_2.fq"], k, t, e, threads=2)
    assert engine.smu_text(plot) == smu
    assert np.array_equal(hist, whist) and st["hetmers"]["nels"] == len(cc) and st["hetmers"]["key_words"] == 2


# ---- the executable -------------------------------------------------------------------------------------------------

def test_smg_count_e_writes_what_smg_count_and_hetmers_write(tmp_path):
    k, e = 21, 6
    text = _TEXT[diploid_reads(11, 150)]
    half = len(text) // 2
    (tmp_path / "reads_1.fq").write_bytes(fastq_bytes(text[:half]))
    (tmp_path / "reads_2.fq").write_bytes(fastq_bytes(text[half:]))
    inputs = ["reads_1.fq", "reads_2.fq"]

    def run(binary, *args):
        r = subprocess.run([binary, *args], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r

    run(COUNT_BIN, f"-k{k}", "-t1", "-H", "-oTwo", *inputs)
    run(HETMERS_BIN, f"-e{e}", "-T4", "-oTwo", "Two.ktab")
    smu = (tmp_path / "Two.smu").read_bytes()
    assert len(smu.splitlines()) > 20

    before = set(os.listdir(tmp_path))
    r = run(COUNT_BIN, f"-k{k}", "-t1", f"-e{e}", "-n", "-v", "-oSample", *inputs)
    assert "het-mers at -e6" in r.stderr
    assert set(os.listdir(tmp_path)) - before == {"Sample.smu"}              # no Sample.ktab, no hidden part, no histogram
    assert (tmp_path / "Sample.smu").read_bytes() == smu

    run(COUNT_BIN, f"-k{k}", "-t1", f"-e{e}", "-H", "-oBoth", *inputs)    # without -n: the table of a run without -e as well
    assert (tmp_path / "Both.ktab").read_bytes() == (tmp_path / "Two.ktab").read_bytes()
    assert (tmp_path / ".Both.ktab.1").read_bytes() == (tmp_path / ".Two.ktab.1").read_bytes()
    assert (tmp_path / "Both.hist.txt").read_bytes() == (tmp_path / "Two.hist.txt").read_bytes()
    assert (tmp_path / "Both.smu").read_bytes() == smu

    before = set(os.listdir(tmp_path))
    run(COUNT_BIN, f"-k{k}", "-t1", "-n", "-H", "-oHist", *inputs)          # -n with -H alone: the histogram and nothing else
    assert set(os.listdir(tmp_path)) - before == {"Hist.hist.txt"}
    assert (tmp_path / "Hist.hist.txt").read_bytes() == (tmp_path / "Two.hist.txt").read_bytes()

    # a run that fails behind the counting leaves nothing: the engine is told that nothing fits (SMG_HBM_LIMIT, its test hook)
    before = set(os.listdir(tmp_path))
    r = subprocess.run([COUNT_BIN, f"-k{k}", "-t1", f"-e{e}", "-H", "-oFail", *inputs], cwd=tmp_path, capture_output=True, text=True,
                       env=dict(os.environ, SMG_HBM_LIMIT="1000"))
    assert r.returncode == 1 and "does not fit the device in core" in r.stderr and "hetmers" in r.stderr, r.stderr
    assert set(os.listdir(tmp_path)) == before


# ---- smg_hetmers_run_device on a table that is not canonical ----------------------------------------------------------

def words_of_packed(packed, k):
    W = (k + 31) // 32
    pad = np.zeros((len(packed), 8 * W), dtype=np.uint8)
    pad[:, : packed.shape[1]] = packed
    return np.ascontiguousarray(pad).view(">u8").astype(np.uint64).reshape(len(packed), W)


@pytest.mark.parametrize("name", ["k31_i1", "k64_i1", "k65_i1", "k100_i1"])
def test_run_device_on_a_closed_table_takes_the_generic_closure(name):
    """a golden table is closed under reverse complement, so half of its entries are larger than their complement: asked to
    close it, the entry finds it not canonical (smg_engine_close_canonical refuses and changes nothing) and falls back to
    the generic closure, which leaves a closed table as it is.  This is the test of that branch; a build with
    RUN_DEVICE_CLOSE_BY_MERGE 0 (smg_hetmers.hip) takes the generic closure at once and passes it as well"""
    import torch
    g = load_golden(name)
    k, n = g["k"], len(g["counts"])
    keys = words_of_packed(g["packed"], k)
    tk = torch.from_numpy(keys.view(np.int64).reshape(-1).copy()).to("cuda:0")
    tc = torch.from_numpy(np.ascontiguousarray(g["counts"], dtype=np.uint16).view(np.int16).copy()).to("cuda:0")
    for cond in (engine.COND_SYMM, engine.COND_SYMM | engine.COND_TRIM, 0):
        plot, st = engine.hetmers_run_device(k, n, tk.data_ptr(), tc.data_ptr(), condition=cond, ethresh=g["L"])
        assert engine.smu_text(plot) == g["smu"], cond
        assert st["nels"] == n and st["path"] == 1
    assert np.array_equal(tk.cpu().numpy().view(np.uint64).reshape(n, -1), keys)      # the borrowed table is as it was
    with pytest.raises(engine.EngineError) as e:
        lib = engine.load_library()
        import ctypes as C
        opts = engine.Opts(0, engine.SYM_HASH, 0, 0, 0, 2)
        buf = C.create_string_buffer(512)
        out = np.zeros(engine.PLOT_CELLS, dtype=np.int64)
        engine._check(lib.smg_hetmers_run_device(k, n, tk.data_ptr(), tc.data_ptr(), C.byref(opts), out.ctypes.data, None, buf, 512), buf)
    assert e.value.code == -2 and "ngpus" in str(e.value)
