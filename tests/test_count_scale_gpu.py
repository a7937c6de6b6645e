"""The k-mer counter where its sorts, scans and store change regime: inputs of 10^6 .. 10^7 windows against the numpy oracle of
tests/count_oracle.py (held to the Python oracle by tests/test_count_oracle_host.py), entry for entry: k-mers, counts,
histogram, distinct, kept, windows.  The small inputs of test_count_gpu.py / test_count_parts_gpu.py test the edges; these
test what only size reaches.  Every case asserts, from the oracle's numbers and the returned stats, that it reached the
regime it is there for, so that a change of a generator cannot quietly turn it back into a small test.

Size thresholds the assertions rely on, and where each comes from (retune one, move the assertion named with it):
  ONE_SWEEP = 2^20   rocPRIM's default radix_sort_config (rocprim/device/device_radix_sort.hpp): one block sorts up to 1024
                     items, a merge sort up to merge_sort_limit = 1024 * 1024, the one-sweep radix sort above.  Cases a, b, c
                     put more than 2^20 items into the key sort, into every word pass of the k > 32 sort (ks_iota,
                     ks_gather_word, stable pair sorts, kc_gather_entries) and into the (k-mer, count) pair sort of merge().
  KC_TILE = 4096     positions per workgroup of the extract kernels (smg_count.hip); GRID = 2048 is the most workgroups
                     kc_bins (one tile each per trip) and kc_finish_flag (256 entries each per trip) are launched with, so
                     their grid-stride loops take a second trip above 2048 * 4096 store positions and 2048 * 256 distinct
                     k-mers.
  RING_BLOCK = 8 MiB the pinned blocks count_files() hands from the reader threads to Counter::add() (smg_count.hip): a file
                     with more sequence than that arrives in several blocks, which alternate with another reader's (case e).
  store slack        Counter::init sizes the packed store of a partitioned run as bound + bound / 32 + 65 536 positions rounded
                     up to KC_TILE; a batch adds a separator, k - 1 re-prefixed bytes and padding to 64 positions, so many small
                     batches outgrow it and need_store() reallocates and copies (case d).
  SMG_COUNT_BATCH_BASES  the test hook of Counter::batch_cap: a batch (and the key buffer of a range) holds that many + k.

All inputs are seeded and generated here: reads of a random genome at 30x, both strands, 0.5 % substitutions, a base replaced
by N with probability 5e-4; 150 bases for k <= 32 and 400 above (150-base reads give too few windows at k = 128).
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import count_oracle
from conftest import HETMERS_BIN, ORACLE_BIN, REF_BIN, ROOT
from smudgeplot_amd import count, ktab
from test_count_gpu import check, fastq_text
from test_count_parts_gpu import same

pytestmark = pytest.mark.gpu

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
ONE_SWEEP = 1 << 20
KC_TILE, GRID, KC_TPB = 4096, 2048, 256
RING_BLOCK = 8 << 20
_TEXT = np.frombuffer(b"ACGTN", np.uint8)

# name -> (seed, reads, read length).  At k = 128 three batches of the 16 000-read input would hold too little above 2^20
# windows each, so k = 128 takes 24 000 reads in every case.
READ_SETS = {"short": (101, 70_000, 150), "long": (102, 16_000, 400), "long128": (103, 24_000, 400), "grow": (104, 3_750, 400),
             "pair": (105, 114_000, 150)}


def input_of(k):
    return "short" if k <= 32 else "long128" if k == 128 else "long"


def sample_reads(rng, genomes, n_each, L, err=0.005, p_n=5e-4):
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


@functools.lru_cache(maxsize=None)
def reads(which):
    """-> base codes [n, L] uint8, 4 = N"""
    seed, n, L = READ_SETS[which]
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, n * L // 30).astype(np.uint8)
    return sample_reads(rng, [genome], n, L)


@functools.lru_cache(maxsize=None)
def stream(which):
    """the reads as the byte stream count_bases takes: one '\\n' behind every read"""
    R = reads(which)
    return np.concatenate([_TEXT[R], np.full((len(R), 1), ord("\n"), np.uint8)], axis=1).reshape(-1)


@functools.lru_cache(maxsize=None)
def oracle(k, which):
    """one oracle run per (k, input): (keys, unclamped counts, windows)"""
    return count_oracle.kmer_counts(reads(which), k)


def want_of(k, which, t):
    keys, counts, _ = oracle(k, which)
    return count_oracle.table(keys, counts, k, t)


def check_all(got, k, which, t):
    """check() of test_count_gpu.py (k-mers, counts, histogram, distinct, kept) plus windows"""
    check(got, want_of(k, which, t), k, t)
    keys, _, windows = oracle(k, which)
    assert got[2]["windows"] == windows and got[2]["distinct"] == len(keys)


@functools.lru_cache(maxsize=None)
def one_pass(k, t):
    """case a's run: one pass, the natural batch"""
    got = count.count_bases(stream(input_of(k)), k, t=t, partitions=1)
    assert got[2]["used"] == 1 and got[2]["store_bytes"] == 0
    return got


# ---- a. one pass, one batch, every key width ------------------------------------------------------------------------

@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("k", [31, 32, 33, 64, 65, 97, 128])
def test_one_pass_one_batch(k, t):
    got = one_pass(k, t)
    check_all(got, k, input_of(k), t)
    st = got[2]
    assert st["batches"] == 1                          # no merge: the table is what one sort and one reduction give
    assert st["windows"] > ONE_SWEEP                   # one-sweep regime of radix_sort_keys (k <= 32) / of each of the W word passes
    assert st["distinct"] > GRID * KC_TPB              # second trip of kc_finish_flag's grid-stride loop
    assert st["bases"] == len(stream(input_of(k)))


# ---- b. one pass, several large batches -----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 65, 128])
def test_one_pass_three_large_batches(k, monkeypatch):
    which, t = input_of(k), 1
    full = one_pass(k, t)
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", str(int(0.4 * len(stream(which)))))
    got = count.count_bases(stream(which), k, t=t, partitions=1)
    check_all(got, k, which, t)
    same(got, full)
    st = got[2]
    assert st["batches"] >= 3
    assert st["windows"] / st["batches"] > ONE_SWEEP   # every batch's key sort / word passes: one-sweep regime
    # merge() sorts the concatenation of the running list and a batch's list as (k-mer, uint32 count) pairs; the last one holds
    # at least the final distinct k-mers: the pair sort (k <= 32) / the word passes with kc_gather_entries' values (k > 32)
    # run above 2^20 entries
    assert st["distinct"] > ONE_SWEEP


# ---- c. key ranges at scale -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts", [3, 64])
@pytest.mark.parametrize("k", [31, 65, 128])
def test_ranges_with_the_natural_batch(k, parts):
    which, t = input_of(k), 3
    got = count.count_bases(stream(which), k, t=t, partitions=parts)
    check_all(got, k, which, t)
    same(got, one_pass(k, t))
    st = got[2]
    assert st["used"] == parts
    assert st["windows"] / parts > (ONE_SWEEP if parts == 3 else 1024)     # a range's sort: one-sweep (3) / merge-sort regime (64)
    if k == 31:
        # second trip of kc_bins' grid-stride loop: the store holds every byte of the stream, more than 2048 tiles of them
        assert len(stream(which)) > (GRID + 1) * KC_TILE and st["store_bytes"] * 8 // 3 > (GRID + 1) * KC_TILE


@pytest.mark.parametrize("k", [31, 65, 128])
def test_ranges_extracted_in_spans_of_many_tiles(k, monkeypatch):
    """a key buffer of 300 000 + k keys, several times smaller than a range: run_ranges() reads the store in spans of `room`
    positions (~70 tiles) that start and end off a tile boundary, sorts the buffer when it is nearly full (cap / 8) and the
    range's lists merge"""
    which, t, hook = input_of(k), 1, 300_000
    assert (hook + k) % KC_TILE != 0 and (hook + k) // KC_TILE > 60
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", str(hook))
    got = count.count_bases(stream(which), k, t=t, partitions=3)
    check_all(got, k, which, t)
    same(got, one_pass(k, t))
    st = got[2]
    assert st["used"] == 3
    assert st["batches"] >= -(-st["windows"] // (hook + k))               # a sorted batch holds at most hook + k keys
    assert st["batches"] > 2 * st["used"]                                 # so ranges sorted more than twice: they merged


@pytest.mark.parametrize("k", [31, 65, 128])
def test_automatic_ranges_of_one_sorted_batch(k, monkeypatch):
    which, t = input_of(k), 3
    full = one_pass(k, t)
    limit = full[2]["distinct"] // 3
    with pytest.raises(count.CountError) as e:
        count.count_bases(stream(which), k, t=t, partitions=1, max_entries=limit)
    assert e.value.code == -3 and "do not fit" in str(e.value)
    got = count.count_bases(stream(which), k, t=t, partitions=0, max_entries=limit)
    check_all(got, k, which, t)
    same(got, full)
    st = got[2]
    assert st["used"] > 3 and st["store_bytes"] > 0 and st["batches"] == st["used"]       # windows > distinct: more than 3 ranges
    assert st["windows"] / st["used"] > 1024                              # a range's sort: beyond one block
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", "300000")                 # a batch below the limit: ranges of at most a batch
    assert 300_000 + k < limit
    many = count.count_bases(stream(which), k, t=t, max_entries=limit)
    check_all(many, k, which, t)
    same(many, got)
    assert many[2]["used"] >= -(-st["windows"] // (300_000 + k)) > st["used"] and many[2]["batches"] == many[2]["used"]


# ---- d. the store grows ---------------------------------------------------------------------------------------------

def test_the_packed_store_is_reallocated_and_copied(monkeypatch):
    which, k, t, hook = "grow", 65, 1, 704
    seq = stream(which)
    n, cap = len(seq), hook + k
    # The first allocation: n + n / 32 + 65 536 positions, rounded up to a tile (Counter::init, bound = n for count_bases).
    # A batch holds cap = hook + k bytes: a separator and the k - 1 re-prefixed bytes in front (only the separator in the
    # first), so all batches after the first take `hook` bytes of the stream; every full batch occupies cap rounded up to 64
    # positions of the store.  The full batches alone outgrow the first allocation:
    first = -(-(n + n // 32 + 65536) // KC_TILE) * KC_TILE
    full_batches = (n - (cap - 1)) // hook
    assert full_batches * (-(-cap // 64) * 64) > first + first // 20
    one = count.count_bases(seq, k, t=t, partitions=1)
    check_all(one, k, which, t)
    assert one[2]["windows"] > ONE_SWEEP
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", str(hook))
    got = count.count_bases(seq, k, t=t, partitions=2)
    check_all(got, k, which, t)
    same(got, one)
    assert got[2]["used"] == 2
    assert got[2]["store_bytes"] > first * 3 // 8                          # need_store() reallocated (and the table says it copied)
    assert got[2]["store_bytes"] * 8 // 3 >= full_batches * (-(-cap // 64) * 64)


# ---- e. files larger than a ring block, alternating -----------------------------------------------------------------

def _digits(n, width=7):
    return ((np.arange(n)[:, None] // 10 ** np.arange(width - 1, -1, -1)) % 10 + ord("0")).astype(np.uint8)


def fasta_bytes(text, width=60):
    """[n, L] sequence bytes -> FASTA with numbered headers and lines of `width` columns"""
    n, L = text.shape
    cols = [np.full((n, 2), ord(">"), np.uint8), _digits(n), np.full((n, 1), ord("\n"), np.uint8)]
    cols[0][:, 1] = ord("s")
    for a in range(0, L, width):
        cols += [text[:, a:a + width], np.full((n, 1), ord("\n"), np.uint8)]
    return np.concatenate(cols, axis=1).tobytes()


def fastq_crlf_bytes(text):
    """[n, L] sequence bytes -> FASTQ with CRLF line ends; quality lines may begin with '@' or '>'"""
    n, L = text.shape
    crlf = np.tile(np.frombuffer(b"\r\n", np.uint8), (n, 1))
    head = np.tile(np.frombuffer(b"@r", np.uint8), (n, 1))
    plus = np.tile(np.frombuffer(b"+", np.uint8), (n, 1))
    qual = np.frombuffer(b"@>I#", np.uint8)[(np.arange(n)[:, None] + np.arange(L)[None, :]) % 4]
    return np.concatenate([head, _digits(n), crlf, text, crlf, plus, crlf, qual, crlf], axis=1).tobytes()


def test_files_larger_than_a_ring_block(tmp_path):
    which, k, t = "pair", 31, 2
    R = reads(which)
    text = _TEXT[R]
    text[::5] |= 0x20                                                     # every fifth read in lower case (N -> n: no base either)
    half = len(R) // 2
    (tmp_path / "a.fa").write_bytes(fasta_bytes(text[:half]))
    (tmp_path / "b.fq").write_bytes(fastq_crlf_bytes(text[half:]))
    # each file's sequence is more than one pinned block: two readers hand over blocks of the two files in turn
    assert text[:half].size > RING_BLOCK and text[half:].size > RING_BLOCK
    a, b = tmp_path / "a.fa", tmp_path / "b.fq"
    for path, rows in ((a, text[:half]), (b, text[half:])):              # the files hold these reads (host-only parser)
        assert count.parse(path) == b"\n".join(bytes(r) for r in rows)
    want = want_of(k, which, t)
    first = None
    for threads in (2, 1):
        for paths in ((a, b), (b, a)):
            for parts in (0, 4):
                got = count.count_files(paths, k, t=t, threads=threads, partitions=parts)
                check_all(got, k, which, t)
                assert got[2]["bases"] == text.size and got[2]["used"] == (parts if parts else 1)
                first = first or got
                same(got, first)
    assert first[2]["windows"] > ONE_SWEEP and first[2]["distinct"] > GRID * KC_TPB
    r = subprocess.run([COUNT_BIN, f"-k{k}", f"-t{t}", "-T2", "-H", "-v", "-oexe", "a.fa", "b.fq"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert f"  {text.size} bases, " in r.stderr
    packed, counts, hist = want
    ktab.write_ktab(str(tmp_path / "py"), k, packed, counts, ibyte=3, nparts=1, minval=t)
    assert (tmp_path / "exe.ktab").read_bytes() == (tmp_path / "py.ktab").read_bytes()
    assert (tmp_path / ".exe.ktab.1").read_bytes() == (tmp_path / ".py.ktab.1").read_bytes()
    top = int(np.nonzero(hist)[0].max())
    assert (tmp_path / "exe.hist.txt").read_text() == "".join(f"{c}\t{int(hist[c])}\n" for c in range(1, top + 1))


# ---- f. reads to .smu above one word --------------------------------------------------------------------------------

def test_reads_to_smu_end_to_end_k51(tmp_path):
    """the recipe of test_count_gpu.py::test_reads_to_smu_end_to_end at k = 51 (two words per key): 100 kb diploid genome, 1 %
    heterozygous SNPs, 400-base reads at ~20x per haplotype: smg_count -k51 -t1, then the drop-in hetmers -e6 on that raw
    table.  Expected .smu: the C oracle (and the reference binary where it was built) on the numpy oracle's table trimmed
    at 6 and closed under reverse complement."""
    rng = np.random.default_rng(12)
    G, k, L, cov, e = 100_000, 51, 400, 20, 6
    h1 = rng.integers(0, 4, G).astype(np.uint8)
    h2 = h1.copy()
    snp = rng.random(G) < 0.01
    h2[snp] = (h2[snp] + rng.integers(1, 4, snp.sum())) & 3
    R = sample_reads(rng, [h1, h2], G * cov // L, L)
    text = _TEXT[R]
    half = len(text) // 2
    (tmp_path / "reads_1.fq").write_bytes(fastq_text([bytes(r) for r in text[:half]]))
    (tmp_path / "reads_2.fq").write_bytes(fastq_text([bytes(r) for r in text[half:]]))

    r = subprocess.run([COUNT_BIN, f"-k{k}", "-t1", "-T8", "-H", "-oSample", "reads_1.fq", "reads_2.fq"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    keys, cnt, windows = count_oracle.kmer_counts(R, k)
    assert windows > ONE_SWEEP and len(keys) > 400_000
    packed, counts, hist = count_oracle.table(keys, cnt, k, 1)
    got = ktab.read_ktab(str(tmp_path / "Sample"))
    assert got.k == k and got.minval == 1 and np.array_equal(got.packed, packed) and np.array_equal(got.counts, counts)
    top = int(np.nonzero(hist)[0].max())
    assert [int(line.split()[1]) for line in open(tmp_path / "Sample.hist.txt")] == [int(x) for x in hist[1:top + 1]]

    r = subprocess.run([HETMERS_BIN, f"-e{e}", "-T8", "-v", "-oSample", "Sample.ktab"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "  The input table is untrimmed and not symmetric\n" in r.stderr
    keep = counts >= e
    cp, cc = ktab.symmetrize(packed[keep], counts[keep], k)
    ktab.write_ktab(str(tmp_path / "cond"), k, cp, cc, ibyte=3, nparts=1, minval=e)
    subprocess.run([ORACLE_BIN, f"-e{e}", f"-o{tmp_path}/orc", str(tmp_path / "cond")], check=True)
    smu = (tmp_path / "orc.smu").read_text()
    assert sum(int(line.split()[2]) for line in smu.splitlines()) >= 1000
    assert (tmp_path / "Sample.smu").read_text() == smu
    if os.path.exists(REF_BIN):
        q = subprocess.run([REF_BIN, f"-e{e}", "-T4", "-oref", "cond"], cwd=tmp_path, capture_output=True, text=True)
        assert q.returncode == 0, q.stderr
        assert (tmp_path / "ref.smu").read_text() == smu
