"""Key-range partitioned counting on the GPU: every number of ranges gives what one pass gives and what the Python oracle of
tests/test_count_gpu.py gives (k-mers, counts, histogram, distinct, kept, windows), also when the batches are a few k-mers
long, from files in either order, and where one pass is refused because its merge would not hold the distinct k-mers."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from smudgeplot_amd import count, ktab
from test_count_gpu import _COMP, check, fastq_text, oracle_counts, oracle_table, random_reads

pytestmark = pytest.mark.gpu

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
KS = [13, 21, 31, 32, 33, 51, 64, 65, 100, 128]
PARTS = [1, 2, 3, 7, 64, 4096]
_RC = bytes.maketrans(b"ACGT", b"TGCA")


@functools.lru_cache(maxsize=None)
def reads_of(k):
    """seeded reads of a 700-base genome, both strands, some lower case, with Ns and stretches shorter than k; for even k
    also sequence whose k-mers are their own reverse complement"""
    rng = np.random.default_rng(7000 + k)
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 700))
    reads = []
    for _ in range(70):
        a = int(rng.integers(0, 700 - 160))
        r = genome[a:a + int(rng.integers(k, 160 + 1))]
        if rng.random() < 0.5:
            r = r.translate(_RC)[::-1]
        if rng.random() < 0.3:
            r = r.lower()
        reads.append(r)
    reads += random_reads(rng, 12, 1, 300, b"ACGTN")
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads.append(b"N".join(bytes(rng.choice(acgt, n)) for n in (k - 1, k, k + 1, k - 1, 1, 2 * k)))
    reads += [b"A" * (k + 40), b"T" * (k + 3), b"tttttt" + genome[:k], genome[-k:] + b"AAAAAA"]
    if k % 2 == 0:
        reads += [b"ACGT" * (k // 2 + 5), b"AT" * (k + 7), b"GATC" * (k // 2 + 3)]
    return b"\n".join(reads)


@functools.lru_cache(maxsize=None)
def want_of(k, t):
    return oracle_table([reads_of(k)], k, t)


@functools.lru_cache(maxsize=None)
def one_pass(k, t):
    got = count.count_bases(reads_of(k), k, t=t, partitions=1)
    assert got[2]["used"] == 1 and got[2]["store_bytes"] == 0
    return got


def same(a, b):
    (ta, ha, sa), (tb, hb, sb) = a, b
    assert np.array_equal(ta.packed, tb.packed) and np.array_equal(ta.counts, tb.counts) and np.array_equal(ha, hb)
    for f in ("bases", "windows", "distinct", "kept"):
        assert sa[f] == sb[f], f


@pytest.mark.parametrize("parts", PARTS)
@pytest.mark.parametrize("k", KS)
def test_ranges_equal_the_oracle_and_one_pass(k, parts):
    t = 2
    seq = reads_of(k)
    got = count.count_bases(seq, k, t=t, partitions=parts)
    check(got, want_of(k, t), k, t)
    st = got[2]
    assert st["windows"] == sum(oracle_counts([seq], k).values())
    assert st["used"] == parts
    if parts > 1:
        assert st["store_bytes"] >= len(seq) * 3 // 8 and st["ms_pack"] > 0 and st["ms_plan"] > 0
        if k % 2 == 0:
            assert any(x == x.translate(_COMP)[::-1] for x in oracle_counts([seq], k))
    same(got, one_pass(k, t))


@pytest.mark.parametrize("mult", [1, 3, 40])
@pytest.mark.parametrize("parts", [2, 7])
@pytest.mark.parametrize("k", [13, 32, 33, 65, 128])
def test_several_batches_per_range(k, parts, mult, monkeypatch):
    """batches of mult * k bases: windows straddle the batch boundaries in the store and the spans the store is read in,
    the key buffer fills several times per range, and a range merges"""
    t = 1
    full = one_pass(k, t)
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", str(mult * k))
    got = count.count_bases(reads_of(k), k, t=t, partitions=parts)
    check(got, want_of(k, t), k, t)
    same(got, full)
    assert got[2]["used"] == parts
    # a sorted batch holds at most cap = (mult + 1) * k keys (SMG_COUNT_BATCH_BASES + k, Counter::init), so a run needs at least
    # windows / cap of them; where that is more than the ranges, some range sorted twice and merged
    need = -(-got[2]["windows"] // ((mult + 1) * k))
    assert got[2]["batches"] >= need
    if mult == 1 and k <= 65:
        assert need > 2 * parts, "the input is too small to make a range merge"


def test_files_in_either_order_give_the_bytes_of_one_pass(tmp_path):
    rng = np.random.default_rng(99)
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 4000))
    r1 = [genome[a:a + 150] for a in rng.integers(0, 3850, 250)]
    r2 = [genome[a:a + 150].translate(_RC)[::-1] for a in rng.integers(0, 3850, 250)]
    r2[3] = r2[3][:60] + b"N" + r2[3][61:]
    (tmp_path / "reads_1.fq").write_bytes(fastq_text(r1))
    (tmp_path / "reads_2.fq").write_bytes(fastq_text(r2))
    k, t = 31, 3
    runs = ((["-p1", "-T2", "-oone", "reads_1.fq", "reads_2.fq"], "one"), (["-p5", "-T2", "-ofive", "reads_1.fq", "reads_2.fq"], "five"),
            (["-p5", "-T2", "-oswap", "reads_2.fq", "reads_1.fq"], "swap"), (["-T2", "-oauto", "reads_2.fq", "reads_1.fq"], "auto"))
    for args, root in runs:
        r = subprocess.run([COUNT_BIN, f"-k{k}", f"-t{t}", "-H", "-v", *args], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want_ranges = "5 key ranges" if "-p5" in args else "1 key range,"
        assert want_ranges in r.stderr and "packed input" in r.stderr, r.stderr
        for name in (f"{root}.ktab", f".{root}.ktab.1", f"{root}.hist.txt"):
            assert (tmp_path / name).read_bytes() == (tmp_path / name.replace(root, "one")).read_bytes(), name
    packed, counts, _ = oracle_table([b"\n".join(r1), b"\n".join(r2)], k, t)
    got = ktab.read_ktab(str(tmp_path / "five"))
    assert got.nparts == 1 and np.array_equal(got.packed, packed) and np.array_equal(got.counts, counts)
    # the binding, from the files
    a = count.count_files([tmp_path / "reads_1.fq", tmp_path / "reads_2.fq"], k, t=t, threads=2, partitions=5)
    b = count.count_files([tmp_path / "reads_2.fq", tmp_path / "reads_1.fq"], k, t=t, threads=1, partitions=1)
    same(a, b)
    assert a[2]["used"] == 5 and b[2]["used"] == 1


@pytest.mark.parametrize("k", [31, 51])
def test_one_pass_refuses_what_the_automatic_mode_counts_in_ranges(k, monkeypatch):
    """a merge that holds fewer entries than the input has distinct k-mers: one pass is refused with the sizes, the
    automatic mode cuts ranges none of which can overflow and gives the oracle's table"""
    t = 2
    seq = reads_of(k)
    want = want_of(k, t)
    distinct = int(want[2].sum())
    limit = distinct // 3
    with pytest.raises(count.CountError) as e:
        count.count_bases(seq, k, t=t, partitions=1, max_entries=limit)
    assert e.value.code == -3
    assert "do not fit" in str(e.value) and f"one merge holds {limit}" in str(e.value) and f"merging {distinct} entries" in str(e.value)
    got = count.count_bases(seq, k, t=t, partitions=0, max_entries=limit)
    check(got, want, k, t)
    assert got[2]["used"] > 3 and got[2]["store_bytes"] > 0                # windows > distinct: more than three ranges
    same(got, one_pass(k, t))
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", str(k))                    # sorted batches of at most 2 k keys: ranges merge
    many = count.count_bases(seq, k, t=t, max_entries=limit)
    same(many, got)
    need = -(-got[2]["windows"] // (2 * k))
    assert many[2]["used"] >= got[2]["used"] and many[2]["batches"] >= need > got[2]["used"]
    # without the hook the same input is one pass in the automatic mode, as before
    monkeypatch.delenv("SMG_COUNT_BATCH_BASES")
    auto = count.count_bases(seq, k, t=t)
    assert auto[2]["used"] == 1 and auto[2]["store_bytes"] == 0 and auto[2]["batches"] == 1
    same(auto, got)


def test_a_bin_that_cannot_be_split_is_refused_and_named():
    rng = np.random.default_rng(3)
    k = 21
    seq = b"A" * 3000 + b"\n" + b"T" * 2000 + b"\n" + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 500))
    with pytest.raises(count.CountError) as e:
        count.count_bases(seq, k, t=1, max_entries=400)
    assert e.value.code == -3
    msg = str(e.value)
    assert "bin 0 " in msg and "aaaaaa" in msg and "one merge holds 400" in msg
    nwin = (3000 - k + 1) + (2000 - k + 1)                                   # poly-A and poly-T windows: all in bin 0
    n0 = int(msg.split(" holds ")[1].split(" windows")[0])
    assert nwin <= n0 <= nwin + 20
    got = count.count_bases(seq, k, t=1, max_entries=n0)                     # enough for bin 0: ranges, and the oracle's table
    check(got, oracle_table([seq], k, 1), k, 1)
    assert got[2]["used"] > 1


@pytest.mark.parametrize("parts,limit", [(3, 0), (0, 5), (4096, 0)])
def test_no_window_anywhere_gives_a_valid_empty_table(parts, limit, tmp_path):
    seq = b"ACGTACGTAC\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\nACGTNACGTNACGTNACGTNACGT\n\n" * 3
    table, hist, st = count.count_bases(seq, 21, t=1, partitions=parts, max_entries=limit)
    assert table.nels == 0 and table.packed.shape == (0, ktab.kbyte_of(21)) and hist.sum() == 0
    assert st["windows"] == 0 and st["distinct"] == 0 and st["kept"] == 0 and st["batches"] == 0
    assert st["used"] == (parts if parts else 1)
    (tmp_path / "r.fq").write_bytes(fastq_text([b"ACGTACGTAC", b"N" * 32, b""]))
    r = subprocess.run([COUNT_BIN, "-k21", "-t1", "-p3", "-H", "r.fq"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = ktab.read_ktab(str(tmp_path / "r"))
    assert t.nels == 0 and t.nparts == 1 and (tmp_path / "r.hist.txt").read_text() == ""
