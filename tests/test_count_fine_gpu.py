"""A bin of six leading bases with more windows than one merge holds, on the GPU: it is split on its next six bases, ranges
begin and end inside it, and the table is the Python oracle's of tests/test_count_gpu.py and that of one pass -- through the
host entries, the device entries, reads_to_plot and the executable; a sub-bin above one merge is still refused, with both
names; a run that needs no split reports none.

The input per k (seed 8100 + k): 3000 reads of k bases that begin with AAAAAA, every second one reverse-complemented, 1500
that begin with CCCCCC, one random read of 2000 bases; max_entries = 400.  Each test asserts from the oracle that the input
still exercises the split: bins aaaaaa and cccccc above the limit, no 24-bit sub-bin above it."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from smudgeplot_amd import count
from test_count_gpu import check, fastq_text, oracle_counts, oracle_table
from test_count_parts_gpu import reads_of, same, want_of

pytestmark = pytest.mark.gpu

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
LIMIT = 400
BIN_C = 0b010101010101                                                      # cccccc
_RC = bytes.maketrans(b"ACGT", b"TGCA")


@functools.lru_cache(maxsize=None)
def split_reads(k):
    rng = np.random.default_rng(8100 + k)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads = []
    for i in range(3000):
        r = b"AAAAAA" + bytes(rng.choice(acgt, k - 6))
        reads.append(r.translate(_RC)[::-1] if i % 2 else r)
    reads += [b"CCCCCC" + bytes(rng.choice(acgt, k - 6)) for _ in range(1500)]
    reads.append(bytes(rng.choice(acgt, 2000)))
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def split_input(k):
    """-> (stream, windows, windows per 12-bit bin, the largest 24-bit sub-bin)"""
    seq = b"\n".join(split_reads(k))
    bins, fine = np.zeros(4096, np.int64), {}
    for kmer, c in oracle_counts([seq], k).items():
        v = 0
        for code in kmer[:12]:
            v = 4 * v + code
        bins[v >> 12] += c
        fine[v] = fine.get(v, 0) + c
    return seq, int(bins.sum()), bins, max(fine.values())


def exercises_the_split(k):
    seq, windows, bins, top = split_input(k)
    assert bins[0] > LIMIT and bins[BIN_C] > LIMIT, (bins[0], bins[BIN_C])
    assert top <= LIMIT, top
    assert int((bins > LIMIT).sum()) == 2
    return seq, windows


@functools.lru_cache(maxsize=None)
def split_want(k, t):
    return oracle_table([split_input(k)[0]], k, t)


@functools.lru_cache(maxsize=None)
def split_one_pass(k, t):
    got = count.count_bases(split_input(k)[0], k, t=t, partitions=1)
    assert got[2]["used"] == 1 and got[2]["split"] == 0
    return got


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("k", [13, 21, 31, 32, 33, 51, 65, 128])
def test_split_bins_give_the_oracle_table(k, t):
    seq, windows = exercises_the_split(k)
    got = count.count_bases(seq, k, t=t, max_entries=LIMIT)
    check(got, split_want(k, t), k, t)
    st = got[2]
    assert st["windows"] == windows
    assert st["split"] == 2 and st["used"] >= -(-windows // LIMIT) and st["store_bytes"] > 0
    same(got, split_one_pass(k, t))


@pytest.mark.parametrize("mult", [1, 3])
@pytest.mark.parametrize("k", [13, 32, 33, 65])
def test_split_bins_with_small_batches(k, mult, monkeypatch):
    """a key buffer of (mult + 1) k keys: the sub-ranges fill it several times and merge"""
    t = 1
    seq, windows = exercises_the_split(k)
    full = split_one_pass(k, t)
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", str(mult * k))
    got = count.count_bases(seq, k, t=t, max_entries=LIMIT)
    check(got, split_want(k, t), k, t)
    same(got, full)
    assert got[2]["split"] == 2 and got[2]["used"] >= -(-windows // LIMIT)
    assert got[2]["batches"] >= -(-windows // ((mult + 1) * k))


def test_a_sub_bin_above_one_merge_is_refused_with_both_names():
    rng = np.random.default_rng(3)                                           # the input of the 12-bit refusal test
    k = 21
    seq = b"A" * 3000 + b"\n" + b"T" * 2000 + b"\n" + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 500))
    with pytest.raises(count.CountError) as e:
        count.count_bases(seq, k, t=1, max_entries=LIMIT)
    assert e.value.code == -3
    msg = str(e.value)
    assert "bin 0 " in msg and "aaaaaa" in msg and "one merge holds 400" in msg and "aaaaaaaaaaaa" in msg
    sub0 = sum(c for kmer, c in oracle_counts([seq], k).items() if not any(kmer[:12]))
    assert sub0 >= (3000 - k + 1) + (2000 - k + 1)
    assert f"sub-bin 0 (canonical k-mers that begin with aaaaaaaaaaaa) holds {sub0} windows" in msg
    with pytest.raises(count.CountError) as e:
        count.count_bases(seq, k, t=1, max_entries=sub0 - 1)
    assert e.value.code == -3 and "aaaaaaaaaaaa" in str(e.value)
    got = count.count_bases(seq, k, t=1, max_entries=sub0)                   # enough for the sub-bin: counted
    check(got, oracle_table([seq], k, 1), k, 1)
    assert got[2]["used"] > 1


@pytest.mark.parametrize("k", [21, 65])
def test_device_table_with_split_bins(k):
    from test_count_device_gpu import same_as_host
    t = 2
    seq, windows = exercises_the_split(k)
    got = count.count_bases_device(seq, k, t=t, max_entries=LIMIT)
    assert got[2]["split"] == 2 and got[2]["used"] >= -(-windows // LIMIT)
    same_as_host(got, split_one_pass(k, t), k, t)


@pytest.mark.parametrize("k", [21, 33])
def test_reads_to_plot_with_split_bins(k):
    t = e = 1
    seq, windows = exercises_the_split(k)
    want_plot, want_hist, want_st = count.reads_to_plot(seq, k, t, e, partitions=1)
    plot, hist, st = count.reads_to_plot(seq, k, t, e, max_entries=LIMIT)
    assert st["split"] == 2 and want_st["split"] == 0 and st["used"] >= -(-windows // LIMIT)
    assert np.array_equal(plot, want_plot) and np.array_equal(hist, want_hist) and np.array_equal(hist, split_want(k, t)[2])
    assert st["hetmers"]["nels"] == want_st["hetmers"]["nels"] > 0
    assert st["kept"] == split_one_pass(k, t)[2]["kept"]


def test_smg_count_splits_and_writes_the_table_of_one_pass(tmp_path):
    k, t = 21, 1                                                            # (nearly every k-mer of this input occurs once)
    seq, windows = exercises_the_split(k)
    (tmp_path / "reads.fq").write_bytes(fastq_text(list(split_reads(k))))
    r = subprocess.run([COUNT_BIN, f"-k{k}", f"-t{t}", "-p1", "-H", "-oone", "reads.fq"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([COUNT_BIN, f"-k{k}", f"-t{t}", "-p0", "-H", "-v", "-osplit", "reads.fq"], cwd=tmp_path, capture_output=True, text=True,
                       env=dict(os.environ, SMG_COUNT_MAX_ENTRIES=str(LIMIT)))
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stderr.splitlines() if " key range" in ln]
    assert len(line) == 1 and "packed input" in line[0] and "2 bins of six leading bases split on the next six" in line[0], r.stderr
    assert int(line[0].split()[0]) >= -(-windows // LIMIT)
    for name in ("split.ktab", ".split.ktab.1", "split.hist.txt"):
        assert (tmp_path / name).read_bytes() == (tmp_path / name.replace("split", "one")).read_bytes(), name
    assert os.path.getsize(tmp_path / ".split.ktab.1") > 1000


@pytest.mark.parametrize("k", [31, 51])
def test_a_run_that_needs_no_split_reports_none(k):
    """the inputs of tests/test_count_parts_gpu.py: as many ranges as before, cut between whole bins"""
    t = 2
    seq = reads_of(k)
    bins = np.zeros(4096, np.uint64)
    for kmer, c in oracle_counts([seq], k).items():
        v = 0
        for code in kmer[:6]:
            v = 4 * v + code
        bins[v] += np.uint64(c)
    limit = int(want_of(k, t)[2].sum()) // 3
    assert int(bins.max()) <= limit
    got = count.count_bases(seq, k, t=t, max_entries=limit)
    check(got, want_of(k, t), k, t)
    assert got[2]["split"] == 0 and got[2]["used"] == len(count.plan(bins, limit)) - 1 > 3
    for parts in (1, 3, 4096):
        st = count.count_bases(seq, k, t=t, partitions=parts)[2]
        assert st["split"] == 0 and st["used"] == parts
    st = count.count_bases(seq, k, t=t)[2]
    assert st["split"] == 0 and st["used"] == 1 and st["store_bytes"] == 0
