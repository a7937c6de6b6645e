"""A key range that keeps nothing, in front of or behind ranges that keep entries: the seam of the counter's output table.

Three requested ranges over an input in which nearly every window is a singleton, so that with t = 4 a range keeps only
what was planted in it: reads of exactly k bases, each present four times.
  first range empty   40 planted reads begin with G or T and end with A or C: the k-mer and its reverse complement both begin
                      with G or T, so the canonical k-mer lies in the upper half of the 4096 bins, behind the first cut
  last range empty    40 planted reads begin with A and do not end with T: the canonical k-mer is the read, in the first
                      quarter of the bins, in front of the last cut
and in both 10 more that begin with CA and end with A or C (canonical as they stand), which land in the middle range: the
cuts of three equal window shares lie in the A's and in the C's behind CA, since the smaller of a random k-mer and its
reverse complement begins with A or C three times out of four.  All of that is checked on the CPU, from the numpy
oracle's k-mers and count.plan, before the GPU is used.  Then: host table and device table against the Python oracle of
test_count_gpu entry for entry, the histogram, three ranges used, device table = host table, no NULL pointer."""
import functools

import numpy as np
import pytest

import count_oracle
from smudgeplot_amd import count
from test_count_gpu import check, oracle_table

pytestmark = pytest.mark.gpu

T, RANGES, READ, NREADS = 4, 3, 60, 3000


def planted(rng, k, first, last, n):
    """n distinct reads of exactly k bases whose first bases are one of `first` (byte strings) and whose last is in `last`"""
    out = set()
    while len(out) < n:
        f = first[int(rng.integers(len(first)))]
        mid = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), k - len(f) - 1))
        out.add(f + mid + bytes([last[int(rng.integers(len(last)))]]))
    return sorted(out)


@functools.lru_cache(maxsize=None)
def case(k, empty):
    """-> (stream for count_bases, oracle_table of it), the precondition checked"""
    rng = np.random.default_rng(100 * k + len(empty))
    reads = [bytes(r) for r in rng.choice(np.frombuffer(b"ACGT", np.uint8), (NREADS, READ))]
    own = planted(rng, k, [b"G", b"T"], b"AC", 40) if empty == "first" else planted(rng, k, [b"A"], b"ACG", 40)
    reads += T * (own + planted(rng, k, [b"CA"], b"AC", 10))
    order = rng.permutation(len(reads))
    stream = b"\n".join(reads[i] for i in order) + b"\n"
    target = 0 if empty == "first" else RANGES - 1

    # the precondition, on the CPU: the plan of three ranges over the oracle's window histogram leaves the target range with
    # windows but nothing to keep, and the other two with something to keep
    keys, counts, windows = count_oracle.kmer_counts(count_oracle.pad_reads([reads[i] for i in order]), k)
    bin_of = (keys[:, 0] >> np.uint64(52)).astype(np.int64)
    bins = np.bincount(bin_of, weights=counts, minlength=count.BINS).astype(np.uint64)
    assert int(bins.sum()) == windows == NREADS * (READ - k + 1) + T * 50
    cuts = count.plan(bins, windows, RANGES)
    assert len(cuts) == RANGES + 1
    for r in range(RANGES):
        inside = (bin_of >= cuts[r]) & (bin_of < cuts[r + 1])
        assert int(bins[cuts[r]:cuts[r + 1]].sum()) > 1000
        kept = int((counts[inside] >= T).sum())
        assert (kept == 0) if r == target else (kept >= 5), (r, kept, cuts)
    want = oracle_table([stream], k, T)
    assert len(want[1]) == 50 and int(want[2][T]) == 50
    return np.frombuffer(stream, np.uint8), want


@pytest.mark.parametrize("empty", ["first", "last"])
@pytest.mark.parametrize("k", [21, 33])
def test_a_range_that_keeps_nothing(k, empty):
    stream, want = case(k, empty)
    host = count.count_bases(stream, k, t=T, partitions=RANGES)
    check(host, want, k, T)
    assert host[2]["used"] == RANGES and host[2]["split"] == 0 and host[2]["store_bytes"] > 0
    table, hist, st = count.count_bases_device(stream, k, t=T, partitions=RANGES)
    with table:
        assert table.keys_ptr and table.counts_ptr
        assert (table.nels, table.words) == (host[0].nels, (k + 31) // 32)
        keys, counts = table.to_host()
    assert np.array_equal(count.keys_to_packed(keys, k), host[0].packed) and np.array_equal(counts, host[0].counts)
    assert np.array_equal(hist, want[2]) and np.array_equal(hist, host[1])
    assert st["used"] == RANGES
    for f in ("bases", "windows", "distinct", "kept"):
        assert st[f] == host[2][f], f
