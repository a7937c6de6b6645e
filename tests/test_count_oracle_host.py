"""The numpy oracle of tests/count_oracle.py against the Python oracle of tests/test_count_gpu.py (a Counter over byte
slices), entry for entry, on inputs small enough for the latter.  This is what makes the fast oracle trustworthy for
tests/test_count_scale_gpu.py; it needs no GPU."""
import numpy as np
import pytest

import count_oracle
from smudgeplot_amd import ktab
from test_count_gpu import oracle_counts, oracle_table, random_reads

KS = [13, 31, 32, 33, 64, 65, 96, 97, 128]
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def reads_of(k, seed):
    """reads of a small genome on both strands (counts well above 1), some lower case, random reads with Ns, reads shorter
    than k, stretches of k - 1, k and k + 1 between Ns, homopolymers, and for even k self-complementary sequence"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = bytes(rng.choice(acgt, 500))
    reads = []
    for _ in range(50):
        a = int(rng.integers(0, 500 - 200))
        r = genome[a:a + int(rng.integers(k, 200 + 1))]
        if rng.random() < 0.5:
            r = r.translate(_RC)[::-1]
        if rng.random() < 0.3:
            r = r.lower()
        reads.append(r)
    reads += random_reads(rng, 12, 1, 300, b"ACGTN")
    reads += random_reads(rng, 5, 1, k - 1)                                # shorter than k: no window
    reads.append(b"N".join(bytes(rng.choice(acgt, n)) for n in (k - 1, k, k + 1, k - 1, 1, 2 * k)))
    reads += [b"A" * (k + 40), b"T" * (k + 3), b"", b"N" * 40, genome[:k], genome[:k].translate(_RC)[::-1].lower()]
    if k % 2 == 0:
        reads += [b"ACGT" * (k // 2 + 5), b"AT" * (k + 7), b"GATC" * (k // 2 + 3)]
    return reads


@pytest.mark.parametrize("k", KS)
def test_numpy_oracle_equals_the_counter_oracle(k):
    reads = reads_of(k, 500 + k)
    keys, counts, windows = count_oracle.kmer_counts(count_oracle.pad_reads(reads), k)
    ref = oracle_counts(reads, k)
    assert windows == sum(ref.values()) and len(keys) == len(ref) > 400
    assert keys.shape == (len(ref), (k + 31) // 32) and keys.dtype == np.uint64
    items = sorted(ref.items())
    bases = np.frombuffer(b"".join(x for x, _ in items), np.uint8).reshape(len(items), k)
    assert np.array_equal(count_oracle.pack_keys(keys, k), ktab.pack_bases(bases))
    assert counts.tolist() == [v for _, v in items]
    if k % 2 == 0:
        assert any(x == bytes(3 - b for b in x[::-1]) for x in ref)          # a k-mer that is its own reverse complement
    for t in (1, 2, 5):
        got, want = count_oracle.table(keys, counts, k, t), oracle_table(reads, k, t)
        assert len(want[1]) > 0 and len(got) == 3
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("k", [13, 32, 64, 128])
def test_even_k_self_complementary_sequence(k):
    reads = [b"ACGT" * 100, b"AT" * 150, b"GATC" * 50]
    keys, counts, windows = count_oracle.kmer_counts(count_oracle.pad_reads(reads), k)
    assert windows == 400 + 300 + 200 - 3 * (k - 1)
    got, want = count_oracle.table(keys, counts, k, 1), oracle_table(reads, k, 1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    if k % 2 == 0:
        # ACGT.. of even length is its own reverse complement: its windows are 4 k-mers (2 canonical), one count per window
        one = count_oracle.kmer_counts(count_oracle.pad_reads(reads[:1]), k)
        assert one[2] == int(one[1].sum()) == 400 - k + 1 and len(one[0]) == len(oracle_counts(reads[:1], k))


def test_one_stream_with_separators_equals_its_reads_as_rows():
    """the counter is handed one byte stream in which '\\n' separates reads; the oracle takes the reads as rows"""
    k = 33
    rng = np.random.default_rng(5)
    code = rng.integers(0, 4, (40, 90)).astype(np.uint8)
    code[rng.random(code.shape) < 0.01] = 4
    code[7:20] = np.where(code[7:20] > 3, 4, 3 - np.minimum(code[7:20], 3))[:, ::-1]
    text = np.frombuffer(b"ACGTN", np.uint8)[code]
    stream = b"\n".join(bytes(r) for r in text)
    assert np.array_equal(count_oracle.encode(text), code) and np.array_equal(count_oracle.encode(bytes(text[3]).lower()), code[3])
    keys, counts, windows = count_oracle.kmer_counts(code, k)
    for g, w in zip(count_oracle.table(keys, counts, k, 1), oracle_table([stream], k, 1)):
        assert np.array_equal(g, w)
    assert windows == sum(oracle_counts([stream], k).values())


def test_counts_clamp_and_thresholds():
    k = 13
    reads = [b"A" * 40000, b"ACGTTGCAAGGCTTAGCATCGATCGGATCGATTAGC" * 3]
    keys, counts, windows = count_oracle.kmer_counts(count_oracle.pad_reads(reads), k)
    assert int(counts.max()) == 40000 - k + 1 and windows == int(counts.sum())
    packed, c16, hist = count_oracle.table(keys, counts, k, 4)
    assert int(c16.max()) == 32767 and hist[32767] == 1 and int(hist.sum()) == len(keys) and c16.min() >= 4
    for g, w in zip((packed, c16, hist), oracle_table(reads, k, 4)):
        assert np.array_equal(g, w)


def test_nothing_to_count():
    for reads in ([b"ACGT" * 3], [b"", b"NNNN"], [b"ACGTACGTACGTN" * 5]):
        keys, counts, windows = count_oracle.kmer_counts(count_oracle.pad_reads(reads), 14)
        assert keys.shape == (0, 1) and len(counts) == 0 and windows == 0
        packed, c16, hist = count_oracle.table(keys, counts, 14, 1)
        assert packed.shape == (0, 4) and len(c16) == 0 and hist.sum() == 0
