"""The k-mer counter on the GPU against a Python oracle, entry for entry: k-mers, counts, histogram.

The oracle shares nothing with the device code: split on non-ACGT, slide, canonicalise (the smaller of the k-mer and its
reverse complement as tuples of base codes, which is the order of the left-aligned big-endian words), count, clamp,
threshold, sort.  All inputs are seeded and generated here.
"""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import brute
from conftest import HETMERS_BIN, REF_BIN, ROOT
from smudgeplot_amd import count, ktab

pytestmark = pytest.mark.gpu

COUNT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_count")
TILE = 4096                                            # KC_TILE of smg_count.hip
_CODE = bytes.maketrans(b"ACGTacgt", bytes([0, 1, 2, 3, 0, 1, 2, 3]))
_COMP = bytes.maketrans(bytes([0, 1, 2, 3]), bytes([3, 2, 1, 0]))


# ---- oracle -------------------------------------------------------------------------------------------------------

def oracle_counts(streams, k):
    """-> Counter {tuple-like bytes of k base codes: count} over the canonical k-mers of all streams"""
    cnt = collections.Counter()
    for s in streams:
        for stretch in re.split(rb"[^ACGTacgt]+", bytes(s)):
            if len(stretch) < k:
                continue
            c = stretch.translate(_CODE)
            r = c.translate(_COMP)[::-1]
            n = len(c)
            for i in range(n - k + 1):
                x, y = c[i:i + k], r[n - k - i:n - i]
                cnt[x if x <= y else y] += 1
    return cnt


def oracle_table(streams, k, t):
    """-> (packed [N,kbyte] sorted, counts uint16, hist uint64[32768])"""
    cnt = oracle_counts(streams, k)
    items = sorted(cnt.items())
    c = np.minimum(np.array([v for _, v in items], dtype=np.int64), 32767)
    hist = np.bincount(c, minlength=32768).astype(np.uint64)
    keep = [i for i in range(len(items)) if c[i] >= t]
    bases = np.frombuffer(b"".join(items[i][0] for i in keep), dtype=np.uint8).reshape(len(keep), k)
    return ktab.pack_bases(bases), c[keep].astype(np.uint16), hist


def oracle_table_u64(codes_2d, k, t):
    """the same for many reads of equal length without N, k <= 32: np.unique on uint64 keys"""
    w = np.lib.stride_tricks.sliding_window_view(codes_2d, k, axis=1).reshape(-1, k)
    key = np.zeros(len(w), np.uint64)
    for j in range(k):
        key = (key << np.uint64(2)) | w[:, j].astype(np.uint64)
    key <<= np.uint64(64 - 2 * k)
    can = np.minimum(key, ktab.revcomp_u64(key, k))
    u, c = np.unique(can, return_counts=True)
    c = np.minimum(c, 32767)
    hist = np.bincount(c, minlength=32768).astype(np.uint64)
    keep = c >= t
    return ktab.u64_to_packed(u[keep], k), c[keep].astype(np.uint16), hist, len(can), len(u)


# ---- input helpers ------------------------------------------------------------------------------------------------

def random_reads(rng, n, lo, hi, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, np.uint8)
    return [bytes(rng.choice(a, int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def fasta_text(reads, width=60):
    out = []
    for i, r in enumerate(reads):
        out.append(b">s%d\n" % i)
        out += [r[j:j + width] + b"\n" for j in range(0, len(r), width)]
    return b"".join(out)


def fastq_text(reads):
    q = b"@>I#"
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, bytes([q[(i + j) % 4] for j in range(len(r))])) for i, r in enumerate(reads))


def check(got, want, k, t):
    table, hist, st = got
    packed, counts, whist = want
    assert table.k == k and table.minval == t and table.ibyte == 3 and table.nparts == 1
    assert table.packed.shape == packed.shape, (table.packed.shape, packed.shape)
    assert np.array_equal(table.packed, packed)
    assert np.array_equal(table.counts, counts)
    assert np.array_equal(hist, whist)
    assert st["distinct"] == int(whist.sum()) and st["kept"] == len(counts)
    assert st["windows"] == int((whist * np.arange(32768, dtype=np.uint64)).sum()) or whist[32767] > 0


# ---- cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [1, 4])
@pytest.mark.parametrize("k", [13, 17, 21, 31, 32, 33, 51, 64, 65, 100, 128])
def test_random_reads(k, t):
    rng = np.random.default_rng(1000 * k + t)
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 600))
    reads = []
    for _ in range(60):                                  # reads of a small genome, both strands: counts well above 1
        a = int(rng.integers(0, 600 - 140))
        r = genome[a:a + int(rng.integers(k, 140 + 1))] if k <= 140 else genome
        if rng.random() < 0.5:
            r = r.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
        if rng.random() < 0.3:
            r = r.lower()
        reads.append(r)
    reads += random_reads(rng, 10, 1, 300, b"ACGTN")
    seq = b"\n".join(reads)
    check(count.count_bases(seq, k, t=t), oracle_table([seq], k, t), k, t)


@pytest.mark.parametrize("k", [13, 31, 32, 33, 64, 65, 128])
def test_stretch_lengths_and_ns(k):
    rng = np.random.default_rng(k)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parts = [bytes(rng.choice(acgt, n)) for n in (k - 1, k, k + 1, k - 1, 2 * k, k)]
    seq = b"N".join(parts) + b"\n" + b"N" * 500 + b"\n"
    r = bytearray(rng.choice(acgt, 3000))
    r[::7] = b"N" * len(r[::7])                          # an N every few bases: no window at all for k > 6
    seq += bytes(r) + b"\n"
    r = bytearray(rng.choice(acgt, 6000))
    r[::(k + 3)] = b"n" * len(r[::(k + 3)])              # stretches of k + 2
    seq += bytes(r)
    check(count.count_bases(seq, k, t=1), oracle_table([seq], k, 1), k, 1)


def test_input_without_any_window_gives_a_valid_empty_table(tmp_path):
    (tmp_path / "r.fq").write_bytes(fastq_text([b"ACGTACGTAC", b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN", b"ACGTNACGTNACGTNACGTNACGT", b""]))
    r = subprocess.run([COUNT_BIN, "-k21", "-t1", "-H", "r.fq"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = ktab.read_ktab(str(tmp_path / "r"))
    assert t.k == 21 and t.nels == 0 and t.ibyte == 3 and t.nparts == 1 and t.minval == 1
    assert int(t.index[-1]) == 0 and len(t.index) == 1 << 24
    assert (tmp_path / "r.hist.txt").read_text() == ""
    table, hist, st = count.count_files([tmp_path / "r.fq"], 21, t=1)
    assert table.nels == 0 and hist.sum() == 0 and st["windows"] == 0 and st["bases"] == 10 + 32 + 24


@pytest.mark.parametrize("k", [14, 32, 34, 64, 128])
def test_even_k_self_complementary_kmers(k):
    seq = b"ACGT" * 100 + b"\n" + b"AT" * 150 + b"\n" + b"GATC" * 50
    got = count.count_bases(seq, k, t=1)
    want = oracle_table([seq], k, 1)
    check(got, want, k, 1)
    # ACGT.. of even length is its own reverse complement and counts once per window
    self_rc = oracle_counts([b"ACGT" * 100], k)
    assert sum(self_rc.values()) == 400 - k + 1


@pytest.mark.parametrize("k,batch", [(21, 0), (21, 9000), (40, 0), (40, 5000)])
def test_counts_saturate_and_sums_pass_16_bits(k, batch, monkeypatch):
    """a 40 000-base poly-A read (one k-mer, count 40 001 - k) and, twice, a tandem repeat of AC with 70 000 windows (two
    k-mers, 70 000 each): counts pass 32767, the uint32 sums pass 65535, all three end in the last bin"""
    if batch:
        monkeypatch.setenv("SMG_COUNT_BATCH_BASES", str(batch))
    tandem = (b"AC" * (35000 + k))[:70000 + k - 1]
    seq = b"A" * 40000 + b"\n" + tandem + b"\n" + tandem + b"\n" + b"ACGTTGCAAGGCTTAGCATCGATCGGATCGATTAGC" * 3
    got = count.count_bases(seq, k, t=4)
    want = oracle_table([seq], k, 4)
    assert want[2][32767] == 3 and int(want[1].max()) == 32767
    assert sorted(oracle_counts([seq], k).values())[-3:] == [40000 - k + 1, 70000, 70000]
    check(got, want, k, 4)
    assert got[2]["windows"] == sum(oracle_counts([seq], k).values())
    if batch:
        assert got[2]["batches"] > 10


@pytest.mark.parametrize("mult", [1, 7, 64])
@pytest.mark.parametrize("k", [21, 65])
def test_batch_size_does_not_change_the_result(k, mult, monkeypatch, tmp_path):
    rng = np.random.default_rng(k * mult)
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 2000))
    reads = [genome[a:a + 150] for a in rng.integers(0, 1850, 40)] + [genome * 10 + b"N" + genome[:500]] \
        + random_reads(rng, 20, 1, 90, b"ACGTN")
    (tmp_path / "a.fa").write_bytes(fasta_text(reads[:30]))
    (tmp_path / "b.fq").write_bytes(fastq_text(reads[30:]))
    paths = [tmp_path / "a.fa", tmp_path / "b.fq"]
    one = count.count_files(paths, k, t=1)
    assert one[2]["batches"] == 1
    want = oracle_table([count.parse(p) for p in paths], k, 1)
    check(one, want, k, 1)
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", str(mult * k))
    many = count.count_files(paths, k, t=1, threads=2)
    assert many[2]["batches"] > 5
    check(many, want, k, 1)
    seq = b"\n".join(reads)
    check(count.count_bases(seq, k, t=1), want, k, 1)


@pytest.mark.parametrize("k", [31, 65])
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 31 - 1, 2 * TILE + 65 - 1])
def test_tile_edges(k, n):
    rng = np.random.default_rng(n + k)
    seq = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    for p in (TILE - k, TILE - 1, TILE, TILE + k):      # stretches that end and begin at the tile boundary
        if 0 <= p < n and (p // 7) % 2:
            seq[p] = ord("N")
    check(count.count_bases(bytes(seq), k, t=1), oracle_table([bytes(seq)], k, 1), k, 1)


def _table_bytes(d, root):
    return (d / f"{root}.ktab").read_bytes(), (d / f".{root}.ktab.1").read_bytes()


def test_executable_threads_and_file_order(tmp_path):
    rng = np.random.default_rng(77)
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000))
    r1 = [genome[a:a + 150] for a in rng.integers(0, 4850, 300)]
    r2 = [genome[a:a + 150].translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1] for a in rng.integers(0, 4850, 300)]
    r2[7] = r2[7][:70] + b"N" + r2[7][71:]
    (tmp_path / "reads_1.fq").write_bytes(fastq_text(r1))
    (tmp_path / "reads_2.fq").write_bytes(fastq_text(r2).replace(b"\n", b"\r\n"))
    k, t = 31, 4
    for args, root in ((["-T1", "-oone", "reads_1.fq", "reads_2.fq"], "one"), (["-T8", "-oeight", "reads_1.fq", "reads_2.fq"], "eight"),
                       (["-T8", "-oswap.ktab", "reads_2.fq", "reads_1.fq"], "swap"), (["-T2", "reads_1.fq", "reads_2.fq"], "reads_1")):
        r = subprocess.run([COUNT_BIN, f"-k{k}", f"-t{t}", "-H", "-v", *args], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "distinct" in r.stderr and "ms: read" in r.stderr
        assert _table_bytes(tmp_path, root) == _table_bytes(tmp_path, "one")
        assert (tmp_path / f"{root}.hist.txt").read_bytes() == (tmp_path / "one.hist.txt").read_bytes()
    packed, counts, hist = oracle_table([b"\n".join(r1), b"\n".join(r2)], k, t)
    got = ktab.read_ktab(str(tmp_path / "one"))
    assert got.k == k and got.minval == t and got.ibyte == 3 and got.nparts == 1
    assert np.array_equal(got.packed, packed) and np.array_equal(got.counts, counts)
    rows = [bytes(r) for r in got.packed]
    assert all(a < b for a, b in zip(rows, rows[1:]))                  # sorted, duplicate free
    lines = (tmp_path / "one.hist.txt").read_text().splitlines()
    parsed = [int(line.split()[1]) for line in lines]                  # as smudgeplot's cutoff() reads it
    top = int(np.nonzero(hist)[0].max())
    assert [int(line.split()[0]) for line in lines] == list(range(1, top + 1))
    assert parsed == [int(x) for x in hist[1:top + 1]]
    # the table written through write_ktab is the same file, byte for byte
    ktab.write_ktab(str(tmp_path / "py"), k, packed, counts, ibyte=3, nparts=1, minval=t)
    assert _table_bytes(tmp_path, "py") == _table_bytes(tmp_path, "one")


def test_smg_condition_still_writes_the_bytes_of_write_ktab(tmp_path):
    """the format-F writer moved from condition_main.c into smg_cli.h: on the golden table k31_i1 (one part) the tool's
    output equals ktab.write_ktab of the numpy-conditioned table, byte for byte, as before the move"""
    from conftest import load_golden
    g = load_golden("k31_i1")
    k, L = g["k"], g["L"] + 2
    rc = ktab.revcomp_packed(g["packed"], k)
    canon = np.array([bytes(a) <= bytes(b) for a, b in zip(g["packed"], rc)])
    rp, rcnt = g["packed"][canon], g["counts"][canon]
    ktab.write_ktab(str(tmp_path / "raw"), k, rp, rcnt, ibyte=1, nparts=1, minval=1)
    tool = os.path.join(ROOT, "smudgeplot_amd", "bin", "smg_condition")
    r = subprocess.run([tool, f"-e{L}", "raw", "cond"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    keep = rcnt >= L
    cp, cc = ktab.symmetrize(rp[keep], rcnt[keep], k)
    ktab.write_ktab(str(tmp_path / "want"), k, cp, cc, ibyte=1, nparts=1, minval=L)
    assert len(cc) > 100
    assert _table_bytes(tmp_path, "cond") == _table_bytes(tmp_path, "want")


def test_reads_to_smu_end_to_end(tmp_path):
    """100 kb diploid genome, 1 % heterozygous SNPs, 150-base reads of both strands at ~20x per haplotype with 0.5 %
    substitution errors: smg_count -k21 -t1, then the drop-in hetmers -e6 on that raw table (neither trimmed nor closed:
    it conditions on the device).  Expected: brute.hetmers_plot on the oracle's counts trimmed at 6 and closed."""
    rng = np.random.default_rng(11)
    G, k, L, cov, err, e = 100_000, 21, 150, 20, 0.005, 6
    h1 = rng.integers(0, 4, G).astype(np.uint8)
    h2 = h1.copy()
    snp = rng.random(G) < 0.01
    h2[snp] = (h2[snp] + rng.integers(1, 4, snp.sum())) & 3
    reads = []
    for h in (h1, h2):
        n = G * cov // L
        st = rng.integers(0, G - L, n)
        R = h[st[:, None] + np.arange(L)]
        m = rng.random(R.shape) < err
        R = np.where(m, (R + rng.integers(1, 4, R.shape)) & 3, R).astype(np.uint8)
        flip = rng.random(n) < 0.5
        R[flip] = 3 - R[flip][:, ::-1]
        reads.append(R)
    R = np.concatenate(reads)
    text = np.frombuffer(b"ACGT", np.uint8)[R]
    half = len(text) // 2
    (tmp_path / "reads_1.fq").write_bytes(fastq_text([bytes(r) for r in text[:half]]))
    (tmp_path / "reads_2.fq").write_bytes(fastq_text([bytes(r) for r in text[half:]]))

    r = subprocess.run([COUNT_BIN, f"-k{k}", "-t1", "-T8", "-H", "-oSample", "reads_1.fq", "reads_2.fq"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    packed, counts, hist, nwin, ndist = oracle_table_u64(R, k, 1)
    assert nwin == len(R) * (L - k + 1) and ndist > 400_000
    got = ktab.read_ktab(str(tmp_path / "Sample"))
    assert np.array_equal(got.packed, packed) and np.array_equal(got.counts, counts)
    top = int(np.nonzero(hist)[0].max())
    assert [int(line.split()[1]) for line in open(tmp_path / "Sample.hist.txt")] == [int(x) for x in hist[1:top + 1]]

    r = subprocess.run([HETMERS_BIN, f"-e{e}", "-T8", "-v", "-oSample", "Sample.ktab"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "  The input table is untrimmed and not symmetric\n" in r.stderr
    keep = counts >= e
    cp, cc = ktab.symmetrize(packed[keep], counts[keep], k)
    plot = brute.hetmers_plot(cp, cc, k)
    assert int(plot.sum()) >= 1000
    smu = (tmp_path / "Sample.smu").read_text()
    assert smu == brute.smu_text(plot)
    if os.path.exists(REF_BIN):
        ktab.write_ktab(str(tmp_path / "cond"), k, cp, cc, ibyte=3, nparts=1, minval=e)
        q = subprocess.run([REF_BIN, f"-e{e}", "-T4", "-oref", "cond"], cwd=tmp_path, capture_output=True, text=True)
        assert q.returncode == 0, q.stderr
        assert (tmp_path / "ref.smu").read_bytes() == (tmp_path / "Sample.smu").read_bytes()
