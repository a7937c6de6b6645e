"""Streams in front of the k-mer counter on the GPU: the same bytes through a FIFO and from a regular file give the same
table, histogram and statistics -- plain FASTQ, BGZF FASTQ, BAM and a k-mer dump, with one- and two-word k-mers, in one
pass and by key range -- although a call with a stream is planned without a bound (count.stream_plan): its packed store
begins at a size that owes nothing to the input and grows.  Then the seam of the BGZF reader where a member straddles its
chunk, the streams that end too early, the refusal of plain gzip, streams next to files on several reader threads, and the
executable.  Both sides of most comparisons come from the library, so one case is held against tests/count_oracle.py."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_craft as bc
import bgzf_craft as bz
import count_oracle
import dump_craft as dc
from fifo_craft import Writer, fifo, refused, through_fifo
from smudgeplot_amd import count

pytestmark = pytest.mark.gpu

T = 2
PIECE = 65537


@pytest.fixture(scope="module")
def reads():
    """3000 reads of 100 .. 150 bases from both strands of a diploid genome of 20 000 bases, an N now and then"""
    rng = np.random.default_rng(17)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 20000)
    other = genome.copy()
    other[40::83] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), other[40::83])]
    out = []
    for i in range(3000):
        a = int(rng.integers(0, 20000 - 150))
        r = bytes((genome if i % 2 else other)[a:a + int(rng.integers(100, 151))])
        if i % 3 == 0:
            r = r.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
        if i % 61 == 0:
            r = r[:70] + b"N" + r[71:]
        out.append(r)
    return out


def fastq_of(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def inputs(reads, tmp_path_factory):
    """format -> (bytes of the input, path of the regular file that holds them)"""
    d = tmp_path_factory.mktemp("stream_inputs")
    fq = fastq_of(reads)
    data = {"fastq": fq,
            "bgzf": bz.bgzf(fq, level=1, sizes=[4099, 65280, 997, 65280]),
            "bam": bz.bgzf(bc.bam_text(bc.header(), [(b"r%d" % i, r, 0x100 if i % 37 == 5 else 4) for i, r in enumerate(reads)]), level=1)}
    for k in (31, 51):
        kmers = dc.random_kmers(k, 4000, seed=k, distinct_canonical=False)
        data[f"dump{k}"] = dc.text([(s, 1 + i % 9) for i, s in enumerate(kmers + kmers[:500])])
    out = {}
    for name, b in data.items():
        p = d / f"{name}.in"
        p.write_bytes(b)
        out[name] = (b, str(p))
    return out


FIELDS = ("bases", "windows", "distinct", "kept")


def same(got, want, what=""):
    (gt, gh, gs), (wt, wh, ws) = got, want
    assert np.array_equal(gt.packed, wt.packed) and np.array_equal(gt.counts, wt.counts), what
    assert np.array_equal(gh, wh), what
    assert {f: gs[f] for f in FIELDS} == {f: ws[f] for f in FIELDS}, what


_FILE = {}


def of_file(inputs, name, k, partitions, **kw):
    """the call on the regular file, once per case"""
    key = (name, k, partitions, tuple(sorted(kw.items())))
    if key not in _FILE:
        _FILE[key] = count.count_files(inputs[name][1], k, t=T, threads=1, partitions=partitions, **kw)
    return _FILE[key]


# ---- 1. the same bytes from a FIFO and from a file ----------------------------------------------------------------------

@pytest.mark.parametrize("partitions", [0, 1, 3])
@pytest.mark.parametrize("k", [31, 51])
def test_plain_fastq_on_a_fifo_equals_the_file(k, partitions, inputs, reads, tmp_path):
    want = of_file(inputs, "fastq", k, partitions)
    got = through_fifo(tmp_path, inputs["fastq"][0], PIECE, lambda f: count.count_files(f, k, t=T, threads=1, partitions=partitions))
    same(got, want)
    # a call with a stream has no bound: unless one pass is asked for it packs, and the ranges it is cut into are its own affair
    assert (got[2]["store_bytes"] > 0) == (partitions != 1) and (partitions != 3 or got[2]["used"] == 3)
    assert want[2]["bases"] == sum(len(r) for r in reads)
    if k == 31 and partitions == 0:                              # both sides are the library's: the oracle, once
        keys, cnts, windows = count_oracle.kmer_counts(count_oracle.pad_reads(reads), k)
        packed, c16, hist = count_oracle.table(keys, cnts, k, T)
        assert np.array_equal(got[0].packed, packed) and np.array_equal(got[0].counts, c16) and np.array_equal(got[1], hist)
        assert got[2]["windows"] == windows and got[2]["distinct"] == len(cnts)


@pytest.mark.parametrize("partitions", [0, 1, 3])
@pytest.mark.parametrize("k", [31, 51])
def test_bgzf_fastq_on_a_fifo_equals_the_file(k, partitions, inputs, tmp_path):
    want = of_file(inputs, "bgzf", k, partitions)
    same(want, of_file(inputs, "fastq", k, partitions))
    same(through_fifo(tmp_path, inputs["bgzf"][0], PIECE, lambda f: count.count_files(f, k, t=T, threads=1, partitions=partitions)), want)


@pytest.mark.parametrize("partitions", [0, 1, 3])
@pytest.mark.parametrize("k", [31, 51])
def test_bam_on_a_fifo_equals_the_file_and_is_reported_under_its_path(k, partitions, inputs, tmp_path):
    want = of_file(inputs, "bam", k, partitions)
    count.count_files(inputs["bam"][1], k, t=T, threads=1, partitions=1)
    report = count.bam_report(inputs["bam"][1])
    path = str(fifo(tmp_path, "reads.bam.fifo"))
    same(through_fifo(tmp_path, inputs["bam"][0], PIECE, lambda f: count.count_files(f, k, t=T, threads=1, partitions=partitions), "reads.bam.fifo"), want)
    got = count.bam_report(path)
    assert (got["records"], got["bases"]) == (report["records"], report["bases"]) and got["records"] == 3000 - len(range(5, 3000, 37))
    with pytest.raises(count.CountError):
        count.bam_report(inputs["bam"][1])                        # (the last call read the FIFO, not the file)


@pytest.mark.parametrize("partitions", [0, 1])
@pytest.mark.parametrize("k", [31, 51])
def test_a_dump_on_a_fifo_equals_the_file(k, partitions, inputs, tmp_path):
    name = f"dump{k}"
    want = of_file(inputs, name, k, partitions, dump=True)
    assert want[2]["windows"] == 4500 and want[2]["distinct"] > 3000
    for piece in (7, PIECE):
        same(through_fifo(tmp_path, inputs[name][0], piece, lambda f: count.count_files(f, k, t=T, threads=1, partitions=partitions, dump=True)), want)
    e = refused(tmp_path, inputs[name][0], lambda f: count.count_files(f, k, t=T, partitions=3, dump=True))
    assert e.code == -2 and "partitions = 3 with the dump option" in str(e)


# ---- 2. the store grows -------------------------------------------------------------------------------------------------

def test_the_store_of_a_stream_grows_from_its_first_size(inputs, reads, tmp_path, monkeypatch):
    k, some = 31, fastq_of(reads[:1600])
    assert 190000 < sum(len(r) for r in reads[:1600]) < 210000
    p = tmp_path / "some.fq"
    p.write_bytes(some)
    want = count.count_files(str(p), k, t=T, threads=1)
    monkeypatch.setenv("SMG_COUNT_BATCH_BASES", "8192")
    monkeypatch.setenv("SMG_COUNT_STREAM_STORE", "4096")
    first = count.stream_plan(k, 64 << 30, 0, 0, batch_bases=8192, store_bases=4096)
    assert first == {"cap": 8192 + k, "parted": True, "store_cap": 4096}
    got = through_fifo(tmp_path, some, PIECE, lambda f: count.count_files(f, k, t=T, threads=1))
    same(got, want)
    # every position is in the store, 3 bits each: it grew from 4096 positions to 200 000 and more, by half at a time
    assert got[2]["store_bytes"] >= want[2]["bases"] // 8 * 3 > 40 * (first["store_cap"] // 8 * 3)
    assert got[2]["store_bytes"] < 2 * (want[2]["bases"] + 1600 * (k + 1)) // 8 * 3
    assert got[2]["used"] >= 10                                  # (ranges of one batch of 8192 bases each)


# ---- 3. the seam of the BGZF reader -------------------------------------------------------------------------------------

def member_offsets(data):
    at, out = 0, []
    while at < len(data):
        out.append(at)
        assert data[at + 12:at + 14] == b"BC"
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
    return out


def test_a_member_that_straddles_the_chunk_of_a_bgzf_stream_is_carried_over(inputs, tmp_path):
    fq = inputs["fastq"][0]
    text = fq * (-(-17 * (1 << 20) // len(fq)))                   # 17 MiB and more
    data = bz.bgzf(text, level=0)
    offs = member_offsets(data)
    assert len(data) > count.BGZF_CHUNK + PIECE and count.BGZF_CHUNK not in offs and 2 * count.BGZF_CHUNK > len(data)
    p = tmp_path / "big.fq.gz"
    p.write_bytes(data)
    k = 31
    want = count.count_files(str(p), k, t=T, threads=1, partitions=1)
    got = through_fifo(tmp_path, data, PIECE, lambda f: count.count_files(f, k, t=T, threads=1, partitions=1))
    same(got, want)
    assert got[2]["bases"] == (len(text) // len(fq)) * of_file(inputs, "fastq", k, 1)[2]["bases"]


def test_a_bgzf_stream_that_ends_inside_a_member_or_a_header(inputs, tmp_path):
    data = inputs["bgzf"][0]
    offs = member_offsets(data)
    for cut, what in ((offs[2] + 100, "member"), (offs[3] + 9, "header")):
        at = offs[2] if what == "member" else offs[3]
        e = refused(tmp_path, data[:cut], lambda f: count.count_files(f, 31, t=T, threads=1))
        assert e.code == -4
        assert str(e) == f"smg_count error -4: {tmp_path / 'bad.fifo'}: BGZF block at offset {at}: the {what} is cut off by the end of the stream"


def test_plain_gzip_on_a_fifo_is_refused_with_and_without_the_option(inputs, tmp_path):
    data = gzip.compress(inputs["fastq"][0][:100000])
    e = refused(tmp_path, data, lambda f: count.count_files(f, 31, t=T, gzip=True))
    assert e.code == -2 and str(e) == (f"smg_count error -2: {tmp_path / 'bad.fifo'} is a stream of plain gzip: its restart index reads the file "
                                       "twice; give the file itself, or decompress it in the pipe")
    e = refused(tmp_path, data, lambda f: count.count_files(f, 31, t=T))
    assert e.code == -2 and str(e).endswith("bad.fifo is gzip compressed: compressed input is not supported, decompress it first")


# ---- 4. streams next to files -------------------------------------------------------------------------------------------

def test_a_fifo_and_a_file_and_two_fifos_equal_the_two_files(inputs, tmp_path):
    k = 31
    want = count.count_files([inputs["fastq"][1], inputs["bam"][1]], k, t=T, threads=2)
    a, b = fifo(tmp_path, "a.fifo"), fifo(tmp_path, "b.fifo")
    wa = Writer(a, inputs["fastq"][0], PIECE)
    try:
        got = count.count_files([str(a), inputs["bam"][1]], k, t=T, threads=2)
    finally:
        wa.finish()
    assert wa.error is None
    same(got, want, "a FIFO and a file")
    wa, wb = Writer(a, inputs["fastq"][0], 7001), Writer(b, inputs["bam"][0], PIECE)
    try:
        got = count.count_files([str(a), str(b)], k, t=T, threads=2)
    finally:
        wa.finish()
        wb.finish()
    assert wa.error is None and wb.error is None
    same(got, want, "two FIFOs")
    assert count.bam_report(str(b))["records"] > 0


# ---- 5. the executable --------------------------------------------------------------------------------------------------

def test_the_executable_reads_standard_input_and_leaves_nothing_behind_a_stream_that_fails(inputs, tmp_path):
    fq, path = inputs["fastq"]
    dirs = {}
    for name in ("file", "redirected", "piped", "cut"):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
    args = ["-k31", "-t2", "-e4", "-n", "-oX"]
    r = subprocess.run([count.BIN_PATH, *args, path], cwd=dirs["file"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with open(path, "rb") as f:
        r = subprocess.run([count.BIN_PATH, *args, "-"], cwd=dirs["redirected"], stdin=f, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([count.BIN_PATH, *args, "-"], cwd=dirs["piped"], input=fq, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    smu = (dirs["file"] / "X.smu").read_bytes()
    assert len(smu) > 0 and (dirs["redirected"] / "X.smu").read_bytes() == smu and (dirs["piped"] / "X.smu").read_bytes() == smu
    assert os.listdir(dirs["piped"]) == ["X.smu"]
    data = inputs["bgzf"][0]
    cut = member_offsets(data)[4] + 300
    r = subprocess.run([count.BIN_PATH, "-k31", "-t2", "-e4", "-H", "-oX", "-"], cwd=dirs["cut"], input=data[:cut], capture_output=True, timeout=300)
    assert r.returncode == 1 and b"the member is cut off by the end of the stream" in r.stderr, r.stderr
    assert os.listdir(dirs["cut"]) == []
