"""The BAM route of the k-mer counter on the GPU: the unpack kernel byte by byte through count.bam_strip (the oracle is
bam_craft.stripped, which tests/test_count_bam_host.py holds against the FASTA parser) at the seams of its tiles and of the
inflate calls, counting from BAM files against the FASTA run and tests/count_oracle.py, and the refusals on the device
route, which `make bam_check` has explored on the CPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_craft as bc
import bgzf_craft as bz
import count_oracle
from smudgeplot_amd import count

pytestmark = pytest.mark.gpu

T = count.BAM_TILE
IUPAC = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)


def bases(rng, n, letters=IUPAC):
    return rng.choice(letters, n).tobytes()


def same_stream(got, want, what):
    if got != want:
        n = min(len(got), len(want))
        a, b = np.frombuffer(got[:n], np.uint8), np.frombuffer(want[:n], np.uint8)
        diff = np.nonzero(a != b)[0]
        at = int(diff[0]) if len(diff) else n
        raise AssertionError(f"{what}: first difference at offset {at} of {len(want)} (got {len(got)} bytes): "
                             f"{got[max(at - 8, 0):at + 8]!r} / {want[max(at - 8, 0):at + 8]!r}")


# ---- 1. tile seams --------------------------------------------------------------------------------------------------------

def seam_set(name, rng):
    if name == "every length 0..70":
        return [bases(rng, n) for n in range(71)]
    if name == "lengths around the tile":
        return [bases(rng, n + odd) for n in (T - 1, T, T + 1, 3 * T + 5) for odd in (0, 1)] + [bases(rng, T - 1)]
    if name == "5000 empty records":
        return [bases(rng, 3)] + [b""] * 5000 + [bases(rng, 2)]
    if name == "one long read":
        return [bases(rng, 1), bases(rng, 300001), bases(rng, 1)]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["every length 0..70", "lengths around the tile", "5000 empty records", "one long read"])
def test_tile_seams_at_every_alignment_of_the_seq_field(name, tmp_path):
    rng = np.random.default_rng(3)
    seqs = seam_set(name, rng)
    for l_name in range(1, 17):                                   # (the NUL counts: the seq field moves by one byte each time)
        recs = [(b"n" * (l_name - 1), s) for s in seqs]
        path = bc.write(tmp_path / f"seam{l_name}.bam", bc.bam_text(bc.header(), recs), isize=65280, level=6)
        got, records, ms = count.bam_strip(path)
        same_stream(got, bc.stripped(recs), f"{name}, l_read_name {l_name}")
        assert records == len(recs) and ms > 0


def test_skipped_records_between_the_tiles(tmp_path):
    rng = np.random.default_rng(4)
    recs = [(b"r%d" % i, bases(rng, int(rng.integers(0, 900))), int(rng.choice([4, 0, 16, 0x100, 0x800, 0x904]))) for i in range(400)]
    got, records, _ = count.bam_strip(bc.write(tmp_path / "mixed.bam", bc.bam_text(bc.header(refs=((b"chr1", 5),)), recs), sizes=[1, 37, 4099]))
    same_stream(got, bc.stripped(recs), "mixed flags")
    assert records == sum(1 for r in recs if r[2] & 0x900 == 0)


def test_what_is_not_bam_is_refused_by_bam_strip(tmp_path):
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(bz.bgzf(b"@r\nACGT\n+\nIIII\n"))
    for path, why in ((fq, "is not BAM"), (tmp_path / "plain.fa", "is not BGZF")):
        if not path.exists():
            path.write_bytes(b">r\nACGT\n")
        with pytest.raises(count.CountError) as e:
            count.bam_strip(str(path))
        assert e.value.code == -2 and why in str(e.value)


# ---- 2. the seam between two inflate calls -----------------------------------------------------------------------------------

MEMBERS, MEMBER = 65536 + 50, 20
SEAM = 65536 * MEMBER                                             # an inflate call takes at most 65536 members
NAME = b"read"                                                   # l_read_name 5: block_size 4, fixed 32, name 5, then the seq field


def seam_file(l_seq, into):
    """records such that text offset SEAM lies `into` bytes behind the start (the block_size field) of a record of l_seq
    bases; the text is MEMBERS * MEMBER bytes exactly"""
    rng = np.random.default_rng(l_seq + into)
    head = bc.header()
    start, size, recs, made = SEAM - into, len(head), [], []

    def add(seq, tags=b""):
        recs.append((NAME, seq))
        made.append(bc.record(NAME, seq, tags=tags))
        return len(made[-1])

    unit = len(bc.record(NAME, b"A" * 150))
    while size + 2 * unit + 64 <= start:
        size += add(bases(rng, 150))
    size += add(bases(rng, 150), tags=b"t" * (start - size - unit))        # the record in front of the seam fills up to it
    assert size == start
    size += add(bases(rng, l_seq))
    total = MEMBERS * MEMBER
    while size + 2 * unit + 64 <= total:
        size += add(bases(rng, 150))
    size += add(bases(rng, 150), tags=b"t" * (total - size - unit))
    assert size == total
    return head + b"".join(made), recs


SEAMS = {"inside block_size": (200, 2), "inside the fixed fields": (200, 4 + 17), "in the middle of an even seq field": (200, 41 + 50),
         "in the middle of an odd seq field": (201, 41 + 51), "inside the qualities": (200, 41 + 100 + 7), "between two records": (200, 0)}


@pytest.mark.parametrize("where", sorted(SEAMS))
def test_the_seam_between_two_inflate_calls(where, tmp_path):
    l_seq, into = SEAMS[where]
    text, recs = seam_file(l_seq, into)
    path = bc.write(tmp_path / "seam.bam", text, isize=MEMBER, level=6)
    # on the CPU, before the device sees it: the file is what it was built to be
    assert count.bgzf_scan(path) == {"blocks": MEMBERS + 1, "text_bytes": MEMBERS * MEMBER}
    at = SEAM - into
    assert struct.unpack_from("<i", text, at + 4 + 16)[0] == l_seq and text[at + 4 + 32:at + 4 + 32 + 5] == NAME + b"\0"
    got, records, _ = count.bam_strip(path)
    same_stream(got, bc.stripped(recs), where)
    assert records == len(recs)


# ---- 4. counting --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reads():
    rng = np.random.default_rng(9)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 200000)
    other = genome.copy()                                         # a second haplotype: a substitution every 997 bases
    other[100::997] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), other[100::997])]
    out = []
    for i in range(20000):
        n = int(rng.integers(50, 301))
        a = int(rng.integers(0, 200000 - n))
        r = (genome if i % 4 < 2 else other)[a:a + n].tobytes()
        if i % 2:
            r = r.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
        if i % 97 == 0:
            r = r[:20] + b"N" + r[21:]
        out.append((b"m%d/ccs" % i, r, 4 if i % 50 else 0x800 | 16))      # (a few supplementary records: not counted)
    return out


@pytest.fixture(scope="module")
def inputs(reads, tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_counting")
    kept = [r for r in reads if r[2] & 0x900 == 0]
    third = len(reads) // 3
    parts = [reads[:third], reads[third:2 * third], reads[2 * third:]]
    fq = lambda rs: b"".join(b"@%s\n%s\n+\n%s\n" % (r[0], r[1], b"I" * len(r[1])) for r in rs if r[2] & 0x900 == 0)
    files = {"bam": bz.bgzf(bc.bam_text(bc.header(), reads)), "fa": b"".join(b">%s\n%s\n" % (r[0], r[1]) for r in kept),
             "bam0": bz.bgzf(bc.bam_text(bc.header(), parts[0])), "fq1": fq(parts[1]), "fqz2": bz.bgzf(fq(parts[2]))}
    paths = {}
    for name, data in files.items():
        paths[name] = str(d / {"bam": "reads.bam", "fa": "reads.fa", "bam0": "part0.bam", "fq1": "part1.fq", "fqz2": "part2.fq.gz"}[name])
        open(paths[name], "wb").write(data)
    return paths


_ORACLE = {}


def oracle(reads, k, t):
    if k not in _ORACLE:
        stream = bc.stripped(reads)
        keys, cnts, _ = count_oracle.kmer_counts(count_oracle.pad_reads(stream.split(bc.SEPARATOR)), k)
        _ORACLE[k] = (keys, cnts)
    return count_oracle.table(*_ORACLE[k], k, t)


def same(got, want_packed, want_counts, want_hist):
    table, hist, _ = got
    assert np.array_equal(table.packed, want_packed) and np.array_equal(table.counts, want_counts) and np.array_equal(hist, want_hist)


@pytest.mark.parametrize("t", [1, 4])
@pytest.mark.parametrize("k", [31, 51])
def test_counting_from_bam_equals_the_fasta_run_and_the_oracle(k, t, reads, inputs):
    got = count.count_files(inputs["bam"], k, t=t, threads=1)
    same(got, *oracle(reads, k, t))
    fa = count.count_files(inputs["fa"], k, t=t, threads=1)
    same(got, fa[0].packed, fa[0].counts, fa[1])
    assert got[2]["bases"] == fa[2]["bases"] == sum(len(r[1]) for r in reads if r[2] & 0x900 == 0)


def test_a_bam_a_fastq_and_a_bgzf_fastq_in_one_call(reads, inputs):
    got = count.count_files([inputs["bam0"], inputs["fq1"], inputs["fqz2"]], 31, t=1, threads=3)
    fa = count.count_files(inputs["fa"], 31, t=1, threads=1)
    same(got, fa[0].packed, fa[0].counts, fa[1])
    parted = count.count_files([inputs["fqz2"], inputs["bam0"], inputs["fq1"]], 31, t=1, threads=2, partitions=3)
    assert parted[2]["used"] == 3
    same(parted, fa[0].packed, fa[0].counts, fa[1])


def test_reads_to_plot_from_bam_equals_reads_to_plot_from_fasta(inputs):
    a, ha, _ = count.reads_to_plot(inputs["bam"], 31, 2, 2)
    b, hb, _ = count.reads_to_plot(inputs["fa"], 31, 2, 2)
    assert np.array_equal(a, b) and np.array_equal(ha, hb) and a.sum() > 0


def test_the_executable_reads_bam_and_names_its_output_after_the_reads(reads, inputs, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    (a / "reads.fa").write_bytes(open(inputs["fa"], "rb").read())
    (b / "reads.bam").write_bytes(open(inputs["bam"], "rb").read())
    for d, name in ((a, "reads.fa"), (b, "reads.bam")):
        r = subprocess.run([count.BIN_PATH, "-k31", "-t2", "-H", "-v", "-osample", name], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        if name.endswith(".bam"):
            kept = [x for x in reads if x[2] & 0x900 == 0]
            assert "reads.bam: BGZF, " in r.stderr
            assert f"reads.bam: BAM, {len(kept)} records, {sum(len(x[1]) for x in kept)} bases, unpacked on the device" in r.stderr
    for name in ("sample.ktab", ".sample.ktab.1", "sample.hist.txt"):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    r = subprocess.run([count.BIN_PATH, "-k31", "-t4", "-H", "reads.bam"], cwd=b, capture_output=True, text=True)      # the default root
    assert r.returncode == 0 and (b / "reads.ktab").exists() and (b / "reads.hist.txt").exists(), r.stderr


# ---- 5. refusals on the device route ----------------------------------------------------------------------------------------

def refusal_files():
    rng = np.random.default_rng(6)
    recs = [(b"r%d" % i, bases(rng, 100 + i)) for i in range(12)]
    made = [bc.record(*r) for r in recs]
    head = bc.header()
    first = len(head) + sum(len(m) for m in made[:4])             # the 2nd member begins with the 5th record
    bad = list(made)
    need = struct.unpack("<i", made[6][:4])[0] - len(recs[6][1])  # without its qualities: too small for its l_seq
    bad[6] = struct.pack("<i", need) + made[6][4:]
    at = len(head) + sum(len(m) for m in made[:6])
    good = head + b"".join(made)
    small = bz.bgzf(head + b"".join(bad), sizes=[first, 65280])
    cut = bz.bgzf(good[:-9], sizes=[first, 65280])
    last = len(head) + sum(len(m) for m in made[:11])
    members = [bz.member(bz.deflate(good[:first]), good[:first]), bz.member(bz.deflate(good[first:]), good[first:], crc=0x12345678)]
    crc = b"".join(members) + bz.EOF_MARKER
    return {"block_size": (small, f"BAM record at text offset {at}: block_size is smaller"),
            "cut": (cut, f"BAM record at text offset {last}: the file ends inside the record"),
            "crc": (crc, f"BGZF block at offset {len(members[0])}: the CRC-32 of the text")}, bz.bgzf(good), recs


@pytest.mark.parametrize("name", ["block_size", "cut", "crc"])
def test_a_bad_bam_file_is_refused_and_a_later_run_succeeds(name, inputs, tmp_path):
    files, good, recs = refusal_files()
    data, message = files[name]
    d = tmp_path / "run"
    d.mkdir()
    path = d / "bad.bam"
    path.write_bytes(data)
    for call in (lambda: count.bam_strip(str(path)), lambda: count.count_files([inputs["fq1"], str(path)], 21, t=1, threads=2)):
        with pytest.raises(count.CountError) as e:
            call()
        assert e.value.code == -4 and f"{path}: {message}" in str(e.value), str(e.value)
    r = subprocess.run([count.BIN_PATH, "-k21", "-t1", "-H", "bad.bam"], cwd=d, capture_output=True, text=True)
    assert r.returncode == 1 and message in r.stderr
    assert sorted(os.listdir(d)) == ["bad.bam"]
    ok = tmp_path / "good.bam"
    ok.write_bytes(good)
    got, records, _ = count.bam_strip(str(ok))                    # valid runs afterwards, same process
    assert got == bc.stripped(recs) and records == len(recs)
    keys, cnts, _ = count_oracle.kmer_counts(count_oracle.pad_reads([r[1] for r in recs]), 21)
    same(count.count_files(str(ok), 21, t=1, threads=1), *count_oracle.table(keys, cnts, 21, 1))


# ---- 6. the report of the last call that read BAM -------------------------------------------------------------------------

def report_files(d):
    """two small BAM files with different records (one of b's is secondary: not counted) and a FASTQ"""
    rng = np.random.default_rng(12)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = [(b"a%d" % i, bases(rng, 40 + i, acgt)) for i in range(3)]
    b = [(b"b%d" % i, bases(rng, 55 + 2 * i, acgt), 0x100 if i == 1 else 4) for i in range(4)]
    fq = d / "reads.fq"
    fq.write_bytes(b"@r\n%s\n+\n%s\n" % (bases(rng, 60, acgt), b"I" * 60))
    paths = {"a": bc.write(d / "a.bam", bc.bam_text(bc.header(), a)), "b": bc.write(d / "b.bam", bc.bam_text(bc.header(), b)), "fq": str(fq)}
    want = {n: {"records": sum(1 for r in rs if len(r) < 3 or r[2] & 0x900 == 0), "bases": len(bc.stripped(rs).replace(bc.SEPARATOR, b""))}
            for n, rs in (("a", a), ("b", b))}
    assert want == {"a": {"records": 3, "bases": 123}, "b": {"records": 3, "bases": 175}}
    return paths, want


def reported(path, want):
    r = count.bam_report(path)
    assert {n: r[n] for n in ("records", "bases")} == want, r
    times = [r[n] for n in ("ms_frame", "ms_inflate", "ms_unpack", "ms_d2h")]
    assert all(isinstance(t, float) and t >= 0 for t in times), r


def not_reported(path):
    with pytest.raises(count.CountError) as e:
        count.bam_report(path)
    assert e.value.code == -2


def test_bam_report_after_bam_strip(tmp_path):
    paths, want = report_files(tmp_path)
    count.bam_strip(paths["a"])
    reported(paths["a"], want["a"])
    not_reported(paths["b"])
    not_reported(str(tmp_path / "never_read.bam"))
    count.bam_strip(paths["b"])                                   # the last call alone is reported
    reported(paths["b"], want["b"])
    not_reported(paths["a"])


def test_bam_report_after_counting_calls(tmp_path):
    paths, want = report_files(tmp_path)
    count.count_files([paths["a"], paths["fq"], paths["b"]], 21, t=1, threads=2)
    reported(paths["a"], want["a"])
    reported(paths["b"], want["b"])
    not_reported(paths["fq"])
    count.count_files([paths["fq"]], 21, t=1, threads=1)          # a call that read no BAM: the report is gone
    not_reported(paths["a"])
    not_reported(paths["b"])


def test_bam_report_keeps_the_files_read_before_a_failure(tmp_path):
    paths, want = report_files(tmp_path)
    bad = bc.write(tmp_path / "bad.bam", bc.bam_text(bc.header(), [bc.record(b"r0", b"ACGT"), bc.record(b"r1", b"ACGT", block_size=10)]))
    with pytest.raises(count.CountError) as e:
        count.count_files([paths["a"], bad], 21, t=1, threads=1)
    assert e.value.code == -4 and "block_size is smaller" in str(e.value)
    reported(paths["a"], want["a"])
    not_reported(bad)
