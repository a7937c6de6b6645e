"""The BAM route of the k-mer counter without a GPU: the framer of the records and the host unpacking (count.bam_text: the
state machine the counting calls feed, in pieces of any size) against bam_craft.stripped, the refusals with their offsets
and reasons, and what stays refused.  (`make bam_check` -- the framer, the tile logic of the unpack kernel compiled for
the host, and mutated texts under the sanitizers -- takes a compiler and is run by hand like `make reader_check`;
profiles/count_bam.md keeps its output.)"""
import gzip
import os
import struct
import subprocess

import pytest

import bam_craft as bc
from conftest import ROOT
from smudgeplot_amd import count

IUPAC = b"=ACMGRSVTWYHKDBN"


def seq_of(n, shift=0):
    return bytes(IUPAC[(i * 7 + shift) % 16] for i in range(n))


LENGTHS = [0, 1, 2, 3, 31, 32, 33]
RECORDS = [(b"r%d" % i, seq_of(n, i)) for i, n in enumerate(LENGTHS)] + [(b"both", IUPAC + IUPAC[::-1] + b"A"), (b"lower", b"acgtn")]


def refused(text, piece=0):
    with pytest.raises(count.CountError) as e:
        count.bam_text(text, piece)
    return e.value.code, str(e.value)


def test_the_binding_has_the_constant_of_the_header():
    text = open(os.path.join(ROOT, "include", "smg_count.h")).read()
    assert "#define SMG_COUNT_BAM_TILE   4096 " in text and count.BAM_TILE == 4096
    assert {"smg_count_bam_text", "smg_count_bam_strip"} <= set(count.EXPORTS)


def test_the_oracle_is_the_stream_of_a_fasta_file_of_the_same_reads(tmp_path):
    recs = RECORDS + [(b"sec", b"ACGT", 0x100), (b"last", b"TTGA", 16)]
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (r[0], r[1].upper()) for r in recs if (r[2] if len(r) > 2 else 4) & 0x900 == 0))
    assert count.parse(str(fa)) == bc.stripped(recs)
    assert bc.pack_seq(b"ACGTN") == bytes([0x12, 0x48, 0xF0])


def test_lengths_and_every_code_in_both_nibbles():
    assert count.bam_text(bc.bam_text(bc.header(), RECORDS)) == bc.stripped(RECORDS)
    for c in range(16):                                           # every code in the high and in the low nibble, next to every other
        recs = [(b"x", bytes([IUPAC[c], IUPAC[d], IUPAC[c]])) for d in range(16)]
        assert count.bam_text(bc.bam_text(bc.header(), recs)) == bc.stripped(recs)
    assert count.bam_text(bc.bam_text(bc.header(), [])) == b""
    assert count.bam_text(bc.bam_text(bc.header(), [(b"e", b"")])) == b""
    assert count.bam_text(bc.bam_text(bc.header(), [(b"e", b""), (b"f", b""), (b"g", b"A")])) == b"\n\nA"


@pytest.mark.parametrize("flag", [0x100, 0x800, 0x900])
def test_secondary_and_supplementary_records_are_skipped(flag):
    skip = lambda i: (b"s%d" % i, seq_of(5 + i, 3), flag | 16)
    for recs in ([RECORDS[2], skip(0), RECORDS[4], skip(1), skip(2), RECORDS[5]],      # between kept records
                 [skip(0)] + RECORDS[:4],                                                # the first record
                 RECORDS[:4] + [skip(0)],                                                # the last record
                 [skip(0), skip(1)],                                                     # nothing else
                 [skip(0), RECORDS[0], skip(1), RECORDS[0], skip(2)]):                   # around empty records
        text = bc.bam_text(bc.header(), recs)
        for piece in (0, 1, 7):
            assert count.bam_text(text, piece) == bc.stripped(recs)
    kept = [(b"k", b"ACGT", f) for f in (0, 4, 16, 0x40 | 0x1, 0x80 | 0x1, 0x400, 0x200, 0x4 | 0x400)]     # every other flag is kept
    assert count.bam_text(bc.bam_text(bc.header(), kept)) == bc.stripped(kept)


@pytest.mark.parametrize("nrefs", [0, 1, 300])
def test_headers_with_references(nrefs):
    refs = [(b"chr%d" % i + b"x" * (i % 9), 1000 + i) for i in range(nrefs)]
    text = bc.bam_text(bc.header(b"@HD\tVN:1.6\n" + b"@SQ\tSN:x\tLN:5\n" * nrefs, refs), RECORDS)
    for piece in (0, 1, 5, 64):
        assert count.bam_text(text, piece) == bc.stripped(RECORDS)
    assert count.bam_text(bc.bam_text(bc.header(b"", refs), RECORDS[:3]), 3) == bc.stripped(RECORDS[:3])


def test_every_piece_size_and_cuts_inside_every_field():
    recs = [(b"read%d" % i, seq_of(n, i)) for i, n in enumerate([33, 0, 1, 32, 2, 31, 3])]
    made = [bc.record(r[0], r[1], cigar=(5 << 4, 3 << 4 | 4), tags=b"RGZgrp\0") for r in recs]
    head = bc.header(refs=((b"chr1", 1000),))
    text, want = head + b"".join(made), bc.stripped(recs)
    for piece in list(range(1, 41)) + [len(text) - 1, len(text), len(text) + 1]:
        assert count.bam_text(text, piece) == want, piece
    # one cut at a chosen place of the 4th record (33 + 1 + 1 bases in front of it): the piece size is that offset
    at = len(head) + sum(len(m) for m in made[:3])
    name, packed = len(recs[3][0]) + 1, (len(recs[3][1]) + 1) // 2
    seq_at = at + 4 + 32 + name + 8
    cuts = {"inside block_size": at + 2, "inside the fixed fields": at + 4 + 17, "inside l_seq": at + 4 + 18, "inside the name": at + 4 + 32 + 2,
            "inside the CIGAR": at + 4 + 32 + name + 5, "at the first seq byte": seq_at, "between the two nibbles' bytes": seq_at + 1,
            "at the last seq byte": seq_at + packed - 1, "at the first quality": seq_at + packed, "inside the qualities": seq_at + packed + 7,
            "inside the tags": at + len(made[3]) - 3, "between two records": at + len(made[3])}
    for what, cut in cuts.items():
        assert count.bam_text(text, cut) == want, what


def test_each_refusal_names_its_offset_and_reason():
    head = bc.header(refs=((b"chr1", 1000),))
    good = bc.record(b"good", b"ACGTACGT")
    at = len(head) + 2 * len(good)

    def case(bad):
        return head + good + good + bad + good

    short = bc.record(b"bad", b"ACGTACGTAC")
    need = struct.unpack("<i", short[:4])[0]
    cases = {
        "l_seq is negative": case(bc.record(b"bad", b"ACGT", l_seq=-1)),
        "block_size is smaller than its name": case(struct.pack("<i", need - 1) + short[4:]),
        "block_size is smaller than the 32 bytes": case(struct.pack("<i", 31) + short[4:]),
        "block_size is smaller than the 32": case(struct.pack("<i", -5) + short[4:]),
    }
    for why, text in cases.items():
        for piece in (0, 1, 13):
            code, msg = refused(text, piece)
            assert code == -4 and f"<text>: BAM record at text offset {at}: " in msg and why in msg, (why, msg)
    assert count.bam_text(case(struct.pack("<i", need) + short[4:])) == b"\n".join([b"ACGTACGT"] * 2 + [b"ACGTACGTAC", b"ACGTACGT"])
    # an l_seq that the block cannot hold is refused before anything of it is unpacked, however large it claims to be
    code, msg = refused(case(bc.record(b"bad", b"ACGT", l_seq=0x7fffffff)))
    assert code == -4 and f"offset {at}: block_size is smaller" in msg
    headers = {
        "l_text is negative": b"BAM\1" + struct.pack("<i", -1) + head[8:],
        "n_ref is negative": bc.header(refs=())[:-4] + struct.pack("<i", -2),
        "l_name is negative": bc.header(refs=())[:-4] + struct.pack("<ii", 1, -3) + b"chr1\0" + struct.pack("<i", 5),
        "the magic": b"BAM\2" + head[4:],
    }
    for why, h in headers.items():
        for piece in (0, 1):
            code, msg = refused(h + good, piece)
            assert code == -4 and "<text>: BAM header: " in msg and why in msg, (why, msg)
    whole = head + good + good
    for cut in range(len(whole)):
        if cut in (len(head), len(head) + len(good)):
            assert count.bam_text(whole[:cut]) == bc.stripped([(b"", b"ACGTACGT")] * ((cut - len(head)) // len(good)))
            continue
        code, msg = refused(whole[:cut], 11)
        if cut < len(head):
            assert code == -4 and "<text>: BAM header: the file ends inside the header" in msg, (cut, msg)
        else:
            rec = len(head) + (cut - len(head)) // len(good) * len(good)
            assert code == -4 and f"<text>: BAM record at text offset {rec}: the file ends inside the record" in msg, (cut, msg)


def test_parse_still_refuses_a_bam_file_and_names_bgzf_inflate(tmp_path):
    path = bc.write(tmp_path / "reads.bam", bc.bam_text(bc.header(), RECORDS))
    with pytest.raises(count.CountError) as e:
        count.parse(path)
    assert e.value.code == -2 and "bgzf_inflate" in str(e.value) and path in str(e.value)
    assert count.bgzf_scan(path)["text_bytes"] == len(bc.bam_text(bc.header(), RECORDS))


@pytest.mark.parametrize("name,root", [("reads.bam", "reads"), ("m84.hifi_reads.BAM", "m84.hifi_reads"), ("reads.bam.gz", "reads"),
                                        ("reads.fq.gz", "reads"), ("reads.cram", "reads.cram")])
def test_the_default_root_strips_the_bam_suffix(name, root, tmp_path):
    """through the report of a run that is refused before it needs a device: the file is gzip, but not BGZF"""
    (tmp_path / name).write_bytes(gzip.compress(b"@r\nACGT\n+\nIIII\n"))
    r = subprocess.run([count.BIN_PATH, "-v", name], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "is gzip compressed" in r.stderr
    assert f"nothing was written under the root name {root}\n" in r.stderr
    assert sorted(os.listdir(tmp_path)) == [name]
    quiet = subprocess.run([count.BIN_PATH, name], cwd=tmp_path, capture_output=True, text=True)
    assert quiet.returncode == 1 and "root name" not in quiet.stderr


def test_the_usage_names_bam(tmp_path):
    r = subprocess.run([count.BIN_PATH], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "unaligned BAM" in r.stderr
