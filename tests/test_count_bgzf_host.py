"""The BGZF route of the k-mer counter without a GPU: finding the members (smg_count_bgzf_scan), what is refused before a
device is touched, what stays refused as it always was, and the hand-made DEFLATE streams of tests/bgzf_craft.py held
against zlib, so that the GPU tests that use them test what they say.  (`make inflate_check` -- the decoder the kernel
compiles, on the host against zlib under the sanitizers, over 120 000 mutated members -- takes a compiler and ten seconds and
is run by hand like `make reader_check`; profiles/count_bgzf.md keeps its output.)"""
import gzip
import os
import subprocess
import zlib

import pytest

import bgzf_craft as bz
from conftest import ROOT
from smudgeplot_amd import count

FASTQ = b"".join(b"@r%d\nACGTTGCAAGGCTTAACCGGTTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n" % i for i in range(400))


def write(tmp_path, data, name="reads.fq.gz"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_the_binding_has_the_constant_of_the_header():
    text = open(os.path.join(ROOT, "include", "smg_count.h")).read()
    assert "#define SMG_COUNT_BGZF_CHUNK (16 << 20)" in text and count.BGZF_CHUNK == 16 << 20
    assert {"smg_count_bgzf_scan", "smg_count_bgzf_inflate"} <= set(count.EXPORTS)


@pytest.mark.parametrize("members,eof", [(0, True), (1, True), (1, False), (5000, True), (5000, False)])     # (no member and no marker:
def test_scan_counts_blocks_and_text_bytes(members, eof, tmp_path):                                            # an empty plain file)
    text = (FASTQ * 9)[:members * 37]
    assert len(text) == members * 37
    data = bz.bgzf(text, isize=37, level=1, eof=eof)
    got = count.bgzf_scan(write(tmp_path, data))
    assert got == {"blocks": members + (1 if eof else 0), "text_bytes": len(text)}


def test_scan_passes_over_subfields_around_bc(tmp_path):
    before, after = bz.subfield(b"XY", b"12345"), bz.subfield(b"RG") + bz.subfield(b"BC", b"123")     # (a BC that is not of length 2)
    data = bz.bgzf(FASTQ, isize=5000, before=before, after=after)
    assert count.bgzf_scan(write(tmp_path, data)) == {"blocks": 6, "text_bytes": len(FASTQ)}
    data = bz.bgzf(FASTQ, isize=5000, before=after, after=before, eof=False)
    assert count.bgzf_scan(write(tmp_path, data)) == {"blocks": 5, "text_bytes": len(FASTQ)}


def test_scan_accepts_empty_blocks_anywhere_and_an_empty_text(tmp_path):
    m = bz.member(bz.deflate(FASTQ[:3000]), FASTQ[:3000])
    data = bz.EOF_MARKER + m + bz.EOF_MARKER + bz.EOF_MARKER + m
    assert count.bgzf_scan(write(tmp_path, data)) == {"blocks": 5, "text_bytes": 6000}
    assert count.bgzf_scan(write(tmp_path, bz.EOF_MARKER * 3)) == {"blocks": 3, "text_bytes": 0}


def refused(path, call=count.bgzf_scan):
    with pytest.raises(count.CountError) as e:
        call(path)
    return e.value.code, str(e.value)


def test_every_refusal_names_the_offset_of_its_block(tmp_path):
    m1, m2 = (bz.member(bz.deflate(t), t) for t in (FASTQ[:4000], FASTQ[4000:9000]))
    at = len(m1)
    cases = {
        "a later header cut off": (m1 + m2[:11], at, "cut off"),
        "a later header cut off inside its extra field": (m1 + m2[:15], at, "cut off"),
        "the first header cut off": (m1[:10], 0, "cut off"),
        "BSIZE past the end": (m1 + m2[:-1], at, "BSIZE reaches past the end"),
        "ISIZE above 65536": (m1 + m2[:-4] + (65537).to_bytes(4, "little") + bz.EOF_MARKER, at, "ISIZE is above 65536"),
        "a later member that is plain gzip": (m1 + gzip.compress(b"@r\nACGT\n+\nIIII\n"), at, "not a BGZF member"),
        "a later member that is no gzip at all": (m1 + b"@r\nACGT\n+\nIIII\n", at, "not a BGZF member"),
        "BSIZE below header and trailer": (m1 + m2[:16] + (20).to_bytes(2, "little") + m2[18:], at, "BSIZE is smaller"),
    }
    for name, (data, off, why) in cases.items():
        path = write(tmp_path, data)
        code, msg = refused(path)
        assert code == -4 and f"{path}: BGZF block at offset {off}: " in msg and why in msg, (name, msg)


def test_gzip_that_is_not_bgzf_keeps_its_message(tmp_path):
    two = gzip.compress(FASTQ[:2000]) + gzip.compress(FASTQ[2000:4000])
    for data in (gzip.compress(FASTQ), two, b"\x1f\x8b\x08\x00anything"):
        path = write(tmp_path, data)
        for call in (count.bgzf_scan, count.parse):
            code, msg = refused(path, call)
            assert code == -2 and msg.endswith(f"{path} is gzip compressed: compressed input is not supported, decompress it first"), msg
    plain = write(tmp_path, FASTQ, "reads.fq")
    code, msg = refused(plain)
    assert code == -2 and "is not BGZF" in msg
    assert refused(str(tmp_path / "none"))[1].endswith("cannot open " + str(tmp_path / "none"))


def test_parse_refuses_bgzf_and_names_bgzf_inflate(tmp_path):
    path = write(tmp_path, bz.bgzf(FASTQ))
    code, msg = refused(path, count.parse)
    assert code == -2 and "bgzf_inflate" in msg and path in msg


def test_the_executable_still_has_no_z_option(tmp_path):
    r = subprocess.run([count.BIN_PATH, "-z", "x.fq"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1 and "illegal option" in r.stderr


# ---- the hand-made streams against zlib: this keeps the GPU fixtures honest ------------------------------------------

def test_hand_made_valid_streams_inflate_to_the_intended_bytes():
    made = {**bz.match_members(), **bz.dynamic_members()}
    assert len(made) == 19 + 6
    for name, (payload, text) in made.items():
        assert zlib.decompress(payload, -15) == text, name
        bz.member(payload, text)                                 # (fits a block)
    for name, (payload, text) in bz.match_members().items():
        assert len(text) == 65536, name
    w = bz.Bits()
    bz.stored_block(w, b"abc", final=False)
    bz.fixed_block(w, [65, 66, (5, 2), (258, 1)], final=False)
    bz.stored_block(w, b"")
    assert zlib.decompress(w.done(), -15) == b"abc" + bz.expand([65, 66, (5, 2), (258, 1)])


def test_hand_made_invalid_streams_are_rejected_by_zlib_too():
    made = bz.invalid_members()
    assert len(made) == 11
    for name, (payload, isize, crc, reason) in made.items():
        d = zlib.decompressobj(-15)
        try:
            text = d.decompress(payload)
            ok = d.eof and not d.unused_data and len(text) == isize and zlib.crc32(text) == crc
        except zlib.error:
            ok = False
        assert not ok, name
