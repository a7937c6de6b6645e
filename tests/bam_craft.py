"""Helper of the BAM tests: BAM text made field by field, so that a test decides every byte of a record, written as BGZF
through bgzf_craft; and `stripped`, the definition of the stream the counter must make of it."""
import struct

import numpy as np

import bgzf_craft as bz

CODES = b"=ACMGRSVTWYHKDBN"
SEPARATOR = b"\n"
_TO_CODE = bytes(CODES.index(bytes([c]).upper()) if bytes([c]).upper() in CODES else 255 for c in range(256))


def pack_seq(seq):
    """bases -> 4-bit codes, high nibble first; an odd length leaves a low nibble of zero"""
    c = np.frombuffer(seq.translate(_TO_CODE) + b"\0", np.uint8)
    assert c.max() < 16, "a base outside =ACMGRSVTWYHKDBN"
    n = len(seq)
    return (c[0:n:2] << 4 | c[1:n + 1:2]).tobytes()


def record(name, seq, flag=4, qual=None, cigar=(), tags=b"", l_seq=None, block_size=None):
    """one alignment record, block_size in front; name without its NUL; cigar: the uint32 values; l_seq and block_size
    override what the fields give (for records that must be refused)"""
    name = name + b"\0"
    qual = b"\xff" * len(seq) if qual is None else qual
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, len(cigar), flag, len(seq) if l_seq is None else l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", c) for c in cigar) + pack_seq(seq) + qual + tags
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def header(text=b"@HD\tVN:1.6\tSO:unknown\n", refs=()):
    """magic, l_text, text, n_ref, and (name, length) per reference"""
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def bam_text(head, records):
    """records: (name, seq, flag) tuples or bytes made by `record`"""
    return head + b"".join(r if isinstance(r, bytes) else record(r[0], r[1], r[2] if len(r) > 2 else 4) for r in records)


def stripped(records):
    """The stream of (name, seq[, flag]) records: in file order the bases of every record that is neither secondary
    (0x100) nor supplementary (0x800), in the letters of "=ACMGRSVTWYHKDBN", one separator between two of them."""
    kept = []
    for r in records:
        flag = r[2] if len(r) > 2 else 4
        if flag & 0x900 == 0:
            kept.append(r[1].upper())
    return SEPARATOR.join(kept)


def write(path, text, **bgzf_args):
    """the text as a BGZF file (members of 65280 bytes at level 6 unless said otherwise)"""
    with open(path, "wb") as f:
        f.write(bz.bgzf(text, **bgzf_args))
    return str(path)
