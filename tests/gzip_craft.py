"""Helper of the plain-gzip tests: the FASTQ text they share, the gzip streams made from it -- by zlib at its levels and
strategies, by hand where a test decides the bits (tests/bgzf_craft.py has the bit writer) -- and the damaged files that must
be refused.  Python's gzip and zlib are the oracle: `streams` gives every file with the text gzip.decompress gives for it, and
`seam_streams` a second family whose files reach the fixed sizes of the code (the spans of a piece, the ring slots of a decode,
the windows of a slab, the intervals and the text of a call)."""
import functools
import gzip
import random
import struct
import zlib

import numpy as np

import bgzf_craft as bz

SPANS = [1 << 10, 4 << 10, 64 << 10, 1 << 20]                   # the last: larger than every file here


def fastq_text(n=300_000, run=40_000, seed=11):
    """about n bytes of FASTQ with one read in its middle that holds a run of `run` times one base"""
    rng = random.Random(seed)
    out, size, i, long_done = [], 0, 0, False
    while size < n:
        if not long_done and size >= (n - 2 * run) // 2:
            seq = "".join(rng.choice("ACGT") for _ in range(100)) + "A" * run + "".join(rng.choice("ACGT") for _ in range(100))
            long_done = True
        else:
            seq = "".join(rng.choice("ACGTN") if rng.random() < 0.01 else rng.choice("ACGT") for _ in range(rng.randint(30, 150)))
        qual = "".join(rng.choice("I9#F,") if rng.random() < 0.2 else "I" for _ in range(len(seq)))
        out.append(("@read%d\n%s\n+\n%s\n" % (i, seq, qual)).encode())
        size += len(out[-1])
        i += 1
    return b"".join(out)


def het_fastq(seed=3, genome=3000, coverage=30, read=100):
    """reads of two copies of a genome that differ in one base every 150: a table with het-mer pairs"""
    rng = random.Random(seed)
    a = [rng.choice("ACGT") for _ in range(genome)]
    b = list(a)
    for i in range(75, genome, 150):
        b[i] = rng.choice([c for c in "ACGT" if c != a[i]])
    out = []
    for i in range(2 * coverage * genome // read):
        g = a if i % 2 else b
        at = rng.randrange(genome - read)
        out.append("@h%d\n%s\n+\n%s\n" % (i, "".join(g[at:at + read]), "I" * read))
    return "".join(out).encode()


def gz(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, sync_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    if sync_at is None:
        return c.compress(text) + c.flush()
    return c.compress(text[:sync_at]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(text[sync_at:]) + c.flush()


def member(payload, text, flags=0, extra=b"", name=b"", comment=b"", isize=None, crc=None, cm=8):
    """one gzip member around the raw DEFLATE `payload`: the header fields the flags ask for, FHCRC computed"""
    head = struct.pack("<4BI2B", 31, 139, cm, flags, 0, 0, 255)
    if flags & 4:
        head += struct.pack("<H", len(extra)) + extra
    if flags & 8:
        head += name + b"\0"
    if flags & 16:
        head += comment + b"\0"
    if flags & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + payload + struct.pack("<II", (zlib.crc32(text) if crc is None else crc) & 0xFFFFFFFF, (len(text) if isize is None else isize) & 0xFFFFFFFF)


def far_match(seed=5):
    """By hand: 40 000 stored bytes, then dynamic blocks of some 800 bytes each that begin with a match of length 258 at
    distance 32768 -- its source lies in front of the block, so in front of the first block of whichever span the block
    begins -- then literals; a fixed block ends the stream -> (raw DEFLATE, text)"""
    rng = random.Random(seed)
    text = bytearray(rng.choice(b"ACGT\nN") for _ in range(40000))
    w = bz.Bits()
    bz.stored_block(w, bytes(text), final=False)
    lit = [0] * 286
    for s in (65, 67, 71, 84, 10, 78, 256, 285):
        lit[s] = 3                                                  # eight codes of three bits: complete
    dist = [0] * 30
    dist[0] = dist[29] = 1                                          # distances 1 and 24577 .. 32768
    for _ in range(24):
        toks = [(258, 32768)] + [rng.choice(b"ACGT\nN") for _ in range(2000)] + [(258, 1)]
        bz.dynamic_block(w, lit, dist, toks, final=False)
        text = bytearray(bz.expand(toks, bytes(text)))
    toks = [(258, 32768)] + list(b"\nthe end\n")
    bz.fixed_block(w, toks, final=True)
    text = bz.expand(toks, bytes(text))
    return w.done(), text


def streams(text):
    """name -> (the bytes of the gzip file, its text)"""
    out = {}
    for level in (1, 6, 9):
        out[f"level{level}"] = (gz(text, level), text)
    out["fixed"] = (gz(text, 6, zlib.Z_FIXED), text)
    out["stored"] = (gz(text, 0), text)
    out["huffman_only"] = (gz(text, 6, zlib.Z_HUFFMAN_ONLY), text)
    out["rle"] = (gz(text, 6, zlib.Z_RLE), text)
    out["memlevel1"] = (gz(text, 6, mem=1), text)                   # blocks of 128 symbols: many block starts per span
    out["sync_flush"] = (gz(text, 6, sync_at=len(text) // 2 + 123), text)
    half = len(text) // 2
    out["two_members"] = (gz(text[:half], 6) + gz(text[half:], 9), text)
    cuts = [len(text) * i // 49 for i in range(50)]
    parts = [text[a:b] for a, b in zip(cuts, cuts[1:])]
    parts.insert(17, b"")                                           # fifty members, one of them empty
    out["fifty_members"] = (b"".join(gz(p, 1 + i % 9) for i, p in enumerate(parts)), text)
    out["header_fields"] = (member(bz.deflate(text), text, flags=2 | 4 | 8 | 16, extra=bz.subfield(b"XY", b"12345"), name=b"reads.fq",
                                   comment=b"a comment"), text)
    out["trailing_zeros"] = (gz(text, 6) + bytes(1000), text)
    payload, far = far_match()
    out["far_match"] = (member(payload, far), far)
    inner = gzip.compress(text, 6)
    out["gzip_in_gzip"] = (gzip.compress(inner, 0), inner)          # stored blocks that carry valid dynamic block headers
    for name, (data, want) in out.items():
        assert gzip.decompress(data) == want, name
    return out


def damaged(text):
    """name -> (the bytes of the file, the offset its refusal names, a word of the reason)"""
    text = text[:60000]
    good = gz(text, 6)
    raw = bz.deflate(text)
    w = bz.Bits()
    bz.stored_block(w, text[:30000], final=False)
    bz.stored_block(w, text[30000:], final=True)
    stored = bytearray(member(w.done(), text))
    stored[10 + 5 + 1000] ^= 0x04                                   # a text byte of the first stored block
    second = len(good)
    return {
        "cut inside the header": (good[:7], 0, "header is cut off"),
        "cut inside a later header": (good + good[:5], second, "header is cut off"),
        "cut inside a block": (good[:len(good) // 2], None, "end inside a symbol"),
        "cut inside the trailer": (good[:-3], 0, "trailer is cut off"),
        "a flipped text byte in a stored block": (bytes(stored), 0, "CRC-32"),
        "a wrong ISIZE": (member(raw, text, isize=len(text) + 1), 0, "ISIZE"),
        "a wrong ISIZE in the second member": (good + member(raw, text, isize=5), second, "ISIZE"),
        "CM is not 8": (member(raw, text, cm=7), 0, "compression method"),
        "a later member whose CM is not 8": (good + member(raw, text, cm=9), second, "compression method"),
        "trailing bytes that are no member": (good + b"@r\nACGT\n+\nIIII\n", second, "neither zeros nor a gzip member"),
        "zeros and then something": (good + bytes(10) + b"x", second, "neither zeros nor a gzip member"),
    }


# ---- the second family: streams that reach the fixed sizes of smg_gzip.hpp (tests/test_count_gzip_seams_*.py) ---------------

KIB = 1 << 10
PIECE_1K = 256 * KIB                                                # a piece at the smallest span: GZ_MAX_SPANS spans of 1 KiB
TEXT_CAP = 64 << 20                                                 # BGZF_TEXT: the text of one call of the second pass
MAX_EXACT = 4096                                                    # GZ_MAX_EXACT: the restart intervals of one launch
SEAM_NAME, SEAM_COMMENT = b"reads_of_the_seam.fastq", b"a comment, 19 bytes"


def np_fastq(n, seed):
    """about n bytes of random FASTQ, whole records of 30 .. 150 bases, by numpy"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(30, 151, size=n // 60 + 1)
    ends = np.cumsum(lens)
    total = int(ends[-1])
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total)]
    seq = np.where(rng.random(total) < 0.01, np.uint8(ord("N")), seq).tobytes()
    qual = np.where(rng.random(total) < 0.2, np.frombuffer(b"I9#F,", np.uint8)[rng.integers(0, 5, total)], np.uint8(ord("I"))).tobytes()
    out, size, a = [], 0, 0
    for i, b in enumerate(ends.tolist()):
        out.append(b"@r%d\n%s\n+\n%s\n" % (i, seq[a:b], qual[a:b]))
        size += len(out[-1])
        a = b
        if size >= n:
            break
    return b"".join(out)


def runs_text(n):
    """one FASTQ record of n times A with n times I"""
    return b"@r\n" + b"A" * n + b"\n+\n" + b"I" * n + b"\n"


@functools.lru_cache(maxsize=None)
def many_members_parts(prefix=4050, tail=400):
    """[(bytes, text, members)] of the three parts of many_members: `prefix` members of one 30-base record each; one member of 300 000
    bytes at memLevel 1; `tail` members more, one of them empty"""
    rng = np.random.default_rng(23)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 30 * (prefix + tail))].tobytes()
    tiny = [b"@t%d\n%s\n+\n%s\n" % (i, bases[30 * i:30 * i + 30], b"I" * 30) for i in range(prefix + tail)]
    tiny[prefix + tail // 2] = b""
    big = fastq_text(300_000, 1000)
    return ((b"".join(gz(t, 6) for t in tiny[:prefix]), b"".join(tiny[:prefix]), prefix), (gz(big, 6, mem=1), big, 1),
            (b"".join(gz(t, 6) for t in tiny[prefix:]), b"".join(tiny[prefix:]), tail))


def seam_header():
    """the header of the second member of piece_seam: the ten fixed bytes, FNAME, FCOMMENT"""
    return member(b"", b"", flags=8 | 16, name=SEAM_NAME, comment=SEAM_COMMENT)[:-8]


def seam_deltas():
    """where the end of the first piece (at span 1 KiB) falls in piece_seam: name -> delta, the bytes of the second member that
    lie in front of it (negative: bytes of the first member behind it), from the header of the second member as it is crafted"""
    hlen, name_at, comment_at = len(seam_header()), 10, 10 + len(SEAM_NAME) + 1
    return {"inside the trailer of the first member": -4, "a member ends with the piece": 0, "inside the fixed header bytes, 1": 1,
            "inside the fixed header bytes, 5": 5, "inside FNAME": name_at + 10, "inside FCOMMENT": comment_at + 11,
            "the header ends with the piece": hlen, "inside the header of the first dynamic block": hlen + 6,
            "inside the symbols of the first blocks": hlen + 146}


def piece_seam(delta, reads=None):
    """Two members: stored blocks of FASTQ, the member exactly 256 KiB - delta bytes long, then a member with FNAME and FCOMMENT
    around 100 000 bytes of FASTQ at memLevel 1 -> (bytes, text)"""
    reads = np_fastq(400_000, 7) if reads is None else reads
    size = PIECE_1K - delta
    blocks = -(-(size - 18) // (5 + 65535))                         # 10 + n + 5 * blocks + 8 bytes
    n = size - 18 - 5 * blocks
    assert 0 < n <= 65535 * blocks and n > 65535 * (blocks - 1)
    first, w = reads[:n], bz.Bits()
    for i in range(blocks):
        bz.stored_block(w, first[65535 * i:65535 * (i + 1)], final=i == blocks - 1)
    m1 = member(w.done(), first)
    assert len(m1) == size
    second = reads[300_000:400_000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    m2 = member(c.compress(second) + c.flush(), second, flags=8 | 16, name=SEAM_NAME, comment=SEAM_COMMENT)
    assert m2.startswith(seam_header()) and len(seam_header()) == 12 + len(SEAM_NAME) + len(SEAM_COMMENT)
    return m1 + m2, first + second


FULL_SLOTS_BLOCKS = 8 + 3 * 64                                      # one speculative decode and three repairs, every ring slot used


def full_slots(blocks=FULL_SLOTS_BLOCKS):
    """By hand: fixed blocks (no candidates) of 6 literals and 64 matches of 258 at distance 6, 16 518 bytes of text each: at a
    span of 1 KiB, where 16 KiB of text lie between two checkpoints, every block boundary is one, and nothing but its ring slots
    or the final block ends a decode -> (bytes, text)"""
    rng = random.Random(13)
    w, text = bz.Bits(), b""
    for i in range(blocks):
        toks = [rng.choice(b"ACGTN") for _ in range(6)] + [(258, 6)] * 64
        bz.fixed_block(w, toks, final=i == blocks - 1)
        text = bz.expand(toks, text)
        if i == 7:
            assert 10 + len(w.out) + 1 < KIB                        # the eighth boundary lies in the first span: the slots end the decode
    assert len(text) == blocks * 16518 and 16518 >= 16 * KIB
    return member(w.done(), text), text


SEAM_SPANS = {"many_members": [KIB], "two_pieces": [KIB], "runs_small_blocks": [KIB], "runs_fixed": [KIB], "full_slots": [KIB],
              "text_cap": [KIB, 0]}
SEAM_SPANS.update({f"piece_seam: {name}": [KIB] for name in seam_deltas()})


@functools.lru_cache(maxsize=None)
def seam_streams():
    """name -> (the bytes of the gzip file, its text); SEAM_SPANS has the spans at which each one reaches what it is made for
    (0: the default span)"""
    out = {}
    parts = many_members_parts()
    out["many_members"] = (b"".join(p[0] for p in parts), b"".join(p[1] for p in parts))
    two = np_fastq(1_500_000, 5)
    out["two_pieces"] = (gz(two, 6, mem=1), two)
    reads = np_fastq(400_000, 7)
    for name, delta in seam_deltas().items():
        out[f"piece_seam: {name}"] = piece_seam(delta, reads)
    runs = runs_text(3_000_000)
    out["runs_small_blocks"] = (gz(runs, 6, mem=1), runs)
    out["runs_fixed"] = (gz(runs, 6, zlib.Z_FIXED, mem=1), runs)
    out["full_slots"] = full_slots()
    cap = runs_text(35_000_000)
    out["text_cap"] = (gz(cap, 6, mem=1), cap)
    assert set(out) == set(SEAM_SPANS)
    for name, (data, want) in out.items():
        assert gzip.decompress(data) == want, name
    return out


def _far_codes():
    """the code lengths of far_match: A C G T \\n N, the end of a block and length 258 in three bits each; distances 1 and
    24577 .. 32768 in one"""
    lit = [0] * 286
    for s in (65, 67, 71, 84, 10, 78, 256, 285):
        lit[s] = 3
    dist = [0] * 30
    dist[0] = dist[29] = 1
    return lit, dist


def damaged_seams(text):
    """Members with a match of 258 at distance 32768 where fewer than 32768 bytes of the member exist, their ISIZE the length
    the text would have: in the first block of a member, and behind four blocks of 2000 literals each, where at a span of 1 KiB
    a later span begins; each as the first member of a file and behind a good member of 60 000 bytes, whose text the distance
    would land in -> name -> (the bytes of the file, the offset its refusal names, a word of the reason)"""
    rng = random.Random(9)
    lit, dist = _far_codes()

    def literals(n):
        return [rng.choice(b"ACGT\nN") for _ in range(n)]

    def bad_member(blocks_in_front):
        w, n = bz.Bits(), 0
        for _ in range(blocks_in_front):
            bz.dynamic_block(w, lit, dist, literals(2000), final=False)
            n += 2000
        bz.dynamic_block(w, lit, dist, literals(300) + [(258, 32768)] + literals(500), final=False)
        bz.fixed_block(w, list(b"\nthe end\n"), final=True)
        n += 300 + 258 + 500 + 9
        assert n < 32768
        payload = w.done()
        if blocks_in_front:                                         # the block with the match begins behind the first span of 1 KiB
            assert blocks_in_front * 2000 * 3 // 8 > 2 * KIB
        return member(payload, b"", isize=n, crc=0)

    good = gz(text[:60000], 6, mem=1)
    assert gzip.decompress(good) == text[:60000]
    why = "a distance reaches before the start of the member"
    out = {"a far match in the first block of the file": (bad_member(0), 0, why),
           "a far match behind four blocks": (bad_member(4), 0, why),
           "a far match in the first block of a second member": (good + bad_member(0), len(good), why),
           "a far match behind four blocks of a second member": (good + bad_member(4), len(good), why)}
    for name, (data, _, _) in out.items():
        try:
            gzip.decompress(data)
        except Exception:
            continue
        raise AssertionError(f"gzip accepts {name}")
    return out


@functools.lru_cache(maxsize=None)
def one_block_above_the_text_of_a_call(n=270_000):
    """One dynamic block of n matches of 258 at distance 1 behind a literal: more than 64 MiB of text between two restart
    points, which no call of the second pass holds -> (bytes, text)"""
    lit, dist = _far_codes()
    w = bz.Bits()
    bz.dynamic_block(w, lit, dist, [65] + [("D", 258, 0, 0)] * n, final=True)
    text = b"A" * (1 + 258 * n)
    assert len(text) > TEXT_CAP
    data = member(w.done(), text)
    assert gzip.decompress(data) == text
    return data, text
