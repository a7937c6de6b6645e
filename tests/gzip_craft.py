"""Helper of the plain-gzip tests: the FASTQ text they share, the gzip streams made from it -- by zlib at its levels and
strategies, by hand where a test decides the bits (tests/bgzf_craft.py has the bit writer) -- and the damaged files that must
be refused.  Python's gzip and zlib are the oracle: `streams` gives every file with the text gzip.decompress gives for it."""
import gzip
import random
import struct
import zlib

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
