"""Helper of the BGZF tests: a BGZF writer over zlib's raw deflate, and a bit writer that emits DEFLATE by hand (stored
blocks, fixed-Huffman blocks from tokens, dynamic blocks from given code lengths), so that a test decides every bit of a
member.  `expand` is the text a token list stands for; the host tests hold every hand-made stream against zlib."""
import struct
import zlib

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_ISIZE = 65536


class BsizeError(AssertionError):
    """the member does not fit the 16 bits of BSIZE"""


def subfield(si, data=b""):
    return si + struct.pack("<H", len(data)) + data


def member(payload, text=None, isize=None, crc=None, before=b"", after=b""):
    """one BGZF member around the raw DEFLATE `payload`; ISIZE and CRC-32 are those of `text` unless given; `before` and
    `after` are extra subfields around BC"""
    total = 12 + len(before) + 6 + len(after) + len(payload) + 8
    if total - 1 > 0xFFFF:
        raise BsizeError(f"a member of {total} bytes")
    extra = before + b"BC" + struct.pack("<HH", 2, total - 1) + after
    head = struct.pack("<4BI2BH", 31, 139, 8, 4, 0, 0, 255, len(extra))
    isize = len(text) if isize is None else isize
    crc = zlib.crc32(text) if crc is None else crc
    return head + extra + payload + struct.pack("<II", crc & 0xFFFFFFFF, isize)


def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, full_flush_at=None):
    """raw DEFLATE of text; full_flush_at: a Z_FULL_FLUSH (an empty stored block) after that many bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if full_flush_at is None:
        return c.compress(text) + c.flush()
    return c.compress(text[:full_flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[full_flush_at:]) + c.flush()


def bgzf(text, isize=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True, before=b"", after=b"", sizes=None):
    """text cut into members of `isize` bytes (or of the given sizes, in turn, the last repeated) -> the bytes of the file"""
    out, at, i = [], 0, 0
    while at < len(text):
        n = isize if sizes is None else sizes[min(i, len(sizes) - 1)]
        piece = text[at:at + n]
        out.append(member(deflate(piece, level, strategy), piece, before=before, after=after))
        at += n
        i += 1
    return b"".join(out) + (EOF_MARKER if eof else b"")


# ---- DEFLATE by hand ------------------------------------------------------------------------------------------------

class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """a number, least significant bit first"""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        """a Huffman code, most significant bit first"""
        for b in range(nbits - 1, -1, -1):
            self.put((code >> b) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
          16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def length_symbol(n):
    i = max(j for j in range(29) if _LBASE[j] <= n) if n < 258 else 28
    return 257 + i, n - _LBASE[i], _LEXT[i]


def distance_symbol(d):
    i = max(j for j in range(30) if _DBASE[j] <= d)
    return i, d - _DBASE[i], _DEXT[i]


def canonical(lens):
    """code lengths -> {symbol: (code, length)} of the canonical Huffman code"""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def _tokens(w, tokens, lit, dist):
    """tokens: an int is a literal, (length, distance) a match, ("L", symbol) a raw literal/length symbol without extra
    bits, ("D", length, symbol, extra) a length followed by a raw distance symbol and its extra bits value"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "L":
            w.code(*lit[t[1]])
        else:
            n = t[1] if t[0] == "D" else t[0]
            s, v, x = length_symbol(n)
            w.code(*lit[s])
            w.put(v, x)
            if t[0] == "D":
                w.code(*dist[t[2]])
                w.put(t[3], _DEXT[t[2]] if t[2] < 30 else 0)
            else:
                s, v, x = distance_symbol(t[1])
                w.code(*dist[s])
                w.put(v, x)
    w.code(*lit[256])


def stored_block(w, data, final=True, nlen=None):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    w.out += data


def fixed_block(w, tokens, final=True):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    _tokens(w, tokens, FIXED_LIT, FIXED_DIST)


# a complete code for the 19 code-length symbols: 13 of 4 bits, 6 of 5 bits
_CLC_LENS = [4] * 13 + [5] * 6
_CLC_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_block(w, lit_lens, dist_lens, tokens, runs=None, final=True, clc_lens=None):
    """lit_lens (257 .. 286 lengths) and dist_lens (1 .. 30): the code lengths; runs: how their one sequence is coded, a list of
    lengths 0 .. 15 and (16, n) / (17, n) / (18, n) repeats (default: every length by itself); clc_lens: the lengths of the
    code-length code (default: a complete one over all 19 symbols)"""
    seq = list(lit_lens) + list(dist_lens)
    runs = seq if runs is None else runs
    flat = []
    for r in runs:
        if isinstance(r, int):
            flat.append(r)
        elif r[0] == 16:
            flat += [flat[-1]] * r[1]
        else:
            flat += [0] * r[1]
    assert flat == seq, "the runs do not spell the code lengths"
    clc_lens = _CLC_LENS if clc_lens is None else clc_lens
    clc = canonical(clc_lens)
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(len(lit_lens) - 257, 5)
    w.put(len(dist_lens) - 1, 5)
    w.put(19 - 4, 4)
    for s in _CLC_ORDER:
        w.put(clc_lens[s], 3)
    for r in runs:
        if isinstance(r, int):
            w.code(*clc[r])
        else:
            w.code(*clc[r[0]])
            w.put(r[1] - (11 if r[0] == 18 else 3), {16: 2, 17: 3, 18: 7}[r[0]])
    _tokens(w, tokens, canonical(lit_lens), canonical(dist_lens))


def expand(tokens, text=b""):
    """the text a token list of literals and (length, distance) matches stands for, behind `text`"""
    out = bytearray(text)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= len(out) and d <= 32768
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                for _ in range(n):
                    out.append(out[-d])
    return bytes(out)


# ---- the hand-made members the host and the GPU tests share: name -> (payload, text) or, invalid, (payload, isize, crc, reason) ---

def match_members():
    """Fixed-code members of 65536 bytes: every length 3 .. 258 at each of the distances, overlapping copies included, and
    copies whose source and whose destination straddle the text offsets 32768 and 65535 -> {name: (payload, text)}"""
    import random
    out = {}
    for d in (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 258, 259, 4095, 4096, 4097, 32767, 32768):
        for half in ((0, 1) if d >= 32767 else (None,)):
            rng = random.Random(d)
            toks = [rng.choice(b"ACGTN\n@+I#") for _ in range(300)]
            text = bytearray(bytes(toks))

            def add(n, dist):
                toks.append((n, dist))
                text.extend(expand([(n, dist)], bytes(text[-32768:]))[min(len(text), 32768):])

            def fill(upto):                                  # copies of varied length and distance up to that offset
                while len(text) < upto:
                    n = min(258, upto - len(text))
                    if n < 3:
                        for _ in range(n):
                            toks.append(65 + len(text) % 7)
                            text.append(toks[-1])
                        break
                    if upto - len(text) - n in (1, 2):
                        n -= 3
                    add(n, rng.choice([1, 5, 64, 200, min(len(text), 3000), min(len(text), 32768)]))

            fill(min(d, 32768 - 129) if d > 300 else 300)
            if len(text) < d:
                fill(32768 - 129)
                add(258, min(d, len(text)))                   # the destination straddles 32768
                fill(d)
            lengths = [n for n in range(3, 259) if half is None or n % 2 == half]
            for n in lengths:
                if len(text) < 32768 - 129 <= len(text) + n:
                    fill(32768 - 129)
                    add(258, min(d, len(text)))
                add(n, d)
            if len(text) < 32768 - 129:
                fill(32768 - 129)
                add(258, min(d, len(text)))
            if len(text) < 32768 + 200:
                fill(32768 + 200)
                add(258, 329)                                 # the source straddles 32768
            fill(65536 - 258)
            add(258, d)                                       # the destination ends at 65535 (d = 32768: the source at 32767)
            assert len(text) == 65536
            w = Bits()
            fixed_block(w, toks)
            out[f"d{d}" + ("" if half is None else f"_{half}")] = (w.done(), bytes(text))
    return out


def dynamic_members():
    """hand-made dynamic blocks -> {name: (payload, text)}"""
    out = {}
    # a 15-bit code: lengths 1, 2, .. 14, 15, 15 over 16 literal/length symbols (a complete code), among them 256
    lit = [0] * 257
    syms = [65, 67, 71, 84, 10, 78, 97, 99, 103, 116, 110, 64, 43, 73, 35, 256]
    for s, n in zip(syms, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]):
        lit[s] = n
    toks = [s for s in syms[:-1] for _ in range(3)]
    w = Bits()
    dynamic_block(w, lit, [1, 1], toks)
    out["fifteen_bit_code"] = (w.done(), expand(toks))
    # HLIT = 257 and HDIST = 1 with a single distance code (of length 1: an incomplete set that is allowed)
    lit = [0] * 257
    for s in (65, 67, 71, 84):
        lit[s] = 3
    lit[10], lit[256], lit[78] = 3, 3, 2
    toks = [65, 67, 71, 84, 10, 78] * 4
    w = Bits()
    dynamic_block(w, lit, [1], toks)
    out["hlit257_hdist1"] = (w.done(), expand(toks))
    # a single distance code that is used: distance symbol 0 only, so every match is at distance 1
    lit2 = [0] * 286
    for s in (65, 67, 71, 84):
        lit2[s] = 3
    lit2[10], lit2[256], lit2[285], lit2[257] = 3, 3, 3, 3
    toks = [65, (258, 1), 67, (3, 1), 71, 84, 10]
    w = Bits()
    dynamic_block(w, lit2, [1], toks)
    out["single_distance_code"] = (w.done(), expand(toks))
    # repeat code 16 carries the last literal/length length (symbol 285, length 3) into the first three distance lengths
    w = Bits()
    runs = lit2[:285] + [3, (16, 3), 3, 3, 3, 3, 3]
    dist = [3] * 8
    toks = [65, 67, 71, 84, 10, (258, 1), (3, 5), (258, 7), (3, 2), (258, 3), (3, 4), (258, 6), (258, 8)]
    dynamic_block(w, lit2, dist, toks, runs=runs)
    out["repeat16_across_the_seam"] = (w.done(), expand(toks))
    # 17 and 18 across the same seam: the zeros behind the last literal/length code go on into the distance lengths
    lit3 = list(lit2[:258]) + [0] * 12                          # 270 lengths, the last 12 zero
    lit3[257] = 3
    lit3[285 - 28] = 3
    for s, n in ((65, 3), (67, 3), (71, 3), (84, 3), (10, 3), (256, 3), (257, 3)):
        lit3[s] = n
    lit3[78] = 3                                                # eight codes of three bits: complete
    dist3 = [0] * 8 + [1, 1]                                    # distance symbols 8 and 9: 17 .. 32
    toks = [65, 67, 71, 84, 10, 78] * 4 + [(3, 17), (3, 24), (3, 25), (3, 32)]
    for name, zeros in (("repeat17_across_the_seam", [(17, 10), (17, 10)]), ("repeat18_across_the_seam", [(18, 20)])):
        w = Bits()
        dynamic_block(w, lit3, dist3, toks, runs=lit3[:258] + zeros + [1, 1])
        out[name] = (w.done(), expand(toks))
    return out


def invalid_members():
    """hand-made members that must be refused -> {name: (payload, isize, crc, reason the library gives)}; the text the
    trailer describes is TEXT"""
    text = TEXT
    crc = zlib.crc32(text)
    out = {}

    def stored(data, **kw):
        w = Bits()
        stored_block(w, data, **kw)
        return w.done()

    flipped = bytearray(stored(text))
    flipped[5 + 100] ^= 0x04
    out["payload_bit_in_a_stored_member"] = (bytes(flipped), len(text), crc, "CRC-32")
    out["crc_field_changed"] = (stored(text), len(text), crc ^ 0x00010000, "CRC-32")
    out["isize_one_too_small"] = (deflate(text), len(text) - 1, crc, "more text than ISIZE")
    out["isize_one_too_large"] = (deflate(text), len(text) + 1, crc, "less text than ISIZE")
    out["nlen_wrong"] = (stored(text, nlen=len(text) ^ 0xFFFE), len(text), crc, "stored block")
    w = Bits()
    w.put(1, 1); w.put(3, 2); w.put(0, 13)
    out["block_type_3"] = (w.done() + text, len(text), crc, "block type 3")
    w = Bits()
    lit = [0] * 257
    for s in (65, 67, 71, 84, 256):
        lit[s] = 2                                              # five codes of two bits
    w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(15, 4)
    clc = canonical(_CLC_LENS)
    for s in _CLC_ORDER:
        w.put(_CLC_LENS[s], 3)
    for n in lit + [1]:
        w.code(*clc[n])
    w.put(0, 16)
    out["over_subscribed_code_set"] = (w.done(), len(text), crc, "over-subscribed")
    w = Bits()
    fixed_block(w, list(text[:50]) + [("L", 286)])
    out["literal_length_symbol_286"] = (w.done(), len(text), crc, "invalid literal/length or distance symbol")
    w = Bits()
    fixed_block(w, list(text[:50]) + [("D", 3, 30, 0)])
    out["distance_symbol_30"] = (w.done(), len(text), crc, "invalid literal/length or distance symbol")
    w = Bits()
    fixed_block(w, list(text[:50]) + [("D", 3, distance_symbol(51)[0], distance_symbol(51)[1])] + list(text[53:]))
    out["distance_one_before_the_start"] = (w.done(), len(text), crc, "before the start of the member")
    w = Bits()
    fixed_block(w, list(text))
    out["cut_inside_the_last_symbol"] = (w.done()[:-1], len(text), crc, "end inside a symbol")
    return out


TEXT = (b"@r1\nACGTACGTTTGACCA\n+\nIIIIIIIIIIIIIII\n" * 40)[:1500]
