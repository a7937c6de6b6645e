"""A vectorised oracle for the k-mer counter: what tests/test_count_gpu.py::oracle_counts computes with a Python Counter
over byte slices, in numpy, so that 10^7 windows take seconds and not minutes.  A helper module, not a test.

It takes a 2-D array of equal-length reads in base codes (a c g t = 0 1 2 3, 4 = no base; shorter reads are padded with 4)
and handles every k the counter accepts (W = ceil(k / 32) words per key).  It shares nothing with the device code or with
ktab.revcomp_*: the reverse complement of a window is never computed from its key.  Instead the reads themselves are
reverse-complemented as base codes and run through the same key builder; window i of a read is window nw - 1 - i of its
reverse complement.  tests/test_count_oracle_host.py holds it to oracle_counts / oracle_table entry for entry.
"""
import numpy as np

MAX_COUNT = 32767                                      # counts are clamped to this, the histogram has MAX_COUNT + 1 bins

_LUT = np.full(256, 4, np.uint8)
for _j, _c in enumerate(b"ACGT"):
    _LUT[_c] = _LUT[_c | 0x20] = _j


def encode(text):
    """sequence bytes (bytes or a uint8 array of any shape) -> base codes, upper and lower case alike, 4 for every other byte"""
    return _LUT[np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.asarray(text, np.uint8)]


def pad_reads(reads):
    """list of byte strings of any lengths -> [n, longest] base codes, 4 behind the end of a read"""
    width = max([len(r) for r in reads] + [1])
    code = np.full((len(reads), width), 4, np.uint8)
    for i, r in enumerate(reads):
        code[i, :len(r)] = encode(r)
    return code


def window_keys(code, k):
    """[n, L] base codes -> (keys uint64 [n, L - k + 1, W], left aligned, big endian, base j of a window in bits
    63 - 2 (j % 32) and the one below of word j // 32; valid bool [n, L - k + 1]: no 4 among the k positions)"""
    n, L = code.shape
    W = (k + 31) // 32
    nw = max(L - k + 1, 0)
    keys = np.zeros((n, nw, W), np.uint64)
    if nw == 0:
        return keys, np.zeros((n, 0), bool)
    c = (code & 3).astype(np.uint64)
    for j in range(k):
        keys[:, :, j // 32] |= c[:, j:j + nw] << np.uint64(62 - 2 * (j % 32))
    bad = np.zeros((n, L + 1), np.int64)
    np.cumsum(code > 3, axis=1, out=bad[:, 1:])
    return keys, (bad[:, k:] - bad[:, :L - k + 1]) == 0


def kmer_counts(code, k):
    """-> (keys uint64 [D, W] of the distinct canonical k-mers in ascending order, counts int64 [D] unclamped, windows)"""
    code = np.asarray(code, np.uint8)
    W = (k + 31) // 32
    fw, valid = window_keys(code, k)
    rc_reads = np.where(code > 3, 4, 3 - np.minimum(code, 3))[:, ::-1].astype(np.uint8)
    rv, _ = window_keys(rc_reads, k)
    fw, rv = fw[valid], rv[:, ::-1, :][valid]
    del valid
    lt = np.zeros(len(fw), bool)                       # rv < fw, word by word from the most significant
    eq = np.ones(len(fw), bool)
    for w in range(W):
        lt |= eq & (rv[:, w] < fw[:, w])
        eq &= rv[:, w] == fw[:, w]
    can = np.where(lt[:, None], rv, fw)
    del fw, rv, lt, eq
    if len(can) == 0:
        return np.zeros((0, W), np.uint64), np.zeros(0, np.int64), 0
    s = can[np.lexsort([can[:, w] for w in range(W - 1, -1, -1)])]    # (the last key of lexsort is the primary one)
    head = np.ones(len(s), bool)
    head[1:] = (s[1:] != s[:-1]).any(axis=1)
    at = np.nonzero(head)[0]
    return s[at], np.diff(np.append(at, len(s))).astype(np.int64), len(s)


def pack_keys(keys, k):
    """[N, W] uint64 -> [N, ceil(k / 4)] uint8, base 0 in the top bits of byte 0 (the layout of a table's k-mers)"""
    kb = (k + 3) // 4
    return np.ascontiguousarray(keys.astype(">u8").view(np.uint8).reshape(len(keys), 8 * keys.shape[1])[:, :kb])


def table(keys, counts, k, t):
    """what kmer_counts returned -> (packed [N, kbyte] uint8, counts uint16, hist uint64[32768]) of the k-mers with a
    clamped count >= t: the triple of test_count_gpu.oracle_table"""
    c = np.minimum(counts, MAX_COUNT)
    hist = np.bincount(c, minlength=MAX_COUNT + 1).astype(np.uint64)
    keep = c >= t
    return pack_keys(keys[keep], k), c[keep].astype(np.uint16), hist
