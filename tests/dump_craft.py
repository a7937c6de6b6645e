"""K-mer dumps for the tests of the dump route, and its oracle in plain Python: lines `<k-mer><sep><count>` as kmc_dump,
`jellyfish dump -c` and `meryl print` write them; per line the canonical k-mer (as the W left-aligned 64-bit words of the
table) and the count saturated at 2^32 - 1; per call the sums per canonical k-mer (exact Python integers, clamped at 32767
only where the table is formed) and their histogram.  Nothing here looks at the library."""
import random

import numpy as np

U32, MAX_COUNT, HIST = 0xFFFFFFFF, 32767, 32768
REASONS = {"bases": "is not {k} bases and a separator (is k right?)", "nocount": "has no count", "zero": "count is 0",
           "noend": "count is not followed by a line end"}
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def revcomp(s):
    return s.translate(_COMP)[::-1]


def canonical(s):
    """the smaller of a k-mer and its reverse complement, upper case (a < c < g < t is the order of the packed words)"""
    s = s.upper()
    r = revcomp(s)
    return min(s, r)


def words(kmer):
    """k-mer (upper case) -> tuple of W left-aligned uint64 words"""
    k = len(kmer)
    w = (k + 31) // 32
    v = 0
    for ch in kmer:
        v = (v << 2) | _CODE[ch]
    v <<= 2 * (32 * w - k)
    return tuple((v >> (64 * (w - 1 - j))) & 0xFFFFFFFFFFFFFFFF for j in range(w))


def unwords(ws, k):
    v = 0
    for x in ws:
        v = (v << 64) | int(x)
    v >>= 2 * (32 * len(ws) - k)
    return "".join("ACGT"[(v >> (2 * (k - 1 - j))) & 3] for j in range(k))


def random_kmers(k, n, seed, distinct_canonical=True):
    rng = random.Random(seed)
    out, seen = [], set()
    while len(out) < n:
        s = "".join(rng.choice("ACGT") for _ in range(k))
        c = canonical(s)
        if distinct_canonical and c in seen:
            continue
        seen.add(c)
        out.append(s)
    return out


def palindromes(k, n, seed):
    """k-mers that are their own reverse complement (even k only)"""
    assert k % 2 == 0
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        h = "".join(rng.choice("ACGT") for _ in range(k // 2))
        out.append(h + revcomp(h))
    return out


def line(kmer, count, sep="\t", end="\n"):
    return f"{kmer}{sep}{count}{end}".encode()


def text(records, sep="\t", end="\n", last_end=None):
    """records: iterable of (k-mer, count[, sep[, end]]) -> the bytes of the dump; last_end replaces the end of the last line"""
    out = []
    recs = list(records)
    for i, r in enumerate(recs):
        s = r[2] if len(r) > 2 else sep
        e = r[3] if len(r) > 3 else end
        if last_end is not None and i == len(recs) - 1:
            e = last_end
        out.append(line(r[0], r[1], s, e))
    return b"".join(out)


def parse_oracle(records):
    """-> (list of key-word tuples, list of counts saturated at 2^32 - 1), in line order"""
    return [words(canonical(r[0])) for r in records], [min(int(r[1]), U32) for r in records]


def sums(records_of_all_files):
    """dict canonical k-mer -> exact sum of the (per line saturated) counts"""
    d = {}
    for r in records_of_all_files:
        c = canonical(r[0])
        d[c] = d.get(c, 0) + min(int(r[1]), U32)
    return d


def table_oracle(d, k, t):
    """-> (keys uint64[n, W] sorted, counts uint16[n] clamped, hist uint64[32768]) of the k-mers with clamped count >= t"""
    w = (k + 31) // 32
    hist = np.zeros(HIST, dtype=np.uint64)
    rows = []
    for s, c in d.items():
        c = min(c, MAX_COUNT)
        hist[c] += 1
        if c >= t:
            rows.append((words(s), c))
    rows.sort()
    keys = np.array([r[0] for r in rows], dtype=np.uint64).reshape(len(rows), w)
    cnts = np.array([r[1] for r in rows], dtype=np.uint16)
    return keys, cnts, hist


def table_keys(tab):
    """the k-mers of a ktab.KTable from count.count_files as uint64[n, W] words"""
    k = tab.k
    w = (k + 31) // 32
    p = np.zeros((tab.packed.shape[0], 8 * w), dtype=np.uint8)
    p[:, : tab.packed.shape[1]] = tab.packed
    return p.view(">u8").astype(np.uint64).reshape(-1, w)
