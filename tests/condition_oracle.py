"""Numpy oracle of table conditioning (trim at -e, then close under reverse complement) and the generator of the raw tables
the conditioning tests run on -- TEST INFRASTRUCTURE ONLY, held to independent code by tests/test_condition_oracle_host.py.

The oracle works from BASE arrays ([n, k] uint8, a c g t = 0 1 2 3): the reverse complement is `3 - b[:, ::-1]` and is never
taken from a packed key, so it shares nothing with the device's revcomp<W>, with ktab.revcomp_packed or with the Python
integers of fake_engine.NumpyEngine.  Words are packed left aligned (base 0 in bits 63..62 of word 0), as the engine holds them.
"""
import numpy as np

from smudgeplot_amd import synth


def nwords(k):
    return (k + 31) // 32


def words_of(bases, k):
    """[n, k] bases -> [n, W] uint64, left aligned"""
    bases = np.asarray(bases, dtype=np.uint8).reshape(-1, k)
    n, W = len(bases), nwords(k)
    pad = np.zeros((n, 32 * W), dtype=np.uint8)
    pad[:, :k] = bases
    q = pad.reshape(n, 8 * W, 4)
    byte = (q[:, :, 0] << 6) | (q[:, :, 1] << 4) | (q[:, :, 2] << 2) | q[:, :, 3]      # most significant byte first
    return np.ascontiguousarray(byte).view(">u8").astype(np.uint64).reshape(n, W)


def bases_of(keys, k):
    """the inverse of words_of"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, nwords(k))
    out = np.empty((len(keys), nwords(k), 32), dtype=np.uint8)
    for j in range(32):
        out[:, :, j] = (keys >> np.uint64(62 - 2 * j)) & np.uint64(3)
    return out.reshape(len(keys), -1)[:, :k]


def packed_of(keys, k):
    """[n, W] words -> the [n, kbyte] bytes of a FastK table (ktab.py)"""
    keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64).reshape(-1, nwords(k)))
    return np.ascontiguousarray(keys.astype(">u8").view(np.uint8).reshape(len(keys), -1)[:, : (k + 3) // 4])


def revcomp(bases):
    return (3 - np.asarray(bases, dtype=np.uint8)[:, ::-1]).astype(np.uint8)


def order_of(keys):
    """the stable order of [n, W] words, word 0 the most significant"""
    return np.lexsort(keys.T[::-1])


def closed(bases, counts, k):
    """entries followed by their complements, stably sorted: (keys[2n, W], counts[2n], is-a-complement[2n])"""
    n = len(counts)
    both = np.concatenate([bases, revcomp(bases)]) if n else np.zeros((0, k), np.uint8)
    keys = words_of(both, k)
    o = order_of(keys)
    return keys[o], np.concatenate([counts, counts])[o], o >= n


def condition(bases, counts, k, L, trim=True, symm=True):
    """-> (keys[m, W] uint64, counts[m] uint16) of the table after: trim (keep count >= L), symm (entries followed by
    their complements, stably sorted by k-mer, the first of a run of equal k-mers kept)"""
    bases = np.asarray(bases, dtype=np.uint8).reshape(-1, k)
    counts = np.asarray(counts, dtype=np.uint16)
    if trim:
        keep = counts >= L
        bases, counts = bases[keep], counts[keep]
    if not symm:
        return words_of(bases, k), counts.copy()
    keys, cnt, _ = closed(bases, counts, k)
    first = np.ones(len(cnt), dtype=bool)
    first[1:] = (keys[1:] != keys[:-1]).any(axis=1)
    return keys[first], cnt[first]


def leading_ties(keys):
    """[number of adjacent rows of sorted keys that agree in words 0..j-1 but are not equal, for j = 1..W-1]"""
    same = keys[1:] == keys[:-1]
    equal = same.all(axis=1)
    return [int((same[:, :j].all(axis=1) & ~equal).sum()) for j in range(1, keys.shape[1])]


def shared_groups(bases, lo, hi):
    """number of rows of `bases` that share columns lo:hi with another row"""
    if len(bases) < 2:
        return 0
    keys = words_of(bases[:, lo:hi], hi - lo)
    keys = keys[order_of(keys)]
    same = (keys[1:] == keys[:-1]).all(axis=1)
    return int((np.concatenate([[False], same]) | np.concatenate([same, [False]])).sum())


def is_canonical(bases, k):
    """row <= its reverse complement, in base order"""
    x, r = words_of(bases, k), words_of(revcomp(bases), k)
    lt = np.zeros(len(x), dtype=bool)
    decided = np.zeros(len(x), dtype=bool)
    for w in range(x.shape[1]):
        lt |= ~decided & (x[:, w] < r[:, w])
        decided |= x[:, w] != r[:, w]
    return lt | ~decided


FAMILY = 64


def _families(rng, k, nfam, shared, suffix):
    """nfam families of up to FAMILY k-mers that share `shared` bases (the first ones, or with suffix the last ones) and
    differ in the others.  Canonical by construction: a prefix family starts with a and does not end with t (its complement
    starts with c g or t), a suffix family ends with a and does not start with t (its complement starts with t)."""
    free = k - shared
    size = min(FAMILY, 3 * 4 ** (free - 1))
    out = np.empty((nfam, size, k), dtype=np.uint8)
    common = rng.integers(0, 4, size=(nfam, 1, shared), dtype=np.uint8)
    total = 3 * 4 ** (free - 1)
    if total <= 4096:                                   # few free bases: distinct completions, all of them if need be
        code = np.argsort(rng.random((nfam, total)), axis=1)[:, :size]
        rest = np.stack([(code // 3 // 4 ** i) % 4 for i in range(free - 1)] + [code % 3], axis=2).astype(np.uint8)
    else:
        rest = rng.integers(0, 4, size=(nfam, size, free), dtype=np.uint8)
        rest[:, :, -1] = rng.integers(0, 3, size=(nfam, size))
    if suffix:                                          # the free bases in front, their restricted base first
        out[:, :, :free] = rest[:, :, ::-1]
        out[:, :, free:] = common
        out[:, :, -1] = 0
    else:
        out[:, :, :shared] = common
        out[:, :, shared:] = rest
        out[:, :, 0] = 0
    return out.reshape(-1, k)


def _canonical(bases, k):
    canon = is_canonical(bases, k)
    bases[~canon] = revcomp(bases[~canon])
    return bases


def raw_table(k, n, seed, L=6, families=0.25, palindromes=500, variants=0.05):
    """A raw table as a counter writes it: n distinct canonical k-mers as bases [n, k], in table order, and counts uint16[n].

    It holds, and asserts that it holds:
      * for every j in 1..W-1, families of (up to) 64 k-mers that share their first 32 j bases: about `families` of the
        entries in all; and as many that share their last 32 j bases, so that their complements share the first;
      * for even k, `palindromes` self-complementary k-mers, among them aaaa..tttt and tttt..aaaa, the smallest and the
        largest there are, both with a count that survives the trim;
      * counts 1 .. 60 and synth.EDGE_COUNTS, about 15 % of them below L;
      * for a share `variants` of the entries a second k-mer that differs from it in one base: the pairs a plot is made of.
    """
    rng = np.random.default_rng(seed)
    W = nwords(k)
    special, nfam = [], 0
    if W > 1 and families > 0:
        nfam = max(2, int(n * families / ((W - 1) * FAMILY)))
        for j in range(1, W):
            special.append(_families(rng, k, nfam, 32 * j, suffix=False))
            special.append(_families(rng, k, nfam, 32 * j, suffix=True))
    npal = palindromes if k % 2 == 0 else 0
    if npal:
        half = rng.integers(0, 4, size=(npal, k // 2), dtype=np.uint8)
        half[0], half[1] = 0, 3
        special.append(np.concatenate([half, 3 - half[:, ::-1]], axis=1))
    nspecial = sum(len(s) for s in special)
    nvar = int(n * variants)
    rand = rng.integers(0, 4, size=(max(n - nspecial - nvar, 0) + 256, k), dtype=np.uint8)
    var = rand[:nvar].copy()
    at = (np.arange(nvar), rng.integers(0, k, size=nvar))
    var[at] = (var[at] + rng.integers(1, 4, size=nvar)) & 3
    bases = np.concatenate(special + [_canonical(var, k), _canonical(rand, k)])
    keys = words_of(bases, k)
    o = order_of(keys)                                  # stable: of equal k-mers the first made (a special one) stays
    ks = keys[o]
    first = np.ones(len(o), dtype=bool)
    first[1:] = (ks[1:] != ks[:-1]).any(axis=1)
    keep = np.sort(o[first])[:n]                        # in order of making: what is cut off is random k-mers
    bases = bases[keep]
    bases = bases[order_of(words_of(bases, k))]
    assert len(bases) == n, "raw_table: n is smaller than the families and palindromes asked for, or too close to 4^k"

    counts = rng.integers(L, 61, size=n)
    edge = rng.random(n) < 0.1
    counts[edge] = rng.choice(synth.EDGE_COUNTS[synth.EDGE_COUNTS >= L], size=int(edge.sum()))
    low = rng.random(n) < 0.15
    counts[low] = rng.integers(1, max(L, 2), size=int(low.sum()))
    self_rc = (bases == revcomp(bases)).all(axis=1)
    if npal:
        counts[0], counts[np.flatnonzero(self_rc)[-1]] = 32767, max(L, 60)
    counts = counts.astype(np.uint16)

    # ---- what the docstring promises
    keys = words_of(bases, k)
    assert ((keys[1:] != keys[:-1]).any(axis=1)).all() and (order_of(keys) == np.arange(n)).all(), "sorted and distinct"
    assert is_canonical(bases, k).all()
    assert counts.max() <= 32767 and counts.min() >= 1
    if L > 1:
        assert 0.10 * n <= int((counts < L).sum()) <= 0.20 * n + 8
    for j in range(1, W if nfam else 1):
        # a family's members are distinct unless two random completions agree: 64 draws from more than 4096 values, less
        # than one of 64 lost on average; below that the completions are drawn without replacement
        want = nfam * min(FAMILY, 3 * 4 ** (k - 32 * j - 1))
        assert shared_groups(bases, 0, 32 * j) >= 0.9 * want, (k, j)
        assert shared_groups(bases, k - 32 * j, k) >= 0.9 * want, (k, j)
    if npal:
        assert int(self_rc.sum()) >= npal - 2            # (two random halves may agree)
        assert (bases[0] == np.repeat([0, 3], k // 2)).all() and counts[0] >= L
        last = np.flatnonzero(self_rc)[-1]
        assert (bases[last] == np.repeat([3, 0], k // 2)).all() and counts[last] >= L
    else:
        assert not self_rc.any()
    return bases, counts
