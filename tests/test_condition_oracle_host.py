"""tests/condition_oracle.py held to independent code at a few thousand entries (no GPU): ktab.symmetrize (bytes and
np.void sorts) and fake_engine.NumpyEngine (Python integers and a dict); and the guarantees of its generator."""
import numpy as np
import pytest
import torch

import condition_oracle as co
from fake_engine import NumpyEngine
from smudgeplot_amd import ktab, synth

KS = [31, 32, 64, 65, 100, 128]
L = 6


def _raw(k, n=3000, seed=0):
    return co.raw_table(k, n, seed + k, L=L, palindromes=40)


@pytest.mark.parametrize("k", [12, 31, 32, 33, 64, 65, 97, 128])
def test_words_are_left_aligned_and_match_the_table_bytes(k):
    rng = np.random.default_rng(k)
    b = rng.integers(0, 4, size=(500, k), dtype=np.uint8)
    w = co.words_of(b, k)
    assert w.shape == (500, co.nwords(k)) and w.dtype == np.uint64
    for i in (0, 17, 499):                                               # base 0 in bits 63..62 of word 0
        v = 0
        for x in b[i]:
            v = (v << 2) | int(x)
        v <<= 64 * co.nwords(k) - 2 * k
        assert [int(x) for x in w[i]] == [(v >> (64 * (co.nwords(k) - 1 - j))) & (2 ** 64 - 1) for j in range(co.nwords(k))]
    assert np.array_equal(co.bases_of(w, k), b)
    assert np.array_equal(co.packed_of(w, k), ktab.pack_bases(b))
    assert np.array_equal(co.packed_of(co.words_of(co.revcomp(b), k), k), ktab.revcomp_packed(ktab.pack_bases(b), k))


@pytest.mark.parametrize("k", KS)
def test_oracle_equals_ktab_symmetrize_on_canonical_input(k):
    bases, counts = _raw(k)
    keep = counts >= L
    sp, sc = ktab.symmetrize(ktab.pack_bases(bases[keep]), counts[keep], k)
    keys, cnt = co.condition(bases, counts, k, L)
    assert np.array_equal(co.packed_of(keys, k), sp) and np.array_equal(cnt, sc)
    keys, cnt = co.condition(bases[keep], counts[keep], k, 0, trim=False)
    assert np.array_equal(co.packed_of(keys, k), sp) and np.array_equal(cnt, sc)
    keys, cnt = co.condition(bases, counts, k, L, symm=False)
    assert np.array_equal(co.packed_of(keys, k), ktab.pack_bases(bases[keep])) and np.array_equal(cnt, counts[keep])


def _numpy_engine(k, bases, counts):
    eng = NumpyEngine("cpu")
    eng.bind(k, torch.from_numpy(co.words_of(bases, k).view(np.int64).reshape(-1).copy()),
             torch.from_numpy(np.ascontiguousarray(counts).view(np.int16).copy()))
    return eng


def _table_of(eng):
    keys = np.array([eng._words(x) for x in eng.keys], dtype=np.uint64).reshape(-1, eng.W)
    return keys, eng.cnt.astype(np.uint16)


@pytest.mark.parametrize("k", KS)
def test_oracle_equals_the_numpy_engine(k):
    bases, counts = _raw(k, n=1500)
    W = co.nwords(k)
    want = co.condition(bases, counts, k, L)
    eng = _numpy_engine(k, bases, counts)
    assert eng.trim(L) == int((counts >= L).sum())
    got = _table_of(eng)
    trimmed = co.condition(bases, counts, k, L, symm=False)
    assert np.array_equal(got[0], trimmed[0]) and np.array_equal(got[1], trimmed[1])
    send = torch.zeros(2 * eng.n * (W + 1), dtype=torch.int64)
    assert eng.symm_route([], 1, send) == [2 * eng.n]
    assert eng.symm_finish(send, 2 * eng.n) == len(want[1])
    got = _table_of(eng)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # two destinations, cut at the middle k-mer of the closed table (a smaller table: every record is compared with the
    # splitter and dealt out in Python)
    bases, counts = bases[::3], counts[::3]
    want = co.condition(bases, counts, k, L)
    split = want[0][len(want[0]) // 2]
    eng = _numpy_engine(k, bases, counts)
    eng.trim(L)
    n2 = 2 * eng.n
    sc = eng.symm_route(split, 2, send)
    assert sum(sc) == n2
    parts, off = [], 0
    for dst in range(2):
        fin = _numpy_engine(k, bases[:1], counts[:1])
        fin.symm_finish(send[off * (W + 1): (off + sc[dst]) * (W + 1)], sc[dst])
        parts.append(_table_of(fin))
        off += sc[dst]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), want[0])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), want[1])
    assert len(parts[0][1]) == len(want[1]) // 2


@pytest.mark.parametrize("k", KS)
def test_generator_guarantees(k):
    n = 4000
    bases, counts = _raw(k, n=n)
    W = co.nwords(k)
    assert bases.shape == (n, k) and counts.shape == (n,) and counts.dtype == np.uint16
    packed = ktab.pack_bases(bases)
    rows = [bytes(r) for r in packed]
    assert rows == sorted(set(rows))                                      # table order, distinct
    assert all(a <= bytes(b) for a, b in zip(rows, ktab.revcomp_packed(packed, k)))          # canonical
    assert set(range(1, 61)) | set(int(c) for c in synth.EDGE_COUNTS) >= set(int(c) for c in counts)
    assert set(int(c) for c in counts) >= set(int(c) for c in synth.EDGE_COUNTS)
    assert 0.10 * n < int((counts < L).sum()) < 0.20 * n
    keep = counts >= L
    keys, cnt, is_copy = co.closed(bases[keep], counts[keep], k)
    ties = co.leading_ties(keys)
    assert len(ties) == W - 1 and all(t >= 8 for t in ties)              # adjacent entries that tie in words 0..j-1, every j
    for j in range(1, W):                                                 # among the entries, and among the complements
        assert co.shared_groups(bases[keep], 0, 32 * j) >= 8 and co.shared_groups(bases[keep], k - 32 * j, k) >= 8
    dup = (keys[1:] == keys[:-1]).all(axis=1)
    want = co.condition(bases, counts, k, L)
    assert len(want[1]) == len(cnt) - int(dup.sum())
    if k % 2 == 0:
        self_rc = (bases == co.revcomp(bases)).all(axis=1)
        assert 38 <= int(self_rc.sum()) <= 40 and int(dup.sum()) == int((self_rc & keep).sum()) > 20
        assert dup[0] and dup[-1]                                         # a duplicate pair at sorted positions 0 / 1, one at the end
        assert not is_copy[0] and is_copy[1]                              # (stable: the entry in front of its complement)
        assert "".join("acgt"[b] for b in bases[0]) == "a" * (k // 2) + "t" * (k // 2)
        assert "".join("acgt"[b] for b in co.bases_of(keys[-1:], k)[0]) == "t" * (k // 2) + "a" * (k // 2)
    else:
        assert not dup.any()


@pytest.mark.parametrize("k", [31, 64])
def test_the_table_holds_pairs_for_a_plot(k):
    bases, counts = _raw(k)
    one_away = 0
    seen = {bytes(r) for r in bases} | {bytes(r) for r in co.revcomp(bases)}
    for r in bases[:: 7]:
        for p in range(k):
            for d in (1, 2, 3):
                v = r.copy()
                v[p] = (v[p] + d) & 3
                one_away += bytes(v) in seen
    assert one_away >= 10


@pytest.mark.parametrize("k", [31, 64])
def test_empty_results(k):
    bases, counts = _raw(k, n=1000)
    W = co.nwords(k)
    for trim, symm in ((True, True), (True, False)):
        keys, cnt = co.condition(bases, counts, k, 40000, trim=trim, symm=symm)                # L above every count
        assert keys.shape == (0, W) and keys.dtype == np.uint64 and cnt.shape == (0,) and cnt.dtype == np.uint16
    for trim, symm in ((True, True), (False, True), (True, False)):
        keys, cnt = co.condition(bases[:0], counts[:0], k, L, trim=trim, symm=symm)            # n = 0
        assert keys.shape == (0, W) and cnt.shape == (0,)
    assert co.words_of(np.zeros((0, k), np.uint8), k).shape == (0, W)
