"""Engine.close_canonical -- the closure of a canonical table by one sort of its complements and a merge-path merge (ks_merge,
smg_keysort.hpp) -- against the numpy oracle of tests/condition_oracle.py, ENTRY FOR ENTRY (k-mers and counts of the table the
engine holds afterwards), and against Engine.condition(0, False, True) on the same bound table as a second reference.

The inputs are condition_oracle.raw_table's: canonical, sorted, with families that share their first / last 32 j bases (so that
the low words decide the merge), self-complementary k-mers at even k (which have no complement to merge in), one-base variants.
The sizes sit where the merge changes path: one output short of a tile of ks_merge, a full tile, one more, several tiles and a
rest -- the tile per key width is read from the library (engine.merge_tile), not repeated here -- and a table whose complements
all sort behind its last entry, so that whole tiles come from one list.
"""
import functools

import numpy as np
import pytest

import condition_oracle as co
from smudgeplot_amd import engine

pytestmark = pytest.mark.gpu

ONE_SWEEP = 1 << 20                                    # rocPRIM's merge_sort_limit: the sort of the complements changes regime above it


def on_device(keys, counts):
    import torch
    dev = torch.device("cuda:0")
    tk = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64).reshape(-1).copy()).to(dev)
    tc = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint16).view(np.int16).copy()).to(dev)
    return tk, tc


def same_table(got, exp):
    assert got[0].shape == exp[0].shape and got[1].shape == exp[1].shape, (got[0].shape, exp[0].shape)
    bad = np.flatnonzero((got[0] != exp[0]).any(axis=1) | (got[1] != exp[1]))
    assert len(bad) == 0, f"{len(bad)} of {len(exp[1])} entries differ, the first at {bad[:5]}"


def check(k, bases, counts):
    """one engine: close_canonical on the bound table against the oracle, then the generic closure of the same bound table
    against both.  Returns the number of entries of the closed table."""
    import torch
    bases = np.asarray(bases, dtype=np.uint8).reshape(-1, k)
    counts = np.asarray(counts, dtype=np.uint16)
    exp = co.condition(bases, counts, k, 0, trim=False, symm=True)
    tk, tc = on_device(co.words_of(bases, k), counts)
    e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
    try:
        e.bind(k, len(counts), tk.data_ptr(), tc.data_ptr())
        n = e.close_canonical()
        got = e.table_host()
        assert n == len(exp[1]) == e.table()[0]
        same_table(got, exp)
        e.bind(k, len(counts), tk.data_ptr(), tc.data_ptr())
        assert e.condition(0, False, True) == n
        same_table(e.table_host(), got)
    finally:
        e.close()
    return n


@functools.lru_cache(maxsize=4)
def raw(k, n=5000):
    return co.raw_table(k, n, 2000 + k, L=6)


@pytest.mark.parametrize("k", [13, 21, 31, 32, 33, 64, 65, 96, 128])
def test_every_key_width(k):
    bases, counts = raw(k)
    self_rc = (bases == co.revcomp(bases)).all(axis=1)
    assert int(self_rc.sum()) >= 400 if k % 2 == 0 else not self_rc.any()     # even k: palindromes, which have no complement to merge in
    n = check(k, bases, counts)
    assert n == 2 * len(counts) - int(self_rc.sum()) > 2 * engine.merge_tile(co.nwords(k))


@pytest.mark.parametrize("k", [32, 64, 96, 128])
def test_around_the_tiles_of_the_merge(k):
    """n + m = T - 1, T, T + 1 and 3 T + 5 outputs: a palindrome gives one output, every other entry two"""
    T = engine.merge_tile(co.nwords(k))
    bases, counts = raw(k)
    self_rc = (bases == co.revcomp(bases)).all(axis=1)
    pal, rest = np.flatnonzero(self_rc), np.flatnonzero(~self_rc)
    for total in (T - 1, T, T + 1, 3 * T + 5):
        p = 10 + (total - 10) % 2                                            # palindromes: the parity of the total
        rows = np.sort(np.concatenate([pal[:p], rest[: (total - p) // 2]]))
        assert p + 2 * ((total - p) // 2) == total and len(rows) == p + (total - p) // 2
        assert check(k, bases[rows], counts[rows]) == total


@pytest.mark.parametrize("k", [21, 64, 100])
def test_one_entry_and_none(k):
    bases, counts = raw(k)
    self_rc = (bases == co.revcomp(bases)).all(axis=1)
    one = int(np.flatnonzero(~self_rc)[3])
    assert check(k, bases[one:one + 1], counts[one:one + 1]) == 2
    assert check(k, bases[:0], counts[:0]) == 0
    if k % 2 == 0:
        p = int(np.flatnonzero(self_rc)[3])
        assert check(k, bases[p:p + 1], counts[p:p + 1]) == 1


@pytest.mark.parametrize("k", [32, 128])
def test_self_complementary_kmers_only(k):
    """m = 0: no complement to sort or merge, the closure is the table"""
    bases, counts = raw(k)
    self_rc = (bases == co.revcomp(bases)).all(axis=1)
    assert int(self_rc.sum()) >= 400
    assert check(k, bases[self_rc], counts[self_rc]) == int(self_rc.sum())


@pytest.mark.parametrize("k", [31, 65, 128])
def test_every_complement_sorts_behind_the_table(k):
    """entries that start with a and do not end with t: their complements start with c, g or t, so the merge takes whole tiles
    from the table and then whole tiles from the complements"""
    rng = np.random.default_rng(k)
    b = rng.integers(0, 4, size=(5200, k), dtype=np.uint8)
    b[:, 0] = 0
    b[:, -1] = rng.integers(0, 3, size=len(b))
    b[:2600, 1:34 if k > 40 else 12] = b[0, 1:34 if k > 40 else 12]          # half of them share their leading bases
    keys = co.words_of(b, k)
    o = co.order_of(keys)
    first = np.ones(len(o), dtype=bool)
    first[1:] = (keys[o][1:] != keys[o][:-1]).any(axis=1)
    b = b[o][first][:5000]
    assert len(b) == 5000 and co.is_canonical(b, k).all()
    assert (co.words_of(co.revcomp(b), k)[:, 0] > co.words_of(b, k)[-1, 0]).all()
    counts = rng.integers(1, 3000, size=len(b)).astype(np.uint16)
    assert check(k, b, counts) == 10000 > 4 * engine.merge_tile(co.nwords(k))


def test_above_the_merge_sort_limit():
    k, n = 31, ONE_SWEEP + 60_000
    bases, counts = co.raw_table(k, n, 2999, L=6)
    assert not (bases == co.revcomp(bases)).all(axis=1).any()                 # m = n > 2^20: the one-sweep regime of the sort of R
    assert check(k, bases, counts) == 2 * n


@pytest.mark.parametrize("k", [31, 64, 97])
def test_a_table_that_is_not_canonical_is_refused_and_left_alone(k):
    import torch
    bases, counts = raw(k)
    bases = bases.copy()
    self_rc = (bases == co.revcomp(bases)).all(axis=1)
    j = int(np.flatnonzero(~self_rc)[len(counts) // 2])
    bases[j] = co.revcomp(bases[j:j + 1])[0]                                 # the larger of the two
    o = co.order_of(co.words_of(bases, k))
    bases, counts = bases[o], counts[o]
    assert int((~co.is_canonical(bases, k)).sum()) == 1
    keys = co.words_of(bases, k)
    tk, tc = on_device(keys, counts)
    e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
    try:
        e.bind(k, len(counts), tk.data_ptr(), tc.data_ptr())
        with pytest.raises(engine.EngineError) as err:
            e.close_canonical()
        assert err.value.code == -2 and "table is not canonical" in str(err.value)
        assert e.table()[0] == len(counts) and e.table()[1] == tk.data_ptr()   # still the bound table
        same_table(e.table_host(), (keys, counts))
        assert e.condition(0, False, True) == len(co.condition(bases, counts, k, 0, trim=False)[1])     # and still usable
    finally:
        e.close()
