"""The one-way request rule of the odd-k look-up chain (smg_fast.hpp) restated in numpy against the
definition.  No GPU.

For odd k, m = (k - 1) / 2, A(x) = pairs of x at p >= m, H(x) = pairs at p > m:  deg(x) = A(x) + H(rc x), and the P flag
P(x) = [H(rc x) > 0] is read only where A(x) = 1.  The rule: the LOWER member of every class {x, rc x} (high bit of the middle
base clear) sends rc(x) with the flag f = [H(x) > 0] when A(x) >= 1; the upper members mark the map (plane C when A = 1, plane H
when H > 0); a request with f = 1 passes on C or H, one with f = 0 on H; at the target y the flag sets P(y), and H(y) > 0 sets
P of the sender.  Pairs are enumerated from the definition: every base at p >= m of every entry is flipped to its three
alternatives and looked up.  k-mers are rows of a base array (k > 32 has no u64)."""
import numpy as np
import pytest

from smudgeplot_amd import ktab, synth

SMAX = 1000


def _keys(bases):
    """rows of bases -> byte strings that sort as the rows do (no zero bytes: numpy strips them from the end of an S string)"""
    return np.ascontiguousarray(bases + 1).view(f"S{bases.shape[1]}").ravel()


def _find(sorted_keys, bases):
    q = _keys(bases)
    j = np.minimum(np.searchsorted(sorted_keys, q), len(sorted_keys) - 1)
    return np.where(sorted_keys[j] == q, j, -1)


def analyse(bases, cnt, k):
    """-> (A, H, rc): pairs at p >= m and at p > m per entry, index of the reverse complement"""
    n, m = len(bases), (k - 1) // 2
    keys = _keys(bases)
    assert (keys[1:] > keys[:-1]).all(), "sorted, no duplicates"
    cnt = cnt.astype(np.int64)
    A, H = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for p in range(m, k):
        for d in (1, 2, 3):
            f = bases.copy()
            f[:, p] = (f[:, p] + d) & 3
            j = _find(keys, f)
            hit = (j >= 0) & (cnt + cnt[np.maximum(j, 0)] <= SMAX)
            A += hit
            if p > m:
                H += hit
    rc = _find(keys, np.ascontiguousarray(3 - bases[:, ::-1]))
    assert (rc >= 0).all(), "closed table"
    assert (cnt[rc] == cnt).all()
    return A, H, rc


def one_way(bases, A, H, rc, k):
    """rules 1-4 with an exact map (one cell per target: a real map's hashed cells can only let MORE requests pass)
    -> (P after the filtered requests, P after all requests, senders, kept)"""
    n, m = len(bases), (k - 1) // 2
    lower = bases[:, m] < 2
    senders = np.nonzero(lower & (A >= 1))[0]
    target, f = rc[senders], H[senders] > 0
    planeC, planeH = ~lower & (A == 1), ~lower & (H > 0)
    keep = np.where(f, planeC[target] | planeH[target], planeH[target])

    def apply(sel):
        P = np.zeros(n, bool)
        P[target[sel & f]] = True
        P[senders[sel & (H[target] > 0)]] = True
        return P
    return apply(keep), apply(np.ones(len(senders), bool)), senders, keep


def check(bases, cnt, k, both=True):
    A, H, rc = analyse(bases, cnt, k)
    n, m = len(bases), (k - 1) // 2
    lower = bases[:, m] < 2
    assert (rc != np.arange(n)).all(), "odd k: no k-mer is its own complement"
    assert (lower != lower[rc]).all(), "exactly one lower member per class"
    P, P_all, senders, keep = one_way(bases, A, H, rc, k)
    want = H[rc] > 0
    cand = A == 1
    assert cand.sum() > 20 and (cand & ~want).sum() > 5
    assert not both or (cand & want).sum() > 5, "the table exercises both answers"
    assert (P[cand] == want[cand]).all(), "the flags of the candidates"
    assert not (P & ~want).any(), "no false flag anywhere"
    # a dropped request has no effect: neither of its two stores could have happened
    dropped = ~keep
    y, x = rc[senders[dropped]], senders[dropped]
    assert not ((H[x] > 0) & (A[y] == 1)).any() and not (H[y] > 0).any()
    assert (P_all[cand] == P[cand]).all()
    two_way = int((H > 0).sum())
    assert len(senders) < two_way, (len(senders), two_way)
    return len(senders), two_way, int(keep.sum())


@pytest.mark.parametrize("k", [17, 27, 31, 33, 51, 63])
def test_one_way_rule_on_adversarial_tables(k):
    packed, cnt = synth.adversarial_table(k, 800, 4, seed=100 + k, low_complexity=60, dense=1)
    check(ktab.unpack_bases(packed, k), cnt, k)


def test_one_way_rule_on_a_diploid_genome():
    """overlapping k-mers of two haplotypes that differ at 1 % of their sites, k = 31: the classes of a real table (a SNP's
    k-mers pair at every position, the middle one included; a k-mer over two SNPs has no partner, so no candidate of such a
    table has a pair on the other side)"""
    k, L = 31, 8000
    rng = np.random.default_rng(5)
    h1 = rng.integers(0, 4, L, dtype=np.uint8)
    h2 = h1.copy()
    snp = rng.random(L) < 0.01
    h2[snp] = (h2[snp] + rng.integers(1, 4, int(snp.sum()), dtype=np.uint8)) & 3
    rows = np.concatenate([np.lib.stride_tricks.sliding_window_view(h, k) for h in (h1, h2)])
    rows = np.concatenate([rows, 3 - rows[:, ::-1]])
    keys, first, mult = np.unique(_keys(rows), return_index=True, return_counts=True)
    bases = np.ascontiguousarray(rows[first])
    rcj = _find(keys, np.ascontiguousarray(3 - bases[:, ::-1]))
    cnt = 20 * np.minimum(mult, mult[rcj])             # (a k-mer that is another one's complement by chance: equal counts)
    sent, two_way, kept = check(bases, cnt, k, both=False)
    assert sent < 0.6 * two_way                          # about half (0.53 on a 3e5 bp genome)
