"""The oracle and the generators of tests/test_pass2_regimes_gpu.py, on the host (no GPU): `classify` against the independent
oracle/brute.py, and what every generator promises at the parameters the GPU tests use -- a queue that overflows in aligned
tiles, more far cells than the cache has slots, far entries on both sides of the look-ups' flag in every lane of the code
scan.  All of it is computed from the oracle; the engine is not asked."""
import numpy as np
import pytest

import brute
import pass2_oracle as po
from smudgeplot_amd import engine, synth

# smg_engine_pass2_limits; tests/test_pass2_regimes_gpu.py asserts that the library says the same
LIMITS = dict(P2_TILE=16384, P2_QCAP=8192, P2_FAR=512, P2_SMAX=208, P2_GRID=512, EX_STAGE=1024, F_TPB=256, EX_GRID=2048)
WAVE_RUN = 1024                            # consecutive entries one wave of kf_pass2 inspects (64 lanes x 16 code bytes)

KS = (31, 32, 51, 70)
STAR = dict(n_star=5200, m=7, n_pair=11000, cnt_lo=3, cnt_hi=519)
RAGGED = dict(n_star=4000, m=7, n_pair=8577, cnt_lo=3, cnt_hi=519)          # 98308 entries: six tiles and four entries
HOT = dict(n_star=5200, m=7, n_pair=11000, cnt_lo=3, cnt_hi=519, fixed=(150, 150))


def star_table(k):
    return po.star_pair_table(k, seed=100 + k, **STAR)


def ragged_table(k):
    return po.star_pair_table(k, seed=200 + k, **RAGGED)


def hot_table(k):
    return po.star_pair_table(k, seed=300 + k, extra=(3000, 2000, LIMITS["P2_SMAX"]), **HOT)


def far_table(k):
    return po.far_flag_families(k, 500 + k)


def cache_slot(cell):
    """the slot of a far cell in kf_pass2's direct-mapped cache: the leading bits of a 32-bit multiplicative hash"""
    bits = LIMITS["P2_FAR"].bit_length() - 1
    return ((cell.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def test_the_limits_need_no_device():
    assert engine.pass2_limits() == LIMITS
    assert LIMITS["P2_QCAP"] < LIMITS["P2_TILE"] and LIMITS["P2_TILE"] % WAVE_RUN == 0
    assert 2 * LIMITS["F_TPB"] <= LIMITS["EX_STAGE"]                   # a round's records always fit the staging buffer


@pytest.mark.parametrize("k,seed", [(31, 3), (64, 5), (70, 7)])
def test_classify_agrees_with_brute(k, seed):
    packed, cnt = synth.adversarial_table(k, 1500, 4, seed, low_complexity=100, dense=2)
    c = po.classify(packed, cnt, k)
    i = np.flatnonzero((c.partner > np.arange(len(cnt))) & (c.pre == 0) & po.counting(c))
    mine = set(zip(i.tolist(), c.partner[i].tolist(), c.pos[i].tolist()))
    a, b, pos = brute.unique_pairs(packed, cnt, k)
    back = pos >= k // 2
    assert mine == set(zip(a[back].tolist(), b[back].tolist(), pos[back].tolist())) and len(mine) > 300
    # the table is closed under reverse complement: brute's pairs in front of k // 2 are the mirror images of the others
    assert int((~back).sum()) == sum(1 for _, _, p in mine if p != k - 1 - p)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("make", [star_table, ragged_table, hot_table], ids=["star", "ragged", "hot"])
def test_star_tables_overflow_the_queue_and_the_far_cache(make, k):
    packed, cnt = make(k)
    n, T = len(cnt), LIMITS["P2_TILE"]
    if make is star_table:
        assert n == 127200
    if make is ragged_table:
        assert n == 98308 and n % 16 != 0 and 0 < n % T < 16
    c = po.classify(packed, cnt, k)
    cand, cnting = po.candidates(c), po.candidates(c) & po.counting(c)
    over = [t for t in range(n // T) if cand[t * T:(t + 1) * T].sum() > LIMITS["P2_QCAP"] + 2000]
    # whichever wave finds the queue full has counting candidates to finish in place: every run of a wave holds 50
    # (the tile in which the first half of the table ends may overflow too, but its last waves see complements only)
    full = [t for t in over if cnting[t * T:(t + 1) * T].reshape(-1, WAVE_RUN).sum(axis=1).min() >= 50]
    assert len(full) >= 3, [int(cand[t * T:(t + 1) * T].sum()) for t in range(n // T)]
    s, m = po.cells(cnt, c, cnting)
    beyond = s >= LIMITS["P2_SMAX"]
    cell = np.unique(s[beyond] * 501 + m[beyond])
    if make is hot_table:
        hot = int((s * 501 + m == 300 * 501 + 150).sum())
        assert hot >= 10000 and 1500 < len(cell) < 2100
        slot = cache_slot(cell)
        assert len(np.unique(slot)) > 450 and np.bincount(slot.astype(np.int64)).max() >= 6       # hits, and misses
    else:
        assert len(cell) > 4 * LIMITS["P2_FAR"] and len(np.unique(cache_slot(cell))) == LIMITS["P2_FAR"]
        assert int((s < LIMITS["P2_SMAX"]).sum()) > 300                  # and the LDS tile is not idle
    assert not po.far(c).any()


@pytest.mark.parametrize("k", [31, 51, 66, 70, 85])
def test_far_flag_families_put_the_flag_on_far_entries_and_their_partners(k):
    packed, cnt = far_table(k)
    c = po.classify(packed, cnt, k)
    i = np.flatnonzero(po.far(c))
    assert set((i % 16).tolist()) == set(range(16))
    assert int((c.pre[i] > 0).sum()) >= 20
    assert int((c.pre[c.partner[i]] > 0).sum()) >= 20
    assert int(((c.pre[i] == 0) & po.counting(c)[i]).sum()) >= 20
    assert int((c.partner[i] - i).min()) > 2 * po.REACH                 # far by a margin, not by chance


@pytest.mark.parametrize("k", [31, 51])
def test_every_cell_table_plants_what_it_says(k):
    packed, cnt, planted = po.every_cell_table(k, 7, 215)
    s_lim = LIMITS["P2_SMAX"]
    assert 215 > s_lim + 4
    # every cell of the LDS tile that two counts >= 1 can reach, and its neighbours beyond
    inside = {(s, m) for s in range(2, s_lim) for m in range(1, s // 2 + 1)}
    assert inside <= {(int(s), int(m)) for s, m, _ in planted}
    c = po.classify(packed, cnt, k)
    kept = po.candidates(c) & po.counting(c)
    assert not po.far(c).any() and not (c.pre[kept] > 0).any()
    s, m = po.cells(cnt, c, kept)
    got = np.zeros((1001, 501), np.int64)
    np.add.at(got, (s, m), 1)
    want = np.zeros((1001, 501), np.int64)
    want[planted[:, 0], planted[:, 1]] = planted[:, 2]
    # a pair at the middle position of an odd k has a mirror image that differs there too: two candidates
    assert (got >= want).all() and (got <= 2 * want).all() and int((got > 0).sum()) == len(planted)
    assert int(c.s_all.sum()) // 2 == int(got.sum())                    # the pairs beyond the sum limit are no pairs
