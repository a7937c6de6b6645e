"""tests/lookup_oracle.py without a device: the geometry, the hash and the formula maps against scalar restatements, the request
list against the definition it is taken from, and what the tables of tests/test_lookup_regimes_gpu.py promise its kernels --
bucket sizes against the sizes at which kl_part, kl_probe and kl_probe_x change regime (engine.lookup_limits: the library
loads without a device)."""
import numpy as np
import pytest

import lookup_oracle as lo
from smudgeplot_amd import engine, ktab, synth

U = np.uint64

LIMITS, PB_WAVES, wave_shares = lo.LIMITS, lo.PB_WAVES, lo.wave_shares


def test_the_library_reports_the_limits_without_a_device():
    assert engine.lookup_limits() == LIMITS
    assert (lo.NB_MAX, lo.SLICE_LG) == (LIMITS["L_NB_MAX"], LIMITS["L_SLICE_LG"])


def test_geometry_table():
    """smallest slice (16 coarse words), largest slice at two buckets, nb = 2, 3, 8, 10"""
    want = {12: (10, 1, 9), 23: (21, 1, 20), 24: (22, 2, 20), 25: (23, 3, 20), 30: (28, 8, 20), 32: (30, 10, 20)}
    assert {fb: lo.lookup_geo(fb) for fb in want} == want
    assert (1 << lo.lookup_geo(12)[2]) // 32 == 16            # fewer coarse words than the 1024 threads of a kl_probe workgroup
    x = np.array([0, 1 << 63, (1 << 64) - 1, 0x7FF0000000000000], dtype=U)
    assert lo.bucket_of(x, 1).tolist() == [0, 1, 1, 0]
    assert lo.bucket_of(x, 10).tolist() == [0, 512, 1023, 511]


def test_hash_position_against_a_scalar_restatement():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 63, 2000, dtype=np.uint64) * U(2) + rng.integers(0, 2, 2000, dtype=np.uint64)
    x[:4] = [0, 1, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF]
    want = [(((int(v) & 0xFFFFFFFF) * 0x9E3779B1) % (1 << 32)) >> 27 for v in x]
    got = lo.hash_pos(x)
    assert got.tolist() == want and set(want) == set(range(32))
    assert lo.hash_pos(x ^ U(0xABCD00000000)).tolist() == want               # the bits above the low word do not count


@pytest.mark.parametrize("fb", [12, 23, 25])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("kind", ["ones", "zero", "one_in_four", "slice_edges"])
def test_formula_and_array_of_every_map_keep_the_same_ids(kind, two, fb):
    """hand-made ids at the boundaries of map words and of the buckets' slices, each with every low word a record can carry
    in its last two bits and a few hashed positions"""
    _, nb, _ = lo.lookup_geo(fb)
    span = 1 << (fb - nb)
    ids = sorted({i for b in range(1 << nb) for base in (b * span,) for i in
                  (base, base + 1, base + 2, base + 3, base + 4, base + 31, base + 32, base + 33, base + 63, base + 64,
                   base + span // 2 - 1, base + span // 2, base + span - 33, base + span - 32, base + span - 4,
                   base + span - 3, base + span - 2, base + span - 1)})
    rec = np.array([(i << (64 - fb)) | low for i in ids for low in (0, 1, 0x9E3779B1, 0xFFFFFFFF, 12345)], dtype=U)
    hi_positions = (None, int(lo.hash_pos(np.array([12345], dtype=U))[0])) if two else (None,)
    for hp in hi_positions:
        f = lo.keep(rec, fb, two, lo.formula(kind, fb, two, hp))
        a = lo.keep(rec, fb, two, lo.map_words(kind, fb, two, hp))
        assert np.array_equal(f, a), (kind, two, fb, hp)
        got = set((rec[f] >> U(64 - fb)).tolist())
        if kind == "zero":
            assert not got
        elif kind == "ones" and hp is None:
            assert got == set(ids)
        elif kind == "one_in_four":
            assert got == {i for i in ids if i % 4 == 3}
        elif kind == "slice_edges":
            assert got == {i for i in ids if i % span in (0, span - 1)}
        if hp is not None and kind != "zero":
            assert 0 < f.sum() == (f & (lo.hash_pos(rec) == U(hp))).sum() < len(rec)


def test_one_id_in_four_passes_the_folded_test_everywhere():
    """every coarse bit -- four neighbouring ids -- holds one set id: a fold that drops the fourth bit of a group keeps nothing"""
    w = lo.map_words("one_in_four", 12, False)
    assert all(((int(v) >> (4 * j)) & 0xF) == 0x8 for v in w[:4] for j in range(8))


@pytest.mark.parametrize("k", [17, 24, 31, 32])
def test_emitted_against_the_pairwise_definition(k):
    packed, cnt = synth.adversarial_table(k, 1200, 4, 40 + k, low_complexity=40, dense=1)
    keys = ktab.packed_to_u64(packed)
    own = np.zeros(len(keys), bool)
    for p in range(k // 2, k):
        if p == k - 1 - p:
            continue
        groups = {}
        for i, x in enumerate(keys.tolist()):
            groups.setdefault(x & ~(3 << (62 - 2 * p)), []).append(i)
        for g in groups.values():
            for a in g:
                own[a] |= any(a != b and int(cnt[a]) + int(cnt[b]) <= 1000 for b in g)
    assert np.array_equal(lo.owns_hi_pair(keys, cnt, k), own) and own.sum() > 1000
    assert np.array_equal(lo.emitted(keys, cnt, k), np.sort(ktab.revcomp_u64(keys[own], k)))
    twice = lo.may_send_twice(keys, k)
    pre = keys >> U(64 - 2 * (k // 2))
    assert twice.tolist() == [int((pre == v).sum()) > 4 for v in pre]


def test_the_diploid_tables_fill_the_buckets():
    keys, cnt = lo.diploid(150000)
    assert len(keys) == 405038
    e = lo.emitted(keys, cnt, 31)
    assert len(e) == 101608
    assert not (lo.may_send_twice(keys, 31) & lo.owns_hi_pair(keys, cnt, 31)).any()      # no request is sent twice
    s23, s25, s32 = lo.bucket_sizes(e, 23), lo.bucket_sizes(e, 25), lo.bucket_sizes(e, 32)
    assert np.array_equal(s23, lo.bucket_sizes(e, 12)) and len(s23) == 2
    # kl_probe: more than two trips of a workgroup per bucket, and a last one that ends inside a wave instruction
    assert s23.min() > 2 * LIMITS["PB_TRIP"] and (s23 % 64 != 0).all()
    assert s25.min() > LIMITS["PB_TRIP"] and (s25 % 64 != 0).all() and len(s25) == 8
    # kl_probe_x at nb = 3: more than three tickets per bucket at either ticket size, the last one partial
    for part in (LIMITS["PX_PART"], 2 * LIMITS["PX_PART"]):
        t = lo.tickets(s25, part)
        assert 3 < t.min() and t.max() <= 7 and (s25 % part != 0).all()
    # nb = 10: a few dozen records per bucket, all 128 buckets of every XCD class in use (two 64-bucket rounds of the scan)
    assert s32.min() >= 1 and s32.max() < 256 and len(s32) // 8 == 128
    # kl_part: with one or two owners every owner holds several batches; by default none holds a full one
    assert len(e) > 3 * LIMITS["PT_BATCH_RW1"] and len(e) // 2 > 3 * LIMITS["PT_BATCH_RW1"]


def test_the_large_diploid_table_rolls_every_chunk_over():
    keys, cnt = lo.diploid(400000)
    assert len(keys) == 1079704
    e = lo.emitted(keys, cnt, 31)
    s = lo.bucket_sizes(e, 23)
    assert len(e) == 270612 and s.tolist() == [135283, 135329]
    for size in s.tolist():
        w = wave_shares(size)
        assert sum(w) == size
        # with a map of ones every wave keeps its whole share: two chunks to the brim at least (a chunk that is exactly full is
        # not rolled over before the next record comes), and nine waves of sixteen open a third
        assert min(w) >= 2 * LIMITS["F_CH"] and sum(x > 2 * LIMITS["F_CH"] for x in w) == 9
        assert sum(x == 2 * LIMITS["F_CH"] for x in w) == 7


def test_the_clustered_table_leaves_six_xcd_classes_without_a_ticket():
    keys, cnt = lo.clustered()
    assert 300000 < len(keys) < 450000
    e = lo.emitted(keys, cnt, 31)
    s = lo.bucket_sizes(e, 32)
    assert np.flatnonzero(s).tolist() == [0, 1023] and s.min() == 0 and s[[0, 1023]].min() > 5 * LIMITS["PB_TRIP"]
    classes = {b % 8 for b in np.flatnonzero(s).tolist()}
    assert classes == {0, 7}                                  # XCD classes 1 .. 6 hold no ticket at all
    assert lo.tickets(s, 2 * LIMITS["PX_PART"])[[0, 1023]].min() > 10
    s25 = lo.bucket_sizes(e, 25)
    assert np.flatnonzero(s25).tolist() == [0, 7]


def test_the_families_table_sends_from_long_blocks():
    keys, cnt = lo.families(31)
    own = lo.owns_hi_pair(keys, cnt, 31)
    assert (lo.may_send_twice(keys, 31) & own).sum() > 5000 and own.sum() > 5000


def test_the_edges_table_sends_to_both_ends_of_every_slice():
    fb = 25
    keys, cnt = lo.edges(fb)
    e = lo.emitted(keys, cnt, 31)
    at_edge = lo.keep_one_bit(e, fb, lo.formula("slice_edges", fb, False))
    ids = lo.ids_of(e[at_edge], fb)
    span = 1 << 22
    assert sorted(set(ids.tolist())) == sorted(b * span + x for b in range(8) for x in (0, span - 1))
    assert np.bincount((ids % U(span) != U(0)).astype(np.int64) + 2 * (ids // U(span)).astype(np.int64)).min() >= 500
    assert at_edge.sum() >= 16 * 500 and (~at_edge).sum() > 10000


def test_a_larger_diploid_table_takes_every_wave_past_two_chunks():
    """n0 = 420000: 17 full trips of a workgroup per bucket, so every wave keeps 8704 records or more under a map of ones and
    rolls its chunk over twice (on the 1.08e6-entry table seven waves of sixteen stop at two chunks exactly)"""
    keys, cnt = lo.diploid(420000)
    e = lo.emitted(keys, cnt, 31)
    s = lo.bucket_sizes(e, 23)
    assert len(keys) == 1133370 and len(e) == 283826 and s.tolist() == [142424, 141402]
    assert all(min(wave_shares(size)) > 2 * LIMITS["F_CH"] for size in s.tolist())


@pytest.mark.parametrize("k", [17, 31])
def test_one_way_list_against_the_pairwise_definition(k):
    packed, cnt = synth.adversarial_table(k, 1200, 4, 60 + k, low_complexity=40, dense=1)
    keys = ktab.packed_to_u64(packed)
    a, h = np.zeros(len(keys), int), np.zeros(len(keys), int)
    for p in range(k // 2, k):
        groups = {}
        for i, x in enumerate(keys.tolist()):
            groups.setdefault(x & ~(3 << (62 - 2 * p)), []).append(i)
        for g in groups.values():
            for i in g:
                n = sum(1 for j in g if i != j and int(cnt[i]) + int(cnt[j]) <= 1000)
                a[i] += n
                h[i] += n if p != k - 1 - p else 0
    want = sorted((int(ktab.revcomp_u64(keys[i:i + 1], k)[0]) | int(h[i] > 0))
                  for i in range(len(keys)) if (int(keys[i]) >> (64 - k)) & 1 == 0 and (h[i] > 0 or a[i] == 1))
    rec, send = lo.emitted_one_way(keys, cnt, k)
    assert rec.tolist() == want and len(want) > 500 and 0 < sum(r & 1 for r in want) < len(want)
    assert np.array_equal(ktab.revcomp_u64(keys[send], k), rec & ~U(1))
    assert np.array_equal(lo.pair_counts(keys, cnt, k, range(k // 2, k)), a)


def test_one_way_filter_against_a_scalar_restatement():
    rng = np.random.default_rng(7)
    fb = 12
    words = rng.integers(0, 1 << 32, 2 << (fb - 5), dtype=np.uint64).astype(np.uint32)
    rec = rng.integers(0, 1 << 63, 4000, dtype=np.uint64) * U(2) + rng.integers(0, 2, 4000, dtype=np.uint64)
    want = []
    for r in rec.tolist():
        i, f, low = r >> (64 - fb), r & 1, r & 0xFFFFFFFE
        pos = ((low * 0x9E3779B1) % (1 << 32)) >> 28
        hw = int(words[2 * (i >> 5) + 1])
        planes = (hw >> 16) | (hw if f else 0)
        want.append(bool((int(words[2 * (i >> 5)]) >> (i & 31)) & (planes >> pos) & 1))
    got = lo.keep_one_way(rec, fb, True, words)
    assert got.tolist() == want and 0 < sum(want) < len(want)
    assert np.array_equal(lo.keep_one_way(rec, fb, False, words), lo.keep_one_bit(rec, fb, words))
