"""One request per complement class in the odd-k look-up chain (smg_fast.hpp): the engine against the
numpy oracle, and against itself with the two-way protocol forced (test hook SMG_TWO_WAY=1)."""
import numpy as np
import pytest

import brute
from conftest import make_table
from smudgeplot_amd import engine, ktab, synth

pytestmark = pytest.mark.gpu

M = 4000                 # base k-mers of the generator's tables: m k <= 400 000 for every k used here
_CACHE = {}


def table(k, seed=None):
    """-> (packed, counts, the oracle's plot), made once per k"""
    key = (k, seed)
    if key not in _CACHE:
        packed, cnt = synth.adversarial_table(k, M, 4, 300 + k if seed is None else seed, low_complexity=60, dense=1)
        _CACHE[key] = (packed, cnt, brute.hetmers_plot(packed, cnt, k))
    return _CACHE[key]


def tab(packed, cnt, k, ibyte):
    return make_table(dict(packed=packed, counts=cnt, k=k, ibyte=ibyte, nparts=1))


# ibyte = 3: the table comes with its prefix index, the hot form of pass 1 runs; ibyte = 1: pass 1 builds the directory
@pytest.mark.parametrize("ibyte", [3, 1])
@pytest.mark.parametrize("k", [17, 23, 25, 31, 33, 51, 63])
def test_odd_k_sends_one_way_and_agrees_with_two_way(k, ibyte, monkeypatch):
    packed, cnt, want = table(k)
    t = tab(packed, cnt, k, ibyte)
    one, st1 = engine.hetmers_run(t, symcheck="hash")
    assert st1["path"] == 1
    assert np.array_equal(one, want), "one-way against the numpy oracle"
    monkeypatch.setenv("SMG_TWO_WAY", "1")
    two, st2 = engine.hetmers_run(t, symcheck="hash")
    assert st2["path"] == 1
    assert np.array_equal(two, want), "two-way against the numpy oracle"
    print(f"k={k} ibyte={ibyte}: emitted {st1['nemitted']} one-way / {st2['nemitted']} two-way, kept {st1['nrequests']} / {st2['nrequests']}")
    assert 0 < st1["nemitted"] < st2["nemitted"]


@pytest.mark.parametrize("k", [24, 32, 64, 65])
def test_the_hook_changes_nothing_where_one_way_does_not_apply(k, monkeypatch):
    """even k (no middle base, no free bit) and three-word k-mers keep the two-way protocol"""
    packed, cnt, want = table(k)
    t = tab(packed, cnt, k, 3)
    base, st0 = engine.hetmers_run(t, symcheck="hash")
    assert st0["path"] == 1 and np.array_equal(base, want)
    monkeypatch.setenv("SMG_TWO_WAY", "1")
    plot, st = engine.hetmers_run(t, symcheck="hash")
    assert np.array_equal(plot, want)
    assert st["nemitted"] == st0["nemitted"] and st["nrequests"] == st0["nrequests"]


def test_the_exact_proof_keeps_the_two_way_protocol(monkeypatch):
    packed, cnt, want = table(31)
    t = tab(packed, cnt, 31, 3)
    base, st0 = engine.hetmers_run(t, symcheck="exact")
    monkeypatch.setenv("SMG_TWO_WAY", "1")
    plot, st = engine.hetmers_run(t, symcheck="exact")
    assert np.array_equal(base, want) and np.array_equal(plot, want)
    assert st["nemitted"] == st0["nemitted"] >= len(cnt)         # (every entry sends; the exact redo sends again)


FORMS = [{"SMG_PROBE_X": "0"}, {"SMG_PROBE_X": "1"}, {"SMG_NO_FILTER": "1"}, {"SMG_ONE_BIT_MAP": "1"},
         {"SMG_NO_INDEX_DIR": "1"}, {"SMG_FILTER_SORT_MIN": "1"}]


@pytest.mark.parametrize("env", FORMS, ids=lambda e: ",".join(f"{a}={b}" for a, b in e.items()))
@pytest.mark.parametrize("k", [31, 33])
def test_every_form_of_the_chain_applies_one_way_requests(k, env, monkeypatch):
    packed, cnt, want = table(k)
    t = tab(packed, cnt, k, 3)
    base, st0 = engine.hetmers_run(t, symcheck="hash")
    assert np.array_equal(base, want)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    plot, st = engine.hetmers_run(t, symcheck="hash")
    assert st["path"] == 1
    assert np.array_equal(plot, want), env
    assert st["nemitted"] == st0["nemitted"], env
    if "SMG_NO_FILTER" in env:
        assert st["nrequests"] == st["nemitted"]
    monkeypatch.setenv("SMG_TWO_WAY", "1")
    _, st2 = engine.hetmers_run(t, symcheck="hash")
    assert st["nemitted"] < st2["nemitted"], env


# ---- a hand-built k = 31 table --------------------------------------------------------------------------------------

def _flip(z, p, d):
    y = z.copy()
    y[p] = (y[p] + d) & 3
    return y


def hand_built_table(reps=12, seed=9):
    """every kind of complement class `reps` times (k = 31, middle position 15):
       a  a pair on the middle position only (both members of both classes: A = 1, H = 0);
       b  TELL: a lower entry z with a pair at p = 20 and one on the middle, whose complement has exactly one pair (the middle
          one): the flag of the complement comes from z's own request;
       c  ASK: the same with z upper: the complement is the lower one, a candidate that sends with f = 0, and only the reverse
          step can set its flag;
       d  both members with several pairs;
       e  a window block of 7 entries with a pair on the middle position at distance 6 (a lower and an upper member), whose
          lower member also has a partner next to it: deferred to the exact redo, which sends its request a second time."""
    k, mid = 31, 15
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(reps):
        z = rng.integers(0, 4, k, dtype=np.uint8)                                        # a
        rows += [z, _flip(z, mid, int(rng.integers(1, 4)))]
        for low in (True, False):                                                        # b, c
            z = rng.integers(0, 4, k, dtype=np.uint8)
            z[mid] = rng.integers(0, 2) + (0 if low else 2)
            rows += [z, _flip(z, 20, int(rng.integers(1, 4))), _flip(z, mid, int(rng.integers(1, 4)))]
        z = rng.integers(0, 4, k, dtype=np.uint8)                                        # d
        rows += [z, _flip(z, 18, 1), _flip(z, 22, 2), _flip(z, 5, 1), _flip(z, 9, 3)]
        z = rng.integers(0, 4, k, dtype=np.uint8)                                        # e
        z[mid], z[30] = 0, 0
        y = z.copy(); y[mid] = 2
        rows += [z, _flip(z, 30, 1), y]
        for _ in range(4):
            f = z.copy(); f[mid] = 1; f[16:] = rng.integers(0, 4, k - 16, dtype=np.uint8)
            rows.append(f)
    packed = ktab.pack_bases(np.array(rows, dtype=np.uint8))
    cnt = rng.integers(20, 60, len(rows)).astype(np.uint16)
    packed, cnt = ktab.sort_unique_packed(packed, cnt)
    packed, cnt = ktab.symmetrize(packed, cnt, k)
    return packed, cnt.astype(np.uint16)


def _labels(plot):
    s, m = np.nonzero(plot[:, :500])
    return {(int(mm), int(ss - mm)): ("1A1B", "3A1B", "2A2B")[(ss + mm) % 3] for ss, mm in zip(s.tolist(), m.tolist())}


@pytest.mark.parametrize("ibyte", [3, 1])
def test_hand_built_classes(ibyte, monkeypatch):
    k = 31
    packed, cnt = hand_built_table()
    want = brute.hetmers_plot(packed, cnt, k)
    assert want.sum() >= 24
    t = tab(packed, cnt, k, ibyte)
    plot, st = engine.hetmers_run(t, symcheck="hash")
    assert st["path"] == 1 and st["nbig"] >= 24, st                 # (kind e went through the exact redo)
    assert np.array_equal(plot, want)
    labels = _labels(want)
    lines = brute.extract_lines(packed, cnt, k, labels)
    p1, got1 = engine.hetmers_extract(t, labels)
    monkeypatch.setenv("SMG_TWO_WAY", "1")
    plot2, st2 = engine.hetmers_run(t, symcheck="hash")
    p2, got2 = engine.hetmers_extract(t, labels)
    assert np.array_equal(plot2, want)           # (middle-only classes send one-way where they never did: no fewer requests HERE)
    assert np.array_equal(p1, want) and np.array_equal(p2, want)
    one, two = {a: sorted(v) for a, v in got1.items()}, {a: sorted(v) for a, v in got2.items()}
    assert one == two == lines


def test_open_table_is_still_refuted(monkeypatch):
    """one complement removed: not symmetric, the general path gives the plot"""
    k = 31
    packed, cnt, _ = table(k)
    keep = np.ones(len(cnt), bool)
    keep[len(cnt) // 3] = False
    pa, ca = packed[keep], cnt[keep]
    want = brute.hetmers_plot(pa, ca, k)
    for ibyte in (3, 1):
        plot, st = engine.hetmers_run(tab(pa, ca, k, ibyte), symcheck="hash")
        assert st["path"] == 2, "asymmetry must be detected"
        assert np.array_equal(plot, want)
