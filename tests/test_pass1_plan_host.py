"""What pass 1 of the fast path decides, host side, no GPU: `smg_engine_pass1_plan` (the p1_plan / p1_form that fast_pass1 itself
calls) over the whole grid of k, proof, caller, index, map cap and no_filter, against the rules the engine states -- restated
here from k alone --, the same under each of the five test hooks it reads, and the (k -> form) cases that section 1 of
tests/test_pass1_forms_gpu.py asserts on a device, as plan look-ups."""
import itertools

import pytest

from smudgeplot_amd import engine

HOOKS = ("SMG_TWO_WAY", "SMG_NO_FILTER", "SMG_ONE_BIT_MAP", "SMG_SIG", "SMG_BM_BITS")
N = 100000
GRID = list(itertools.product(range(1, 86), ("hash", "exact"), (True, False), (True, False), (30, 32), (False, True)))


def clear(monkeypatch, **env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv("SMG_" + name, str(val))


def expected(k, sym, own, index, cap, no_filter, env, n=N):
    """the rules of smg_hetmers.hip (p1_plan, p1_form, bm_id_bits, filter_ok), from k and the switches alone"""
    W = (k + 31) // 32
    exact, hashp = sym == "exact", sym == "hash"
    rw = W + (1 if exact or W == 3 else 0)
    key_only = rw == W
    narrow = W <= 2
    one_way = k % 2 == 1 and 3 <= k <= 63 and key_only and hashp and own and "TWO_WAY" not in env
    covered = k >= 2 and ((W == 1 and rw == 1) or (W == 2 and rw != 1) or (W == 3 and rw == 4))
    bits = 0
    if covered and not exact and not no_filter and "NO_FILTER" not in env:
        if 8 <= int(env.get("BM_BITS", 0)) <= 32:
            cap = int(env["BM_BITS"])
        bits = min(cap, 2 * k if cap > 30 else 2 * (k // 2))
    chain = bits >= 12 and narrow and key_only
    bm2 = chain and k >= 24 and "ONE_BIT_MAP" not in env
    sig = narrow and not (chain and bm2 and bits >= 32)
    if "SIG" in env and narrow:
        sig = int(env["SIG"]) != 0
    preset = index and not exact and narrow and n > 0
    hot = key_only and preset and not sig and bm2 and hashp and chain
    var = 0 if (not narrow or n == 0) else 1 if not hot else 6 if (k % 2 == 1 and not one_way) else 2
    nb = max(1, min(10, bits - 2 - 20)) if chain else 0
    return {"rw": rw, "one_way": int(one_way), "narrow": int(narrow), "dir_per": 8 if (exact or W > 1) else 64,
            "dir_preset": int(preset), "bm_bits": bits, "bm2": int(bm2), "nb": nb, "use_sig": int(sig), "var": var,
            "kf": int(W == 1 and 17 <= k <= 32), "w": W}


def check_grid(env, n=N):
    for k, sym, own, index, cap, no_filter in GRID:
        got = engine.pass1_plan(k, n, sym, own, index, cap, no_filter)
        want = expected(k, sym, own, index, cap, no_filter, env, n)
        assert got == want, (k, sym, own, index, cap, no_filter, env)
        # ... and the invariants one by one, as the engine's comments state them
        W = (k + 31) // 32
        assert got["rw"] == W + (sym == "exact" or W == 3)
        assert got["var"] in ((1, 2, 6) if W <= 2 and n > 0 else (0,))
        assert (got["nb"] > 0) == (got["bm_bits"] >= 12 and W <= 2 and got["rw"] == W)
        assert got["bm2"] <= (got["nb"] > 0)
        if got["var"] in (2, 6):
            assert got["rw"] == W and got["dir_preset"] and not got["use_sig"] and got["bm2"] and sym == "hash" and got["nb"]
            assert got["var"] == (6 if k % 2 and not got["one_way"] else 2)
        if got["one_way"]:
            assert k % 2 == 1 and 3 <= k <= 63 and got["rw"] == W and sym == "hash" and own


def test_the_whole_grid_without_hooks(monkeypatch):
    clear(monkeypatch)
    check_grid({})
    # the rules that have no hook in them, spelled out
    for k, sym, own, index, cap, no_filter in GRID:
        got = engine.pass1_plan(k, N, sym, own, index, cap, no_filter)
        W = (k + 31) // 32
        key_only = got["rw"] == W
        assert got["one_way"] == int(k % 2 == 1 and 3 <= k <= 63 and key_only and sym == "hash" and own)
        chain = got["nb"] > 0
        assert got["bm2"] == int(chain and k >= 24)
        if W <= 2:
            assert (not got["use_sig"]) == (chain and got["bm2"] == 1 and got["bm_bits"] == 32)
        hot = key_only and index and not got["use_sig"] and got["bm2"] and sym == "hash" and chain
        assert (got["var"] in (2, 6)) == bool(hot)
        if W == 3:
            assert got["var"] == 0 and got["narrow"] == 0 and got["use_sig"] == 0


@pytest.mark.parametrize("env", [{"TWO_WAY": 1}, {"NO_FILTER": 1}, {"ONE_BIT_MAP": 1}, {"SIG": 0}, {"SIG": 1},
                                 {"BM_BITS": 14}, {"BM_BITS": 8}, {"BM_BITS": 30}, {"BM_BITS": 32}, {"BM_BITS": 7}, {"BM_BITS": 33}],
                         ids=lambda e: "-".join(f"{a}={b}" for a, b in e.items()))
def test_the_whole_grid_under_each_hook(env, monkeypatch):
    clear(monkeypatch, **env)
    check_grid({a: str(b) for a, b in env.items()})


def test_an_empty_table_launches_nothing(monkeypatch):
    clear(monkeypatch)
    check_grid({}, n=0)
    assert engine.pass1_plan(31, 0)["var"] == 0 and engine.pass1_plan(31, 0)["dir_preset"] == 0


def test_what_the_plan_refuses():
    for args in ((0, N), (86, N), (31, -1)):
        with pytest.raises(engine.EngineError):
            engine.pass1_plan(*args)
    with pytest.raises(engine.EngineError):
        engine.pass1_plan(31, N, "none")


# ---- the cases of tests/test_pass1_forms_gpu.py, section 1 ("which form a run launches") ------------------------------------

def words_of(k):
    return (k + 31) // 32


def form(plan):
    return {"var": plan["var"], "w": plan["w"], "rw": plan["rw"]}


@pytest.mark.parametrize("k", [25, 31, 33, 63])
def test_odd_k_with_its_index_plans_the_one_way_hot_form(k, monkeypatch):
    clear(monkeypatch)
    assert form(engine.pass1_plan(k, N)) == {"var": 2, "w": words_of(k), "rw": words_of(k)}
    clear(monkeypatch, TWO_WAY=1)
    assert form(engine.pass1_plan(k, N)) == {"var": 6, "w": words_of(k), "rw": words_of(k)}


@pytest.mark.parametrize("k", [25, 31, 33, 63])
def test_the_phase_api_plans_the_two_way_hot_form(k, monkeypatch):
    clear(monkeypatch)
    p = engine.pass1_plan(k, N, own_lookups=False, bm_cap=32)               # (set_blockmap_bits(32))
    assert p["one_way"] == 0 and p["bm2"] == 1 and p["bm_bits"] == 32
    assert form(p) == {"var": 6, "w": words_of(k), "rw": words_of(k)}
    # the default map of the phase API (30 id bits, to be exchanged) comes with signatures: the general form
    assert engine.pass1_plan(k, N, own_lookups=False, bm_cap=30)["var"] == 1


@pytest.mark.parametrize("k", [24, 32, 64])
def test_even_k_has_one_hot_form(k, monkeypatch):
    for env in ({}, {"TWO_WAY": 1}):
        clear(monkeypatch, **env)
        assert form(engine.pass1_plan(k, N)) == {"var": 2, "w": words_of(k), "rw": words_of(k)}, env


@pytest.mark.parametrize("what", ["ibyte1", "k17", "k23", "exact", "no_index_hook"])
def test_what_keeps_the_general_form(what, monkeypatch):
    k = {"k17": 17, "k23": 23}.get(what, 31)
    clear(monkeypatch)
    # (an index of one byte per prefix, or SMG_NO_INDEX_DIR: smg_engine_set_prefix_index keeps no directory)
    p = engine.pass1_plan(k, N, "exact" if what == "exact" else "hash", have_index=what not in ("ibyte1", "no_index_hook"))
    assert p["var"] == 1 and p["w"] == 1 and p["rw"] == (2 if what == "exact" else 1), p
