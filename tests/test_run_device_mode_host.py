"""Which way a table that is already on the device runs, host side, no GPU: `smg_hetmers_run_device_mode` (the run_device_plan
that smg_hetmers_run_device itself calls) over a grid of k, entries, conditioning and free memory.  In core exactly where the
two tests that entry has always made pass -- restated here from core_bytes' constants --, elsewhere, for a table that is to be
closed, the smallest number of prefix shards that meets the two conditions of the plan, recomputed here from the price
function stated in DESIGN.md section 7e; the two hooks of this plan, the three of the other plan that must not move it, and the
refusals."""
import itertools

import pytest

from smudgeplot_amd import engine

HOOKS = ("SMG_VIRTUAL_SHARDS", "SMG_SHARD_LIMIT", "SMG_SEQUENTIAL_SHARDS", "SMG_HBM_LIMIT", "SMG_FORCE_MULTI", "SMG_DEVICE_SHARDS",
         "SMG_DEVICE_SHARD_LIMIT")
TRIM, SYMM = engine.COND_TRIM, engine.COND_SYMM
ONE_SHARD_MAX = 2**32 - 32
TWO_STEP = "hetmers"
GRID = list(itertools.product((21, 31, 33, 65, 100), (0, 1000, 10**6, 10**8, 10**9, 2 * 10**9, 2147483631, 2147483632, 4 * 10**9, 5 * 10**9),
                              (0, SYMM, TRIM | SYMM), ("hash", "exact"), (1e9, 1e10, 6e10, 2.5e11)))


def set_hooks(monkeypatch, **env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv("SMG_" + name, str(val))


def core_need(k, nels, cond):
    """today's second test: core_bytes, less the table itself where it is run as it is"""
    W = (k + 31) // 32
    ne = float(nels) * (2.0 if cond & SYMM else 1.0)
    per_run = 10.6 * W + 5.5
    per_cond = (24.0 * W + 30.0 if cond & SYMM else 8.0 * W + 12.0) if cond else 0.0
    return ne * max(per_run, per_cond) + 1.1e9 - (0.0 if cond else float(nels) * (8.0 * W + 2.0))


def closure_price(W):
    """bytes per entry of a shard while it is closed: sorting its complements, then merging them with the slice"""
    return max(8.0 * W + 2.0 + 24.0, 2.0 * (8.0 * W + 2.0) + 4.0)


def expected(k, nels, cond, sym, free, limit=ONE_SHARD_MAX, forced=0, mem=None):
    W = (k + 31) // 32
    symm = bool(cond & SYMM)
    ne = float(nels) * (2.0 if symm else 1.0)
    mem = 0.9 * free if mem is None else mem
    by_size = ne >= limit
    if nels >= ONE_SHARD_MAX or (by_size and not symm):
        return (-3, "one engine does not address them")
    by_mem = core_need(k, nels, cond) > mem
    if not by_size and not by_mem and not (forced and symm):
        return ("core", 1, 0)
    q = 0
    if symm and forced:
        q = forced
    elif symm:
        resident = (float(nels) * (8.0 * W + 2.0) if cond & TRIM else 0.0) \
            + ne * (1.0 + (8.0 * (W + 1) if sym == "exact" else 0.36 * 8.0 * (W + 1 if k > 85 else W)))
        shard = max(closure_price(W), 10.6 * W + 5.5)
        for c in range(2, 17):
            if ne / c < limit and resident + ne / c * shard <= mem:
                q = c
                break
    if not q:
        return (-3, "does not fit the device in core")
    return ("sequential", q, q if by_size else 0)


def got(k, nels, cond, sym, free, ngpus=0):
    try:
        m = engine.run_device_mode(k, nels, free, sym, cond, ngpus)
    except engine.EngineError as err:
        return err
    return (m["mode"], m["count"], m["cut_by_limit"])


def check(case, **kw):
    want, have = expected(*case, **kw), got(*case)
    if isinstance(want[0], int):
        assert isinstance(have, engine.EngineError) and have.code == want[0] and want[1] in str(have) and TWO_STEP in str(have), (case, kw, have)
    else:
        assert have == want, (case, kw)
    return want


def test_the_plan_over_the_grid(monkeypatch):
    set_hooks(monkeypatch)
    seen = set()
    for case in GRID:
        want = check(case)
        k, nels, cond, sym, free = case
        in_core_today = nels * (2 if cond & SYMM else 1) < ONE_SHARD_MAX and core_need(k, nels, cond) <= 0.9 * free
        assert (want == ("core", 1, 0)) == in_core_today, case          # in core exactly where today's two tests pass
        if not in_core_today and not cond & SYMM:
            assert isinstance(want[0], int), case                          # nothing to close: no shards
        seen.add((want[0], bool(want[2])) if not isinstance(want[0], int) else want)
    assert ("core", False) in seen and ("sequential", False) in seen and ("sequential", True) in seen
    assert (-3, "does not fit the device in core") in seen and (-3, "one engine does not address them") in seen


def test_the_smallest_number_of_shards_that_fits(monkeypatch):
    set_hooks(monkeypatch)
    # a human read set at k = 31: 2.5e9 canonical entries close to 5e9, beyond one engine; two shards of 2.5e9 fit 288 GB
    assert got(31, 2_500_000_000, TRIM | SYMM, "hash", 2.8e11) == ("sequential", 2, 2)
    # the same table and a tenth of the memory: more shards, the size still being what forced the cut
    q = got(31, 2_500_000_000, TRIM | SYMM, "hash", 1.2e11)
    assert q[0] == "sequential" and q[1] > 2 and q[2] == q[1]
    assert expected(31, 2_500_000_000, TRIM | SYMM, "hash", 1.2e11) == q
    # memory alone: out[2] stays 0
    m = got(31, 10**9, SYMM, "hash", 6e10)
    assert m[0] == "sequential" and m[2] == 0 and m == expected(31, 10**9, SYMM, "hash", 6e10)


def test_the_two_hooks_of_this_plan(monkeypatch):
    set_hooks(monkeypatch, DEVICE_SHARDS=3)
    assert got(31, 1000, TRIM | SYMM, "hash", 2.5e11) == ("sequential", 3, 0)
    assert got(31, 1000, 0, "hash", 2.5e11) == ("core", 1, 0)               # nothing to close: nothing to shard
    set_hooks(monkeypatch, DEVICE_SHARDS=40)
    assert got(31, 1000, SYMM, "hash", 2.5e11) == ("sequential", 16, 0)
    set_hooks(monkeypatch, DEVICE_SHARDS=1)
    assert got(31, 1000, SYMM, "hash", 2.5e11) == ("core", 1, 0)
    set_hooks(monkeypatch, DEVICE_SHARD_LIMIT=1999)
    assert got(31, 1000, SYMM, "hash", 2.5e11) == ("sequential", 2, 2)      # 2 n = 2000 >= 1999, 2 n / 2 below it
    assert got(31, 999, SYMM, "hash", 2.5e11) == ("core", 1, 0)
    assert got(31, 5000, SYMM, "hash", 2.5e11) == ("sequential", 6, 6)      # 10000 / 5 = 2000 is not below 1999
    for case in GRID:
        check(case, limit=1999)
    set_hooks(monkeypatch, DEVICE_SHARD_LIMIT=1999, DEVICE_SHARDS=2)
    assert got(31, 5000, SYMM, "hash", 2.5e11) == ("sequential", 2, 2)      # (the run raises the number where a shard is too large)


def test_the_hooks_of_the_other_plan_change_nothing(monkeypatch):
    for env in ({"VIRTUAL_SHARDS": 3}, {"SHARD_LIMIT": 1000}, {"SEQUENTIAL_SHARDS": 5}, {"FORCE_MULTI": 1}):
        set_hooks(monkeypatch, **env)
        for case in GRID:
            check(case)


def test_the_memory_hook_stands_in_for_the_free_bytes(monkeypatch):
    set_hooks(monkeypatch, HBM_LIMIT=1000)
    for cond in (0, SYMM, TRIM | SYMM):
        err = got(21, 20000, cond, "hash", 2.5e11)
        assert err.code == -3 and "does not fit the device in core" in str(err) and TWO_STEP in str(err)
        assert ("16 prefix shards" in str(err)) == bool(cond & SYMM)
    set_hooks(monkeypatch, HBM_LIMIT=10**12)
    assert got(31, 10**9, SYMM, "hash", 1.0) == ("core", 1, 0)
    set_hooks(monkeypatch, HBM_LIMIT=3 * 10**10)
    for case in GRID:
        check(case, mem=3e10)


def test_the_refusals_that_stay(monkeypatch):
    set_hooks(monkeypatch)
    err = got(31, 1000, SYMM, "hash", 2.5e11, ngpus=2)
    assert err.code == -2 and "ngpus" in str(err)
    set_hooks(monkeypatch, DEVICE_SHARDS=4)
    for cond in (0, SYMM):
        err = got(31, ONE_SHARD_MAX, cond, "hash", 1e13)                       # C itself beyond one engine: the hook does not help
        assert err.code == -3 and "one engine does not address them" in str(err) and TWO_STEP in str(err)
    err = got(31, 3 * 10**9, 0, "hash", 1e13)
    assert isinstance(err, tuple) and err == ("core", 1, 0)                    # not closed, below 2^32 - 32: in core as ever
