"""Which path a table takes, host side, no GPU: `smg_hetmers_run_mode` (the run_mode_plan that host_run itself calls) over a grid
of k, entries, conditioning, proof, GPUs and free memory, against the rule restated here from the code that host_run held
before the plan was taken out of it -- with no hook and with each of the five hooks alone -- and the cases the GPU tests rely on."""
import itertools

import pytest

from conftest import load_golden
from smudgeplot_amd import engine

HOOKS = ("SMG_VIRTUAL_SHARDS", "SMG_SHARD_LIMIT", "SMG_SEQUENTIAL_SHARDS", "SMG_HBM_LIMIT", "SMG_FORCE_MULTI")
TRIM, SYMM = engine.COND_TRIM, engine.COND_SYMM
ONE_SHARD_MAX = 0xFFFFFFF0 - 16
BIG = 2.5e11
GRID = list(itertools.product((21, 31, 51, 100), (10**3, 10**6, 10**9, 5 * 10**9), (0, TRIM, TRIM | SYMM), ("hash", "exact"), (0, 4),
                              (1e9, 1e10, BIG)))
EINVAL = (-2, "more than 16 shards of 3e9 entries")
ENOMEM = (-3, "does not fit the device even shard by shard")
PINNED_SHARDS = 3          # (a code byte and the requests of every entry, and a third of the table's k-mers: what that limit was made for)


def set_hooks(monkeypatch, **env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv("SMG_" + name, str(val))
    return {"SMG_" + name: str(val) for name, val in env.items()}


def expected(k, nels, cond, sym, ngpus, free, env):
    """host_run's rule: (mode, count, cut_by_limit), or (code, part of the message)"""
    W = (k + 31) // 32
    symm = bool(cond & SYMM)
    v = env.get("SMG_VIRTUAL_SHARDS")
    ng, virt, cut = ngpus, False, 0
    if v is not None and int(v) > 1:
        ng, virt = int(v), True
    limit = int(env.get("SMG_SHARD_LIMIT", 0)) if int(env.get("SMG_SHARD_LIMIT", 0)) > 0 else ONE_SHARD_MAX
    closed = 2 * nels if symm else nels
    if ng <= 1 and closed >= limit:
        per = min(limit, 3000000000)
        ng = max(2, (closed + per - 1) // per)
        if ng > 16:
            return EINVAL
        virt, cut = True, ng
    seq = 0
    if ng <= 1 or virt:
        if int(env.get("SMG_SEQUENTIAL_SHARDS", 0)) > 1:
            seq = min(int(env["SMG_SEQUENTIAL_SHARDS"]), 16)
        else:
            mem = float(env["SMG_HBM_LIMIT"]) if float(env.get("SMG_HBM_LIMIT", 0)) > 0 else 0.9 * free
            ne = float(nels) * (2.0 if symm else 1.0)
            per_run = 10.6 * W + 5.5
            per_cond = (24.0 * W + 30.0 if symm else 8.0 * W + 12.0) if cond else 0.0
            if ne * max(per_run, per_cond) + 1.1e9 > mem:
                keep = ne * (1.0 + (8.0 * (W + 1) if sym == "exact" else 0.36 * 8.0 * (W + 1 if k > 85 else W)))
                for q in range(2, 17):
                    if keep + ne / q * per_run <= mem and ne / q * per_cond <= mem and ne / q < ONE_SHARD_MAX:
                        seq = q
                        break
                if not seq:
                    return ENOMEM
    if seq:
        return ("sequential", seq, cut)
    if ng > 1:
        return ("virtual" if virt or (v is not None and int(v) > 0) else "multi", min(ng, 16), cut)
    if "SMG_FORCE_MULTI" in env and v is None:
        return ("one_rank_forced", 1, cut)
    return ("core", 1, cut)


def got(k, nels, cond, sym, ngpus, free):
    try:
        m = engine.run_mode(k, nels, free, sym, cond, ngpus)
    except engine.EngineError as err:
        return err
    return (m["mode"], m["count"], m["cut_by_limit"])


def check(k, nels, cond, sym, ngpus, free, env):
    want, have = expected(k, nels, cond, sym, ngpus, free, env), got(k, nels, cond, sym, ngpus, free)
    if isinstance(want[0], int):
        assert isinstance(have, engine.EngineError) and have.code == want[0] and want[1] in str(have), (k, nels, cond, sym, ngpus, free, env)
    else:
        assert have == want, (k, nels, cond, sym, ngpus, free, env)
    return want


@pytest.mark.parametrize("env", [{}, {"VIRTUAL_SHARDS": 3}, {"VIRTUAL_SHARDS": 1}, {"SHARD_LIMIT": 1000}, {"SHARD_LIMIT": 10**8},
                                 {"SEQUENTIAL_SHARDS": 5}, {"HBM_LIMIT": 2 * 10**9}, {"HBM_LIMIT": 3 * 10**10}, {"FORCE_MULTI": 1}],
                         ids=lambda e: "-".join(f"{a}={b}" for a, b in e.items()) or "no_hook")
def test_the_plan_is_host_runs_rule_over_the_grid(monkeypatch, env):
    env = set_hooks(monkeypatch, **env)
    seen = set()
    for case in GRID:
        want = check(*case, env)
        seen.add(want[0])
    if not env:                        # the grid reaches every outcome that needs no hook
        assert seen == {"core", "virtual", "sequential", "multi", -3}


def test_the_shard_limit_cuts_a_table_by_its_closed_size(monkeypatch):
    set_hooks(monkeypatch, SHARD_LIMIT=1000)
    assert got(31, 5000, 0, "hash", 0, BIG) == ("virtual", 5, 5)
    assert got(31, 2500, TRIM | SYMM, "hash", 0, BIG) == ("virtual", 5, 5)
    err = got(31, 17000, 0, "hash", 0, BIG)
    assert err.code == -2 and "more than 16 shards of 3e9 entries" in str(err)
    assert got(31, 999, 0, "hash", 0, BIG) == ("core", 1, 0)


def test_the_forced_modes(monkeypatch):
    set_hooks(monkeypatch, VIRTUAL_SHARDS=3)
    assert got(31, 10**6, 0, "hash", 0, BIG) == ("virtual", 3, 0)
    set_hooks(monkeypatch, VIRTUAL_SHARDS=3, SEQUENTIAL_SHARDS=4)
    assert got(31, 10**6, 0, "hash", 0, BIG) == ("sequential", 4, 0)
    set_hooks(monkeypatch, SEQUENTIAL_SHARDS=20)
    assert got(31, 10**6, 0, "hash", 0, BIG) == ("sequential", 16, 0)
    set_hooks(monkeypatch)
    assert got(31, 5 * 10**9, 0, "hash", 4, 1.0) == ("multi", 4, 0)              # several GPUs: no memory check, no cut
    set_hooks(monkeypatch, FORCE_MULTI=1)
    assert got(31, 10**6, 0, "hash", 0, BIG) == ("one_rank_forced", 1, 0)
    set_hooks(monkeypatch, FORCE_MULTI=1, VIRTUAL_SHARDS=1)
    assert got(31, 10**6, 0, "hash", 0, BIG) == ("core", 1, 0)
    set_hooks(monkeypatch, FORCE_MULTI=1, VIRTUAL_SHARDS=2)
    assert got(31, 10**6, 0, "hash", 0, BIG) == ("virtual", 2, 0)


def test_the_memory_hook_overrides_the_free_bytes(monkeypatch):
    set_hooks(monkeypatch, HBM_LIMIT=1000)
    err = got(31, 10**6, 0, "hash", 0, BIG)
    assert err.code == -3 and "does not fit the device even shard by shard" in str(err)
    set_hooks(monkeypatch, HBM_LIMIT=10**12)
    assert got(31, 10**9, 0, "hash", 0, 1.0) == ("core", 1, 0)
    set_hooks(monkeypatch)
    assert got(31, 10**9, 0, "hash", 0, 1e10)[0] == "sequential" and got(31, 10**9, 0, "hash", 0, BIG) == ("core", 1, 0)


def test_the_limits_of_the_out_of_core_test(monkeypatch):
    """the two SMG_HBM_LIMIT values of test_out_of_core_mode_is_chosen_from_the_free_memory.. (tests/test_gpu_parity.py; the
    executable's default proof is the hash proof)"""
    n = len(load_golden("k31_i3_p4")["counts"])
    env = set_hooks(monkeypatch, HBM_LIMIT=int(n * 3.4 + n / 3 * 22 + 1000))
    assert check(31, n, 0, "hash", 0, BIG, env) == ("sequential", PINNED_SHARDS, 0)
    env = set_hooks(monkeypatch, HBM_LIMIT=int(n * 3.0))
    assert check(31, n, 0, "hash", 0, BIG, env) == ENOMEM
