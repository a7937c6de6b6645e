"""What the stage between pass 1 and pass 2 of the fast path decides, host side, no GPU: `smg_engine_lookup_plan` (the
list_capacity / presort_plan / filter_plan / probe_plan / apply_plan that the launch functions of smg_fast_lookup.hpp themselves
call) over grids of k, record, bucket bits, counts and compute units, against the rules the engine states -- restated here --,
the same under each of the seven test hooks the plans see (five they read; SMG_P1_GRID arrives as the grid, SMG_TWO_WAY as
one_way), and the cases that tests/test_list_lookups_gpu.py, tests/test_lookup_regimes_gpu.py and
tests/test_wide_fast_path_gpu.py assert on a device through apply_state / lookup_state, as plan look-ups.  Every threshold comes
from the library's own smg_engine_*_limits."""
import functools
import itertools

import pytest

import list_oracle as lz
import lookup_oracle as lo
from smudgeplot_amd import engine

HOOKS = ("SMG_FILTER_SORT_MIN", "SMG_FILTER_GRID", "SMG_PROBE_X", "SMG_PX_ONE_XCC", "SMG_APPLY_SORT_MIN")
KS = (17, 24, 31, 32, 33, 51, 63, 64, 65, 85)
NBS = (0, 2, 3, 10)
PX_WGS = 4                                 # workgroups of kl_probe_x per compute unit (smg_lookup.hpp; not among the exported limits)
CAP = 0x7FFFFFFF
NONE, BUCKETED, ASIS, CHAIN = range(4)                                   # engine.PRESORTS
R_NONE, R_FUSED, R_SENTINELS, R_COMPACTED, R_FLAT = range(5)             # engine.APPLY_ROUTES
K_NONE, K_PLAIN, K_INDEXED, K_SORTED = range(4)                          # Engine.APPLY_KERNELS
H_NONE, H_SENTINELS, H_COMPACTED = range(3)                              # Engine.APPLY_HOLES


@functools.lru_cache(maxsize=None)
def lim():
    L = dict(engine.list_limits())
    L.update(engine.lookup_limits())
    assert L["SORT_MIN"] == engine.wide_limits()["SORT_MIN"]
    return L


def clear(monkeypatch, **env):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv("SMG_" + name, str(val))


def words_of(k):
    return (k + 31) // 32


def floor_at_sort_min(env, name, default):
    """SMG_APPLY_SORT_MIN / SMG_FILTER_SORT_MIN: any integer, raised to SORT_MIN"""
    return max(lim()["SORT_MIN"], int(env[name]) if name in env else default)


def fewer_never_more(env, name, grid):
    """the *_GRID hooks: 1 <= g < grid lowers the grid, anything else is ignored"""
    g = int(env.get(name, 0))
    return g if 1 <= g < grid else grid


# ---- the rules of smg_fast_host.hpp (list_capacity) and smg_fast_lookup.hpp, restated -------------------------------------------

def want_capacity(want_rec, grid, chain, have):
    L = lim()
    maxc = -(-want_rec // L["F_CH"])
    if chain:
        G = grid + L["BF_MAXGRID"]
        per = -(-maxc // grid) + 2
        if maxc < per * G < CAP:
            maxc = per * G
    if maxc < have < CAP:
        maxc = have
    return maxc


def want_presort(k, rw, nb, n_chunks, env):
    if nb:
        return CHAIN
    L = lim()
    long = n_chunks * L["F_CH"] >= floor_at_sort_min(env, "FILTER_SORT_MIN", L["FILTER_SORT_MIN"])
    return BUCKETED if rw == 1 and long and k < 32 else ASIS


def want_filter(cus, n_chunks, nrequests, chain, seen, env):
    L = lim()
    grid = fewer_never_more(env, "FILTER_GRID", min(2 * cus, n_chunks))
    maxout = n_chunks + grid + 16
    if chain:
        maxout = max(min(cus * lo.PB_WAVES + nrequests // (L["F_CH"] - 63) + 16, CAP), n_chunks + 16)
    if seen >= 0 and seen + 64 < maxout:
        maxout = seen + 64
    return grid, maxout


def want_probe(lst, nb, one_way, nbig, nemitted, n, cus, env):
    """-> (form, requests per ticket, one XCD, grid)"""
    if not nb:
        return 0, 0, 0, 0
    L = lim()
    many = nemitted * 100 > n * (14 if one_way else 28)
    x = (nbig > 0 and nbig * 400 > n) or many
    if "PROBE_X" in env:
        x = int(env["PROBE_X"]) != 0
    if not lst and nb >= 3 and x:
        return 2, L["PX_PART"] if many else 2 * L["PX_PART"], int("PX_ONE_XCC" in env), cus * PX_WGS
    return 3 if lst else 1, 0, 0, min(cus, 1 << nb)


def want_apply(flat, k, rw, n_chunks, nrec, filtered, bm_bits, nb, env):
    """-> route, kernel, sorted, holes, covered, filter_first"""
    L = lim()
    keys_only = words_of(k) == 1 and rw == 1
    if not flat and bm_bits and not filtered:
        return (R_FUSED, K_NONE, 0, H_NONE, 0, 0) if nb else (R_NONE, K_NONE, 0, H_NONE, 0, 1)
    if nrec <= 0 or (not flat and n_chunks == 0):
        return R_NONE, K_NONE, 0, H_NONE, 0, 0
    nslots = n_chunks * L["F_CH"]
    if flat:
        route, holes, covered = R_FLAT, H_NONE, nrec
    elif keys_only and nslots <= nrec + nrec // 8 and nslots >= L["SORT_MIN"] and k < 32:
        route, holes, covered = R_SENTINELS, H_SENTINELS, nslots
    else:
        route, holes, covered = R_COMPACTED, H_COMPACTED, nrec
    if keys_only:
        return route, K_SORTED, int(covered >= floor_at_sort_min(env, "APPLY_SORT_MIN", L["APPLY_SORT_MIN"])), holes, covered, 0
    long = L["SORT_MIN"] <= covered < 0xFFFFFFF0
    return route, K_INDEXED if long else K_PLAIN, int(long), holes, covered, 0


def expected(env, k, **a):
    a = {**engine.LOOKUP_PLAN_IN, "k": k, "rw": words_of(k), **a}
    chain = a["nb"] != 0
    grid, maxout = want_filter(a["cus"], a["n_chunks"], a["nrequests"], chain, a["seen_chunks"], env)
    form, part, one_xcd, pgrid = want_probe(a["list"], a["nb"], a["one_way"], a["nbig"], a["nemitted"], a["n"], a["cus"], env)
    route, kernel, srt, holes, covered, first = want_apply(a["flat"], k, a["rw"], a["n_chunks"], a["nrec"], a["filtered"], a["bm_bits"],
                                                           a["nb"], env)
    return {"max_chunks": want_capacity(a["want_rec"], a["grid"], chain, a["have_chunks"]),
            "presort": want_presort(k, a["rw"], a["nb"], a["n_chunks"], env), "filter_grid": grid, "maxout": maxout,
            "probe_form": form, "probe_part": part, "one_xcd": one_xcd, "probe_grid": pgrid,
            "route": route, "kernel": kernel, "sorted": srt, "holes": holes, "covered": covered, "filter_first": first}


def check(env, k, **a):
    got, want = engine.lookup_plan(k, **a), expected(env, k, **a)
    assert got == want, (env, k, a, {f: (got[f], want[f]) for f in got if got[f] != want[f]})
    return got


# ---- the grids -----------------------------------------------------------------------------------------------------------

def records_of(k):
    """(rw, nb, bm_bits) an engine can have at this k: the chain wants key-only records of k <= 64 and a map of >= 12 id bits"""
    W = words_of(k)
    for rw in ((W, W + 1) if W < 3 else (4,)):
        for nb in NBS:
            if nb and (rw != W or W > 2):
                continue
            for bm_bits in ((32,) if nb else (0, 10)):
                yield rw, nb, bm_bits


def chunk_counts():
    """chunks whose slots lie on both sides of SORT_MIN (none at all, or one chunk), APPLY_SORT_MIN and FILTER_SORT_MIN"""
    L = lim()
    a, f = L["APPLY_SORT_MIN"] // L["F_CH"], L["FILTER_SORT_MIN"] // L["F_CH"]
    assert L["SORT_MIN"] == L["F_CH"] and a * L["F_CH"] == L["APPLY_SORT_MIN"] and f * L["F_CH"] == L["FILTER_SORT_MIN"]
    return (0, 1, 3, a - 1, a, f - 1, f)


def record_counts(n_chunks):
    """records on both sides of SORT_MIN, APPLY_SORT_MIN, FILTER_SORT_MIN and of nslots <= nreq + nreq / 8"""
    L = lim()
    nslots = n_chunks * L["F_CH"]
    brim = next(r for r in range(nslots * 8 // 9 - 2, nslots + 1) if nslots <= r + r // 8)       # the fewest records that are "brim-full"
    assert nslots > (brim - 1) + (brim - 1) // 8 or brim == 0
    out = {0, 1, L["SORT_MIN"] - 1, L["SORT_MIN"], L["APPLY_SORT_MIN"] - 1, L["APPLY_SORT_MIN"], L["FILTER_SORT_MIN"] - 1,
           L["FILTER_SORT_MIN"], max(brim - 1, 0), brim, nslots}
    return sorted(out)


def sweep_lists(env):
    """presort and apply (and the filter's sizes with them): every record, bucket count and list length"""
    seen_routes, seen_presorts = set(), set()
    for k in KS:
        for rw, nb, bm_bits in records_of(k):
            for n_chunks in chunk_counts():
                for nrec, flat, filtered in itertools.product(record_counts(n_chunks), (0, 1), (0, 1)):
                    got = check(env, k, rw=rw, nb=nb, bm_bits=bm_bits, n_chunks=n_chunks, nrequests=nrec, nrec=nrec, flat=flat,
                                filtered=filtered)
                    seen_routes.add((got["route"], got["kernel"], got["sorted"]))
                    seen_presorts.add(got["presort"])
    assert seen_presorts == {BUCKETED, ASIS, CHAIN}
    assert {r for r, _, _ in seen_routes} == {R_NONE, R_FUSED, R_SENTINELS, R_COMPACTED, R_FLAT}
    assert {(c, s) for _, c, s in seen_routes} == {(K_NONE, 0), (K_PLAIN, 0), (K_INDEXED, 1), (K_SORTED, 0), (K_SORTED, 1)}


def sweep_probe(env):
    """nbig * 400 and nemitted * 100 on both sides of their thresholds, one-way and two-way, list and fused, nb = 2, 3, 10"""
    n = 100000
    forms = set()
    for k in (17, 24, 31, 32, 33, 51, 63, 64):
        for nb, lst, one_way, cus in itertools.product((2, 3, 10), (0, 1), (0, 1) if k % 2 else (0,), (1, 6, 256, 304)):
            share = 14 if one_way else 28
            for nbig, nemitted in itertools.product((0, 1, n // 400, n // 400 + 1), (0, n * share // 100, n * share // 100 + 1)):
                got = check(env, k, nb=nb, bm_bits=32, list=lst, one_way=one_way, cus=cus, nbig=nbig, nemitted=nemitted, n=n,
                            n_chunks=100, nrequests=nemitted, nrec=nemitted)
                forms.add((got["probe_form"], got["probe_part"]))
    L = lim()
    if "PROBE_X" not in env:
        assert forms == {(1, 0), (3, 0), (2, L["PX_PART"]), (2, 2 * L["PX_PART"])}


def sweep_filter(env):
    L = lim()
    for cus, n_chunks, chain, seen in itertools.product((1, 104, 256), (1, 2, 207, 208, 209, 511, 512, 513, 100000), (0, 1),
                                                        (-1, 0, 10, 10 ** 6)):
        for nreq in (0, n_chunks * L["F_CH"] * 3 // 4, n_chunks * L["F_CH"], 1 << 43):
            check(env, 31, nb=10 if chain else 0, bm_bits=32 if chain else 10, cus=cus, n_chunks=n_chunks, nrequests=nreq, nrec=nreq,
                  seen_chunks=seen)


def capacity_edge(grid):
    """the fewest chunks at which the owners' stride no longer fits 31 bits"""
    G = grid + lim()["BF_MAXGRID"]
    c = (CAP // G - 2) * grid
    while not (-(-c // grid) + 2) * G >= CAP:
        c += 1
    while (-(-(c - 1) // grid) + 2) * G >= CAP:
        c -= 1
    return c


def sweep_capacity(env):
    """SMG_P1_GRID arrives as the grid: one workgroup, two, a device's worth, the most"""
    L = lim()
    for grid, chain in itertools.product((1, 2, 1280, 4096), (0, 1)):
        edge = capacity_edge(grid)
        for chunks in (0, 1, 100, 1280, 5000, edge - 1, edge, edge + 1, CAP // 2):
            for have in (0, 1, chunks, chunks + 1, 10 * chunks + 7, (grid + L["BF_MAXGRID"]) * (chunks // grid + 3), CAP - 1, CAP):
                want_rec = chunks * L["F_CH"] - (1 if chunks else 0)
                got = check(env, 31, nb=10 if chain else 0, bm_bits=32, want_rec=want_rec, grid=grid, have_chunks=have)
                assert chunks <= got["max_chunks"] < CAP and (have >= CAP or got["max_chunks"] >= have), (grid, chain, chunks, have, got)
        # where per * G first exceeds 31 bits the stride is dropped, the capacity stays a chunk count and does not wrap
        if chain:
            below = engine.lookup_plan(31, nb=10, bm_bits=32, want_rec=(edge - 1) * L["F_CH"], grid=grid)["max_chunks"]
            at = engine.lookup_plan(31, nb=10, bm_bits=32, want_rec=edge * L["F_CH"], grid=grid)["max_chunks"]
            assert edge - 1 < below < CAP and at == edge, (grid, edge, below, at)


def sweep(env):
    sweep_lists(env)
    sweep_probe(env)
    sweep_filter(env)
    sweep_capacity(env)


def test_the_whole_grid_without_hooks(monkeypatch):
    clear(monkeypatch)
    sweep({})


def hook_cases():
    L = engine.list_limits()
    s = L["SORT_MIN"]
    return [{"FILTER_SORT_MIN": s}, {"FILTER_SORT_MIN": s - 1}, {"FILTER_SORT_MIN": 0}, {"FILTER_SORT_MIN": L["APPLY_SORT_MIN"]},
            {"APPLY_SORT_MIN": s}, {"APPLY_SORT_MIN": s - 1}, {"APPLY_SORT_MIN": -5}, {"APPLY_SORT_MIN": 3 * s},
            {"FILTER_GRID": 1}, {"FILTER_GRID": 2}, {"FILTER_GRID": 0}, {"FILTER_GRID": 207}, {"FILTER_GRID": 100000000},
            {"PROBE_X": 0}, {"PROBE_X": 1}, {"PX_ONE_XCC": 1}, {"PROBE_X": 1, "PX_ONE_XCC": 1}]


@pytest.mark.parametrize("env", hook_cases(), ids=lambda e: "-".join(f"{a}={b}" for a, b in e.items()))
def test_the_whole_grid_under_each_hook(env, monkeypatch):
    clear(monkeypatch, **env)
    sweep({a: str(b) for a, b in env.items()})


def test_two_way_hook_and_grid_hook_arrive_as_inputs(monkeypatch):
    """SMG_TWO_WAY and SMG_P1_GRID are read by p1_plan / p1_reserve; what the look-up stage sees of them is one_way and the grid"""
    clear(monkeypatch)
    N = 100000
    for k in (31, 33, 63):
        monkeypatch.delenv("SMG_TWO_WAY", raising=False)
        one = engine.pass1_plan(k, N)["one_way"]
        monkeypatch.setenv("SMG_TWO_WAY", "1")
        two = engine.pass1_plan(k, N)["one_way"]
        assert (one, two) == (1, 0)
        # 20 % of the entries sent a request: many for a one-way run (> 14 %), not for a two-way one (<= 28 %)
        a = dict(nb=10, bm_bits=32, n=N, nemitted=N // 5, nrequests=N // 5, n_chunks=30)
        assert check({}, k, one_way=one, **a)["probe_form"] == 2 and check({}, k, one_way=two, **a)["probe_form"] == 1
    monkeypatch.delenv("SMG_TWO_WAY", raising=False)
    L = lim()
    whole = check({}, 31, nb=10, bm_bits=32, want_rec=10 ** 6, grid=1280)["max_chunks"]
    lone = check({}, 31, nb=10, bm_bits=32, want_rec=10 ** 6, grid=1)["max_chunks"]
    assert lone == (-(-10 ** 6 // L["F_CH"]) + 2) * (1 + L["BF_MAXGRID"]) > whole


def test_what_the_plan_refuses():
    ok = dict(nb=10, bm_bits=32, n_chunks=3, nrequests=100, nrec=100, n=1000)
    engine.lookup_plan(31, **ok)
    for k, bad in ((0, {}), (86, {}), (31, {"rw": 3}), (65, {"rw": 3}), (31, {"nb": 11}), (31, {"nb": -1}), (31, {"bm_bits": 7}),
                   (31, {"bm_bits": 33}), (31, {"bm_bits": 10}), (65, {"rw": 4}), (31, {"rw": 2}), (32, {"one_way": 1}),
                   (31, {"n_chunks": -1}), (31, {"nrequests": -1}), (31, {"cus": 0}), (31, {"seen_chunks": -2}), (31, {"list": 2}),
                   (31, {"flat": -1}), (31, {"filtered": 2}), (31, {"nbig": -1}), (31, {"nemitted": -1}), (31, {"n": -1}),
                   (31, {"n": 1 << 32}), (31, {"nrec": -1}), (31, {"want_rec": -1}), (31, {"grid": 0}), (31, {"grid": 4097}),
                   (31, {"have_chunks": -1})):
        with pytest.raises(engine.EngineError):
            engine.lookup_plan(k, **dict(ok, **bad))
    with pytest.raises(TypeError):
        engine.lookup_plan(31, chunks=3)


# ---- the cases of tests/test_list_lookups_gpu.py ---------------------------------------------------------------------------------

def apply_of(plan):
    return (engine.Engine.APPLY_KERNELS[plan["kernel"]], bool(plan["sorted"]), engine.Engine.APPLY_HOLES[plan["holes"]], plan["covered"])


@pytest.mark.parametrize("hook", [False, True], ids=["real threshold", "hook at its floor"])
@pytest.mark.parametrize("k", lz.KS1)
def test_key_only_flat_list_on_both_sides_of_the_sort(k, hook, monkeypatch):
    L = lim()
    clear(monkeypatch, **({"APPLY_SORT_MIN": L["SORT_MIN"]} if hook else {}))
    m = L["SORT_MIN"] if hook else L["APPLY_SORT_MIN"]
    for cut in (m - 1, m, 2 * m + 3):
        p = engine.lookup_plan(k, flat=1, nrec=cut, bm_bits=30, nb=8)      # (the phase API's default map; a flat list is never fused)
        assert apply_of(p) == ("kf_apply_sorted", cut >= m, None, cut) and p["route"] == R_FLAT and not p["filter_first"]


@pytest.mark.parametrize("k,exact", [(k, False) for k in lz.KS2] + [(k, True) for k in lz.KS])
def test_wider_records_on_both_sides_of_the_index_sort(k, exact):
    L = lim()
    W = words_of(k)
    for cut in (L["SORT_MIN"] - 1, L["SORT_MIN"], 3 * L["SORT_MIN"]):
        p = engine.lookup_plan(k, rw=W + exact, flat=1, nrec=cut, bm_bits=0 if exact else 30, nb=0 if exact else 8)
        long = cut >= L["SORT_MIN"]
        assert apply_of(p) == ("kf_apply_indexed" if long else "kf_apply", long, None, cut)


@pytest.mark.parametrize("floor", [False, True], ids=["as it comes", "sorted"])
@pytest.mark.parametrize("k", [31, 24, 32])
def test_own_unfiltered_list_through_sentinels_and_through_compaction(k, floor, monkeypatch):
    """SMG_NO_FILTER: no map.  Chunks filled to the brim keep their holes as sentinels -- but for k = 32 --, ragged ones are squeezed"""
    L = lim()
    clear(monkeypatch, **({"APPLY_SORT_MIN": L["SORT_MIN"]} if floor else {}))
    nreq = 4 * L["F_CH"] - 100
    full, ragged = -(-nreq // L["F_CH"]), 1280
    p = engine.lookup_plan(k, n_chunks=full, nrequests=nreq, nrec=nreq)
    if k < 32:
        assert apply_of(p) == ("kf_apply_sorted", floor, "sentinels", full * L["F_CH"]) and nreq < p["covered"] < nreq + nreq // 8 + 1
    else:
        assert apply_of(p) == ("kf_apply_sorted", floor, "compacted", nreq)
    assert apply_of(engine.lookup_plan(k, n_chunks=ragged, nrequests=nreq, nrec=nreq)) == ("kf_apply_sorted", floor, "compacted", nreq)


@pytest.mark.parametrize("exact", [False, True], ids=["hash", "exact"])
def test_two_word_run_compacts_and_looks_up_through_the_index_sort(exact):
    L = lim()
    for nreq in (L["SORT_MIN"] - 1, L["SORT_MIN"]):
        p = engine.lookup_plan(51, rw=2 + exact, n_chunks=40, nrequests=nreq, nrec=nreq)
        long = nreq >= L["SORT_MIN"]
        assert apply_of(p) == ("kf_apply_indexed" if long else "kf_apply", long, "compacted", nreq)


@pytest.mark.parametrize("bucketed", [False, True], ids=["chunk list", "bucketed first"])
def test_short_kmers_filter_their_chunk_list(bucketed, monkeypatch):
    """k = 10 has no 12 id bits: no chain; the filter reads the chunk list, or with SMG_FILTER_SORT_MIN at its floor the bucketed one"""
    L = lim()
    clear(monkeypatch, **({"FILTER_SORT_MIN": L["SORT_MIN"]} if bucketed else {}))
    bits = engine.pass1_plan(10, 3000, own_lookups=False, have_index=False, bm_cap=30)["bm_bits"]
    p = engine.lookup_plan(10, bm_bits=bits, n_chunks=1, nrequests=700, nrec=700)
    assert engine.Engine.PRESORTED[p["presort"]] == ("bucketed" if bucketed else "as it is")
    assert p["filter_first"] == 1 and p["route"] == R_NONE
    p = engine.lookup_plan(10, bm_bits=bits, n_chunks=1, nrequests=300, nrec=300, filtered=1)
    assert apply_of(p)[0] == "kf_apply_sorted" and apply_of(p)[2] in ("sentinels", "compacted")


# ---- the cases of tests/test_lookup_regimes_gpu.py and tests/test_wide_fast_path_gpu.py ------------------------------------------

@pytest.mark.parametrize("fb", [23, 25, 32])
def test_the_phase_filter_writes_a_list_and_a_run_fuses(fb, monkeypatch):
    """filter(map): kl_probe to a list, no ticket.  run: kl_probe_x where SMG_PROBE_X says so and there are eight buckets"""
    L = lim()
    nb = lo.lookup_geo(fb)[1]
    n, nemitted = 405000, 70000                                           # (17 % of the entries send, as on a diploid table)
    clear(monkeypatch)
    p = engine.lookup_plan(31, nb=nb, bm_bits=fb, list=1, n=n, nemitted=nemitted, nrequests=nemitted, n_chunks=1800)
    assert (p["probe_form"], p["probe_part"], engine.Engine.PRESORTED[p["presort"]]) == (3, 0, "chain")
    for probe in ({"PROBE_X": 0}, {"PROBE_X": 1}, {"PROBE_X": 1, "PX_ONE_XCC": 1}):
        clear(monkeypatch, **probe)
        for one_way in (0, 1):
            p = engine.lookup_plan(31, nb=nb, bm_bits=fb, one_way=one_way, n=n, nemitted=nemitted, nrequests=nemitted, n_chunks=1800,
                                   nrec=nemitted)
            assert p["route"] == R_FUSED and apply_of(p) == (None, False, None, 0)
            if probe["PROBE_X"] and nb >= 3:
                part = L["PX_PART"] if nemitted * 100 > n * (14 if one_way else 28) else 2 * L["PX_PART"]
                assert (p["probe_form"], p["probe_part"], p["one_xcd"]) == (2, part, int("PX_ONE_XCC" in probe))
            else:
                assert (p["probe_form"], p["probe_part"], p["one_xcd"]) == (1, 0, 0)       # kl_probe_x needs eight buckets


@pytest.mark.parametrize("k", [65, 85])
def test_three_word_kmers_filter_their_chunk_list_with_fewer_workgroups(k, monkeypatch):
    """records of four words, no chain: kf_filter<4> over the chunk list with all its workgroups, two, one"""
    for fgrid, chunks in itertools.product((None, 1, 2), (3, 5000)):
        clear(monkeypatch, **({} if fgrid is None else {"FILTER_GRID": fgrid}))
        p = engine.lookup_plan(k, rw=4, bm_bits=20, n_chunks=chunks, nrequests=chunks * 3000, nrec=chunks * 3000, cus=256)
        grid = min(fgrid or 512, chunks, 512)
        assert (p["presort"], p["filter_grid"], p["maxout"], p["filter_first"]) == (ASIS, grid, chunks + grid + 16, 1)
        p = engine.lookup_plan(k, rw=4, bm_bits=20, n_chunks=chunks, nrec=chunks * 1000, filtered=1)
        assert apply_of(p) == ("kf_apply_indexed" if chunks * 1000 >= lim()["SORT_MIN"] else "kf_apply", chunks * 1000 >= lim()["SORT_MIN"],
                               "compacted", chunks * 1000)
