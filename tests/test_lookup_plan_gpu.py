"""The plans of the stage between pass 1 and pass 2 (smg_engine_lookup_plan) against what an engine did: one run per route of
the look-ups, then the plan is asked with the inputs that engine had -- read back through lookup_state, stats and the table --
and must equal apply_state / lookup_state field by field; the plot must be the oracle's.  Tables of tests/list_oracle.py: a
few thousand entries each, but for the two brim-full ones, which are the very tables (same arguments, built once per session)
tests/test_list_lookups_gpu.py runs, 1.1e5 entries: a request list that fills its chunks to the brim needs that many."""
import pytest
import torch

import list_oracle as lz
from smudgeplot_amd import engine
from test_list_lookups_gpu import HOOKS, Bound, lim, same_plot

pytestmark = pytest.mark.gpu

PLAN_HOOKS = HOOKS + ("SMG_PROBE_X", "SMG_PX_ONE_XCC")
ROUTES = engine.APPLY_ROUTES


def hooks(monkeypatch, **env):
    for name in PLAN_HOOKS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv("SMG_" + name, str(val))


def plan_for(b, st, ls, **more):
    """the plan for the list this engine's pass 1 left (st, ls: read before anything filtered it)"""
    a = dict(rw=ls["rw"], nb=ls["nb"], bm_bits=ls["fb"], one_way=ls["one_way"], n_chunks=ls["p1_chunks"], nrequests=st["nemitted"],
             nrec=st["nemitted"], nbig=st["nbig"], nemitted=st["nemitted"], n=len(b.t.cnt),
             cus=torch.cuda.get_device_properties(0).multi_processor_count, grid=ls["p1_grid"])
    a.update(more)
    return engine.lookup_plan(b.t.k, **a)


def same_apply(p, ap, route, what):
    E = engine.Engine
    got = (ROUTES[p["route"]], E.APPLY_KERNELS[p["kernel"]], bool(p["sorted"]), E.APPLY_HOLES[p["holes"]], p["covered"])
    assert got == (route, ap["kernel"], ap["sorted"], ap["holes"], ap["covered"]), (what, p, ap)


def same_chain(p, ap, ls, what):
    assert engine.Engine.PRESORTED[p["presort"]] == ap["presorted"] == "chain", (what, p, ap)
    assert (p["probe_form"], p["probe_part"]) == (ls["probe"], ls["ticket"]), (what, p, ls)


@pytest.mark.parametrize("probe", [{}, {"PROBE_X": 0}, {"PROBE_X": 1}, {"PROBE_X": 1, "PX_ONE_XCC": 1}],
                         ids=["as the counts say", "kl_probe", "kl_probe_x", "kl_probe_x one XCC"])
def test_own_requests_through_the_fused_chain(probe, monkeypatch):
    """without a hook the share of entries that sent a request decides the kernel (a third of this table's: kl_probe_x)"""
    hooks(monkeypatch, **probe)
    b = Bound(lz.adversarial(31, 3000, 7))
    plot, st = b.run("hash")
    ls, ap = b.e.lookup_state(), b.e.apply_state()
    assert st["path"] == 1 and ls["nb"] == 10 and ls["fb"] == 32 and ls["p1_chunks"] > 0
    p = plan_for(b, st, ls)
    same_apply(p, ap, "fused", probe)
    same_chain(p, ap, ls, probe)
    x = probe.get("PROBE_X", int(st["nemitted"] * 100 > len(b.t.cnt) * 14))
    assert ls["one_way"] == 1 and ls["probe"] == (2 if x else 1) and (ls["ticket"] > 0) == bool(x)
    assert p["one_xcd"] == int("PX_ONE_XCC" in probe) and not ap["kernel"]
    same_plot(plot, b.t.plot, probe)
    b.close()


def test_the_phase_filter_keeps_a_list_that_is_compacted(monkeypatch):
    """filter with the engine's own map: kl_probe writes the kept list; its look-ups squeeze the ragged chunks (every wave of the
    probe fills chunks of its own, and the list is shorter than 8/9 of a chunk: whatever their number, they are not brim-full)"""
    hooks(monkeypatch)
    L = lim()
    b = Bound(lz.adversarial(31, 2000, 7))
    b.e.set_blockmap_bits(32)
    b.e.pass1("hash")
    st, ls = b.e.stats(), b.e.lookup_state()
    assert ls["nb"] == 10 and ls["one_way"] == 0 and ls["probe"] == 0
    kept = b.e.filter(None)
    ls2, ap = b.e.lookup_state(), b.e.apply_state()
    p = plan_for(b, st, ls, list=1)
    same_chain(p, ap, ls2, "filter")
    assert p["probe_form"] == 3 and 0 < kept <= st["nemitted"] and st["nemitted"] + st["nemitted"] // 8 < L["F_CH"]
    assert b.e.apply_own() == 0
    ap = b.e.apply_state()
    for chunks in (1, ls["p1_chunks"], p["maxout"]):
        same_apply(plan_for(b, st, ls, filtered=1, n_chunks=chunks, nrec=kept), ap, "compacted", chunks)
    assert ap["kernel"] == "kf_apply_sorted" and not ap["sorted"] and ap["covered"] == kept
    same_plot(b.pass2(), b.t.plot, "filter")
    b.close()


@pytest.mark.parametrize("k", [31, 32], ids=["k=31 sentinels", "k=32 compacted"])
def test_brim_full_chunks_keep_their_holes_unless_k_is_32(k, monkeypatch):
    """one workgroup of pass 1 fills its chunks to the brim, nothing is filtered; the sort at its floor"""
    L = lim()
    hooks(monkeypatch, NO_FILTER=1, P1_GRID=1, VERIFY_SORT=1, APPLY_SORT_MIN=L["SORT_MIN"])
    args = (31, True, L["F_CH"], 3 * L["SORT_MIN"]) if k == 31 else (32, False, L["F_CH"], 3 * L["SORT_MIN"], True)
    b = Bound(lz.brim_full_table(*args))                                   # (the arguments of tests/test_list_lookups_gpu.py: one build)
    plot, st = b.run("hash")
    ls, ap = b.e.lookup_state(), b.e.apply_state()
    assert st["path"] == 1 and ls["nb"] == 0 and ls["fb"] == 0 and ls["p1_grid"] == 1 and ap["presorted"] is None
    p = plan_for(b, st, ls)
    same_apply(p, ap, "sentinels" if k == 31 else "compacted", k)
    assert ap["kernel"] == "kf_apply_sorted" and ap["sorted"] and not p["filter_first"]
    assert ap["covered"] == (ls["p1_chunks"] * L["F_CH"] if k == 31 else st["nemitted"])
    same_plot(plot, b.t.plot, k)
    b.close()


@pytest.mark.parametrize("m", [1100, 500], ids=["kf_apply_indexed", "kf_apply"])
def test_exact_proof_of_two_word_kmers_on_both_sides_of_the_index_sort(m, monkeypatch):
    """every entry sends a record of three words: the same builder and seed at 4.5e3 entries (>= SORT_MIN) and at 2.2e3 (below)"""
    hooks(monkeypatch)
    L = lim()
    b = Bound(lz.adversarial(51, m, 11))
    plot, st = b.run("exact")
    ls, ap = b.e.lookup_state(), b.e.apply_state()
    long = m == 1100
    assert st["path"] == 1 and ls["rw"] == 3 and ls["nb"] == 0 and ls["fb"] == 0 and st["nemitted"] >= len(b.t.cnt)
    assert (st["nemitted"] >= L["SORT_MIN"]) == long
    same_apply(plan_for(b, st, ls), ap, "compacted", m)
    assert ap["kernel"] == ("kf_apply_indexed" if long else "kf_apply") and ap["sorted"] == long
    same_plot(plot, b.t.plot, m)
    b.close()


def test_three_word_kmers_filter_and_compact(monkeypatch):
    """k = 65: records of four words, no chain; the filter reads the chunk list as it is, the kept list is squeezed and looked up
    by kf_apply (fewer than SORT_MIN records survive)"""
    hooks(monkeypatch)
    L = lim()
    b = Bound(lz.adversarial(65, 1500, 5))
    plot, st = b.run("hash")
    ls, ap = b.e.lookup_state(), b.e.apply_state()
    assert st["path"] == 1 and ls["rw"] == 4 and ls["nb"] == 0 and ls["fb"] > 0 and ls["probe"] == 0
    p = plan_for(b, st, ls)
    assert p["filter_first"] == 1 and engine.Engine.PRESORTED[p["presort"]] == ap["presorted"] == "as it is"
    kept = st["nrequests"]
    assert 0 < kept <= st["nemitted"] and kept < L["SORT_MIN"]
    for chunks in (1, p["maxout"]):
        same_apply(plan_for(b, st, ls, filtered=1, n_chunks=chunks, nrec=kept), ap, "compacted", chunks)
    assert ap["kernel"] == "kf_apply" and not ap["sorted"]
    same_plot(plot, b.t.plot, "k=65")
    b.close()
