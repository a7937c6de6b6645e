"""One engine bound to a SEQUENCE of different tables (run with -m gpu on an MI355X).

The other reuse tests run one engine again on the same table.  The engine keeps its device buffers from run to run and
only ever grows them, so what can go wrong between two DIFFERENT tables is its bookkeeping: a capacity that no longer
belongs to its buffer, contents a smaller or a narrower table left behind, the bit map of deferred entries that is
cleared only when its memory is fresh, a request list sized for records of another width, the byte array that is code
bytes on the fast path and degrees on the counted one.  Every plot is compared cell for cell with the numpy oracle, or
with the reference's golden .smu."""
import functools

import numpy as np
import pytest

import brute
from conftest import load_golden
from lookup_oracle import packed_to_words
from smudgeplot_amd import engine, ktab, synth

pytestmark = pytest.mark.gpu

K = 31


@functools.lru_cache(maxsize=None)
def tables():
    """the two closed k = 31 tables of this file with the oracle's plots, made once"""
    small_k, small_c = synth.diploid_table_u64(700, k=K, seed=5, het_frac=0.4, cov=30, L=5)
    large_k, large_c = synth.diploid_table_u64(11000, k=K, seed=6, het_frac=0.4, cov=30, L=5)
    assert 1500 < len(small_c) < 2500 and 25000 < len(large_c) < 35000
    small_want = brute.hetmers_plot(ktab.u64_to_packed(small_k, K), small_c, K)
    large_want = brute.hetmers_plot(ktab.u64_to_packed(large_k, K), large_c, K)
    assert small_want.sum() > 0 and large_want.sum() > small_want.sum()
    return small_k, small_c, small_want, large_k, large_c, large_want


@functools.lru_cache(maxsize=None)
def open_table():
    """the large table with one count moved: not closed under reverse complement any more -> (counts, the oracle's plot)"""
    _, _, _, large_k, large_c, _ = tables()
    rc = ktab.revcomp_u64(large_k, K)
    j = int(np.nonzero(rc != large_k)[0][len(large_k) // 3])
    open_c = large_c.copy()
    open_c[j] += 7
    return open_c, brute.hetmers_plot(ktab.u64_to_packed(large_k, K), open_c, K)


def test_one_engine_through_a_sequence_of_different_tables():
    import torch
    from smudgeplot_amd import sharded
    dev = torch.device("cuda:0")
    eng = sharded.TorchEngine(dev)

    def run(k, words, cnt, mode):
        tk = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1).copy()).to(dev)
        tc = torch.from_numpy(np.ascontiguousarray(cnt).view(np.int16).copy()).to(dev)
        plot, st = sharded.hetmers_sharded(k, tk, tc, symcheck=mode, eng=eng)      # (binds the engine to these tensors)
        assert st["nels"] == len(cnt)
        return plot.cpu().numpy().reshape(1001, 501), st

    k = K
    small_k, small_c, small_want, large_k, large_c, large_want = tables()

    # 1. a small table, hash proof: every buffer at its first size
    plot, st = run(k, small_k, small_c, "hash")
    assert st["path"] == 1 and np.array_equal(plot, small_want)
    # 2. fifteen times the entries: the per-entry buffers grow
    plot, st = run(k, large_k, large_c, "hash")
    assert st["path"] == 1 and np.array_equal(plot, large_want)
    # 3. the same table under the exact proof: every entry sends, and the records gain a word
    plot, st = run(k, large_k, large_c, "exact")
    assert st["path"] == 1 and np.array_equal(plot, large_want)
    # 4. two-word k-mers
    p51, c51 = synth.adversarial_table(51, 2500, 4, seed=17, low_complexity=100, dense=2)
    plot, st = run(51, packed_to_words(p51, 51), c51, "hash")
    assert st["path"] == 1 and np.array_equal(plot, brute.hetmers_plot(p51, c51, 51))
    # 5. three-word k-mers: the generic pass 1
    g = load_golden("k65_i1")
    plot, st = run(g["k"], packed_to_words(g["packed"], g["k"]), g["counts"], "hash")
    assert st["path"] == 1 and engine.smu_text(plot) == g["smu"]
    # 6. k > 85, the counted path: the byte array holds degrees, the request list is flat
    g = load_golden("k100_i1")
    plot, st = run(g["k"], packed_to_words(g["packed"], g["k"]), g["counts"], "hash")
    assert st["path"] == 1 and engine.smu_text(plot) == g["smu"]
    # 7. back to one-word k-mers, one count moved: the table is not closed any more, the general path takes it
    open_c, open_want = open_table()
    plot, st = run(k, large_k, open_c, "hash")
    assert st["path"] == 2 and np.array_equal(plot, open_want)
    # 8. and the small table again, in buffers that have held all of the above
    plot, st = run(k, small_k, small_c, "hash")
    assert st["path"] == 1 and np.array_equal(plot, small_want)


ZERO_FORM = {"var": 0, "w": 0, "rw": 0, "inner_only": 0}
ZERO_LOOKUP = dict.fromkeys(engine.Engine.LOOKUP_STATE, 0)
EINVAL = -2


def clean(check):
    """a check that holds since the engine's run state is reset in one place (begin_run): before that the export or the call
    answered from what an EARLIER run had left behind.  Each use names its case."""
    assert check() in (None, True)


def test_the_state_exports_and_refusals_through_every_kind_of_run():
    """one engine.Engine through the phase calls and the one-shot run on tables of all three paths: after every step what it
    reports about itself (lookup_state, pass1_form, record_words, nreq, replay_state) and what it refuses"""
    import torch
    dev = torch.device("cuda:0")
    _, _, _, large_k, large_c, large_want = tables()
    n = len(large_c)
    e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
    plot_t = torch.zeros(engine.PLOT_CELLS, dtype=torch.int64, device=dev)
    keep = []                                                      # (the tensors the engine is bound to)

    def bind(k, words, cnt, index=True):
        tk = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).reshape(-1).copy()).to(dev)
        tc = torch.from_numpy(np.ascontiguousarray(cnt).view(np.int16).copy()).to(dev)
        keep[:] = [tk, tc]
        e.bind(k, len(cnt), tk.data_ptr(), tc.data_ptr())
        if index:
            lead = torch.from_numpy((np.ascontiguousarray(words).reshape(len(cnt), -1)[:, 0] >> np.uint64(40)).astype(np.int64)).to(dev)
            keep.append(torch.cumsum(torch.bincount(lead, minlength=1 << 24), 0))
            e.set_prefix_index(keep[-1].data_ptr(), 3, 0)

    def plot():
        torch.cuda.synchronize()
        return plot_t.cpu().numpy().reshape(engine.PLOT_ROWS, engine.PLOT_COLS)

    def refused(call, message):
        with pytest.raises(engine.EngineError) as err:
            call()
        assert err.value.code == EINVAL and message in str(err.value), err.value

    def one_pixel(p):
        """extract, counting only, with a label on the fullest cell of p -> (records, the cell's weight)"""
        cell = int(np.argmax(p))
        labels = torch.zeros(engine.PLOT_CELLS, dtype=torch.int16, device=dev)
        labels[cell] = 1
        return e.extract(labels.data_ptr(), 0, 0), int(p.reshape(-1)[cell])

    def phase_calls_refused():
        refused(lambda: e.apply(0, 0), "apply before pass1")
        refused(lambda: e.apply_own(), "apply before pass1")
        refused(lambda: e.pass2(plot_t.data_ptr()), "pass2 before pass1")

    def fast_state(plan):
        ls, form = e.lookup_state(), e.pass1_form()
        assert form == {"var": plan["var"], "w": plan["w"], "rw": plan["rw"], "inner_only": 0}, form
        assert (ls["fb"], ls["nb"], ls["bm2"], ls["one_way"], ls["rw"]) == \
               (plan["bm_bits"], plan["nb"], plan["bm2"], plan["one_way"], plan["rw"]), ls
        assert e.record_words() == plan["rw"]
        return ls

    try:
        # 1. a fresh bind: nothing has run
        bind(K, large_k, large_c)
        phase_calls_refused()
        refused(lambda: one_pixel(large_want), "extract needs a completed run")
        assert e.lookup_state() == ZERO_LOOKUP and e.pass1_form() == ZERO_FORM
        assert (e.record_words(), e.nreq(), e.replay_state()) == (0, 0, 0)

        # 2. the one-shot run, hash proof, with the table's index: what p1_plan says, one-way
        plan = engine.pass1_plan(K, n)
        assert plan["var"] == 2 and plan["one_way"] == 1
        st2 = e.run(plot_t.data_ptr(), "hash")
        p2 = plot()
        assert st2["path"] == 1 and np.array_equal(p2, large_want)
        ls2 = fast_state(plan)
        assert ls2["probe"] in (1, 2) and ls2["p1_grid"] > 0 and ls2["nown"] > ls2["p1_grid"]
        assert e.nreq() == st2["nrequests"] and e.replay_state() == 0
        got, want = one_pixel(p2)
        assert got == want > 0

        # 3. the phase calls on the same table: two-way, the hot form with a 32-bit map, the general one with the default map
        for bits in (32, 0):
            e.set_blockmap_bits(bits)
            plan = engine.pass1_plan(K, n, own_lookups=False, bm_cap=bits or 30)
            assert plan["var"] == (6 if bits else 1) and plan["one_way"] == 0
            e.pass1("hash")
            ls = fast_state(plan)
            assert ls["probe"] == 0 and ls["ticket"] == 0
            nreq = e.nreq()
            assert nreq > st2["nemitted"]                          # (two-way: both members of a class send)
            # [case E1] pass 1 has run again and pass 2 has not: the code bytes are unfinished
            clean(lambda: refused(lambda: one_pixel(p2), "extract needs a completed run"))
            kept = e.filter()
            assert 0 <= kept <= nreq and e.nreq() == kept             # (few targets of this table own a scanned pair themselves)
            assert e.lookup_state()["probe"] == 3
            assert e.apply_own() == 0
            e.pass2(plot_t.data_ptr())
            assert np.array_equal(plot(), large_want)
            assert e.stats()["path"] == 1 and e.pass1_form()["var"] == plan["var"]
            got, want = one_pixel(p2)
            assert got == want
        e.set_blockmap_bits(0)

        # 4. k > 85: the counted path
        g = load_golden("k100_i1")
        bind(g["k"], packed_to_words(g["packed"], g["k"]), g["counts"], index=False)
        clean(lambda: e.lookup_state() == ZERO_LOOKUP)              # [case E2] the rebind itself
        st = e.run(plot_t.data_ptr(), "hash")
        p4 = plot()
        assert st["path"] == 1 and engine.smu_text(p4) == g["smu"]
        assert e.pass1_form() == ZERO_FORM
        clean(lambda: e.lookup_state() == ZERO_LOOKUP)              # [case E2] map bits, bm2, one_way, rw, probe of the k = 31 run
        clean(lambda: e.record_words() == 0)                        # [case E2] rw of the k = 31 run
        got, want = one_pixel(p4)
        assert got == want > 0
        phase_calls_refused()

        # 5. the k = 31 table with one count moved: the fast pass 1 runs, the proof fails, the general path takes the table
        open_c, open_want = open_table()
        bind(K, large_k, open_c)
        st = e.run(plot_t.data_ptr(), "hash")
        p5 = plot()
        assert st["path"] == 2 and np.array_equal(p5, open_want)
        assert e.pass1_form() == ZERO_FORM
        clean(lambda: e.lookup_state() == ZERO_LOOKUP)              # [case E3] the state of the fast pass 1 that the run abandoned
        got, want = one_pixel(p5)
        assert got == want > 0
        # [case E4] degrees over all positions are not what the phase calls' kernels read
        clean(lambda: refused(lambda: e.pass2(plot_t.data_ptr()), "pass2 before pass1"))
        clean(lambda: refused(lambda: e.apply_own(), "apply before pass1"))

        # 6. the closed table once more: step 2 again, bit for bit
        bind(K, large_k, large_c)
        st6 = e.run(plot_t.data_ptr(), "hash")
        assert np.array_equal(plot(), p2)
        ls6 = e.lookup_state()
        ls6["p1_chunks"] = ls2["p1_chunks"]                         # (which owner draws which tile is not a function of the table)
        assert ls6 == ls2 and e.nreq() == st2["nrequests"]
        assert {a: st6[a] for a in ("path", "nemitted", "nrequests", "nbig", "npairs")} == \
               {a: st2[a] for a in ("path", "nemitted", "nrequests", "nbig", "npairs")}
        fast_state(engine.pass1_plan(K, n))
    finally:
        e.close()

