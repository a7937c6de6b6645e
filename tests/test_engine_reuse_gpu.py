"""One engine bound to a SEQUENCE of different tables (run with -m gpu on an MI355X).

The other reuse tests run one engine again on the same table.  The engine keeps its device buffers from run to run and
only ever grows them, so what can go wrong between two DIFFERENT tables is its bookkeeping: a capacity that no longer
belongs to its buffer, contents a smaller or a narrower table left behind, the bit map of deferred entries that is
cleared only when its memory is fresh, a request list sized for records of another width, the byte array that is code
bytes on the fast path and degrees on the counted one.  Every plot is compared cell for cell with the numpy oracle, or
with the reference's golden .smu."""
import numpy as np
import pytest

import brute
from conftest import load_golden
from lookup_oracle import packed_to_words
from smudgeplot_amd import engine, ktab, synth

pytestmark = pytest.mark.gpu


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

    k = 31
    small_k, small_c = synth.diploid_table_u64(700, k=k, seed=5, het_frac=0.4, cov=30, L=5)
    large_k, large_c = synth.diploid_table_u64(11000, k=k, seed=6, het_frac=0.4, cov=30, L=5)
    assert 1500 < len(small_c) < 2500 and 25000 < len(large_c) < 35000
    small_want = brute.hetmers_plot(ktab.u64_to_packed(small_k, k), small_c, k)
    large_want = brute.hetmers_plot(ktab.u64_to_packed(large_k, k), large_c, k)
    assert small_want.sum() > 0 and large_want.sum() > small_want.sum()

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
    rc = ktab.revcomp_u64(large_k, k)
    j = int(np.nonzero(rc != large_k)[0][len(large_k) // 3])
    open_c = large_c.copy()
    open_c[j] += 7
    plot, st = run(k, large_k, open_c, "hash")
    assert st["path"] == 2 and np.array_equal(plot, brute.hetmers_plot(ktab.u64_to_packed(large_k, k), open_c, k))
    # 8. and the small table again, in buffers that have held all of the above
    plot, st = run(k, small_k, small_c, "hash")
    assert st["path"] == 1 and np.array_equal(plot, small_want)
