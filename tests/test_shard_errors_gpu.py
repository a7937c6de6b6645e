"""One shard fails while its peers do not (run with -m gpu on an MI355X).

The shard drivers (smg_multi.hpp) keep a failing shard's peers out of every collective and every peer copy, and hand the
failing shard's error to the caller.  The table here is sorted everywhere but at two neighbouring entries in the middle of the
middle shard of three: they share their leading 12 bases, so the prefix index and the cuts are those of the sorted table, the
first and the last shard are in order, and the middle one is refused (SMG_EFORMAT) by its pass 1.  Three shards is the smallest
shape that has a failing middle shard with a live shard on either side.  The process must be left usable: the sorted table
runs in it afterwards, against the numpy oracle."""
import functools

import numpy as np
import pytest

import brute
from conftest import make_table
from smudgeplot_amd import engine, synth

pytestmark = pytest.mark.gpu

K = 31


@functools.lru_cache(maxsize=None)
def tables():
    """(the sorted table, the same with two entries of the middle shard swapped, the oracle's plot of the sorted one)"""
    packed, cnt = synth.adversarial_table(K, 3000, 4, seed=8)
    n = len(cnt)
    same = np.nonzero((packed[1:, :3] == packed[:-1, :3]).all(axis=1))[0]         # i and i + 1 share their leading 12 bases
    i = int(same[np.argmin(np.abs(same - n // 2))])
    assert 0.4 * n < i < 0.6 * n                                                  # well inside the middle shard of three
    swapped, scnt = packed.copy(), cnt.copy()
    swapped[[i, i + 1]] = packed[[i + 1, i]]
    scnt[[i, i + 1]] = cnt[[i + 1, i]]
    table = lambda p, c: make_table(dict(packed=p, counts=c, k=K, ibyte=1, nparts=1))
    return table(packed, cnt), table(swapped, scnt), brute.hetmers_plot(packed, cnt, K)


def fails_then_runs(monkeypatch, hook):
    good, bad, want = tables()
    monkeypatch.setenv(hook, "3")
    with pytest.raises(engine.EngineError) as ei:
        engine.hetmers_run(bad, symcheck="hash")
    plot, st = engine.hetmers_run(good, symcheck="hash")          # the same process, the same mode, the sorted table
    assert np.array_equal(plot, want) and st["path"] == 1 and st["nels"] == good.nels
    return ei.value


def test_a_failing_middle_shard_among_virtual_shards(monkeypatch):
    err = fails_then_runs(monkeypatch, "SMG_VIRTUAL_SHARDS")
    assert err.code == -4
    assert str(err).startswith("smg_hetmers error -4: GPU ")      # (the failing rank's message, named by its device)


def test_a_failing_middle_shard_out_of_core(monkeypatch):
    err = fails_then_runs(monkeypatch, "SMG_SEQUENTIAL_SHARDS")
    assert err.code == -4
