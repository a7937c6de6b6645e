"""What `sharded.hetmers_sharded` remembers between two calls on one engine (sharded.ShardState), on CPU with the numpy stand-in.

Splitters and sizes, the replay record and the fact that the engine is on the caller's shard all depend on the table under
the engine; `ShardState.table_changed` is the one place that drops them.  Each case changes the table in another way --
other tensors under `prebound`, the fall-back that leaves rank 0 on the gathered table, a table the engine conditioned and
owns, a bind to a table of the same size at the same addresses -- and holds the next call's plot to `brute.hetmers_plot`.
One-rank cases need no process group; two-rank cases run under gloo.

(a) and (b) hold because every engine records what it is bound to (`ShardEngine.bind`, `run_general`), (c) because the end
of `condition_sharded` reports the change, (d) because a bind drops the driver's replay record with the engine's.
Case (e): an engine class that does not derive from `sharded.ShardEngine` and has the methods such classes had before it
existed (`bind`, `apply_own`, `symhash`, `proof_into`) is adopted by the drivers, on one rank and on two."""
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import brute
from smudgeplot_amd import ktab, sharded, synth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@functools.lru_cache(maxsize=None)
def tab(k, seed):
    """(keys uint64[n], counts uint16[n], the oracle's plot) of a closed table of at most 1 500 entries"""
    keys, cnt = synth.diploid_table_u64(300, k=k, seed=seed, het_frac=0.5, cov=30, L=5)
    assert 200 < len(cnt) <= 1500
    return keys, cnt, plot_of(k, keys, cnt)


def plot_of(k, keys, cnt):
    want = brute.hetmers_plot(ktab.u64_to_packed(keys, k), cnt, k)
    assert want.sum() > 0
    return want


def shard(k, keys, cnt, rank, world):
    """this rank's (keys int64, counts int16) tensors of the table cut evenly on a window-block boundary"""
    cuts = [sharded.fix_cut(keys, 1, k, c) for c in sharded.shard_bounds(len(cnt), world)]
    lo, hi = cuts[rank], cuts[rank + 1]
    return (torch.from_numpy(np.ascontiguousarray(keys[lo:hi]).view(np.int64).copy()),
            torch.from_numpy(np.ascontiguousarray(cnt[lo:hi]).view(np.int16).copy()), lo, hi)


def counting_engine():
    from fake_engine import NumpyEngine

    class Counting(NumpyEngine):
        """the stand-in, counting the binds and the pass 1s the driver asks of it"""
        binds = pass1s = 0

        def _bind(self, *a, **kw):
            self.binds += 1
            super()._bind(*a, **kw)

        def pass1(self, *a, **kw):
            self.pass1s += 1
            super().pass1(*a, **kw)

    return Counting(torch.device("cpu"))


def couple_with_counts(k, keys, cnt, value, every):
    """counts with every `every`-th (k-mer, complement) couple at `value`: another closed table on the same k-mers"""
    rc = ktab.revcomp_u64(keys, k)
    pos = {int(x): i for i, x in enumerate(keys)}
    out = cnt.copy()
    for i in range(0, len(cnt), every):
        if int(rc[i]) != int(keys[i]):
            out[i] = out[pos[int(rc[i])]] = value
    assert not np.array_equal(out, cnt)
    return out


# ---- the cases: run by every rank, return what the parent checks ---------------------------------------------------------------

def case_a(k, rank, world):
    """prebound=True, first on table A, then on DIFFERENT tensors B"""
    eng = counting_engine()
    out = []
    for seed in (21, 22):
        keys, cnt, _ = tab(k, seed)
        tk, tc, _, _ = shard(k, keys, cnt, rank, world)
        if seed == 21:
            eng.bind(k, tk, tc)
        plot, st = sharded.hetmers_sharded(k, tk, tc, eng=eng, prebound=True)
        out.append((plot.numpy().copy(), st["path"], st["shard_nels"] == tc.numel(), eng.binds))
    return out


def case_b(k, rank, world):
    """a count on rank 0's shard moves: the proof fails, rank 0 runs the gathered table; the count is put back in place"""
    keys, cnt, _ = tab(k, 23)
    tk, tc, lo, hi = shard(k, keys, cnt, rank, world)
    j = case_b_entry(k)
    eng = counting_engine()
    out = []
    for value in (int(cnt[j]) + 7, int(cnt[j])):
        if lo <= j < hi:
            tc[j - lo] = value
        if not out:
            eng.bind(k, tk, tc)
        plot, st = sharded.hetmers_sharded(k, tk, tc, eng=eng, prebound=True)
        out.append((plot.numpy().copy(), st["path"], eng.binds))
    return out


def case_b_entry(k):
    keys, cnt, _ = tab(k, 23)
    rc = ktab.revcomp_u64(keys, k)
    return int(np.flatnonzero(rc != keys)[3])            # (on rank 0's shard: among the first entries of the table)


def case_c(k, rank, world):
    """condition_sharded on the canonical half of a table, the owned run, then a plain call on another table"""
    keys, cnt, _ = tab(k, 24)
    canon = keys <= ktab.revcomp_u64(keys, k)
    tk, tc, _, _ = shard(k, keys[canon], cnt[canon], rank, world)      # (a raw table: any cut will do)
    eng, split = sharded.condition_sharded(k, tk, tc, ethresh=5, trim=True, engine_factory=lambda dev: counting_engine())
    owned, st1 = sharded.hetmers_sharded(k, None, None, eng=eng, splitters=split)
    keys2, cnt2, _ = tab(k, 25)
    tk2, tc2, _, _ = shard(k, keys2, cnt2, rank, world)
    plain, st2 = sharded.hetmers_sharded(k, tk2, tc2, eng=eng)
    return [(owned.numpy().copy(), st1["path"]), (plain.numpy().copy(), st2["path"], st2["shard_nels"] == tc2.numel())]


def case_d(k, rank, world):
    """SMG_REPLAY=1: a step leaves a record, the next is replayed; then the tensors are overwritten IN PLACE with another
    table of the same size and the engine is bound again"""
    os.environ["SMG_REPLAY"] = "1"
    keys, cnt, _ = tab(k, 26)
    tk, tc, lo, hi = shard(k, keys, cnt, rank, world)
    eng = counting_engine()
    eng.bind(k, tk, tc)
    out = []
    for step in range(3):
        if step == 2:
            tc.copy_(torch.from_numpy(couple_with_counts(k, keys, cnt, 900, 7)[lo:hi].view(np.int16).copy()))
            eng.bind(k, tk, tc)
        before = eng.pass1s
        plot, st = sharded.hetmers_sharded(k, tk, tc, eng=eng, prebound=True)
        out.append((plot.numpy().copy(), st["path"], bool(st["replayed"]), eng.pass1s - before))
    return out


def case_e(k, rank, world):
    """an engine class that knows nothing of ShardEngine (bind, proof_into, no state, no proof_tail): the drivers adopt it"""
    from fake_engine import NumpyEngine
    os.environ["SMG_REPLAY"] = "1"
    ns = {n: f for n, f in vars(NumpyEngine).items() if callable(f) and n not in ("__init__", "_bind", "proof_tail", "run_single")}

    def init(self, device):
        self.device = device
        self._rp_want, self._rp_rec, self._rp_active, self._rp_bad = False, None, False, 0

    old = type("OldEngine", (), dict(ns, __init__=init, bind=NumpyEngine._bind, apply_own=lambda self: self._apply(self.req),
                                     symhash=lambda self: list(self.fp)))
    assert not issubclass(old, sharded.ShardEngine)
    keys, cnt, _ = tab(k, 27)
    tk, tc, _, _ = shard(k, keys, cnt, rank, world)
    eng, out = None, []
    for _ in range(2):
        if world == 1 and eng is not None:      # second one-rank call: a count moved in place, the general path on this shard
            tc[case_e_entry(k)] += 7
            eng.reload_table(tk, tc)
        plot, st = sharded.hetmers_sharded(k, tk, tc, engine_factory=old, eng=eng, prebound=eng is not None)
        eng = st["engine"]
        out.append((plot.numpy().copy(), st["path"], bool(st.get("replayed")), isinstance(eng, old) and isinstance(eng, sharded.ShardEngine)))
    return out


def case_e_entry(k):
    keys = tab(k, 27)[0]
    return int(np.flatnonzero(ktab.revcomp_u64(keys, k) != keys)[3])


def _worker(rank, world, port, case, k, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, case(k, rank, world)))
    finally:
        dist.destroy_process_group()


def run_case(case, k, world):
    """-> the case's result of every rank, in rank order"""
    if world == 1:
        return [case(k, 0, 1)]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, k, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [res[r] for r in range(world)]


def same(plot, want):
    return np.array_equal(plot.reshape(1001, 501), want)


@pytest.mark.parametrize("world,k", [(1, 12), (2, 13)])
def test_a_prebound_on_other_tensors_binds_them_and_answers_for_them(world, k):
    for rank, (first, second) in enumerate(run_case(case_a, k, world)):
        assert same(first[0], tab(k, 21)[2]) and first[1:] == (1, True, 1), rank
        # B was bound (once, by the driver) and answers as B; with A's splitters or sizes the exchange would not be B's own
        assert same(second[0], tab(k, 22)[2]) and second[1:] == (1, True, 2), rank


@pytest.mark.parametrize("k", [12, 13])
def test_b_after_the_fallback_rank_0_binds_its_shard_again(k):
    keys, cnt, whole = tab(k, 23)
    moved = cnt.copy()
    moved[case_b_entry(k)] += 7
    res = run_case(case_b, k, 2)
    for rank, (first, second) in enumerate(res):
        assert first[1] == 2 and same(first[0], plot_of(k, keys, moved)), rank
        assert second[1] == 1 and same(second[0], whole), rank
    assert [r[1][2] - r[0][2] for r in res] == [1, 0]           # rank 0 was left on the gathered table, rank 1 on its shard


@pytest.mark.parametrize("world,k", [(1, 13), (2, 12)])
def test_c_a_plain_call_after_the_owned_run_finds_its_own_splitters(world, k):
    for rank, (owned, plain) in enumerate(run_case(case_c, k, world)):
        assert owned[1] == 1 and same(owned[0], tab(k, 24)[2]), rank
        assert plain[1:] == (1, True) and same(plain[0], tab(k, 25)[2]), rank


@pytest.mark.parametrize("k", [12, 13])
def test_d_a_bind_at_the_same_addresses_ends_the_replay(k):
    keys, cnt, whole = tab(k, 26)
    other = plot_of(k, keys, couple_with_counts(k, keys, cnt, 900, 7))
    assert not np.array_equal(other, whole)
    for rank, steps in enumerate(run_case(case_d, k, 2)):
        assert [s[1] for s in steps] == [1, 1, 1], rank
        assert same(steps[0][0], whole) and same(steps[1][0], whole) and same(steps[2][0], other), rank
        assert [s[2] for s in steps] == [False, True, False], rank      # the record was there, and the bind dropped it
        assert steps[2][3] == 1, rank                                   # ... so the step ran once: not replayed and run again


def test_e_an_engine_class_from_before_the_protocol_is_adopted():
    k = 12
    keys, cnt, whole = tab(k, 27)
    for rank, steps in enumerate(run_case(case_e, k, 2)):
        assert [s[1:] for s in steps] == [(1, False, True), (1, True, True)], rank     # the tail's replay words too
        assert same(steps[0][0], whole) and same(steps[1][0], whole), rank
    moved = cnt.copy()
    moved[case_e_entry(k)] += 7
    (first, second), = run_case(case_e, k, 1)                  # one rank, no group: the one-shard run by the phase calls
    assert first[1:] == (1, False, True) and same(first[0], whole)
    assert second[1:] == (2, False, True) and same(second[0], plot_of(k, keys, moved))
