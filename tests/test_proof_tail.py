"""The proof tail of a sharded step's reduction buffer: ONE test body over both engines.

`sharded.hetmers_sharded` has one layout for the words behind the plot, the one `k_proof_tail` writes (smg_hetmers.hip):
tail[0] = missing complements, this rank's 128-bit residue in words 1 + 2 slot and 2 + 2 slot (zeros in the other ranks'
slots: the SUM over the ranks hands everybody all residues), tail[n - 2] = a replayed step found other counts, tail[n - 1] =
the step was a replayed one, n = 3 + 2 nslots.  The numpy stand-in of the CPU suite has to mirror it word for word, so both
are held to the same rule here: the four words of proof_into, laid out by that rule.  Each table runs whole and with one
k-mer removed -- against a closed table alone a tail of zeros would pass."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from lookup_oracle import packed_to_words
from smudgeplot_amd import ktab

ENGINES = [pytest.param("numpy"), pytest.param("torch", marks=pytest.mark.gpu)]
SLOTS = [(1, 0), (3, 1), (16, 0), (16, 15)]
GUARD, SENTINEL = 8, 0x5A5A5A5A5A5A5A5A


def make_engine(kind):
    if kind == "numpy":
        from fake_engine import NumpyEngine
        return NumpyEngine(torch.device("cpu"))
    from smudgeplot_amd import sharded
    return sharded.TorchEngine(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def table(name, damaged):
    """(k, k-mer words int64[n * W], counts int16[n]) of a committed golden: k31_i1 takes the fast path, k100_i1 the counted
    one (the other source of the missing word); damaged: without one k-mer that is not its own complement"""
    g = load_golden(name)
    k, packed, cnt = g["k"], g["packed"], g["counts"]
    if damaged:
        rc = ktab.revcomp_packed(packed, k)
        other = np.flatnonzero((rc != packed).any(axis=1))
        keep = np.ones(len(cnt), bool)
        keep[other[len(other) // 2]] = False
        packed, cnt = packed[keep], cnt[keep]
    words = np.ascontiguousarray(packed_to_words(packed, k)).view(np.int64).reshape(-1)
    return k, torch.from_numpy(words.copy()), torch.from_numpy(np.ascontiguousarray(cnt).view(np.int16).copy())


@pytest.mark.parametrize("symcheck", ["hash", "exact"])
@pytest.mark.parametrize("damaged", [False, True])
@pytest.mark.parametrize("name", ["k31_i1", "k100_i1"])
@pytest.mark.parametrize("kind", ENGINES)
def test_proof_tail_is_the_four_proof_words_laid_out_by_the_rule(kind, name, damaged, symcheck):
    eng = make_engine(kind)
    dev = eng.device
    k, tk, tc = table(name, damaged)
    tk, tc = tk.to(dev), tc.to(dev)
    eng.bind(k, tk, tc)
    # pass 1 and the look-ups of this shard's own requests, by the calls of a sharded step (one rank: nothing to cut by)
    eng.pass1(symcheck)
    rw, nreq = eng.record_words(), eng.nreq()
    send = torch.zeros(max(nreq, 1) * rw, dtype=torch.int64, device=dev)
    assert eng.route(np.zeros(0, np.uint64), 1, send) == [nreq]
    eng.apply(send, nreq, wait=False)
    four = torch.zeros(4, dtype=torch.int64, device=dev)
    eng.proof_into(four)
    p = four.cpu().numpy().view(np.uint64)
    if damaged and symcheck == "hash":
        assert p[1] != 0 or p[2] != 0               # the partner of the k-mer that went is not cancelled
    elif damaged:
        assert p[0] > 0                             # the exact proof: its request finds nothing (no fingerprint is taken)
    else:
        assert not p[:3].any()
    assert p[3] == 0                                # (not a replayed step)
    for nslots, slot in SLOTS:
        n = 3 + 2 * nslots
        buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
        eng.proof_tail(buf[:n], nslots, slot)
        got = buf.cpu().numpy().view(np.uint64)
        want = np.zeros(n, dtype=np.uint64)
        want[0], want[1 + 2 * slot], want[2 + 2 * slot], want[n - 2], want[n - 1] = p[0], p[1], p[2], p[3], 0
        assert np.array_equal(got[:n], want), (nslots, slot)
        others = np.ones(n, bool)
        others[[0, 1 + 2 * slot, 2 + 2 * slot, n - 2, n - 1]] = False
        assert not got[:n][others].any(), (nslots, slot)             # zeros outside this rank's slot and the end words
        assert (got[n:] == np.uint64(SENTINEL)).all(), (nslots, slot)     # nothing behind the 3 + 2 nslots words


def test_stand_in_replay_verdict_sees_the_router_totals_move():
    """What the engine does with rp_totals (k_proof_replay) and the stand-in has to do alike: the recorded step stores the
    router's per-destination totals, a replayed step compares its own with them.  Same table, so the same requests emitted
    and kept; only the splitter moves between two replayed steps, and only the second one's verdict word is set."""
    from fake_engine import NumpyEngine
    from smudgeplot_amd import synth
    k = 12
    keys, cnt = synth.diploid_table_u64(300, k=k, seed=31, het_frac=0.5, cov=30, L=5)
    eng = NumpyEngine(torch.device("cpu"))
    eng.bind(k, torch.from_numpy(keys.view(np.int64).copy()), torch.from_numpy(cnt.view(np.int16).copy()))
    eng.set_replay(True)

    def step(splitter):
        eng.pass1("hash")
        kept = eng.filter(None)
        send = torch.zeros(max(kept, 1) * eng.record_words(), dtype=torch.int64)
        totals = eng.route(np.array([splitter], dtype=np.uint64), 2, send)
        eng.apply(send, kept, wait=False)
        tail = torch.zeros(3 + 2 * 2, dtype=torch.int64)
        eng.proof_tail(tail, 2, 1)
        replayed = bool(eng.replay_state() & 1)
        eng.replay_done(True)
        return kept, totals, [int(v) for v in tail[-2:]], replayed

    mid, third = keys[len(keys) // 2], keys[len(keys) // 3]
    kept, recorded, words, replayed = step(mid)
    assert kept > 0 and min(recorded) > 0 and words == [0, 0] and not replayed and eng.replay_state() & 2
    assert step(mid) == (kept, recorded, [0, 1], True)                 # replayed, and every count as recorded
    kept3, moved, words, replayed = step(third)
    assert kept3 == kept and sum(moved) == sum(recorded) and moved != recorded
    assert words == [1, 1] and replayed                                 # only the split moved: the verdict says so
