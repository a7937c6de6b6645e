"""`extract_kmer_pairs` on tables that are NOT closed under reverse complement (the general path).  The reference only
probes entry #1 for symmetry, so it streams such a table as it is.  Goldens come from the REFERENCE binaries
(tests/golden/make_golden_extract_general.py, gzip-compressed JSON); smudge files are compared as sorted lists of lines."""
import glob
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import brute
from conftest import GOLDEN, HETMERS_BIN, ROOT, load_golden, make_table
from smudgeplot_amd import engine, ktab, synth

EXTRACT_BIN = os.path.join(ROOT, "smudgeplot_amd", "bin", "extract_kmer_pairs")
NAMES = sorted(os.path.basename(p)[len("general_extract_"):-len(".json.gz")]
               for p in glob.glob(os.path.join(GOLDEN, "general_extract_*.json.gz")))


def load_variant(name):
    """-> (derived table as a golden dict, labels {(covB, covA): smudge}, {smudge: sorted lines}, .sma rows)"""
    with gzip.open(os.path.join(GOLDEN, f"general_extract_{name}.json.gz"), "rt") as f:
        j = json.load(f)
    g = load_golden(j["table"])
    packed, counts = g["packed"], g["counts"].copy()
    if j["variant"] == "a":
        keep = np.ones(len(counts), bool)
        keep[j["dropped"]] = False
        packed, counts = packed[keep], counts[keep]
    else:
        counts[j["changed"]] = j["count"]
    lines = {lab: [l + "\n" for l in v] for lab, v in j["lines"].items()}
    return dict(g, packed=packed, counts=counts, smu=j["smu"]), {(b, a): lab for b, a, _, lab in j["labels"]}, lines, j["labels"]


def tab(packed, cnt, k):
    return make_table(dict(packed=packed, counts=cnt, k=k, ibyte=1, nparts=1))


def is_closed(packed, counts, k):
    have = {bytes(p): int(c) for p, c in zip(packed, counts)}
    return all(have.get(bytes(r)) == int(c) for r, c in zip(ktab.revcomp_packed(packed, k), counts))


def unclosed(packed, cnt, k, how, seed):
    """a: about 5 % of the entries dropped; b: one k-mer's count differs from its complement's"""
    rng = np.random.default_rng(seed)
    if how == "a":
        keep = rng.random(len(cnt)) > 0.05
        return packed[keep], cnt[keep]
    cand = np.nonzero((packed != ktab.revcomp_packed(packed, k)).any(axis=1))[0]
    cb = cnt.copy()
    cb[int(cand[rng.integers(0, len(cand))])] += 1
    return packed, cb


def all_labels(plot):
    s, m = np.nonzero(plot[:, :500])
    return {(int(mm), int(ss - mm)): ("1A1B", "3A1B", "2A2B")[(ss + mm) % 3] for ss, mm in zip(s.tolist(), m.tolist())}


def check(table, labels, want_plot, want, **kw):
    plot, got = engine.hetmers_extract(table, labels, **kw)
    assert np.array_equal(plot, want_plot), kw
    assert {lab: sorted(v) for lab, v in got.items()} == want, kw


# ---------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", NAMES)
def test_numpy_oracle_matches_reference_on_unclosed_tables(name):
    g, labels, lines, _ = load_variant(name)
    k, packed = g["k"], g["packed"]
    assert len(NAMES) == 10
    assert brute.smu_text(brute.hetmers_plot(packed, g["counts"], k)) == g["smu"]
    assert brute.extract_lines(packed, g["counts"], k, labels) == lines
    # not closed, yet the reference's probe (PloidyPlot.c:1199-1229) passes: from entry #1 on, the first k-mer that is
    # not its own complement finds its complement; and nothing is below the threshold
    assert not is_closed(packed, g["counts"], k) and int(g["counts"].min()) >= g["L"]
    where = {bytes(p): i for i, p in enumerate(packed)}
    rc = ktab.revcomp_packed(packed, k)
    i = 1
    while where.get(bytes(rc[i])) == i:
        i += 1
    assert bytes(rc[i]) in where


# ---------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("how", ["a", "b"])
@pytest.mark.parametrize("k", [19, 31, 32, 33, 51, 64, 65, 85, 86, 100, 128])
def test_extract_on_unclosed_fresh_tables_vs_oracle(k, how):
    packed, cnt = unclosed(*synth.adversarial_table(k, 2000, 4, 300 + k, low_complexity=100, dense=1), k, how, k)
    assert not is_closed(packed, cnt, k)
    want_plot = brute.hetmers_plot(packed, cnt, k)
    labels = {px: lab for px, lab in all_labels(want_plot).items() if (px[0] * 7 + px[1]) % 4}
    want = brute.extract_lines(packed, cnt, k, labels)
    assert sum(len(v) for v in want.values()) >= 300
    for mode in ("hash", "exact"):
        assert engine.hetmers_run(tab(packed, cnt, k), symcheck=mode)[1]["path"] == 2
        check(tab(packed, cnt, k), labels, want_plot, want, symcheck=mode)


@pytest.mark.gpu
def test_extract_on_canonical_only_table():
    """half of every complement pair missing (a raw, unsymmetrised FastK table), run as it is (condition=0)"""
    k = 25
    packed, cnt = synth.adversarial_table(k, 3000, 4, seed=34, low_complexity=100, dense=1)
    canon = np.array([bytes(a) <= bytes(b) for a, b in zip(packed, ktab.revcomp_packed(packed, k))])
    pa, ca = packed[canon], cnt[canon]
    want_plot = brute.hetmers_plot(pa, ca, k)
    want = brute.extract_lines(pa, ca, k, all_labels(want_plot))
    assert sum(len(v) for v in want.values()) >= 300
    check(tab(pa, ca, k), all_labels(want_plot), want_plot, want, condition=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_executables_on_unclosed_golden_tables(name, tmp_path):
    g, labels, lines, rows = load_variant(name)
    ktab.write_ktab(str(tmp_path / "t"), g["k"], g["packed"], g["counts"], ibyte=g["ibyte"], nparts=g["nparts"])
    for mode in ({}, {"SMUDGEPLOT_ONE_PROCESS": "1"}):
        r = subprocess.run([HETMERS_BIN, "-oout", f"-e{g['L']}", "-T4", "-v", "t.ktab"], cwd=tmp_path, capture_output=True,
                           text=True, env=dict(os.environ, **mode))
        assert r.returncode == 0 and "  The input table is trimmed and symmetric\n" in r.stderr, r.stderr
        assert (tmp_path / "out.smu").read_text() == g["smu"], mode
        (tmp_path / "out.smu").unlink()
    (tmp_path / "s.sma").write_text("covB\tcovA\tfreq\tsmudge\n" + "".join(f"{b}\t{a}\t{f}\t{lab}\n" for b, a, f, lab in rows))
    r = subprocess.run([EXTRACT_BIN, "-oout", f"-e{g['L']}", "-T4", "-v", "t.ktab", "s.sma"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "path=general" in r.stderr, r.stderr
    for lab, want in lines.items():
        assert sorted(open(tmp_path / f"out.{lab}.txt").readlines()) == want, lab


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k31_i1_a", "k31_i1_b", "k21_i2_p2_a", "k51_i1_p3_a", "k65_i1_b", "k100_wrap_b"])
def test_extract_general_over_virtual_shards(name, monkeypatch):
    """the shards of one device run the general path together, a prefix-side partner looked up in whichever shard holds
    it (TabSet) -- the extract leg too.  SMG_FORCE_MULTI: one rank notices the failed proof, one GPU takes over."""
    g, labels, lines, _ = load_variant(name)
    want_plot = brute.hetmers_plot(g["packed"], g["counts"], g["k"])
    for shards in (0, 2, 3, 5):
        if shards:
            monkeypatch.setenv("SMG_SHARD_LIMIT", str(len(g["counts"]) // shards + 1))
        for mode in ("hash", "exact"):
            check(make_table(g), labels, want_plot, lines, symcheck=mode)
    monkeypatch.delenv("SMG_SHARD_LIMIT")
    monkeypatch.setenv("SMG_FORCE_MULTI", "1")
    check(make_table(g), labels, want_plot, lines)


def _two_partner_hub(k=100, seed=11):
    """x has 255 partners at positions 0..84 plus y1 (position 90) and y2 (position 91): degree 257, wrapped to 1.  y1 and
    y2 have 255 partners of their own at positions 0..84 besides x: degree 256, wrapped to 0.  So x, the lower member, owns
    TWO pairs of the plot.  Not symmetrised: the table is not closed."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 3, size=k, dtype=np.uint8)               # (x[90], x[91] < 3: y1, y2 sort behind x)
    y1, y2 = x.copy(), x.copy()
    y1[90] += 1
    y2[91] += 1
    rows = [x, y1, y2]
    for z in (x, y1, y2):
        for p in range(85):
            for d in (1, 2, 3):
                v = z.copy(); v[p] = (v[p] + d) & 3; rows.append(v)
    packed = ktab.pack_bases(np.concatenate([np.array(rows), rng.integers(0, 4, size=(50, k), dtype=np.uint8)]))
    return ktab.sort_unique_packed(packed, rng.integers(5, 60, size=len(packed)).astype(np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("shards", [0, 3])
def test_extract_general_wrapped_degrees(shards, monkeypatch):
    """k > 85: a degree of 0 or 1 may have wrapped (PloidyPlot.c:163) and stand for hundreds of partners, so an entry can
    own more than one pair of the plot -- the records of such a lane take one atomic each"""
    k = 100
    packed, cnt = _two_partner_hub(k)
    a, _, _ = brute.unique_pairs(packed, cnt, k)
    want_plot = brute.hetmers_plot(packed, cnt, k)
    want = brute.extract_lines(packed, cnt, k, all_labels(want_plot))
    assert not is_closed(packed, cnt, k)
    assert sum(len(v) for v in want.values()) == len(a) > len(set(a.tolist())), "some entry must own more than one pair"
    cases = [(load_variant(n)[:3]) for n in ("k100_wrap_a", "k100_wrap_b")]
    cases = [(make_table(g), labels, brute.hetmers_plot(g["packed"], g["counts"], k), lines) for g, labels, lines in cases]
    cases.append((tab(packed, cnt, k), all_labels(want_plot), want_plot, want))
    for table, labels, wp, wl in cases:
        if shards:
            monkeypatch.setenv("SMG_SHARD_LIMIT", str(table.nels // shards + 1))
        for mode in ("hash", "exact"):
            check(table, labels, wp, wl, symcheck=mode)


@pytest.mark.gpu
def test_out_of_core_extract_still_refuses_an_unclosed_table(monkeypatch):
    """unchanged: out of core (shard after shard) a table that fails the proof is refused, for the extract leg too"""
    k = 31
    packed, cnt = unclosed(*synth.adversarial_table(k, 3000, 4, seed=5, low_complexity=40, dense=1), k, "a", 9)
    monkeypatch.setenv("SMG_SEQUENTIAL_SHARDS", "3")
    with pytest.raises(engine.EngineError, match="not closed under reverse complement"):
        engine.hetmers_extract(tab(packed, cnt, k), all_labels(brute.hetmers_plot(packed, cnt, k)))
