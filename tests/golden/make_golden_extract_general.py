#!/usr/bin/env python3
"""Regenerate tests/golden/general_extract_*.json.gz: tables that are NOT closed under reverse complement but pass the
reference's one-entry probe (PloidyPlot.c:1199-1229), so that the reference runs them as they are.  Two variants of
each source table, with a fixed seed: (a) about 5 % of the entries dropped, entry #1 and its complement kept; (b) one
k-mer's count raised by one.  Per variant: the derivation, the REFERENCE hetmers' .smu and the lines the REFERENCE
extract_kmer_pairs writes for a label set built like make_golden_extract.py's, sorted per smudge.  In the build container:

    make -C oracle ref && python tests/golden/make_golden_extract_general.py
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from smudgeplot_amd import ktab  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2024


def variants(name, packed, cnt, k):
    rng = np.random.default_rng(SEED + sum(map(ord, name)))
    rc = ktab.revcomp_packed(packed, k)
    where = {bytes(p): i for i, p in enumerate(packed)}
    drop = rng.random(len(cnt)) < 0.05
    i = 1                                          # what the probe looks at: entry #1 on, up to the first non-palindrome
    while True:
        j = where[bytes(rc[i])]
        drop[[i, j]] = False
        if j != i:
            break
        i += 1
    yield "a", {"dropped": np.nonzero(drop)[0].tolist()}, packed[~drop], cnt[~drop]
    cand = np.nonzero((packed != rc).any(axis=1))[0]
    j = int(cand[rng.integers(0, len(cand))])
    cb = cnt.copy()
    cb[j] += 1
    yield "b", {"changed": j, "count": int(cb[j])}, packed, cb


def run(tool, args, tmp):
    r = subprocess.run([os.path.join(REF, tool), *args], cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "trimmed and symmetric" in r.stderr and "Making" not in r.stderr and "Trimming" not in r.stderr, r.stderr


for name in ["k31_i1", "k21_i2_p2", "k51_i1_p3", "k65_i1", "k100_wrap"]:
    d = np.load(os.path.join(OUT, name + ".npz"))
    k, ibyte, nparts, L = int(d["k"]), int(d["ibyte"]), int(d["nparts"]), int(d["L"])
    for tag, how, vp, vc in variants(name, d["packed"], d["counts"], k):
        have = {bytes(p): int(c) for p, c in zip(vp, vc)}
        assert int(vc.min()) >= L and any(have.get(bytes(r)) != int(c) for r, c in zip(ktab.revcomp_packed(vp, k), vc))
        with tempfile.TemporaryDirectory() as tmp:
            ktab.write_ktab(os.path.join(tmp, "t"), k, vp, vc, ibyte=ibyte, nparts=nparts)
            run("hetmers_ref", [f"-e{L}", "-T3", "-v", "-oout", "t.ktab"], tmp)
            smu = open(os.path.join(tmp, "out.smu")).read()
            rows = [tuple(int(v) for v in line.split("\t")) for line in smu.splitlines()]
            labels = [(b, a, f, ["1A1B", "2A1B", "2A2B"][(b + a) % 3]) for n, (b, a, f) in enumerate(rows) if n % 3 != 2]
            with open(os.path.join(tmp, "s.sma"), "w") as f:
                f.write("covB\tcovA\tfreq\tsmudge\n" + "".join(f"{b}\t{a}\t{q}\t{lab}\n" for b, a, q, lab in labels))
            run("extract_ref", [f"-e{L}", "-T3", "-v", "-oout", "t.ktab", "s.sma"], tmp)
            lines = {lab: sorted(open(os.path.join(tmp, f"out.{lab}.txt")).read().splitlines())
                     for lab in sorted({l[3] for l in labels})}
        path = os.path.join(OUT, f"general_extract_{name}_{tag}.json.gz")
        doc = {"table": name, "variant": tag, "seed": SEED, **how, "smu": smu, "labels": labels, "lines": lines}
        with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:      # (mtime 0: same bytes every time)
            f.write(json.dumps(doc, separators=(",", ":")).encode())
        assert os.path.getsize(path) < 100_000, path
        print(name, tag, len(vc), {s: len(v) for s, v in lines.items()})
