#!/usr/bin/env python3
"""Regenerate the fixtures on which the pair-sum limit decides degrees: tests/golden/k*_sumlimit.npz + .smu and, for k = 31 and
k = 100, extract_k*_sumlimit.json.

The tables come from tests/sum_limit_oracle.fixture_table (decoy families on every route; k = 100 with the two cases in which
the limit meets the uint8 wrap); every count is at or below 32767, beyond which the reference binary takes a table for
unsymmetric.  The `.smu` bytes and the extract lines are what the REFERENCE binaries wrote (oracle/_ref/hetmers_ref and
extract_ref, built by oracle/Makefile); every non-empty pixel of the plot is labelled, the decoy-decided ones among them.
Same keys and layout as make_golden.py and make_golden_extract.py.  Run from the repo root, where the reference sources are:

    make -C oracle ref && make -C smudgeplot_amd/csrc && python tests/golden/make_golden_sum_limit.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import sum_limit_oracle as so  # noqa: E402
from make_golden import run_ref  # noqa: E402
from smudgeplot_amd import engine, ktab  # noqa: E402

EXTRACT_REF = os.path.join(ROOT, "oracle", "_ref", "extract_ref")
OUT = os.path.dirname(os.path.abspath(__file__))
SMUDGES = ["1A1B", "2A1B", "2A2B"]
L = 4


def extract_ref(packed, cnt, k, labels):
    with tempfile.TemporaryDirectory() as tmp:
        ktab.write_ktab(os.path.join(tmp, "t"), k, packed, cnt, ibyte=1, nparts=1)
        with open(os.path.join(tmp, "s.sma"), "w") as f:
            f.write("covB\tcovA\tfreq\tsmudge\n")
            for covb, cova, freq, lab in labels:
                f.write(f"{covb}\t{cova}\t{freq}\t{lab}\n")
        r = subprocess.run([EXTRACT_REF, f"-e{L}", "-T3", "-oout", "t.ktab", "s.sma"], cwd=tmp, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return {lab: sorted(open(os.path.join(tmp, f"out.{lab}.txt")).read().splitlines()) for lab in sorted({l[3] for l in labels})}


def main():
    p1, wide = engine.pass1_limits(), engine.wide_limits()
    for name, k in sorted(so.FIXTURES.items()):
        t = so.fixture_table(name, so.mid_of(k, p1["D_WIN"], wide["F_HALO"]))
        assert int(t.cnt.max()) <= 32767
        smu = run_ref(t.packed, t.cnt, k, 1, 1, L, 2)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), packed=t.packed, counts=t.cnt, k=k, ibyte=1, nparts=1, L=L)
        open(os.path.join(OUT, name + ".smu"), "w").write(smu)
        print(f"{name}: n={len(t.cnt)} lines={smu.count(chr(10))}")
        if k in (31, 100):
            rows = [tuple(int(v) for v in line.split("\t")) for line in smu.splitlines()]
            labels = [(b, a, f, SMUDGES[(a + b) % 3]) for b, a, f in rows]
            lines = extract_ref(t.packed, t.cnt, k, labels)
            with open(os.path.join(OUT, f"extract_{name}.json"), "w") as f:
                json.dump({"table": name, "labels": labels, "lines": lines}, f, separators=(",", ":"))
            print(name, {lab: len(v) for lab, v in lines.items()})


if __name__ == "__main__":
    main()
