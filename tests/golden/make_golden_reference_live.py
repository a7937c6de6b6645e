#!/usr/bin/env python3
"""Regenerate tests/golden/reference_live.json: what the REFERENCE hetmers binary (oracle/_ref/hetmers_ref, compiled from
the reference's sources by oracle/Makefile) writes for the fresh random tables of tests/test_oracle.py::test_reference_live,
with a checksum of each table, so that the three-way check runs where the reference binary is not present too.
Run from the repo root where the reference sources exist:

    make -C oracle ref && python tests/golden/make_golden_reference_live.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from smudgeplot_amd import ktab, synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "hetmers_ref")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_live.json")

# k, ibyte, nparts, L, T, seed: the cases of test_reference_live
CASES = [(31, 1, 1, 5, 1, 101), (31, 2, 3, 5, 8, 102), (25, 1, 2, 4, 4, 103), (48, 2, 2, 4, 5, 104), (72, 1, 1, 4, 2, 105)]


def case_key(k, ibyte, nparts, L, T, seed):
    return "k%d_i%d_p%d_L%d_T%d_s%d" % (k, ibyte, nparts, L, T, seed)


def table_sha256(packed, cnt):
    return hashlib.sha256(packed.tobytes() + cnt.astype("<u2").tobytes()).hexdigest()


def main():
    out = {}
    for k, ibyte, nparts, L, T, seed in CASES:
        packed, cnt = synth.adversarial_table(k, 2000, L, seed, low_complexity=120, dense=2)
        with tempfile.TemporaryDirectory() as d:
            ktab.write_ktab(os.path.join(d, "t"), k, packed, cnt, ibyte=ibyte, nparts=nparts)
            subprocess.run([REF, f"-e{L}", f"-T{T}", "-oref", "t.ktab"], cwd=d, check=True, capture_output=True)
            smu = open(os.path.join(d, "ref.smu")).read()
        out[case_key(k, ibyte, nparts, L, T, seed)] = {"entries": int(len(cnt)), "table_sha256": table_sha256(packed, cnt),
                                                        "smu": smu}
        print(case_key(k, ibyte, nparts, L, T, seed), len(cnt), len(smu))
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
