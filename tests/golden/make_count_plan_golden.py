#!/usr/bin/env python3
"""Writes tests/golden/count_plan.json: what `smg_count_plan` returns on the histograms of tests/test_count_parts_host.py --
number of ranges and SHA-256 of the int32 cuts per (histogram, budget, partitions), and the text of its refusals.  Run
once, on the build BEFORE the flat planner (`smg_count_plan_fine`) was added; tests/test_count_fine_host.py holds every
later build to it.  Needs the built library, no GPU:  python tests/golden/make_count_plan_golden.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from smudgeplot_amd import count            # noqa: E402
from test_count_parts_host import HISTS     # noqa: E402


def main():
    cuts, refused = [], []
    for name in sorted(HISTS):
        w = HISTS[name]
        top, total = max(int(w.max()), 1), max(int(w.astype(object).sum()), 1)
        runs = [(b, 0) for b in sorted({top, top + 1, 2 * top, max(total // 7, top), max(total // 2, top), total, 10 * total})]
        runs += [(0, p) for p in (1, 2, 3, 7, 64, 4096)]
        for budget, parts in runs:
            c = count.plan(w, budget, partitions=parts)
            cuts.append({"hist": name, "budget": budget, "partitions": parts, "ranges": len(c) - 1,
                         "sha256": hashlib.sha256(c.astype("<i4").tobytes()).hexdigest()})
        if top > 1:
            try:
                count.plan(w, top - 1)
            except count.CountError as e:
                refused.append({"hist": name, "budget": top - 1, "message": str(e)})
    with open(os.path.join(HERE, "count_plan.json"), "w") as f:
        json.dump({"cuts": cuts, "refused": refused}, f, indent=1)
        f.write("\n")
    print(len(cuts), "plans,", len(refused), "refusals")


if __name__ == "__main__":
    main()
