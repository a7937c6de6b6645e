"""Stage times of counting a k-mer dump (profiles/count_dump.md): a synthetic both-strand dump written from a
smudgeplot_amd.synth table, then, `--repeats` times each,
  records   count.dump_records: the HIP-event time of the line kernel alone, and its text bytes/s
  count     count.count_files(dump=True): the stage split of the whole call
  parse     count.dump_parse on the same file: the host twin's wall time, the host yardstick (once)
Every step is a child process under `timeout -k 10`; the tool stops at the first that fails.

    python tools/dump_time.py --lines 1e8 --k 31 --repeats 3
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def gen(a):
    """a dump of about a.lines lines: the both-strand table of synth.diploid_table_u64 (k <= 32: as it is; above: its 32-mers
    with k - 32 seeded random bases behind them), counts as five digits with leading zeros, written 4e6 lines at a time"""
    from smudgeplot_amd import synth
    t0 = time.time()
    k = a.k
    keys, cnt = synth.diploid_table_u64(int(a.lines / 2.6) + 1, k=min(k, 32), seed=a.seed)
    rng = np.random.default_rng(a.seed + 1)
    order = rng.permutation(len(keys)) if a.shuffle else None
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    sh = (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64))[None, :]
    width = k + 1 + 5 + 1
    n = len(keys)
    with open(a.path, "wb") as f:
        for lo in range(0, n, 4_000_000):
            idx = slice(lo, min(n, lo + 4_000_000)) if order is None else order[lo: lo + 4_000_000]
            kk, cc = keys[idx], cnt[idx].astype(np.int64)
            m = len(kk)
            out = np.empty((m, width), dtype=np.uint8)
            out[:, : min(k, 32)] = lut[((kk[:, None] >> sh) & np.uint64(3)).astype(np.intp)][:, : min(k, 32)]
            if k > 32:
                out[:, 32:k] = lut[rng.integers(0, 4, size=(m, k - 32))]
            out[:, k] = 9                                           # a tab
            for d in range(5):
                out[:, k + 1 + d] = 48 + (cc // 10 ** (4 - d)) % 10
            out[:, k + 6] = 10
            f.write(out.tobytes())
    print(json.dumps({"step": "gen", "lines": n, "bytes": n * width, "k": k, "seconds": round(time.time() - t0, 1)}), flush=True)


def records(a):
    from smudgeplot_amd import count
    keys, cnts, ms = count.dump_records(a.path, a.k)
    size = os.path.getsize(a.path)
    print(json.dumps({"step": "records", "lines": int(len(cnts)), "ms_lines": ms, "text_GB_per_s": size / ms * 1e-6}), flush=True)


def counting(a):
    from smudgeplot_amd import count
    tab, hist, st = count.count_files(a.path, a.k, t=a.t, dump=True)
    st = {n: (round(v, 3) if isinstance(v, float) else v) for n, v in st.items()}
    print(json.dumps({"step": "count", **st}), flush=True)


def parse(a):
    from smudgeplot_amd import count
    t0 = time.time()
    keys, cnts = count.dump_parse(a.path, a.k)
    print(json.dumps({"step": "parse", "lines": int(len(cnts)), "ms_wall": round((time.time() - t0) * 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("step", nargs="?", default="all", choices=["all", "gen", "records", "count", "parse"])
    ap.add_argument("--lines", type=float, default=1e8)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--t", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shuffle", action="store_true", help="lines in random order (the table is sorted)")
    ap.add_argument("--path", default=None)
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.step != "all":
        return {"gen": gen, "records": records, "count": counting, "parse": parse}[a.step](a)
    path = a.path or os.path.join(os.environ.get("TMPDIR", "/tmp"), f"dump_time_k{a.k}.txt")
    base = [sys.executable, os.path.abspath(__file__), "--lines", str(a.lines), "--k", str(a.k), "--t", str(a.t), "--seed", str(a.seed),
            "--path", path] + (["--shuffle"] if a.shuffle else [])
    steps = ["gen"] + ["records"] * a.repeats + ["count"] * a.repeats + ["parse"]
    try:
        for s in steps:
            r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), *base, s])
            if r.returncode != 0:
                print(json.dumps({"step": s, "failed": r.returncode}), flush=True)
                return r.returncode
    finally:
        if not a.keep and os.path.exists(path):
            os.remove(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
