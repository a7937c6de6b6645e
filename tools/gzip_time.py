#!/usr/bin/env python3
"""Times the plain-gzip route of the k-mer counter (smg_count -g) on one MI355X against the same session's alternatives.

    python tools/gzip_time.py [--bases 6e8] [--repeats 3] [--warmup 1] [--spans 262144,65536] [--levels 6,1] [--dir DIR]

The reads are those of tools/count_time.py (its `gen` step: 150-base reads of a 5e7-base genome, FASTQ records of fixed width).
reads.fq is written as plain gzip at every level asked for (the `gzip` tool where there is one, zlib otherwise) and as BGZF at
level 6.  Then, each figure the median (min - max) of --repeats runs after --warmup:
  - count.gzip_inflate of every gzip file at every span: the three kernel times (finder + marker decoder, resolver, exact
    decoder: HIP events), the wall time, and what count.gzip_report says (spans, linked, repaired);
  - count.count_files: the plain file, the BGZF file, every gzip file with gzip=True (stats["ms_wall"]), the tables compared;
  - the executable: `smg_count -g -n -H reads.fq.gz` against `gzip -dc reads.fq.gz > back.fq` followed by `smg_count -n -H
    back.fq` (wall clock of the processes).
One JSON line at the end; profiles/count_gzip.md is written from it."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}


def write_gzip(fq, gz, level):
    if shutil.which("gzip"):
        with open(gz, "wb") as f:
            subprocess.run(["gzip", f"-{level}", "-c", fq], stdout=f, check=True)
        return "gzip"
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    with open(fq, "rb") as f, open(gz, "wb") as g:
        for piece in iter(lambda: f.read(1 << 24), b""):
            g.write(c.compress(piece))
        g.write(c.flush())
    return "zlib"


def write_bgzf(fq, gz):
    import multiprocessing
    import count_time
    data = open(fq, "rb").read()
    with multiprocessing.Pool(8) as pool, open(gz, "wb") as f:
        for m in pool.imap(count_time._bgzf_member, (data[a:a + 65280] for a in range(0, len(data), 65280)), chunksize=64):
            f.write(m)
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=6e8)
    ap.add_argument("--genome", type=float, default=5e7)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--t", type=int, default=4)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--spans", default="262144,65536")
    ap.add_argument("--levels", default="6,1")
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    args.random, args.steps = False, "files"
    own = args.dir is None
    args.dir = args.dir or tempfile.mkdtemp(prefix="gzip_time_")
    import count_time
    from smudgeplot_amd import count
    t0 = time.perf_counter()
    count_time.gen(args)
    fq = os.path.join(args.dir, "reads.fq")
    levels = [int(x) for x in args.levels.split(",")]
    spans = [int(x) for x in args.spans.split(",")]
    out = {"text_bytes": os.path.getsize(fq), "k": args.k, "t": args.t, "repeats": args.repeats, "warmup": args.warmup, "files": {}, "count": {}}
    print(f"reads written in {time.perf_counter() - t0:.1f} s", flush=True)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(len(levels) + 1) as ex:
        jobs = {lv: ex.submit(write_gzip, fq, os.path.join(args.dir, f"reads{lv}.fq.gz"), lv) for lv in levels}
        jobs["bgzf"] = ex.submit(write_bgzf, fq, os.path.join(args.dir, "reads.bgzf.fq.gz"))
        out["writer"] = [j.result() for j in jobs.values()][0]
    print(f"compressed in {time.perf_counter() - t0:.1f} s", flush=True)
    n = args.warmup + args.repeats
    for lv in levels:
        gz = os.path.join(args.dir, f"reads{lv}.fq.gz")
        rec = out["files"][f"level{lv}"] = {"file_bytes": os.path.getsize(gz), "spans": {}}
        for span in spans if lv == levels[0] else spans[:1]:
            runs = []
            for i in range(n):
                t0 = time.perf_counter()
                text, ms = count.gzip_inflate(gz, span)
                runs.append(ms + ((time.perf_counter() - t0) * 1e3,))
                assert len(text) == out["text_bytes"]
                del text
            rep = count.gzip_report(gz)
            rec["spans"][str(span)] = {"ms_marker": spread([r[0] for r in runs[args.warmup:]]), "ms_resolve": spread([r[1] for r in runs[args.warmup:]]),
                                       "ms_exact": spread([r[2] for r in runs[args.warmup:]]), "ms_call": spread([r[3] for r in runs[args.warmup:]]),
                                       "report": {c: rep[c] for c in ("members", "text_bytes", "spans", "linked", "repaired")}}
            print(f"level {lv} span {span}: {rec['spans'][str(span)]}", flush=True)
    tables = {}
    series = [("plain", fq, False), ("bgzf", os.path.join(args.dir, "reads.bgzf.fq.gz"), False)] + \
             [(f"gzip{lv}", os.path.join(args.dir, f"reads{lv}.fq.gz"), True) for lv in levels]
    for name, path, gz in series:
        walls, reads = [], []
        for i in range(n):
            table, hist, st = count.count_files([path], args.k, t=args.t, threads=args.threads, gzip=gz)
            walls.append(st["ms_wall"]); reads.append(st["ms_read"])
        tables[name] = (table.packed, table.counts, hist)
        out["count"][name] = {"ms_wall": spread(walls[args.warmup:]), "ms_read": spread(reads[args.warmup:])}
        print(f"count {name}: {out['count'][name]}", flush=True)
    out["tables_equal"] = all(all(np.array_equal(a, b) for a, b in zip(tables["plain"], tables[name])) for name in tables)
    del tables
    gz, back = os.path.join(args.dir, f"reads{levels[0]}.fq.gz"), os.path.join(args.dir, "back.fq")
    exe, base, dec = [], [], []
    for i in range(n):
        t0 = time.perf_counter()
        subprocess.run([count.BIN_PATH, "-g", "-n", "-H", f"-k{args.k}", f"-t{args.t}", f"-T{args.threads}", "-o" + os.path.join(args.dir, "g"), gz], check=True)
        exe.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        if shutil.which("gzip"):
            with open(back, "wb") as f:
                subprocess.run(["gzip", "-dc", gz], stdout=f, check=True)
        else:
            import gzip
            with gzip.open(gz, "rb") as g, open(back, "wb") as f:
                shutil.copyfileobj(g, f, 1 << 22)
        dec.append((time.perf_counter() - t0) * 1e3)
        subprocess.run([count.BIN_PATH, "-n", "-H", f"-k{args.k}", f"-t{args.t}", f"-T{args.threads}", "-o" + os.path.join(args.dir, "p"), back], check=True)
        base.append((time.perf_counter() - t0) * 1e3)
    out["same_hist"] = open(os.path.join(args.dir, "g.hist.txt"), "rb").read() == open(os.path.join(args.dir, "p.hist.txt"), "rb").read()
    out["smg_count_g_ms"] = spread(exe[args.warmup:])
    out["decompress_ms"] = spread(dec[args.warmup:])
    out["decompress_then_smg_count_ms"] = spread(base[args.warmup:])
    print(json.dumps(out))
    if own:
        shutil.rmtree(args.dir, ignore_errors=True)


if __name__ == "__main__":
    main()
