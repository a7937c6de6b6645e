#!/usr/bin/env python3
"""count_time.py -- stage times of the k-mer counter (libsmg_count.so) on seeded reads; the source of profiles/count_reads.md
and profiles/count_partitioned.md.

  python tools/count_time.py [--bases 2e9] [--k 31] [--repeats 5] [--warmup 1] [--dir DIR]
                             [--partitions 1,2,4,8,16] [--max-entries N] [--random] [--steps gen,bases]

The driver runs three steps, each a child process of its own under `timeout -k 10 <seconds>`, and stops at the first that
fails:  gen    reads of 150 bases from both strands of a seeded random genome (0.5 % substitutions), written to DIR as a
               stripped byte stream (reads.seq, one newline between reads) and as FASTQ (reads.fq)
        bases  smg_count_bases on reads.seq read into host memory: warm-up runs, then `repeats` timed runs
        files  smg_count_files on reads.fq (page cache warm after the first run), the same way
Stage times are the library's own (HIP events around extract, sort, reduce+merge, finish; host clock for read and wall).
Printed: one JSON line per step and a markdown table of medians with the min-max spread.
--partitions runs every timed step once per listed number of key ranges (0 = automatic); --max-entries is the library's test
hook of that name: with --partitions 0 a value below the windows of the fullest 12-bit bin forces bins to be split; --random replaces the reads of a genome
by independent random reads (nearly every window distinct); --steps picks the steps (the FASTQ is written only for `files`).
A binding without the `partitions` argument (an older build, for comparison) is run as it is.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ = 150
STAGES = ("ms_read", "ms_pack", "ms_plan", "ms_extract", "ms_sort", "ms_reduce", "ms_finish", "ms_wall")
HBM_PEAK = 8.0e12                     # bytes/s: what the project prices its roofline with


def gen(args):
    """torch on the device if there is one (plumbing only: a generator of test input), numpy otherwise"""
    nreads = int(args.bases) // READ
    G = int(args.genome)
    try:
        import torch
        dev = "cuda" if torch.cuda.is_available() else "cpu"
    except ImportError:
        torch, dev = None, "cpu"
    seq = np.empty((nreads, READ + 1), dtype=np.uint8)
    seq[:, READ] = ord("\n")
    step = 1 << 20
    if torch is not None:
        g = torch.Generator(device=dev); g.manual_seed(args.seed)
        genome = torch.randint(0, 4, (G,), generator=g, device=dev, dtype=torch.uint8)
        letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
        ar = torch.arange(READ, device=dev)
        for a in range(0, nreads, step):
            n = min(step, nreads - a)
            if args.random:
                seq[a:a + n, :READ] = letters[torch.randint(0, 4, (n, READ), generator=g, device=dev)].cpu().numpy()
                continue
            st = torch.randint(0, G - READ, (n,), generator=g, device=dev)
            R = genome[st[:, None] + ar]
            m = torch.rand((n, READ), generator=g, device=dev) < 0.005
            R = torch.where(m, (R + torch.randint(1, 4, (n, READ), generator=g, device=dev, dtype=torch.uint8)) & 3, R)
            flip = torch.rand((n,), generator=g, device=dev) < 0.5
            R = torch.where(flip[:, None], 3 - R.flip(1), R)
            seq[a:a + n, :READ] = letters[R.long()].cpu().numpy()
    else:
        rng = np.random.default_rng(args.seed)
        genome = rng.integers(0, 4, G).astype(np.uint8)
        letters = np.frombuffer(b"ACGT", np.uint8)
        for a in range(0, nreads, step):
            n = min(step, nreads - a)
            if args.random:
                seq[a:a + n, :READ] = letters[rng.integers(0, 4, (n, READ))]
                continue
            R = genome[rng.integers(0, G - READ, n)[:, None] + np.arange(READ)]
            m = rng.random(R.shape) < 0.005
            R = np.where(m, (R + rng.integers(1, 4, R.shape)) & 3, R).astype(np.uint8)
            flip = rng.random(n) < 0.5
            R[flip] = 3 - R[flip][:, ::-1]
            seq[a:a + n, :READ] = letters[R]
    seq.tofile(os.path.join(args.dir, "reads.seq"))
    # FASTQ with fixed-width records: @<10 digits>\n <read>\n +\n <quality>\n
    rec = np.empty((step, 12 + READ + 1 + 2 + READ + 1), dtype=np.uint8)
    with open(os.path.join(args.dir, "reads.fq"), "wb") as f:
        for a in range(0, nreads if "files" in args.steps.split(",") else 0, step):
            n = min(step, nreads - a)
            r = rec[:n]
            r[:, 0] = ord("@")
            ids = np.arange(a, a + n, dtype=np.int64)
            for d in range(10):
                r[:, 10 - d] = ord("0") + (ids // 10 ** d) % 10
            r[:, 11] = ord("\n")
            r[:, 12:12 + READ + 1] = seq[a:a + n]
            r[:, 12 + READ + 1] = ord("+"); r[:, 12 + READ + 2] = ord("\n")
            r[:, 12 + READ + 3:12 + 2 * READ + 3] = ord("I")
            r[:, -1] = ord("\n")
            r.tofile(f)
    print(json.dumps({"step": "gen", "reads": nreads, "bases": nreads * READ, "genome": G, "generator": dev,
                      "fastq_bytes": os.path.getsize(os.path.join(args.dir, "reads.fq"))}))


def timed(args, what):
    import inspect
    from smudgeplot_amd import count
    ranged = "partitions" in inspect.signature(count.count_bases).parameters
    if what == "bases":
        seq = np.fromfile(os.path.join(args.dir, "reads.seq"), dtype=np.uint8)
        run = lambda **kw: count.count_bases(seq, args.k, t=args.t, **kw)
    else:
        path = os.path.join(args.dir, "reads.fq")
        run = lambda **kw: count.count_files([path], args.k, t=args.t, threads=args.threads, **kw)
    out = {"step": what, "k": args.k, "t": args.t, "warmup": args.warmup, "repeats": args.repeats, "by_partitions": {}}
    for parts in [int(x) for x in args.partitions.split(",")] if ranged else [1]:
        kw = {"partitions": parts, "max_entries": args.max_entries} if ranged else {}
        runs = []
        try:
            for i in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                table, hist, st = run(**kw)
                st["ms_call"] = (time.perf_counter() - t0) * 1e3      # with the binding's copy of the table
                st["hist_sum"] = int(hist.sum())
                st["hist_weighted"] = int((hist.astype(object) * np.arange(len(hist)).astype(object)).sum())
                if i >= args.warmup:
                    runs.append(st)
        except count.CountError as e:                                 # a refusal is a result: recorded, the next value runs
            out["by_partitions"][str(parts)] = {"refused": str(e)}
            continue
        out["by_partitions"][str(parts)] = {"entries": int(table.nels), "runs": runs}
    print(json.dumps(out))


def summarise(res):
    lines = []
    for what in ("bases", "files"):
        for parts, got in res.get(what, {}).get("by_partitions", {}).items():
            if "refused" in got:
                lines.append(f"\n### {what}, partitions = {parts}: refused: {got['refused']}")
                continue
            runs = got["runs"]
            r0 = runs[0]
            med = lambda s: sorted(r.get(s, 0.0) for r in runs)[len(runs) // 2]
            lines.append(f"\n### {what}, partitions = {parts} ({r0.get('used', 1)} used, {r0.get('split', 0)} bins split, "
                         f"store {r0.get('store_bytes', 0) * 1e-9:.3f} GB): "
                         f"{r0['bases']:.3e} bases, {r0['windows']:.3e} windows, {r0['distinct']:.3e} distinct, "
                         f"{got['entries']:.3e} kept, {r0['batches']} batches, {len(runs)} runs after {res[what]['warmup']} warm-up\n")
            lines.append("| stage | median ms | min | max |")
            lines.append("|---|---|---|---|")
            for s in STAGES:
                v = sorted(r.get(s, 0.0) for r in runs)
                lines.append(f"| {s[3:]} | {v[len(v) // 2]:.2f} | {v[0]:.2f} | {v[-1]:.2f} |")
            dev = med("ms_pack") + med("ms_extract") + med("ms_sort") + med("ms_reduce") + med("ms_finish")
            lines.append(f"\nbases/s overall (wall): {r0['bases'] / med('ms_wall') * 1e3:.3e}; device stages {dev:.1f} ms; "
                         f"sum(hist) = {r0['hist_sum']}, sum(c * hist[c]) = {r0['hist_weighted']}")
            if r0.get("used", 1) == 1:
                ext_bytes = r0["bases"] + 8 * r0["windows"]
                lines.append(f"kc_extract<1>: {ext_bytes:.3e} bytes (1 in per base + 8 out per window) in {med('ms_extract'):.2f} ms = "
                             f"{ext_bytes / med('ms_extract') * 1e3 / 1e12:.2f} TB/s = {ext_bytes / med('ms_extract') * 1e3 / HBM_PEAK:.2f} of 8.0 TB/s")
            lines.append(f"sort: {med('ms_sort') / dev:.2f} of the device time, {r0['windows'] / med('ms_sort') * 1e3:.3e} keys/s")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", nargs="?", default="all", choices=["all", "gen", "bases", "files"])
    ap.add_argument("--bases", type=float, default=2e9)
    ap.add_argument("--genome", type=float, default=5e7)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--t", type=int, default=4)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--partitions", default="0", help="comma list of key-range counts, one timed series each (0 = automatic)")
    ap.add_argument("--max-entries", type=int, default=0)
    ap.add_argument("--random", action="store_true", help="independent random reads instead of reads of a genome")
    ap.add_argument("--steps", default="gen,bases,files")
    args = ap.parse_args()
    if args.step == "gen":
        return gen(args)
    if args.step in ("bases", "files"):
        return timed(args, args.step)
    own = args.dir is None
    d = args.dir or tempfile.mkdtemp(prefix="count_time_")
    res = {}
    try:
        for step in args.steps.split(","):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), step, "--dir", d,
                   "--bases", str(args.bases), "--genome", str(args.genome), "--k", str(args.k), "--t", str(args.t),
                   "--threads", str(args.threads), "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--seed", str(args.seed),
                   "--partitions", args.partitions, "--max-entries", str(args.max_entries), "--steps", args.steps] + (["--random"] if args.random else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                print(f"step {step} failed with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}", file=sys.stderr)
                return r.returncode
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            res[step] = json.loads(line)
        print(summarise(res))
    finally:
        if own:
            shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
