#!/usr/bin/env python3
"""reads_to_smu_time.py -- the measurements behind profiles/reads_to_smu.md: closing a counted table by merge against the
generic closure, and reads to .smu in one process against `smg_count` followed by `hetmers`.

  python tools/reads_to_smu_time.py closure [--bases 1e6,1e8] [--k 31,51] [--repeats 5] [--warmup 1]
  python tools/reads_to_smu_time.py e2e --dir DIR [--bases 2e8] [--k 31] [--t 4] [--e 12] [--two-step-bin DIR2]
  python tools/reads_to_smu_time.py memory [--bases 2e8] [--k 31] [--t 4] [--e 12]
  python tools/reads_to_smu_time.py shards [--bases 1e8] [--k 31,51] [--shards 4] [--repeats 5] [--warmup 1]

closure  A canonical table is counted on the device from a seeded random sequence of `bases` bases (t = 1: nearly every
         window a distinct k-mer) and stays there.  Engine.close_canonical and Engine.condition(0, False, True) run on it in
         turn, `warmup` + `repeats` times each; the time is the engine's own (HIP events around the conditioning call,
         stats["ms_decode"]).  Prints one JSON line per (k, bases) with the medians and every run, and asserts that both routes
         leave tables of the same size.
e2e      Process wall clock, no device timing in the same command: `smg_count -e -n` against `smg_count` + `hetmers -e` on the
         reads.fq that `count_time.py gen --dir DIR` wrote, each route twice, alternating.  --two-step-bin names a directory
         with another build's bin/smg_count and bin/hetmers for the two-step route (default: this build's).
shards   One counted table (as for closure) handed to engine.hetmers_run_device, closed and run two ways in turn: in core, and
         forced into `shards` prefix shards of the closed table one after the other (SMG_DEVICE_SHARDS).  `warmup` + `repeats`
         times each; per run the wall clock of the call and the engine's own times.  Prints one JSON line per k with the
         medians and every run, and asserts that both ways give the same plot.
memory   hipMemGetInfo before and after count.reads_to_plot on a seeded stream, and the peak the run reports on the way
         (a sampling thread: 2 ms period), next to the size of the counted table.
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_stream(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(n), dtype=np.uint8)]


def closure(args):
    import torch
    from smudgeplot_amd import count, engine
    for k in [int(x) for x in args.k.split(",")]:
        for bases in [float(x) for x in args.bases.split(",")]:
            table, _, st = count.count_bases_device(random_stream(bases, 7), k, t=1)
            with table:
                e = engine.Engine(0, torch.cuda.current_stream().cuda_stream)
                runs = {"merge": [], "generic": []}
                sizes = set()
                try:
                    for i in range(args.warmup + args.repeats):
                        for route in ("merge", "generic"):
                            e.bind(k, table.nels, table.keys_ptr, table.counts_ptr)
                            n = e.close_canonical() if route == "merge" else e.condition(0, False, True)
                            sizes.add(n)
                            if i >= args.warmup:
                                runs[route].append(e.stats()["ms_decode"])
                finally:
                    e.close()
            assert len(sizes) == 1, sizes
            med = {r: sorted(v)[len(v) // 2] for r, v in runs.items()}
            print(json.dumps({"step": "closure", "k": k, "bases": bases, "entries": table.nels, "closed": sizes.pop(),
                              "median_ms": med, "runs_ms": runs, "warmup": args.warmup}), flush=True)


def shards(args):
    from smudgeplot_amd import count, engine
    fields = ("ms_decode", "ms_pass1", "ms_rclookup", "ms_pass2", "ms_total")
    for k in [int(x) for x in args.k.split(",")]:
        table, _, st = count.count_bases_device(random_stream(float(args.bases), 7), k, t=1)
        runs = {"core": [], "shards": []}
        plots, closed = {}, set()
        with table:
            for i in range(args.warmup + args.repeats):
                for way in ("core", "shards"):
                    os.environ.pop("SMG_DEVICE_SHARDS", None)
                    if way == "shards":
                        os.environ["SMG_DEVICE_SHARDS"] = str(args.shards)
                    t0 = time.perf_counter()
                    plot, est = engine.hetmers_run_device(k, table.nels, table.keys_ptr, table.counts_ptr, condition=engine.COND_SYMM)
                    wall = (time.perf_counter() - t0) * 1e3
                    os.environ.pop("SMG_DEVICE_SHARDS", None)
                    closed.add(est["nels"])
                    assert way not in plots or np.array_equal(plots[way], plot)
                    plots[way] = plot
                    if i >= args.warmup:
                        runs[way].append(dict({f: round(est[f], 3) for f in fields}, wall_ms=round(wall, 3)))
        assert np.array_equal(plots["core"], plots["shards"]) and len(closed) == 1, closed
        med = {w: {f: sorted(r[f] for r in v)[len(v) // 2] for f in fields + ("wall_ms",)} for w, v in runs.items()}
        print(json.dumps({"step": "shards", "k": k, "bases": float(args.bases), "entries": table.nels, "closed": closed.pop(),
                          "shards": args.shards, "pairs": int(plots["core"].sum()), "median": med, "runs": runs, "warmup": args.warmup}),
              flush=True)


def e2e(args):
    reads = os.path.join(args.dir, "reads.fq")
    here = os.path.join(ROOT, "smudgeplot_amd", "bin")
    two = os.path.join(os.path.abspath(args.two_step_bin), "bin") if args.two_step_bin else here
    fs = subprocess.run(["stat", "-f", "-c", "%T", args.dir], capture_output=True, text=True).stdout.strip()
    out = {"step": "e2e", "k": args.k, "t": args.t, "e": args.e, "fastq_bytes": os.path.getsize(reads), "filesystem": fs,
           "two_step_binaries": two, "one_process_s": [], "two_step_s": [], "two_step_count_s": [], "two_step_hetmers_s": []}

    def run(cmd):
        t0 = time.perf_counter()
        subprocess.run(cmd, cwd=args.dir, check=True, capture_output=True)
        return time.perf_counter() - t0

    for rep in range(args.repeats):
        for f in ("One.smu", "Two.smu", "Two.ktab", ".Two.ktab.1"):
            if os.path.exists(os.path.join(args.dir, f)):
                os.remove(os.path.join(args.dir, f))
        out["one_process_s"].append(run([os.path.join(here, "smg_count"), f"-k{args.k}", f"-t{args.t}", f"-e{args.e}", "-n", "-T8", "-oOne", reads]))
        a = run([os.path.join(two, "smg_count"), f"-k{args.k}", f"-t{args.t}", "-T8", "-oTwo", reads])
        b = run([os.path.join(two, "hetmers"), f"-e{args.e}", "-T8", "-oTwo", "Two.ktab"])
        out["two_step_count_s"].append(a); out["two_step_hetmers_s"].append(b); out["two_step_s"].append(a + b)
        same = open(os.path.join(args.dir, "One.smu"), "rb").read() == open(os.path.join(args.dir, "Two.smu"), "rb").read()
        assert same, "the two routes wrote different .smu files"
    out["table_bytes"] = os.path.getsize(os.path.join(args.dir, ".Two.ktab.1")) + os.path.getsize(os.path.join(args.dir, "Two.ktab"))
    out["smu_rows"] = sum(1 for _ in open(os.path.join(args.dir, "One.smu")))
    print(json.dumps(out), flush=True)


def memory(args):
    import torch
    from smudgeplot_amd import count
    seq = np.fromfile(os.path.join(args.dir, "reads.seq"), dtype=np.uint8) if args.dir else random_stream(args.bases, 7)
    torch.cuda.init()
    free0, total = torch.cuda.mem_get_info()
    low = [free0]
    stop = threading.Event()

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.002)

    th = threading.Thread(target=sample)
    th.start()
    try:
        plot, hist, st = count.reads_to_plot(seq, args.k, args.t, args.e)
    finally:
        stop.set(); th.join()
    free1, _ = torch.cuda.mem_get_info()
    W = (args.k + 31) // 32
    print(json.dumps({"step": "memory", "k": args.k, "t": args.t, "e": args.e, "bases": int(len(seq)), "kept": st["kept"],
                      "counted_table_bytes": st["kept"] * (8 * W + 2), "closed_entries": st["hetmers"]["nels"],
                      "free_before": free0, "lowest_free_sampled": low[0], "peak_in_use": free0 - low[0], "free_after": free1,
                      "device_total": total, "pairs": int(plot.sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=["closure", "e2e", "memory", "shards"])
    ap.add_argument("--bases", default=None)
    ap.add_argument("--k", default=None)
    ap.add_argument("--t", type=int, default=4)
    ap.add_argument("--e", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--two-step-bin", default=None)
    ap.add_argument("--shards", type=int, default=4)
    args = ap.parse_args()
    if args.step == "closure":
        args.bases = args.bases or "1e6,1e8"
        args.k = args.k or "31,51"
        args.repeats = args.repeats or 5
        return closure(args)
    if args.step == "shards":
        args.bases = args.bases or "1e8"
        args.k = args.k or "31,51"
        args.repeats = args.repeats or 5
        return shards(args)
    args.k = int(args.k or 31)
    args.bases = float(args.bases or 2e8)
    args.repeats = args.repeats or 2
    return e2e(args) if args.step == "e2e" else memory(args)


if __name__ == "__main__":
    sys.exit(main())
