#!/usr/bin/env python3
"""count_time.py -- stage times of the k-mer counter (libsmg_count.so) on seeded reads; the source of profiles/count_reads.md
profiles/count_partitioned.md, profiles/count_bgzf.md and profiles/count_bam.md.

  python tools/count_time.py [--bases 2e9] [--k 31] [--repeats 5] [--warmup 1] [--dir DIR]
                             [--partitions 1,2,4,8,16] [--max-entries N] [--random] [--steps gen,bases] [--read 150]

The driver runs three steps, each a child process of its own under `timeout -k 10 <seconds>`, and stops at the first that
fails:  gen    reads of 150 bases from both strands of a seeded random genome (0.5 % substitutions), written to DIR as a
               stripped byte stream (reads.seq, one newline between reads) and as FASTQ (reads.fq)
        bases  smg_count_bases on reads.seq read into host memory: warm-up runs, then `repeats` timed runs
        files  smg_count_files on reads.fq (page cache warm after the first run), the same way
        bgzf   (only where --steps names it) reads.fq written once more as BGZF at level 6 (reads.fq.gz, members of 65280 bytes);
               then the survey (smg_count_bgzf_scan), smg_count_bgzf_inflate alone (kernel time, text bytes per second of kernel
               and of wall time), smg_count_files on reads.fq.gz next to reads.fq, and as the baseline what a refused gzip file
               used to cost: one zlib thread (`gzip -dc`, or Python's gzip where there is none) to a plain file, then the plain
               run; and, where torch is there, the copy of the text to pinned host memory and back, which the route pays for
               parsing on the host
        bam    (only where --steps names it) the reads of reads.seq written as unaligned BAM (reads.bam: one record a read, FLAG 4,
               qualities 40; BGZF at level 6, members of 65280 bytes) and, where it is not there yet, as BGZF FASTQ; then
               smg_count_bam_strip (the unpack and the inflate kernel's time, the framer's host time, the copy of the stripped
               bytes to the host: smg_count_bam_report), smg_count_files on reads.bam next to reads.fq.gz with the two tables
               compared in every run, and, where torch is there, the copy of the stripped bytes from pinned memory to the device,
               which the ring pays
--read is the length of the reads (gen, and every step that reads what it wrote).
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
    step = min(1 << 20, max(1, (1 << 28) // READ))               # reads made at a time
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
        for a in range(0, nreads if {"files", "bgzf", "bam"} & set(args.steps.split(",")) else 0, step):
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


def _bgzf_member(piece):
    import struct
    import zlib
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = c.compress(piece) + c.flush()
    return (struct.pack("<4BI2BH2sHH", 31, 139, 8, 4, 0, 0, 255, 6, b"BC", 2, len(z) + 25) + z +
            struct.pack("<II", zlib.crc32(piece), len(piece)))


def bgzf(args):
    import multiprocessing
    import shutil as sh
    from smudgeplot_amd import count
    fq, gz, back = (os.path.join(args.dir, n) for n in ("reads.fq", "reads.fq.gz", "reads.back.fq"))
    data = open(fq, "rb").read()
    t0 = time.perf_counter()
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool, open(gz, "wb") as f:
        for m in pool.imap(_bgzf_member, (data[a:a + 65280] for a in range(0, len(data), 65280)), chunksize=64):
            f.write(m)
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    out = {"step": "bgzf", "k": args.k, "t": args.t, "warmup": args.warmup, "repeats": args.repeats, "text_bytes": len(data),
           "file_bytes": os.path.getsize(gz), "write_s": time.perf_counter() - t0}
    spread = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}
    scan, runs = [], []
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        got = count.bgzf_scan(gz)
        scan.append((time.perf_counter() - t0) * 1e3)
    out["blocks"] = got["blocks"]
    out["scan_ms"] = spread(scan[args.warmup:])
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        text, ms = count.bgzf_inflate(gz)
        runs.append((ms, (time.perf_counter() - t0) * 1e3))
        assert len(text) == len(data) and (i or text == data)
    del text
    out["inflate_kernel_ms"] = spread([r[0] for r in runs[args.warmup:]])
    out["inflate_wall_ms"] = spread([r[1] for r in runs[args.warmup:]])
    tables = {}
    for name, path in (("plain", fq), ("bgzf", gz)):
        walls = []
        for i in range(args.warmup + args.repeats):
            table, hist, st = count.count_files([path], args.k, t=args.t, threads=args.threads)
            walls.append(st["ms_wall"])
        tables[name] = (table.packed, table.counts, hist)
        out[f"count_{name}_wall_ms"] = spread(walls[args.warmup:])
        out[f"count_{name}_read_ms"] = st["ms_read"]
    out["tables_equal"] = all(np.array_equal(a, b) for a, b in zip(tables["plain"], tables["bgzf"]))
    base = []
    for i in range(max(1, args.repeats // 2)):
        t0 = time.perf_counter()
        if sh.which("gzip"):
            with open(back, "wb") as f:
                subprocess.run(["gzip", "-dc", gz], stdout=f, check=True)
            out["baseline_tool"] = "gzip -dc"
        else:
            import gzip
            with gzip.open(gz, "rb") as g, open(back, "wb") as f:
                sh.copyfileobj(g, f, 1 << 22)
            out["baseline_tool"] = "python gzip"
        t1 = time.perf_counter()
        _, _, st = count.count_files([back], args.k, t=args.t, threads=args.threads)
        base.append(((t1 - t0) * 1e3, st["ms_wall"]))
    out["baseline_decompress_ms"] = spread([b[0] for b in base])
    out["baseline_total_ms"] = spread([b[0] + b[1] for b in base])
    try:
        import torch
        h = torch.empty(len(data), dtype=torch.uint8).pin_memory()
        d = torch.empty(len(data), dtype=torch.uint8, device="cuda")
        trips = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.copy_(d); d.copy_(h)
            torch.cuda.synchronize()
            trips.append((time.perf_counter() - t0) * 1e3)
        out["text_trip_ms"] = spread(trips[args.warmup:])
    except Exception as e:                                            # (no torch, no device: the figure is left out)
        out["text_trip_ms"] = None
        out["text_trip_error"] = str(e)
    print(json.dumps(out))


def summarise_bgzf(b):
    f = lambda v: f"{v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f})"
    n = b["text_bytes"]
    lines = [f"\n### bgzf: {n:.3e} text bytes in {b['blocks']} blocks, {b['file_bytes']:.3e} bytes of file, {b['repeats']} runs after "
             f"{b['warmup']} warm-up; ms as median (min - max)\n",
             "| what | ms | text bytes/s at the median |", "|---|---|---|",
             f"| survey (bgzf_scan) | {f(b['scan_ms'])} | {b['scan_ms']['median'] / b['blocks'] * 1e6:.0f} ms per million blocks |",
             f"| bgzf_inflate, kernel | {f(b['inflate_kernel_ms'])} | {n / b['inflate_kernel_ms']['median'] * 1e3:.3e} |",
             f"| bgzf_inflate, wall | {f(b['inflate_wall_ms'])} | {n / b['inflate_wall_ms']['median'] * 1e3:.3e} |",
             f"| count_files, plain file, wall | {f(b['count_plain_wall_ms'])} | {n / b['count_plain_wall_ms']['median'] * 1e3:.3e} |",
             f"| count_files, BGZF file, wall | {f(b['count_bgzf_wall_ms'])} | {n / b['count_bgzf_wall_ms']['median'] * 1e3:.3e} |",
             f"| baseline: {b['baseline_tool']} to a plain file | {f(b['baseline_decompress_ms'])} | {n / b['baseline_decompress_ms']['median'] * 1e3:.3e} |",
             f"| baseline: that and the plain run | {f(b['baseline_total_ms'])} | {n / b['baseline_total_ms']['median'] * 1e3:.3e} |"]
    if b.get("text_trip_ms"):
        lines.append(f"| the text to pinned host memory and back | {f(b['text_trip_ms'])} | "
                     f"{b['text_trip_ms']['median'] / b['count_bgzf_wall_ms']['median']:.2f} of the BGZF run's wall time |")
    lines.append(f"\ntables of the plain and the BGZF run equal: {b['tables_equal']}")
    return "\n".join(lines)


def _bam_records(seq, first):
    """[n, READ + 1] sequence bytes (the last column the newline) -> [n, record size] uint8: the BAM records of these reads"""
    import struct
    n, L = seq.shape[0], seq.shape[1] - 1
    packed = (L + 1) // 2
    size = 4 + 32 + 11 + packed + L
    rec = np.zeros((n, size), dtype=np.uint8)
    fixed = struct.pack("<iiiBBHHHiiii", size - 4, -1, -1, 11, 0, 4680, 0, 4, L, -1, -1, 0)
    rec[:, :36] = np.frombuffer(fixed, np.uint8)
    ids = np.arange(first, first + n, dtype=np.int64)
    for d in range(10):
        rec[:, 36 + 9 - d] = ord("0") + (ids // 10 ** d) % 10
    lut = np.full(256, 15, np.uint8)
    for code, c in enumerate(b"=ACMGRSVTWYHKDBN"):
        lut[c] = code
    codes = np.zeros((n, 2 * packed), dtype=np.uint8)
    codes[:, :L] = lut[seq[:, :L]]
    rec[:, 47:47 + packed] = codes[:, 0::2] << 4 | codes[:, 1::2]
    rec[:, 47 + packed:] = 40
    return rec


def _bgzf_file(pool, path, pieces):
    with open(path, "wb") as f:
        for m in pool.imap(_bgzf_member, pieces, chunksize=64):
            f.write(m)
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def bam(args):
    import multiprocessing
    from smudgeplot_amd import count
    seqp, fq, gz, bamp = (os.path.join(args.dir, n) for n in ("reads.seq", "reads.fq", "reads.fq.gz", "reads.bam"))
    seq = np.fromfile(seqp, dtype=np.uint8).reshape(-1, READ + 1)
    sam = b"@HD\tVN:1.6\tSO:unknown\n"
    head = b"BAM\1" + len(sam).to_bytes(4, "little") + sam + (0).to_bytes(4, "little")
    t0 = time.perf_counter()
    step = max(1, (1 << 27) // (2 * READ))
    text = head + b"".join(_bam_records(seq[a:a + step], a).tobytes() for a in range(0, len(seq), step))
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        _bgzf_file(pool, bamp, (text[a:a + 65280] for a in range(0, len(text), 65280)))
        if not os.path.exists(gz):
            data = open(fq, "rb").read()
            _bgzf_file(pool, gz, (data[a:a + 65280] for a in range(0, len(data), 65280)))
            del data
    out = {"step": "bam", "k": args.k, "t": args.t, "warmup": args.warmup, "repeats": args.repeats, "reads": len(seq), "read": READ,
           "text_bytes": len(text), "file_bytes": os.path.getsize(bamp), "fastq_text_bytes": os.path.getsize(fq),
           "fastq_file_bytes": os.path.getsize(gz), "write_s": time.perf_counter() - t0}
    del text
    spread = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}
    runs = []
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        got, records, ms = count.bam_strip(bamp)
        wall = (time.perf_counter() - t0) * 1e3
        rep = count.bam_report(bamp)
        assert records == len(seq) and len(got) == seq.size - 1 and abs(rep["ms_unpack"] - ms) < 1e-6
        if i == 0:                                                    # the stream is the file gen wrote, less its last newline
            assert np.array_equal(np.frombuffer(got, np.uint8), seq.reshape(-1)[:-1])
        runs.append(dict(rep, wall=wall))
        del got
    out["stripped_bytes"] = int(seq.size - 1)
    for key in ("ms_unpack", "ms_inflate", "ms_frame", "ms_d2h", "wall"):
        out["strip_" + key] = spread([r[key] for r in runs[args.warmup:]])
    walls, tables = {"bam": [], "fastq": []}, {}
    for i in range(args.warmup + args.repeats):
        for name, path in (("bam", bamp), ("fastq", gz)):
            table, hist, st = count.count_files([path], args.k, t=args.t, threads=args.threads)
            walls[name].append(st["ms_wall"])
            tables[name] = (table.packed, table.counts, hist)
            if name == "bam":
                out["count_bam_report"] = count.bam_report(bamp)
        assert all(np.array_equal(a, b) for a, b in zip(tables["bam"], tables["fastq"])), "the BAM and the FASTQ tables differ"
    out["tables_equal_in_every_run"] = True
    out["count_bam_wall_ms"] = spread(walls["bam"][args.warmup:])
    out["count_fastq_wall_ms"] = spread(walls["fastq"][args.warmup:])
    try:
        import torch
        h = torch.empty(seq.size, dtype=torch.uint8).pin_memory()
        d = torch.empty(seq.size, dtype=torch.uint8, device="cuda")
        trips = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.copy_(h)
            torch.cuda.synchronize()
            trips.append((time.perf_counter() - t0) * 1e3)
        out["ring_h2d_ms"] = spread(trips[args.warmup:])
    except Exception as e:                                            # (no torch, no device: the figure is left out)
        out["ring_h2d_ms"] = None
        out["ring_h2d_error"] = str(e)
    print(json.dumps(out))


def summarise_bam(b):
    f = lambda v: f"{v['median']:.1f} ({v['min']:.1f} - {v['max']:.1f})"
    n, s = b["text_bytes"], b["stripped_bytes"]
    per = lambda v, m: f"{m / v['median'] * 1e3:.3e}"
    lines = [f"\n### bam: {b['reads']} reads of {b['read']} bases, {n:.3e} bytes of BAM text in {b['file_bytes']:.3e} bytes of file, "
             f"{s:.3e} stripped bytes; {b['repeats']} runs after {b['warmup']} warm-up; ms as median (min - max)\n",
             "| what | ms | bytes/s at the median |", "|---|---|---|",
             f"| bam_unpack, kernel (bam_strip) | {f(b['strip_ms_unpack'])} | {per(b['strip_ms_unpack'], s)} stripped |",
             f"| inf_members, kernel, same file | {f(b['strip_ms_inflate'])} | {per(b['strip_ms_inflate'], n)} text |",
             f"| the framer, host | {f(b['strip_ms_frame'])} | {per(b['strip_ms_frame'], n)} text |",
             f"| the stripped bytes to the host (D2H) | {f(b['strip_ms_d2h'])} | {per(b['strip_ms_d2h'], s)} stripped |",
             f"| bam_strip, wall | {f(b['strip_wall'])} | {per(b['strip_wall'], s)} stripped |",
             f"| count_files, BAM, wall | {f(b['count_bam_wall_ms'])} | {per(b['count_bam_wall_ms'], s)} stripped |",
             f"| count_files, BGZF FASTQ of the same reads, wall | {f(b['count_fastq_wall_ms'])} | {per(b['count_fastq_wall_ms'], s)} stripped |"]
    if b.get("ring_h2d_ms"):
        lines.append(f"| the stripped bytes from pinned memory to the device (what the ring pays) | {f(b['ring_h2d_ms'])} | {per(b['ring_h2d_ms'], s)} stripped |")
    r = b["count_bam_report"]
    lines.append(f"\nin the last counting run the reader thread spent on the BAM file: framing {r['ms_frame']:.1f} ms, inflate kernel "
                 f"{r['ms_inflate']:.1f} ms, unpack kernel {r['ms_unpack']:.1f} ms, D2H of the stripped bytes {r['ms_d2h']:.1f} ms")
    lines.append(f"tables of the BAM and the BGZF FASTQ run equal in every run: {b['tables_equal_in_every_run']}")
    return "\n".join(lines)


def summarise(res):
    lines = [summarise_bgzf(res["bgzf"])] if "bgzf" in res else []
    if "bam" in res:
        lines.append(summarise_bam(res["bam"]))
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
    ap.add_argument("step", nargs="?", default="all", choices=["all", "gen", "bases", "files", "bgzf", "bam"])
    ap.add_argument("--read", type=int, default=150, help="bases of a read")
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
    global READ
    READ = args.read
    if args.step == "bam":
        return bam(args)
    if args.step == "gen":
        return gen(args)
    if args.step in ("bases", "files"):
        return timed(args, args.step)
    if args.step == "bgzf":
        return bgzf(args)
    own = args.dir is None
    d = args.dir or tempfile.mkdtemp(prefix="count_time_")
    res = {}
    try:
        for step in args.steps.split(","):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), step, "--dir", d,
                   "--bases", str(args.bases), "--genome", str(args.genome), "--k", str(args.k), "--t", str(args.t),
                   "--threads", str(args.threads), "--read", str(args.read), "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--seed", str(args.seed),
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
