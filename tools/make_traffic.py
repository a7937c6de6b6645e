#!/usr/bin/env python3
"""profiles/hbm_traffic.json entry from two PMC passes (tools/pmc_summary.py outputs: one with FETCH_SIZE, one with WRITE_SIZE).

usage: make_traffic.py <key> <entries> <pmc_fetch.txt> <pmc_write.txt> <label> [json]
HBM bytes of a kernel = (2 x FETCH_SIZE + WRITE_SIZE) KiB: the counters are in KiB and FETCH_SIZE reports one half of a
coalesced read on gfx950 (MI355X_MICROARCH.md, section HBM; profiles/r01_calibration_fetch_size.txt).  The entry carries
the hash of the engine's gfx950 code object the counters were read on: bench.py gives no traffic figure for another one.

How the entries on file were made, per workload (R = the repository, O = an output directory, ARGS = the workload's bench
arguments; run from a scratch directory).  The counter passes run on their own, never combined with tracing:
  B="python $R/bench.py --full --steps 3 --warmup 1 --no-cpu $ARGS"
  timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o run -- $B > $O/stats.log 2>&1
  timeout 400 rocprofv3 --pmc FETCH_SIZE GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_c -o run -- $B > $O/pmc_c.log 2>&1
  timeout 400 rocprofv3 --pmc WRITE_SIZE SQ_INSTS_VALU SQ_INSTS_SALU --output-format csv -d $O/pmc_d -o run -- $B > $O/pmc_d.log 2>&1
  timeout 60 python $R/tools/pmc_summary.py $O/pmc_c > $O/pmc_c.txt
  timeout 60 python $R/tools/pmc_summary.py $O/pmc_d > $O/pmc_d.txt
  timeout 60 python $R/tools/make_traffic.py <key> <entries> $O/pmc_c.txt $O/pmc_d.txt <label>
<entries> is the "<n> table entries" of config.workload in the JSON line of $O/stats.log.  Keys and ARGS on file: k31 (none),
k31_repeats (--workload repeats), k51 (--k 51 --genome 5e8), k31_octoploid (--workload octoploid), k51_hexaploid
(--workload hexaploid); the labels name the summaries as profiles/r06_pmc_<workload>.txt."""
import collections, hashlib, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
key, n, fc, fw, label = sys.argv[1], int(float(sys.argv[2])), sys.argv[3], sys.argv[4], sys.argv[5]
out = sys.argv[6] if len(sys.argv) > 6 else os.path.join(ROOT, "profiles", "hbm_traffic.json")


def read(path, counter):
    res, cur = {}, None
    for line in open(path):
        if not line.startswith(" "):
            cur = line.strip()
        else:
            m = re.match(r"\s+(\S+)\s+mean=\s*([0-9.]+)", line)
            if m and m.group(1) == counter and cur:
                res[cur] = float(m.group(2))
    return res


f, w = read(fc, "FETCH_SIZE"), read(fw, "WRITE_SIZE")
kern = {}
for k in sorted(set(f) | set(w)):
    kern[k] = round((2 * f.get(k, 0.0) + w.get(k, 0.0)) * 1024 / n, 3)
p1 = sum(v for k, v in kern.items() if k.startswith(("kf_pass1", "kf_collect", "kf_bigfix")))
p2 = sum(v for k, v in kern.items() if k.startswith("kf_pass2"))
sys.path.insert(0, ROOT)
from smudgeplot_amd import codeobj
h = codeobj.code_object_hash()
doc = json.load(open(out)) if os.path.exists(out) else {}
doc[key] = {"source": f"rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, {label}: (2 x FETCH_SIZE + WRITE_SIZE) KiB / {n} entries "
                      "(the counters are in KiB and FETCH_SIZE reports 1/2 on gfx950: profiles/r01_calibration_fetch_size.txt); "
                      "ms_pass1 = kf_pass1* + kf_collect + kf_bigfix (the launches inside the pass-1 event bracket); ms_pass2 = kf_pass2 + kf_pass2_far",
            "code_object_sha256_16": h,
            "bytes_per_entry": {"ms_pass1": round(p1, 3), "ms_pass2": round(p2, 3)},
            "kernels": {k: v for k, v in kern.items() if v >= 0.001}}
json.dump(doc, open(out, "w"), indent=1)
print(key, "pass1 %.3f pass2 %.3f B/entry" % (p1, p2), "lib", h)
