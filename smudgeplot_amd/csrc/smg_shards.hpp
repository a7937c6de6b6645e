// smg_shards.hpp -- what the shard drivers (smg_multi.hpp) and the one-shot entries (smg_hetmers.hip) share: who owns an
// engine, where a table is cut, the pieces of a sharded run that every driver needs, and the choice of the run mode.
// Host code only; included behind smg_ingest.hpp (uses the engine's internals).

#pragma once

#define SMG_MAXGPU 16
#define SMG_ONE_SHARD_MAX (0xFFFFFFF0ll - 16)          // a shard addresses its entries with 32 bits

// An engine for the length of a scope.  Declare it BEFORE the buffers of that scope: it is destroyed after them.
struct EngineOwner
{ smg_engine *e = NULL;
  EngineOwner() = default;
  EngineOwner(const EngineOwner &) = delete;
  EngineOwner &operator=(const EngineOwner &) = delete;
  ~EngineOwner() { if (e) smg_engine_destroy(e); }
  smg_engine *create(int device, char *errbuf, size_t errlen) { return e = smg_engine_create(device, NULL, errbuf, errlen); }
};

// ---- where a table is cut -------------------------------------------------------------------------------------------------

// cut points: about n*r/N, moved to a prefix-index boundary that is also a window-block boundary
static void multi_cuts(const smg_table_source *tv, int n, int64_t *cut)
{ const int64_t ixlen = 1ll << (8 * tv->ibyte);
  const int p0 = tv->kmer / 2, ib = 4 * tv->ibyte;          // bases in a window-block prefix / in an index bucket
  // an index bucket fixes the first `ib` bases; a window block the first `p0`: when ib > p0 only every
  // 4^(ib-p0)-th bucket boundary is also a block boundary
  const int64_t gran = ib > p0 ? 1ll << (2 * (ib - p0)) : 1;
  cut[0] = 0; cut[n] = tv->nels;
  for (int r = 1; r < n; r++)
    { const int64_t target = tv->nels / n * r;
      int64_t lo = 0, hi = ixlen - 1;                         // smallest bucket b with index[b] >= target
      while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (tv->prefix_index[m] < target) lo = m + 1; else hi = m; }
      int64_t b = lo + 1;                                      // the cut goes in front of bucket b
      b = (b + gran / 2) / gran * gran;
      if (b >= ixlen) b = ixlen;
      int64_t cpos = b == 0 ? 0 : tv->prefix_index[b - 1];
      if (cpos < cut[r - 1]) cpos = cut[r - 1];
      cut[r] = cpos;
    }
}

// out[(s - 1) * W ..] = the first k-mer shard s of a table cut at cut[] can hold: the prefix bucket its piece starts with
// (cuts are bucket boundaries, everything in front is smaller); all ones for a shard behind the last bucket
static void index_splitters(const smg_table_source *tv, const int64_t *cut, int n, int W, u64 *out)
{ const int64_t ixlen = 1ll << (8 * tv->ibyte);
  for (int sh = 1; sh < n; sh++)
    { int64_t lo = 0, hi = ixlen;                            // smallest bucket b with index[b] > cut[sh]
      while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (tv->prefix_index[m] > cut[sh]) hi = m; else lo = m + 1; }
      u64 *s = out + (size_t) (sh - 1) * W;
      for (int w = 0; w < W; w++) s[w] = lo >= ixlen ? ~0ull : 0;
      if (lo < ixlen) s[0] = (u64) lo << (64 - 8 * tv->ibyte);
    }
}

// hist[0 .. nbin) entries and hist[nbin .. 2 nbin) complements per leading `bits` bits, summed over the whole input: shard s of
// the CLOSED table starts at the first bin at which that table has reached s / n of its entries -> out[(s - 1) * W ..], all ones
// for the shards that nothing is left for.  Returns the size of the closed table.
static int64_t balanced_splitters(const int64_t *hist, int nbin, int bits, int n, int W, u64 *out)
{ int64_t total = 0, acc = 0;
  int next = 1;
  for (int b = 0; b < 2 * nbin; b++) total += hist[b];
  for (int i = 0; i < (n - 1) * W; i++) out[i] = 0;
  for (int b = 0; b < nbin && next < n; b++)
    { while (next < n && acc >= total / n * next) { out[(size_t) (next - 1) * W] = (u64) b << (64 - bits); next++; }
      acc += hist[b] + hist[nbin + b];
    }
  for (; next < n; next++) for (int w = 0; w < W; w++) out[(size_t) (next - 1) * W + w] = ~0ull;
  return total;
}

// (symm_split_bits, the bits of the leading k-mer prefix that the closed table is cut on: smg_condition.hpp)

// ---- the pieces of a sharded run ------------------------------------------------------------------------------------------

// the engine's own table for the entries [lo, hi) of the input, and their records into it: read piece by piece, copied, every
// piece decoded behind its copy (entry lo of the table = entry 0 of the engine's).  d_index: the table's prefix index on the
// device; wait_event: what the copies wait for first (the upload of that index, where it is still in flight).
static int ingest_range(smg_engine *e, const smg_table_source *tv, int64_t lo, int64_t hi, const int64_t *d_index, int device,
                        int threads, double *h2d_s, hipEvent_t wait_event, char *errbuf, size_t errlen)
{ const int rc = decode_begin(e, tv->kmer, tv->ibyte, hi - lo, errbuf, errlen);
  if (rc) return rc;
  const int pbyte = ((tv->kmer + 3) >> 2) + 2 - tv->ibyte;
  DecodeHook hk; hk.e = e; hk.d_index = d_index; hk.ibyte = tv->ibyte; hk.ibase = lo;
  return ingest_records(tv, pbyte, lo, hi, NULL, device, threads, h2d_s, errbuf, errlen, decode_hook, &hk, wait_event);
}

// the table's prefix index on the device (a blocking copy)
static int upload_index(const smg_table_source *tv, DevBuf<int64_t> &d_index, const char *what, char *errbuf, size_t errlen)
{ const size_t ixbytes = sizeof(int64_t) << (8 * tv->ibyte);
  if (d_index.alloc(ixbytes) != hipSuccess) return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory for %s", what);
  if (hipMemcpy(d_index, tv->prefix_index, ixbytes, hipMemcpyHostToDevice) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENODEV, "host to device copy failed%s");
  return SMG_OK;
}

// records: what shard dst receives of the `rw`-word records that every shard src grouped by destination in send[src]
// (counts[src][0 .. n), destination-major), one shard's after the other's
static int64_t received_total(const int64_t *const counts[], int n, int dst)
{ int64_t t = 0;
  for (int s = 0; s < n; s++) t += counts[s][dst];
  return t;
}

static bool gather_received(const int64_t *const counts[], int n, int dst, const uint64_t *const send[], int rw, uint64_t *recv)
{ int64_t roff = 0;
  for (int s = 0; s < n; s++)
    { int64_t soff = 0;
      for (int d = 0; d < dst; d++) soff += counts[s][d];
      const int64_t cnt = counts[s][dst];
      if (cnt && hipMemcpy(recv + roff * rw, send[s] + soff * rw, sizeof(uint64_t) * (size_t) cnt * rw, hipMemcpyDeviceToDevice) != hipSuccess)
        return false;
      roff += cnt;
    }
  return true;
}

// the table is closed under reverse complement with equal counts: no look-up missed, and under the hash proof the
// fingerprints of the entries and of their complements (XOR over the shards) agree
static bool proof_holds(int symcheck, int64_t missing, const u64 fp[4])
{ return missing == 0 && (symcheck != SMG_SYM_HASH || (fp[0] == fp[2] && fp[1] == fp[3])); }

// as everywhere: the number of records of the extract leg is the plot's weight on the labelled pixels (path 1 counts a
// mirrored pair twice and writes it twice, path 2 counts and writes every pair once)
static int64_t pair_weight(const uint16_t *labels, const int64_t *plot)
{ int64_t w = 0;
  for (int cell = 0; cell < SMG_PLOT_CELLS; cell++) if (labels[cell]) w += plot[cell];
  return w;
}

static int upload_labels(const uint16_t *labels, DevBuf<uint16_t> &d_labels, char *errbuf, size_t errlen)
{ if (d_labels.alloc(sizeof(uint16_t) * SMG_PLOT_CELLS) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory for the pair list%s");
  if (hipMemcpy(d_labels, labels, sizeof(uint16_t) * SMG_PLOT_CELLS, hipMemcpyHostToDevice) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENODEV, "host to device copy failed%s");
  return SMG_OK;
}

// the extract leg of the engine's completed run, appended to `out` (records of W + 1 words).  known >= 0: the number of
// records there must be (pair_weight) -- one launch; known < 0: counted first, then listed.  set: engine_extract's d_set.
static int extract_to_host(smg_engine *e, const uint16_t *d_labels, const TabSet *set, int64_t known, std::vector<uint64_t> &out,
                           char *errbuf, size_t errlen)
{ int rc;
  int64_t cnt = known, got = 0;
  if (known < 0 && (rc = engine_extract(e, d_labels, NULL, 0, &cnt, set, errbuf, errlen))) return rc;
  if (known < 0 && cnt == 0) return SMG_OK;
  const size_t at = out.size(), words = (size_t) cnt * (e->tab.W + 1);
  DevBuf<uint64_t> d_out;
  if (d_out.alloc(sizeof(uint64_t) * words) != hipSuccess) return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory for the pair list%s");
  if ((rc = engine_extract(e, d_labels, d_out, cnt, &got, set, errbuf, errlen))) return rc;
  if (got != cnt)
    return fail(errbuf, errlen, SMG_ENODEV, known < 0 ? "internal error: the pair list changed between two passes%s"
                                                      : "internal error: pair list and plot disagree%s");
  out.resize(at + words);
  if (words && hipMemcpy(out.data() + at, d_out, sizeof(uint64_t) * words, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENODEV, "device to host copy failed%s");
  return SMG_OK;
}

// the records of a run to the caller of the C ABI (smg_free releases them), after the check that every driver makes
static int records_to_caller(const std::vector<uint64_t> &rec, int rw, const uint16_t *labels, const int64_t *plot,
                             uint64_t **records, int64_t *nrec, int *rec_words, char *errbuf, size_t errlen)
{ const int64_t have = (int64_t) (rec.size() / (size_t) rw);
  if (have != pair_weight(labels, plot)) return fail(errbuf, errlen, SMG_ENODEV, "internal error: pair list and plot disagree%s");
  uint64_t *all = (uint64_t *) malloc(sizeof(uint64_t) * (rec.size() ? rec.size() : 1));
  if (!all) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory for the pair list%s");
  if (!rec.empty()) memcpy(all, rec.data(), sizeof(uint64_t) * rec.size());
  *records = all; *nrec = have; *rec_words = rw;
  return SMG_OK;
}

// ---- the run mode -----------------------------------------------------------------------------------------------------------

// What a run in core takes per entry, in bytes: k-mers 8 W, count 2, code byte 1, deferred-entry map and lists 0.6, the
// request list (a quarter of the entries + slack) and its partitioned copy ~2.6 W.  Conditioning a table takes more than
// running it: its records (2 (W + 1) words per entry of the piece), the sort's copies and scratch.
struct EntryPrice { double run, cond; };
static EntryPrice entry_price(int W, int condition)
{ EntryPrice p;
  p.run = 10.6 * W + 5.5;
  p.cond = condition ? ((condition & SMG_COND_SYMM) ? 24.0 * W + 30.0 : 8.0 * W + 12.0) : 0.0;
  return p;
}

// bytes of device memory that `nels` entries take in core, the candidate map (1 GiB at most) included.  A table that is to be
// symmetrised counts with the size of the CLOSED table: at most twice the entries.
static double core_bytes(int W, int64_t nels, int condition)
{ const EntryPrice p = entry_price(W, condition);
  const double ne = (double) nels * ((condition & SMG_COND_SYMM) ? 2.0 : 1.0);
  return ne * (p.run > p.cond ? p.run : p.cond) + 1.1e9;
}

// the device memory a run may plan with: SMG_HBM_LIMIT=<bytes> (tests) as it is, else nine tenths of `free_bytes`, else
// (free_bytes <= 0) of what `device` reports free.  0: unknown.
static double memory_limit(int device, double free_bytes)
{ const char *hl = getenv("SMG_HBM_LIMIT");
  if (hl && atof(hl) > 0) return atof(hl);
  if (free_bytes > 0) return 0.9 * free_bytes;
  size_t fr = 0, tot = 0;
  if (hipSetDevice(device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess) return 0.9 * (double) fr;
  return 0;
}

struct RunMode
{ int mode = SMG_MODE_CORE;     // SMG_MODE_*
  int count = 1;                // shards or GPUs that run
  int cut_by_limit = 0;         // > 0: the table was cut into this many prefix shards because of its size alone
};

// Which path a table takes: a pure function of (k, entries, options, the five hooks, free bytes), and the only reader of
// SMG_VIRTUAL_SHARDS, SMG_SHARD_LIMIT, SMG_SEQUENTIAL_SHARDS, SMG_HBM_LIMIT (memory_limit) and SMG_FORCE_MULTI.
//   * SMG_VIRTUAL_SHARDS=N (tests): N shards on ONE device, the 1-GPU stand-in of several GPUs.
//   * A shard addresses its entries with 32 bits.  A table beyond that is cut into prefix shards of ~3e9 entries that all
//     live on this one device (288 GB of HBM hold ~1.5e10 k=31 entries with their side arrays) -- the same code path as
//     several GPUs, with device-to-device copies for the exchange: the reference streams a table of any size
//     (PloidyPlot.c:931-1038), this engine must not refuse one just because of an index width.  SMG_SHARD_LIMIT (tests) lowers
//     the threshold.  A table that still has to be symmetrised closes to at most twice its entries: it is cut for that size.
//   * Out of core (host_run_sequential): a table whose shards do not fit the device TOGETHER is run shard after shard, the
//     table read twice.  What stays between the two rounds is a code byte per entry and the requests -- every entry's (W + 1
//     words) under the exact proof, those of the owners of a pair at p > k-1-p otherwise (17 % of a diploid table, 36 % of a
//     polyploid one; k > 85: records carry a count word) -- and there is no candidate map.  Several real GPUs are not
//     checked: each holds its shard.  SMG_SEQUENTIAL_SHARDS=<n> forces the mode, SMG_HBM_LIMIT stands in for the memory.
//   * SMG_FORCE_MULTI=1 (tests): the multi-GPU code path with one GPU -- a one-rank RCCL communicator, send/recv to self,
//     all-reduce: checks the dlopen'ed RCCL entry points on a 1-GPU box.
static int run_mode_plan(int kmer, int64_t nels, int ngpus, int condition, int symcheck, int device, double free_bytes, RunMode *out,
                         char *errbuf, size_t errlen)
{ RunMode m;
  const int W = (kmer + 31) / 32;
  const bool want_symm = (condition & SMG_COND_SYMM) != 0;
  const char *v = getenv("SMG_VIRTUAL_SHARDS");
  int ng = ngpus;
  bool virt = false;
  if (v && atoi(v) > 1) { ng = atoi(v); virt = true; }
  int64_t limit = SMG_ONE_SHARD_MAX;
  { const char *sl = getenv("SMG_SHARD_LIMIT"); if (sl && atoll(sl) > 0) limit = atoll(sl); }
  const int64_t closed = want_symm ? 2 * nels : nels;
  if (ng <= 1 && closed >= limit)
    { const int64_t per = limit > 3000000000ll ? 3000000000ll : limit;     // ~3e9 entries per shard
      ng = (int) ((closed + per - 1) / per);
      if (ng < 2) ng = 2;
      if (ng > SMG_MAXGPU)
        return fail(errbuf, errlen, SMG_EINVAL, "table too large for one GPU (more than 16 shards of 3e9 entries): use SMUDGEPLOT_GPUS%s");
      virt = true;
      m.cut_by_limit = ng;
    }
  int seq = 0;
  if (ng <= 1 || virt)
    { const char *sv = getenv("SMG_SEQUENTIAL_SHARDS");
      if (sv && atoi(sv) > 1) seq = atoi(sv) > SMG_MAXGPU ? SMG_MAXGPU : atoi(sv);     // (the router groups by at most 16 destinations)
      const double mem = seq ? 0 : memory_limit(device, free_bytes);
      if (mem > 0 && core_bytes(W, nels, condition) > mem)
        { const EntryPrice p = entry_price(W, condition);
          const double ne = (double) nels * (want_symm ? 2.0 : 1.0);
          const double keep = ne * (1.0 + (symcheck == SMG_SYM_EXACT ? 8.0 * (W + 1) : 0.36 * 8.0 * (kmer > FAST_MAX_K ? W + 1 : W)));
          for (int q = 2; q <= SMG_MAXGPU && !seq; q++)
            if (keep + ne / q * p.run <= mem && ne / q * p.cond <= mem && ne / q < SMG_ONE_SHARD_MAX) seq = q;
          if (!seq)
            { *out = m;
              return fail(errbuf, errlen, SMG_ENOMEM, "the table does not fit the device even shard by shard (16 shards, a code byte and "
                          "the requests of every entry resident): use SMUDGEPLOT_GPUS%s");
            }
        }
    }
  if (seq) { m.mode = SMG_MODE_SEQUENTIAL; m.count = seq; }
  else if (ng > 1)
    { // (SMG_VIRTUAL_SHARDS=1 beside several GPUs: their shards on one device)
      m.mode = virt || (v && atoi(v) > 0) ? SMG_MODE_VIRTUAL : SMG_MODE_MULTI;
      m.count = ng > SMG_MAXGPU ? SMG_MAXGPU : ng;
    }
  else if (getenv("SMG_FORCE_MULTI") && !v) m.mode = SMG_MODE_ONE_RANK_FORCED;
  *out = m;
  return SMG_OK;
}

extern "C" int smg_hetmers_run_mode(int kmer, int64_t nels, const smg_opts *opts, double free_bytes, int32_t out[3],
                                    char *errbuf, size_t errlen)
{ if (!out || kmer < 1 || kmer > SMG_MAX_KMER || nels < 0) return fail(errbuf, errlen, SMG_EINVAL, "bad argument%s");
  RunMode m;
  const int rc = run_mode_plan(kmer, nels, opts ? opts->ngpus : 0, opts ? opts->condition : 0, opts ? opts->symcheck : SMG_SYM_EXACT,
                               opts ? opts->device : 0, free_bytes, &m, errbuf, errlen);
  out[0] = m.mode; out[1] = m.count; out[2] = m.cut_by_limit;
  return rc;
}

// ---- the run mode of a table that is ALREADY ON THE DEVICE (smg_hetmers_run_device) -------------------------------------------

// What the range closure of one shard (close_canonical_range, smg_condition.hpp) allocates per entry of the SHARD, in bytes,
// at its worst -- every entry of the shard a complement, none from the slice.  While the complements are sorted: the selected
// k-mers and counts (8 W + 2), sort_permutation's two word and two permutation buffers (2 * 8 + 2 * 4).  While they are
// merged: the selected k-mers and counts again, the permutation (4), the shard itself (8 W + 2).
static double closure_price(int W)
{ const double sorting = 8.0 * W + 2.0 + 24.0, merging = 2.0 * (8.0 * W + 2.0) + 4.0;
  return sorting > merging ? sorting : merging;
}

// what a run of the table in core needs FREE: the table handed in is in device memory already and not part of what is free
static double device_core_need(int W, int64_t nels, int condition)
{ return core_bytes(W, nels, condition) - (condition ? 0.0 : (double) nels * (8.0 * W + 2.0)); }

// what stays on the device for the whole of a run in shards: the trimmed copy of the table where trimming is asked for, a code
// byte per closed entry and the requests (run_mode_plan's `keep`)
static double device_resident_bytes(int kmer, int64_t nels, int condition, int symcheck)
{ const int W = (kmer + 31) / 32;
  const double ne = 2.0 * (double) nels;
  const double keep = ne * (1.0 + (symcheck == SMG_SYM_EXACT ? 8.0 * (W + 1) : 0.36 * 8.0 * (kmer > FAST_MAX_K ? W + 1 : W)));
  return ((condition & SMG_COND_TRIM) ? (double) nels * (8.0 * W + 2.0) : 0.0) + keep;
}

static const char *DEVICE_TWO_STEP = ": write the table (smg_count without -e) and run hetmers on it, which runs out of core";

// SMG_DEVICE_SHARD_LIMIT=<entries> (tests) stands in for SMG_ONE_SHARD_MAX
static int64_t device_shard_limit(bool hooks)
{ const char *sl = hooks ? getenv("SMG_DEVICE_SHARD_LIMIT") : NULL;
  return sl && atoll(sl) > 0 ? atoll(sl) : SMG_ONE_SHARD_MAX;
}

// Which way a table on the device runs: a pure function of (k, entries, options, two hooks and SMG_HBM_LIMIT, free bytes).
//   * In core wherever the closed table is addressed by one engine and fits next to the lists of its run or the buffers of
//     its closure: the two tests this entry has always made, with their arithmetic.
//   * Elsewhere a table that is to be closed (SMG_COND_SYMM) runs in the smallest number q = 2 .. 16 of prefix shards of its
//     CLOSED table, one after the other (SeqRun, smg_multi.hpp), such that 2 n / q is below the shard limit and the resident
//     part (device_resident_bytes) plus one shard -- the larger of its closure and its run -- fits the memory.
//   * SMG_DEVICE_SHARDS=<2..16> (tests) forces that many shards, SMG_DEVICE_SHARD_LIMIT=<entries> (tests) lowers the limit.
//     hooks = false: neither is read (a table that turns out not to be canonical: the generic closure runs in core or not at all).
//   The hooks of run_mode_plan are not read here.
static int run_device_plan(int kmer, int64_t nels, int ngpus, int condition, int symcheck, int device, double free_bytes, bool hooks,
                           RunMode *out, char *errbuf, size_t errlen)
{ RunMode m;
  *out = m;
  const int W = (kmer + 31) / 32;
  const bool want_symm = (condition & SMG_COND_SYMM) != 0;
  if (ngpus > 1)
    return fail(errbuf, errlen, SMG_EINVAL, "a table that is already on one device runs on that device only (ngpus > 1)%s");
  const double ne = (double) nels * (want_symm ? 2.0 : 1.0);
  const int64_t limit = device_shard_limit(hooks);
  const bool by_size = ne >= (double) limit;
  int forced = 0;
  { const char *fs = hooks ? getenv("SMG_DEVICE_SHARDS") : NULL;
    if (fs && atoi(fs) >= 2) forced = atoi(fs) > SMG_MAXGPU ? SMG_MAXGPU : atoi(fs);
  }
  if (nels >= SMG_ONE_SHARD_MAX || (by_size && !want_symm))
    return fail(errbuf, errlen, SMG_ENOMEM, "more than 2^32 - 32 entries in the closed table: one engine does not address them%s", DEVICE_TWO_STEP);
  const double mem = memory_limit(device, free_bytes);
  if (mem <= 0) return fail(errbuf, errlen, SMG_ENODEV, "no usable HIP device%s");
  const double need = device_core_need(W, nels, condition);
  const bool by_mem = need > mem;
  if (!by_size && !by_mem && !(forced && want_symm)) return SMG_OK;             // in core, as ever
  int q = 0;
  if (want_symm && forced) q = forced;
  else if (want_symm)
    { const double resident = device_resident_bytes(kmer, nels, condition, symcheck);
      const EntryPrice p = entry_price(W, condition);
      const double shard = closure_price(W) > p.run ? closure_price(W) : p.run;
      for (int c = 2; c <= SMG_MAXGPU && !q; c++)
        if (ne / c < (double) limit && resident + ne / c * shard <= mem) q = c;
    }
  if (!q)
    { char msg[320];
      snprintf(msg, sizeof(msg), "the table does not fit the device in core: %lld entries need %.3f GB, %.3f GB are free%s",
               (long long) nels, need * 1e-9, mem * 1e-9, want_symm ? ", and 16 prefix shards one after the other do not fit either" : "");
      if (errbuf && errlen) snprintf(errbuf, errlen, "%s%s", msg, DEVICE_TWO_STEP);
      return SMG_ENOMEM;
    }
  m.mode = SMG_MODE_SEQUENTIAL; m.count = q; m.cut_by_limit = by_size ? q : 0;
  *out = m;
  return SMG_OK;
}

extern "C" int smg_hetmers_run_device_mode(int kmer, int64_t nels, const smg_opts *opts, double free_bytes, int32_t out[3],
                                           char *errbuf, size_t errlen)
{ if (!out || kmer < 1 || kmer > SMG_MAX_KMER || nels < 0) return fail(errbuf, errlen, SMG_EINVAL, "bad argument%s");
  RunMode m;
  const int rc = run_device_plan(kmer, nels, opts ? opts->ngpus : 0, opts ? opts->condition : 0, opts ? opts->symcheck : SMG_SYM_HASH,
                                 opts ? opts->device : 0, free_bytes, true, &m, errbuf, errlen);
  out[0] = m.mode; out[1] = m.count; out[2] = m.cut_by_limit;
  return rc;
}
