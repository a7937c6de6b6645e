// smg_fast_lookup.hpp -- the fast path (k <= 85) between pass 1 and pass 2: what becomes of the request list.  First the PLANS:
// pure functions of k, the record, the counts pass 1 reported, the device's compute units and the test hooks -- no engine, no
// device (smg_engine_lookup_plan hands them to the tests) -- which say whether the list is bucketed or partitioned in front of
// the filter (presort_plan), the filter's grid and the chunks of the kept list (filter_plan), the probe kernel of the look-up
// chain with its tickets (probe_plan), and the route of the look-ups with its kernel (apply_plan).  Then the LAUNCHES, which
// reserve, launch and read back what their plan says: filter_presort, lookup_probe, fast_filter, compact_chunks, apply_sorted,
// apply_indexed, fast_apply.  Part of the one translation unit smg_hetmers.hip, included behind smg_fast_host.hpp.

// key-only records of one-word k-mers: radix sort on the leading 32 bits, then look up in order.
// rocPRIM's mid-size (merge sort) variant returned garbage with a partial bit range on gfx950 /
// ROCm 7.2, so Onesweep is forced (MergeSortLimit = 0) and small batches are not sorted at all
// (their look-ups are too few to matter).  SMG_VERIFY_SORT=1 checks every sort (order + checksums).
#define SORT_MIN 4096
#define APPLY_SORT_MIN  (1 << 21)     // apply_plan: key-only lists of one-word k-mers are sorted from here on (SMG_APPLY_SORT_MIN)
#define FILTER_SORT_MIN (1 << 22)     // presort_plan: chunk slots from which a key-only list is bucketed first (SMG_FILTER_SORT_MIN)
typedef rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                   rocprim::default_config, 0> smg_sort_config;

// ---- the plans ----------------------------------------------------------------------------------------------------------

// a list length from which something is sorted: the hook's value or dflt, never below SORT_MIN
static int64_t sort_min(const char *hook, int64_t dflt)
{ const int64_t v = hook_int(hook, HOOK_ANY, dflt);
  return v < SORT_MIN ? SORT_MIN : v;
}

// First half of the request filter, which does not need the map (a sharded run overlaps it with the exchange of the block maps).
// The look-up chain (nb bucket bits) partitions the list into its buckets.  Without it long key-only lists of one-word k-mers
// are bucketed on their leading 8 bits: the probes of the 128 MB map are random 64-byte fetches otherwise (7 ms for the 4.4e8
// requests of the 1 Gbp table); one radix pass (holes of the chunk array as sentinels, as for the look-ups -- hence k < 32)
// keeps the map words that the resident workgroups probe inside the L2s.  Below FILTER_SORT_MIN the probes are too few to matter.
static Presort presort_plan(int kmer, int rw, int nb, unsigned n_chunks)
{ if (nb) return PRESORT_CHAIN;
  const int64_t nslots = (int64_t) n_chunks * F_CH;
  return rw == 1 && nslots >= sort_min("SMG_FILTER_SORT_MIN", FILTER_SORT_MIN) && kmer < 32 ? PRESORT_BUCKETED : PRESORT_ASIS;
}

// The filter of n_chunks chunks holding nrequests records: workgroups of kf_filter, chunks of the kept list (what the kernel may
// fill; RequestLists::reserve makes room for them).  seen_chunks >= 0: a replayed step, whose filter gets as many chunks as the
// recorded step's filled, and some -- the device checks that this step stayed inside.
struct FilterPlan { unsigned grid, maxout; };
static FilterPlan filter_plan(int cus, unsigned n_chunks, int64_t nrequests, bool chain, int64_t seen_chunks)
{ FilterPlan f;
  // two workgroups per CU, chunks dealt round-robin: the chunks in flight then span one or two of the 256 sorted
  // buckets, i.e. <= 1 MB of the map (measured: 512 workgroups 3.0 ms, 256 / 1024 / 2048 workgroups 3.4-3.7 ms)
  f.grid = 2u * (unsigned) cus;
  if (f.grid > n_chunks) f.grid = n_chunks;
  f.grid = hook_grid("SMG_FILTER_GRID", f.grid);
  f.maxout = n_chunks + f.grid + 16;
  if (chain)
    { // kl_probe: every wave of every workgroup (one per CU, probe_plan) fills chunks of its own, each to the brim
      // but for the < 64 records that did not fit: size the list from the launch and the request count, not from 256 CUs
      const int64_t need = (int64_t) cus * PB_WAVES + nrequests / (F_CH - 63) + 16;
      f.maxout = need < 0x7FFFFFFFll ? (unsigned) need : 0x7FFFFFFFu;
      if (f.maxout < n_chunks + 16) f.maxout = n_chunks + 16;
    }
  if (seen_chunks >= 0 && seen_chunks + 64 < (int64_t) f.maxout) f.maxout = (unsigned) (seen_chunks + 64);
  return f;
}

// The probe of the look-up chain against the map; list: the survivors go to the kept list, else they are looked up at once.
// The fused probe + look-up of a single shard has two forms.  kl_probe (a bucket per workgroup, the bucket's map folded
// into LDS) is the faster one on a table without long window blocks: 2.5 against 2.7 ms at 2.5e9 entries.  kl_probe_x
// (XCD by XCD straight from the full-resolution map, small independent workgroups) does not care how long a look-up
// takes: with 5 % repeats in the genome the survivors' look-ups bisect directory buckets of thousands of k-mers, the
// sixteen waves of a kl_probe workgroup wait for each other at every bucket, and it takes 4.5 ms against 2.9.  The
// share of deferred entries that pass 1 reported tells the two kinds of table apart (0.13 % / 0.39 % in the two
// bench workloads); SMG_PROBE_X=0/1 overrides.
struct ProbePlan
{ ProbeForm form;
  unsigned  part;             // kl_probe_x: requests per ticket, bit 31: every workgroup claims XCD 0 (SMG_PX_ONE_XCC); else 0
  unsigned  grid;
};
static ProbePlan probe_plan(bool list, int nb, bool one_way, int64_t nbig, int64_t nemitted, int64_t n, int cus)
{ ProbePlan p;
  // ... and so does the share of entries that sent a request: 17.5 % on the diploid tables, a third on the polyploid ones, where
  // one request in seven survives the filter (2.5e7 look-ups at 6.4e8 entries) and kl_probe_x is 7-8 % ahead as well
  // (a one-way run sends one request per complement class: half the share says the same about the table)
  const int64_t share = one_way ? 14 : 28;
  const bool many = nemitted * 100 > n * share;
  const bool auto_x = (nbig > 0 && nbig * 400 > n) || many;
  if (!list && nb >= 3 && hook_int("SMG_PROBE_X", HOOK_ANY, auto_x) != 0)
    { // tickets of 2048 requests where many requests survive (polyploid tables: one in seven, all real hits -- half as many
      // buckets in flight per XCD keep more of a bucket's k-mer lines in reach: -0.25 ms on the hexaploid table), 4096 where the
      // kernel is mostly streaming (a table with repeats: 1 request in 50 survives, and a ticket's fixed cost shows: +0.5 ms at 2048)
      p.form = PROBE_X;
      p.part = many ? PX_PART : 2 * PX_PART;
      if (test_hook("SMG_PX_ONE_XCC")) p.part |= 0x80000000u;                      // (tests: every workgroup claims XCD 0)
      p.grid = (unsigned) cus * PX_WGS;
      return p;
    }
  p.form = list ? PROBE_LIST : PROBE_FUSED;
  p.part = 0;
  p.grid = (unsigned) cus;                                                         // (one workgroup per CU, a bucket each)
  if (p.grid > 1u << nb) p.grid = 1u << nb;
  return p;
}

// The look-ups of a list of nrec records: this engine's own n_chunks chunks (flat = false) or a flat array of received records.
//   ROUTE_FUSED      own requests, own map, the look-up chain: partition, then filter and look-ups in one kernel (no survivor
//                    list, no sort)
//   filter_first     own requests and a map they were not filtered by yet: fast_filter, then ask again
//   ROUTE_SENTINELS  key-only records of one-word k-mers where nearly every chunk is full (pass 1 and the filter split their
//                    batches): the chunk array is sorted as it is, holes as sentinels behind the requests
//   ROUTE_COMPACTED  ragged chunks, k = 32 (the all-T k-mer equals the sentinel) or records with a count/flag word (W > 1, exact
//                    proof): compacted first
//   ROUTE_FLAT       a flat array
// and the kernel behind it: key-only records of one-word k-mers go through kf_apply_sorted, radix sorted from APPLY_SORT_MIN
// records on (a short list -- what one rank of eight receives -- is looked up as it comes: the sort is eight launches, ~90 us, to
// put a few hundred thousand look-ups in order, which take 70 us either way); every other record through kf_apply_indexed behind
// an index sort, or below SORT_MIN records (and where 32-bit record numbers would not do) through kf_apply as they come.
enum ApplyRoute { ROUTE_NONE = 0, ROUTE_FUSED = 1, ROUTE_SENTINELS = 2, ROUTE_COMPACTED = 3, ROUTE_FLAT = 4 };
struct ApplyPlan
{ ApplyRoute  route;
  bool        filter_first;
  ApplyKernel kernel;
  bool        sorted, verify;   // radix sorted first; ... and every sort checked (SMG_VERIFY_SORT=1)
  ApplyHoles  holes;
  int64_t     covered;        // records (flat and compacted lists) or chunk slots (sentinels) the look-up kernel walks
};
static ApplyPlan apply_plan(bool flat, int kmer, int rw, unsigned n_chunks, int64_t nrec, bool filtered, int bm_bits, int nb)
{ ApplyPlan p = {};
  const int W = (kmer + 31) / 32;
  const bool keys_only = W == 1 && rw == 1, own_map = !flat && bm_bits && !filtered;
  if (own_map && nb) { p.route = ROUTE_FUSED; return p; }
  if (own_map) { p.filter_first = true; return p; }
  if (nrec <= 0 || (!flat && n_chunks == 0)) return p;
  const int64_t nslots = (int64_t) n_chunks * F_CH;
  if (flat) p.route = ROUTE_FLAT;
  else p.route = keys_only && nslots <= nrec + nrec / 8 && nslots >= SORT_MIN && kmer < 32 ? ROUTE_SENTINELS : ROUTE_COMPACTED;
  p.holes = flat ? HOLES_NONE : p.route == ROUTE_SENTINELS ? HOLES_SENTINELS : HOLES_COMPACTED;
  p.covered = p.route == ROUTE_SENTINELS ? nslots : nrec;
  p.verify = test_hook("SMG_VERIFY_SORT") != NULL;
  if (keys_only) { p.kernel = APPLY_SORTED; p.sorted = p.covered >= sort_min("SMG_APPLY_SORT_MIN", APPLY_SORT_MIN); }
  else { p.sorted = p.covered >= SORT_MIN && p.covered < 0xFFFFFFF0ll; p.kernel = p.sorted ? APPLY_INDEXED : APPLY_PLAIN; }
  return p;
}

// in[19]: k, words per record, bucket bits of the chain, chunks in use, requests in them, compute units, chunks the recorded
// step's filter filled (-1: no replay), probe to a list, one-way, deferred entries, requests emitted, table entries, flat list,
// records the look-ups see, filtered, id bits of the map, pass 1: records wanted, its grid, chunks already allocated
extern "C" int smg_engine_lookup_plan(const int64_t in[19], int64_t out[14])
{ if (!in || !out) return SMG_EINVAL;
  const int64_t kmer = in[0], rw = in[1], nb = in[2], n_chunks = in[3], nreq = in[4], cus = in[5], seen = in[6], list = in[7], one_way = in[8],
                nbig = in[9], nemitted = in[10], n = in[11], flat = in[12], nrec = in[13], filtered = in[14], bm_bits = in[15],
                want_rec = in[16], grid = in[17], have = in[18];
  if (kmer < 1 || kmer > FAST_MAX_K) return SMG_EINVAL;
  const int W = ((int) kmer + 31) / 32;
  const auto flag = [](int64_t v) { return v == 0 || v == 1; };
  if ((rw != W && rw != W + 1) || (W == 3 && rw != 4) || nb < 0 || nb > L_NB_MAX || (bm_bits != 0 && (bm_bits < 8 || bm_bits > 32))
      || (nb > 0 && (bm_bits < 12 || W > 2 || rw != W)) || n_chunks < 0 || n_chunks > 0x7FFFFFFFll || nreq < 0 || cus < 1 || cus > 65536
      || seen < -1 || seen > 0xFFFFFFFFll || !flag(list) || !flag(one_way) || !flag(flat) || !flag(filtered)
      || (one_way && (rw != W || !(kmer & 1))) || nbig < 0 || nemitted < 0 || n < 0 || n >= 0xFFFFFFF0ll || nrec < 0
      || want_rec < 0 || grid < 1 || grid > P1_MAXGRID || have < 0)
    return SMG_EINVAL;
  const FilterPlan f = filter_plan((int) cus, (unsigned) n_chunks, nreq, nb != 0, seen);
  const ProbePlan pr = probe_plan(list != 0, (int) nb, one_way != 0, nbig, nemitted, n, (int) cus);
  const ApplyPlan ap = apply_plan(flat != 0, (int) kmer, (int) rw, (unsigned) n_chunks, nrec, filtered != 0, (int) bm_bits, (int) nb);
  const int64_t v[14] = { list_capacity(want_rec, (unsigned) grid, nb != 0, have), presort_plan((int) kmer, (int) rw, (int) nb, (unsigned) n_chunks),
                          f.grid, f.maxout, nb ? pr.form : PROBE_NONE, nb ? pr.part & 0x7FFFFFFFu : 0, nb ? pr.part >> 31 : 0, nb ? pr.grid : 0,
                          ap.route, ap.kernel, ap.sorted, ap.holes, ap.covered, ap.filter_first };
  memcpy(out, v, sizeof(v));
  return SMG_OK;
}

// ---- the launches -------------------------------------------------------------------------------------------------------

// look the keys of a plan up, sorted first where it says so (HOLES_SENTINELS: the list contains sentinel words, kf_fill_holes)
static int apply_sorted(smg_engine *e, const u64 *keys_in, const ApplyPlan &p, char *errbuf, size_t errlen)
{ FastArgs a = make_fast(e);
  const int64_t nsort = p.covered;
  const int holes = p.holes == HOLES_SENTINELS;
  int64_t nb = (nsort + F_TPB - 1) / F_TPB;
  if (nb > 16384) nb = 16384;
  const u64 *src = keys_in;
  if (p.sorted)
    { HIPCHK(e->srt.req2.reserve(nsort * (int64_t) sizeof(u64)));
      const unsigned lobit = 40;             // sort on bits [lobit, 64) of the k-mer
      HIPCHK(with_scratch(e->sort_tmp, [&](void *tmp, size_t &bytes)
        { return rocprim::radix_sort_keys<smg_sort_config>(tmp, bytes, (u64 *) keys_in, (u64 *) e->srt.req2, (size_t) nsort, lobit, 64u, e->stream); }));
      src = e->srt.req2;
      if (p.verify)
        { DevBuf<u64> d_chk; u64 h[4];
          HIPCHK(d_chk.alloc(32));
          HIPCHK(hipMemsetAsync(d_chk, 0, 32, e->stream));
          hipLaunchKernelGGL(kf_check_sorted, dim3((unsigned) nb), dim3(F_TPB), 0, e->stream, keys_in, e->srt.req2, nsort, (int) lobit, d_chk);
          HIPCHK(hipMemcpyAsync(h, d_chk, 32, hipMemcpyDeviceToHost, e->stream));
          HIPCHK(hipStreamSynchronize(e->stream));
          if (h[0] || h[1] != h[2] || h[3])
            return fail(errbuf, errlen, SMG_ENODEV, "request sort self-check failed (rocPRIM radix sort)%s");
        }
    }
  hipLaunchKernelGGL(kf_apply_sorted<1>, dim3((unsigned) nb), dim3(F_TPB), 0, e->stream, a, src, nsort, holes, &e->ctrl->fast);
  return SMG_OK;
}

// records with a count/flag word: sort (leading 32 k-mer bits, record number) pairs on the upper 24 bits, look up in
// that order (a plan that does not sort: the batch is looked up as it comes, kf_apply)
static int apply_indexed(smg_engine *e, const u64 *rec, int check_count, const ApplyPlan &p, char *errbuf, size_t errlen)
{ FastArgs a = make_fast(e);
  const int64_t n = p.covered;
  int64_t nb = (n + F_TPB - 1) / F_TPB;
  if (nb > 16384) nb = 16384;
  if (!p.sorted)
    { with_words<3>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_apply<w()>, dim3((unsigned) (nb > 8192 ? 8192 : nb)), dim3(F_TPB), 0, e->stream, a, rec,
          (const uint32_t *) NULL, n, check_count, &e->ctrl->fast, e->run.rw); });
      return SMG_OK;
    }
  for (int q = 0; q < 2; q++)
    { HIPCHK(e->srt.skey[q].reserve(n * 4 + 16));
      HIPCHK(e->srt.sidx[q].reserve(n * 4 + 16));
    }
  hipLaunchKernelGGL(kf_sortkey, dim3((unsigned) nb), dim3(F_TPB), 0, e->stream, rec, e->run.rw, n, e->srt.skey[0], e->srt.sidx[0]);
  uint32_t *const ki = e->srt.skey[0], *const ko = e->srt.skey[1], *const vi = e->srt.sidx[0], *const vo = e->srt.sidx[1];
  HIPCHK(with_scratch(e->sort_tmp, [&](void *tmp, size_t &bytes)
    { return rocprim::radix_sort_pairs<smg_sort_config>(tmp, bytes, ki, ko, vi, vo, (size_t) n, 8u, 32u, e->stream); }));
  with_words<3>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_apply_indexed<w()>, dim3((unsigned) nb), dim3(F_TPB), 0, e->stream, a, rec, e->srt.sidx[1], n,
      check_count, &e->ctrl->fast, e->run.rw); });
  return SMG_OK;
}

// first half of the request filter (presort_plan): the list partitioned for the chain, bucketed, or left as it is
static int filter_presort(smg_engine *e, char *errbuf, size_t errlen)
{ RunState &r = e->run;
  hipEventRecord(e->ev[EV_LOOKUP_BEG], e->stream);                      // start of the filter's time
  r.presorted = presort_plan(e->tab.kmer, r.rw, r.lg.nb, r.n_chunks);
  if (r.presorted == PRESORT_CHAIN)
    { // smg_lookup.hpp: bucket offsets from pass 1's histogram, one-pass partition into the dense array req2
      const int64_t nreq = e->st.nrequests;
      HIPCHK(e->srt.req2.reserve((nreq > 0 ? nreq : 1) * (int64_t) sizeof(u64) * r.rw));
      const int nbk = 1 << r.lg.nb;
      // bucket sizes = column sums of the owners' histogram rows -> bucket offsets -> first slot of every owner in every bucket
      hipLaunchKernelGGL(kl_tot, dim3(L_BK / LW_BPW), dim3(LW_SL * LW_BPW), 0, e->stream, (const unsigned *) e->chain.whist, r.nown, e->chain.ghist);
      hipLaunchKernelGGL(kl_scan, dim3(1), dim3(L_BK), 0, e->stream, e->chain.ghist, nbk, e->chain.boff, e->chain.boff + L_BK + 2, e->chain.ghist + L_BK);
      hipLaunchKernelGGL(kl_woff, dim3(L_BK / LW_BPW), dim3(LW_SL * LW_BPW), 0, e->stream, e->chain.whist, r.nown, (const u64 *) e->chain.boff);
      if (r.n_chunks)
        with_words<2>(r.rw, [&](auto rw) { hipLaunchKernelGGL(kl_part<rw()>, dim3(r.nown), dim3(PT_TPB), 0, e->stream, e->lists.cur.rec, e->lists.cur.fill, r.nown,
            (const unsigned *) e->chain.whist, r.max_chunks, r.lg.nb, e->srt.req2); });
      HIPCHK(hipGetLastError());
    }
  else if (r.presorted == PRESORT_BUCKETED)
    { const int64_t nslots = (int64_t) r.n_chunks * F_CH;
      hipLaunchKernelGGL(kf_fill_holes, dim3(r.n_chunks), dim3(F_TPB), 0, e->stream, e->lists.cur.rec, e->lists.cur.fill);
      HIPCHK(e->srt.req2.reserve(nslots * (int64_t) sizeof(u64)));
      HIPCHK(with_scratch(e->sort_tmp, [&](void *tmp, size_t &bytes)
        { return rocprim::radix_sort_keys<smg_sort_config>(tmp, bytes, (u64 *) e->lists.cur.rec, (u64 *) e->srt.req2, (size_t) nslots, 56u, 64u, e->stream); }));
    }
  return SMG_OK;
}

// smg_lookup.hpp: filter the partitioned requests against `map` (probe_plan); list = false: look the survivors up at once
static int lookup_probe(smg_engine *e, const uint32_t *map, bool list, unsigned maxout, char *errbuf, size_t errlen)
{ RunState &r = e->run;
  const bool two = r.bm2 != 0;                                  // (a map that came from outside was built by the same rule)
  const ProbePlan p = probe_plan(list, r.lg.nb, r.one_way != 0, e->st.nbig, e->st.nemitted, e->tab.n, e->cus);
  FastArgs a = make_fast(e);
  if (p.form == PROBE_X)
    { HIPCHK(e->chain.xtick.reserve((int64_t) PX_NXCD * PX_TICKW * 4));
      HIPCHK(hipMemsetAsync(e->chain.xtick, 0, (size_t) PX_NXCD * PX_TICKW * 4, e->stream));
      with_bool(two, [&](auto t) { with_words<2>(r.rw, [&](auto rw)
        { hipLaunchKernelGGL((kl_probe_x<t(), rw()>), dim3(p.grid), dim3(PX_TPB), 0, e->stream, a, (const u64 *) e->srt.req2,
                             (const u64 *) e->chain.boff, map, r.lg, e->chain.xtick, &e->ctrl->fast, p.part); }); });
    }
  else
    { u64 *const out = list ? (u64 *) e->lists.kept.rec : (u64 *) NULL;              // (the fused form keeps no survivor list)
      uint32_t *const fill = list ? (uint32_t *) e->lists.kept.fill : (uint32_t *) NULL;
      with_bool(list, [&](auto l) { with_bool(two, [&](auto t) { with_words<2>(r.rw, [&](auto rw)
        { hipLaunchKernelGGL((kl_probe<l(), t(), rw()>), dim3(p.grid), dim3(PB_TPB), 0, e->stream, a, (const u64 *) e->srt.req2, (const u64 *) e->chain.boff,
                             map, r.lg, e->chain.ghist + L_BK, out, fill, list ? maxout : 0u, &e->ctrl->fast); }); }); });
    }
  HIPCHK(hipGetLastError());
  r.probe_form = p.form; r.probe_part = p.part & 0x7FFFFFFFu;
  return SMG_OK;
}

// drop the requests whose target window block holds no candidate (filter_plan); map = NULL: this engine's own map
static int fast_filter(smg_engine *e, const uint32_t *map, char *errbuf, size_t errlen)
{ int rc;
  RunState &r = e->run;
  if (!filter_ok(e) || r.n_chunks == 0) return SMG_OK;
  if (!map) map = r.bm_bits ? e->bmap : NULL;
  if (!map) return SMG_OK;
  const int nbits = bm_id_bits(e->tab.kmer, e->set.bm_cap);
  const FilterPlan f = filter_plan(e->cus, r.n_chunks, e->st.nrequests, r.lg.nb != 0, e->rp.active ? (int64_t) e->rp.seen_chunks : -1);
  HIPCHK(e->lists.reserve(e->lists.kept, f.maxout, r.rw));
  if (e->rp.active)
    { // replayed step: WHICH chunks the waves of the probe kernel fill is decided by an atomic counter, and how many by the
      // way the buckets fall to the workgroups -- so the routing kernels walk the whole list, and a chunk nobody opened must
      // read as empty
      hipEventRecord(e->ev[EV_REPLAY_FILTER_BEG], e->stream);
      HIPCHK(hipMemsetAsync(e->lists.kept.fill, 0, (size_t) f.maxout * 4, e->stream));
    }
  if (!r.presorted && (rc = filter_presort(e, errbuf, errlen))) return rc;
  const int64_t nslots = (int64_t) r.n_chunks * F_CH;
  if (r.presorted == PRESORT_CHAIN)
    { if ((rc = lookup_probe(e, map, true, f.maxout, errbuf, errlen))) return rc; }
  else if (r.presorted == PRESORT_BUCKETED)
    hipLaunchKernelGGL(kf_filter<1>, dim3(f.grid), dim3(F_TPB), 0, e->stream, e->srt.req2, (const uint32_t *) NULL, r.n_chunks, nslots,
                       map, 64 - nbits, e->lists.kept.rec, e->lists.kept.fill, f.maxout, &e->ctrl->fast);
  else
    with_words<4>(r.rw, [&](auto rw) { hipLaunchKernelGGL(kf_filter<rw()>, dim3(f.grid), dim3(F_TPB), 0, e->stream, e->lists.cur.rec, e->lists.cur.fill, r.n_chunks, (int64_t) 0,
        map, 64 - nbits, e->lists.kept.rec, e->lists.kept.fill, f.maxout, &e->ctrl->fast); });
  hipEventRecord(e->ev[EV_LOOKUP_END], e->stream);
  HIPCHK(hipGetLastError());
  if (e->rp.active)
    { // replayed step: the kept list is as long as last time (the device checks it: smg_engine_proof) -- nothing is read
      hipEventRecord(e->ev[EV_REPLAY_FILTER_END], e->stream);
      e->rp.nf_chunks = f.maxout;           // (the device checks that the probe kernel stayed inside the list)
    }
  else
    { if ((rc = read_ctrl(e, errbuf, errlen))) return rc;
      if (e->h_ctrl->fast.nf_chunks > f.maxout) return fail(errbuf, errlen, SMG_ENODEV, "request filter overflowed its chunk list%s");
    }
  e->lists.swap();
  if (e->rp.active)
    { r.n_chunks = e->rp.nf_chunks; e->st.nrequests = e->rp.nf_req; r.filtered = true;
      return SMG_OK;
    }
  r.n_chunks = e->h_ctrl->fast.nf_chunks;
  e->st.nrequests = (int64_t) e->h_ctrl->fast.nf_req;
  r.filtered = true;
  e->st.ms_filter = ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
  e->st.ms_rclookup += e->st.ms_filter;
  // what a replayed step on this table may take for granted (key-only records through the look-up chain, k <= 64)
  e->rp.have = e->set.rp_want && r.presorted == PRESORT_CHAIN && e->tab.W <= 2 && r.rw == e->tab.W;
  if (e->rp.have)
    { e->rp.nreq = e->st.nemitted; e->rp.nbig = e->st.nbig; e->rp.nf_req = e->st.nrequests; e->rp.bm_bits = r.bm_bits;
      e->rp.seen_chunks = r.n_chunks; e->rp.nranks = 0;
    }
  return SMG_OK;
}

// squeeze the request chunks (ragged fills) into the dense array srt.dense: exclusive scan of the fills + one copy
static int compact_chunks(smg_engine *e, int64_t nreq, char *errbuf, size_t errlen)
{ HIPCHK(e->srt.dense.reserve(nreq * (int64_t) sizeof(u64) * e->run.rw));
  HIPCHK(e->srt.chunk_off.reserve((int64_t) e->run.n_chunks * 4 + 4));
  HIPCHK(with_scratch(e->sort_tmp, [&](void *tmp, size_t &bytes)
    { return rocprim::exclusive_scan(tmp, bytes, (uint32_t *) e->lists.cur.fill, (uint32_t *) e->srt.chunk_off, 0u, (size_t) e->run.n_chunks,
                                     rocprim::plus<uint32_t>(), e->stream); }));
  hipLaunchKernelGGL(kf_compact, dim3(e->run.n_chunks), dim3(F_TPB), 0, e->stream, e->lists.cur.rec, e->lists.cur.fill, e->srt.chunk_off, e->run.rw, e->srt.dense);
  return SMG_OK;
}

// look-ups of this engine's own request chunks (flat = NULL; filtered first if a block map was built) or of a flat
// array of received records, by the route of apply_plan
static int fast_apply(smg_engine *e, const u64 *flat, int64_t nflat, int check_count, int64_t *missing,
                      char *errbuf, size_t errlen)
{ int rc = SMG_OK;
  RunState &r = e->run;
  r.ap = ApplyState{};
  const auto plan = [&]() { return apply_plan(flat != NULL, e->tab.kmer, r.rw, r.n_chunks, flat ? nflat : e->st.nrequests, r.filtered, r.bm_bits, r.lg.nb); };
  ApplyPlan p = plan();
  if (p.route == ROUTE_FUSED)
    { if (r.n_chunks == 0 || e->st.nrequests == 0) { if (missing) *missing = 0; return SMG_OK; }
      if (!r.presorted && (rc = filter_presort(e, errbuf, errlen))) return rc;
      hipEventRecord(e->ev[EV_PROBE_BEG], e->stream);
      if ((rc = lookup_probe(e, e->bmap, false, 0u, errbuf, errlen))) return rc;
      hipEventRecord(e->ev[EV_LOOKUP_END], e->stream);
      if ((rc = read_ctrl(e, errbuf, errlen))) return rc;
      e->st.ms_filter = ms_between(e, EV_LOOKUP_BEG, EV_PROBE_BEG);       // scan + partition
      e->st.ms_rclookup += ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
      e->st.nrequests = (int64_t) e->h_ctrl->fast.nf_req;
      r.filtered = true;
      r.n_chunks = 0;                                                 // nothing left to route or to look up
      if (missing) *missing = e->h_ctrl->fast.missing;
      return SMG_OK;
    }
  if (p.filter_first)
    { if ((rc = fast_filter(e, NULL, errbuf, errlen))) return rc;
      p = plan();                                                     // (of the list the filter kept)
    }
  hipEventRecord(e->ev[EV_LOOKUP_BEG], e->stream);
  const u64 *rec = flat;
  if (p.route == ROUTE_SENTINELS)
    { hipLaunchKernelGGL(kf_fill_holes, dim3(r.n_chunks), dim3(F_TPB), 0, e->stream, e->lists.cur.rec, e->lists.cur.fill);
      rec = e->lists.cur.rec;
    }
  else if (p.route == ROUTE_COMPACTED)
    { if ((rc = compact_chunks(e, p.covered, errbuf, errlen))) return rc;
      rec = e->srt.dense;
    }
  if (p.kernel == APPLY_SORTED) rc = apply_sorted(e, rec, p, errbuf, errlen);
  else if (p.kernel != APPLY_NONE) rc = apply_indexed(e, rec, check_count, p, errbuf, errlen);
  if (rc) return rc;
  r.ap = ApplyState{ p.kernel, p.sorted, p.holes, p.covered, p.kernel != APPLY_NONE && make_fast(e).sig != NULL };
  hipEventRecord(e->ev[EV_LOOKUP_END], e->stream);
  HIPCHK(hipGetLastError());
  if (!missing && flat)                   // (sharded run: the count of missing complements stays on the device -- smg_engine_proof)
    { r.lookup_pending = true; return SMG_OK; }
  rc = read_ctrl(e, errbuf, errlen);
  if (rc) return rc;
  e->st.ms_rclookup += ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
  if (missing) *missing = e->h_ctrl->fast.missing;
  return SMG_OK;
}
