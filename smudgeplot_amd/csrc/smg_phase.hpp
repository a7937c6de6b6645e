// smg_phase.hpp -- the public phase API of sharded runs: pass1 / presort / filter / route / apply / apply_own / pass2 / stats,
// the proof words, the replay of a step with its three proof kernels, and the block map calls with km_merge_maps.  Part of the
// one translation unit smg_hetmers.hip, included behind smg_fast_lookup.hpp.
//
// k <= 85: the fast path.  k > 85: the counted path in the same steps (counted_phase_* above) -- pass 1 leaves ONE flat
// list of (rc(x), count | S_hi << 16) records, presented to the router as full chunks; no block map, nothing is filtered.

#define NEED_FAST(e)                                                                          \
  if (!(e)) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");                          \
  if ((e)->tab.kmer > FAST_MAX_K)                                                                \
    return fail(errbuf, errlen, SMG_EINVAL, "no block map and no request filter above k = 85%s");
#define NEED_ENGINE(e)  if (!(e)) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");

extern "C" int smg_engine_pass1(smg_engine *e, int symcheck, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  HIPCHK(hipSetDevice(e->device));
  e->st.ms_rclookup = 0;
  if (e->tab.kmer > FAST_MAX_K) return counted_phase_pass1(e, symcheck, errbuf, errlen);
  e->set.bm_cap = e->set.bm_want ? e->set.bm_want : 30;  // default: the maps of the shards are exchanged, 128 MB in total
  e->rp.active = false;
  if (e->set.rp_want && e->rp.have && symcheck == SMG_SYM_HASH && e->rp.sym == symcheck && e->tab.n > 0
      && e->rp.bm_bits == bm_id_bits(e->tab.kmer, e->set.bm_cap))
    { // the step before this one, on this very table, went through the look-up chain: queue this one from its counts
      const int rc = fast_pass1(e, 0, 0, 1, errbuf, errlen, true);
      if (rc) return rc;
      e->rp.active = true; e->rp.routed = false;
      return SMG_OK;
    }
  e->rp.sym = symcheck;
  return fast_pass1(e, symcheck == SMG_SYM_EXACT, symcheck == SMG_SYM_EXACT, symcheck == SMG_SYM_HASH, errbuf, errlen);
}

extern "C" int smg_engine_set_replay(smg_engine *e, int on)
{ if (!e) return SMG_EINVAL;
  e->set.rp_want = on != 0;
  if (!on) e->rp.have = false;
  return SMG_OK;
}

// is the current step a replayed one (1), and did the LAST finished step leave a record (2)?
extern "C" int smg_engine_replay_state(smg_engine *e) { return e ? (e->rp.active ? 1 : 0) | (e->rp.have ? 2 : 0) : 0; }

// after the caller has read the proof words of a replayed step: ok != 0 = the device found every count as recorded (the
// run stands: the engine's bookkeeping is brought up to date from the control words, which are complete by now),
// ok == 0 = the record is dropped and the next step runs the plain way
extern "C" int smg_engine_replay_done(smg_engine *e, int ok, char *errbuf, size_t errlen)
{ if (!e) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");
  if (!e->rp.active) return SMG_OK;
  e->rp.active = false;
  HIPCHK(hipSetDevice(e->device));
  if (!ok) { e->rp.have = false; e->p1.dbits_dirty = true; e->run.lookup_pending = false; return SMG_OK; }
  int rc = read_ctrl(e, errbuf, errlen);
  if (rc) return rc;
  e->p1.dbits_dirty = false;
  fold_fp(e, e->rp.grid);
  e->st.ms_pass1 = ms_between(e, EV_PASS1_BEG, EV_PASS1_END);
  e->st.ms_bigfix = ms_between(e, EV_BIGFIX_BEG, EV_PASS1_END);
  e->st.ms_filter = ms_between(e, EV_REPLAY_FILTER_BEG, EV_REPLAY_FILTER_END); e->st.ms_rclookup += e->st.ms_filter;
  return SMG_OK;
}

extern "C" int64_t smg_engine_nreq(smg_engine *e) { return e ? e->st.nrequests : 0; }
extern "C" int smg_engine_record_words(smg_engine *e) { return e ? e->run.rw : 0; }

extern "C" int smg_engine_apply(smg_engine *e, const uint64_t *d_recv, int64_t nrecv,
                                int64_t *missing, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!e->run.pass1_done) return fail(errbuf, errlen, SMG_EINVAL, "apply before pass1%s");
  HIPCHK(hipSetDevice(e->device));
  if (!ran_fast(e)) return counted_phase_apply(e, (const u64 *) d_recv, nrecv, missing, errbuf, errlen);
  return fast_apply(e, (const u64 *) d_recv, nrecv, 1, missing, errbuf, errlen);
}

__global__ void k_proof_words(const Ctrl *__restrict__ ctrl, int fast, u64 f0, u64 f1, u64 *__restrict__ dst)
{ if (threadIdx.x == 0) { dst[0] = fast ? (u64) ctrl->fast.missing : ctrl->missing; dst[1] = f0; dst[2] = f1; dst[3] = 0; } }

// the same for a replayed step: the fingerprint residue is folded from the workgroups' partial words on the device, and the
// counts the step was queued with are compared with what its kernels reported -- any difference sets dst[3], on which the
// caller (all ranks of a sharded run: the word is summed with the proof) drops the record and runs the step again the plain way
struct ReplayExpect { u64 nreq, nf_req; unsigned nbig, nf_chunks, max_chunks, grid; const u64 *totals; int nranks; };
__global__ void __launch_bounds__(64)
k_proof_replay(const Ctrl *__restrict__ ctrl, const u64 *__restrict__ partials, ReplayExpect x, u64 *__restrict__ dst)
{ u64 f0 = 0, f1 = 0;
  for (unsigned b = threadIdx.x; b < x.grid; b += 64)
    { f0 ^= partials[(size_t) b * 4] ^ partials[(size_t) b * 4 + 2]; f1 ^= partials[(size_t) b * 4 + 1] ^ partials[(size_t) b * 4 + 3]; }
  f0 = wave_xor_u64(f0); f1 = wave_xor_u64(f1);
  // the router's per-destination totals: recorded step in totals[0..16), this step in totals[16..32)
  bool moved = x.totals == NULL;
  if (x.totals && (int) threadIdx.x < x.nranks) moved = x.totals[threadIdx.x] != x.totals[16 + threadIdx.x];
  const bool anymoved = __ballot(moved) != 0;
  if (threadIdx.x == 0)
    { const FastCtl &f = ctrl->fast;
      const bool bad = f.unsorted != 0 || f.n_chunks > x.max_chunks || f.nbig != x.nbig || f.nreq != x.nreq
                       || f.nf_chunks > x.nf_chunks || f.nf_req != x.nf_req || anymoved;
      dst[0] = (u64) f.missing; dst[1] = f0; dst[2] = f1; dst[3] = bad ? 1ull : 0ull;
    }
}

// the proof tail of a sharded step's reduction buffer in ONE launch: tail[0] = missing, tail[1 + 2 s .. 2 + 2 s] = this rank's
// residue in ITS slot s (zeros in the others'), tail[1 + 2 nslots] = a replayed step found other counts, tail[2 + 2 nslots] =
// this step was a replayed one; src = the four words of k_proof_words / k_proof_replay
__global__ void __launch_bounds__(64)
k_proof_tail(const u64 *__restrict__ src, int nslots, int slot, int replayed, u64 *__restrict__ tail)
{ const int n = 3 + 2 * nslots;
  for (int i = threadIdx.x; i < n; i += 64)
    { u64 v = 0;
      if (i == 0) v = src[0];
      else if (i == 1 + 2 * slot) v = src[1];
      else if (i == 2 + 2 * slot) v = src[2];
      else if (i == n - 2) v = src[3];
      else if (i == n - 1) v = replayed ? 1ull : 0ull;
      tail[i] = v;
    }
}

static int proof_words(smg_engine *e, u64 *d_dst, char *errbuf, size_t errlen)
{ if (e->rp.active)
    { ReplayExpect x;
      x.nreq = (u64) e->rp.nreq; x.nf_req = (u64) e->rp.nf_req; x.nbig = (unsigned) e->rp.nbig; x.nf_chunks = e->rp.nf_chunks;
      x.max_chunks = e->run.max_chunks; x.grid = e->rp.grid;
      x.totals = e->rp.routed ? e->router.rp_totals : (const u64 *) NULL; x.nranks = e->rp.nranks;     // (not routed: nothing to vouch for the split)
      hipLaunchKernelGGL(k_proof_replay, dim3(1), dim3(64), 0, e->stream, (const Ctrl *) e->ctrl, (const u64 *) e->p1.partials, x, d_dst);
    }
  else
    hipLaunchKernelGGL(k_proof_words, dim3(1), dim3(64), 0, e->stream,
                       (const Ctrl *) e->ctrl, ran_fast(e) ? 1 : 0, e->run.fp[0] ^ e->run.fp[2], e->run.fp[1] ^ e->run.fp[3], d_dst);
  HIPCHK(hipGetLastError());
  return SMG_OK;
}

extern "C" int smg_engine_proof(smg_engine *e, uint64_t *d_dst, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!e->run.pass1_done || !d_dst) return fail(errbuf, errlen, SMG_EINVAL, "proof before pass1%s");
  HIPCHK(hipSetDevice(e->device));
  return proof_words(e, (u64 *) d_dst, errbuf, errlen);
}

extern "C" int smg_engine_proof_tail(smg_engine *e, uint64_t *d_tail, int nslots, int slot, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!e->run.pass1_done || !d_tail || nslots < 1 || nslots > 16 || slot < 0 || slot >= nslots)
    return fail(errbuf, errlen, SMG_EINVAL, "proof_tail: 1..16 slots, after pass1%s");
  HIPCHK(hipSetDevice(e->device));
  u64 *tmp = e->p1.partials + (size_t) 4 * P1_MAXGRID;           // (the row behind the workgroups' partial sums)
  int rc = proof_words(e, tmp, errbuf, errlen);
  if (rc) return rc;
  hipLaunchKernelGGL(k_proof_tail, dim3(1), dim3(64), 0, e->stream, (const u64 *) tmp, nslots, slot, e->rp.active ? 1 : 0, (u64 *) d_tail);
  HIPCHK(hipGetLastError());
  return SMG_OK;
}

extern "C" int smg_engine_apply_own(smg_engine *e, int64_t *missing, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!e->run.pass1_done) return fail(errbuf, errlen, SMG_EINVAL, "apply before pass1%s");
  HIPCHK(hipSetDevice(e->device));
  if (!ran_fast(e)) return counted_phase_apply(e, e->lists.cur.rec, e->st.nrequests, missing, errbuf, errlen);
  return fast_apply(e, NULL, 0, 1, missing, errbuf, errlen);
}

extern "C" int smg_engine_set_blockmap_bits(smg_engine *e, int id_bits)
{ if (!e || (id_bits != 0 && (id_bits < 8 || id_bits > 32))) return SMG_EINVAL;
  e->set.bm_want = id_bits;
  return SMG_OK;
}

extern "C" int smg_engine_blockmap(smg_engine *e, int *id_bits, int64_t *nwords)
{ if (!e || !id_bits || !nwords) return SMG_EINVAL;
  *id_bits = e->run.pass1_done ? e->run.bm_bits : 0;
  *nwords = *id_bits ? bm_words(*id_bits, e->run.bm2) : 0;
  return SMG_OK;
}

extern "C" int smg_engine_blockmap_copy(smg_engine *e, int64_t word_lo, int64_t nw, uint32_t *d_dst,
                                        char *errbuf, size_t errlen)
{ NEED_FAST(e)
  if (!e->run.pass1_done || !e->run.bm_bits) return fail(errbuf, errlen, SMG_EINVAL, "no block map: pass 1 (hash proof, k <= 85) has not run%s");
  const int64_t nwords = bm_words(e->run.bm_bits, e->run.bm2);
  if (word_lo < 0 || nw < 0 || word_lo + nw > nwords || (nw > 0 && !d_dst))
    return fail(errbuf, errlen, SMG_EINVAL, "block map range out of bounds%s");
  HIPCHK(hipSetDevice(e->device));
  if (nw > 0) HIPCHK(hipMemcpyAsync(d_dst, e->bmap + word_lo, (size_t) nw * 4, hipMemcpyDeviceToDevice, e->stream));
  return SMG_OK;
}

struct MapGeo { int64_t lo[16], ln[16]; };

__global__ void __launch_bounds__(256)
km_merge_maps(const uint32_t *__restrict__ parts, int64_t width, int nranks, MapGeo geo, uint32_t *__restrict__ full, int64_t nwords)
{ __shared__ int64_t lo[16], ln[16];
  if (threadIdx.x < 16) { lo[threadIdx.x] = geo.lo[threadIdx.x]; ln[threadIdx.x] = geo.ln[threadIdx.x]; }
  __syncthreads();
  for (int64_t w = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (int64_t) gridDim.x * blockDim.x)
    { uint32_t v = 0;
      for (int r = 0; r < nranks; r++)
        { const int64_t o = w - lo[r];
          if (o >= 0 && o < ln[r]) v |= parts[(size_t) r * width + o];
        }
      full[w] = v;
    }
}

extern "C" int smg_engine_merge_maps(smg_engine *e, const uint32_t *d_parts, int64_t width, int nranks,
                                     const int64_t *word_lo, const int64_t *nwords_of, uint32_t *d_full,
                                     char *errbuf, size_t errlen)
{ NEED_FAST(e)
  if (!e->run.pass1_done || !e->run.bm_bits) return fail(errbuf, errlen, SMG_EINVAL, "no block map: pass 1 (hash proof, k <= 85) has not run%s");
  if (!d_parts || !d_full || !word_lo || !nwords_of || nranks < 1 || nranks > 16 || width < 1)
    return fail(errbuf, errlen, SMG_EINVAL, "bad merge_maps arguments (1..16 ranks)%s");
  const int64_t nwords = bm_words(e->run.bm_bits, e->run.bm2);
  MapGeo geo;
  for (int r = 0; r < 16; r++) { geo.lo[r] = r < nranks ? word_lo[r] : 0; geo.ln[r] = r < nranks ? nwords_of[r] : 0; }
  for (int r = 0; r < nranks; r++)
    if (geo.lo[r] < 0 || geo.ln[r] < 0 || geo.ln[r] > width || geo.lo[r] + geo.ln[r] > nwords)
      return fail(errbuf, errlen, SMG_EINVAL, "block map range out of bounds%s");
  HIPCHK(hipSetDevice(e->device));
  hipLaunchKernelGGL(km_merge_maps, dim3(2048), dim3(256), 0, e->stream, d_parts, width, nranks, geo, d_full, nwords);
  HIPCHK(hipGetLastError());
  return SMG_OK;
}

extern "C" int smg_engine_presort(smg_engine *e, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!e->run.pass1_done) return fail(errbuf, errlen, SMG_EINVAL, "presort before pass1%s");
  if (!ran_fast(e) || !filter_ok(e) || !e->run.bm_bits || e->run.filtered || e->run.presorted || e->run.n_chunks == 0) return SMG_OK;
  HIPCHK(hipSetDevice(e->device));
  return filter_presort(e, errbuf, errlen);
}

extern "C" int smg_engine_filter(smg_engine *e, const uint32_t *d_map, int64_t *kept, char *errbuf, size_t errlen)
{ NEED_FAST(e)
  if (!e->run.pass1_done) return fail(errbuf, errlen, SMG_EINVAL, "filter before pass1%s");
  if (!filter_ok(e)) return fail(errbuf, errlen, SMG_EINVAL, "the request filter covers the hash proof at k <= 85%s");
  if (!d_map && !e->run.bm_bits) return fail(errbuf, errlen, SMG_EINVAL, "no block map to filter with%s");
  HIPCHK(hipSetDevice(e->device));
  int rc = e->run.filtered ? SMG_OK : fast_filter(e, d_map, errbuf, errlen);
  if (kept) *kept = e->st.nrequests;
  return rc;
}

extern "C" int smg_engine_symhash(smg_engine *e, uint64_t out[4], char *errbuf, size_t errlen)
{ if (!e || !out) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  for (int i = 0; i < 4; i++) out[i] = e->run.fp[i];
  return SMG_OK;
}

// records (rw words each, the first W of them a k-mer) in chunks of F_CH -> d_send, grouped by the rank whose k-mer
// range holds the k-mer (splitters = first k-mer of ranks 1..nranks-1); counts[nranks] on the host
// or, counts == NULL, d_counts[nranks] on the device: the totals stay there, no host wait
static int route_records(smg_engine *e, const u64 *req, const uint32_t *chunk_fill, unsigned nc, int rw,
                         const uint64_t *splitters, int nranks, uint64_t *d_send, int64_t capacity, int64_t *counts, int64_t *d_counts,
                         char *errbuf, size_t errlen)
{ if (counts) for (int r = 0; r < nranks; r++) counts[r] = 0;
  if (nc == 0)
    { if (d_counts) HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * nranks, e->stream));
      return SMG_OK;
    }
  if (nranks > 1)
    HIPCHK(hipMemcpyAsync(e->router.d_split, splitters, sizeof(u64) * (nranks - 1) * e->tab.W,
                          hipMemcpyHostToDevice, e->stream));
  HIPCHK(e->router.route_cnt.reserve((int64_t) nc * nranks * 4));
  HIPCHK(e->router.route_off.reserve(((int64_t) nc * nranks + 16) * 8));
  u64 *totals = e->router.route_off + (size_t) nc * nranks;           // [nranks], behind the offsets
  with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_route_count<w()>, dim3(nc), dim3(F_TPB), 0, e->stream, req,
      chunk_fill, rw, e->router.d_split, nranks, e->router.route_cnt); });
  // offsets and scatter follow on the device; the host only learns the totals (what the exchange needs): ONE round trip
  hipLaunchKernelGGL(kf_route_offsets, dim3(nranks), dim3(1024), 0, e->stream, (const uint32_t *) e->router.route_cnt, nc, nranks, e->router.route_off, totals);
  with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_route_scatter<w()>, dim3(nc), dim3(F_TPB), 0, e->stream, req,
      chunk_fill, rw, e->router.d_split, nranks, (const u64 *) e->router.route_off, (const u64 *) totals, (u64 *) d_send,
      (u64) (capacity < 0 ? 0 : capacity)); });
  HIPCHK(hipGetLastError());
  if (d_counts)
    { HIPCHK(hipMemcpyAsync(d_counts, totals, sizeof(u64) * nranks, hipMemcpyDeviceToDevice, e->stream));
      return SMG_OK;
    }
  u64 ht[16];
  HIPCHK(hipMemcpyAsync(ht, totals, sizeof(u64) * nranks, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int r = 0; r < nranks; r++) counts[r] = (int64_t) ht[r];
  return SMG_OK;
}

// what both route calls ask of their arguments and of the engine (counts: where the totals go, host or device); selects the device
static int route_check(smg_engine *e, int nranks, const int64_t *counts, int64_t capacity, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!counts || nranks < 1 || nranks > 16)
    return fail(errbuf, errlen, SMG_EINVAL, "bad route arguments (1..16 ranks)%s");
  if (!e->run.pass1_done) return fail(errbuf, errlen, SMG_EINVAL, "route before pass1%s");
  if (e->run.one_way) return fail(errbuf, errlen, SMG_EINVAL, "one-way requests cannot be routed: their senders are local to this engine%s");
  HIPCHK(hipSetDevice(e->device));
  if (e->st.nrequests > capacity) return fail(errbuf, errlen, SMG_EINVAL, "send buffer too small%s");
  return SMG_OK;
}

extern "C" int smg_engine_route(smg_engine *e, const uint64_t *splitters, int nranks,
                                uint64_t *d_send, int64_t capacity, int64_t *counts,
                                char *errbuf, size_t errlen)
{ int rc = route_check(e, nranks, counts, capacity, errbuf, errlen);
  if (rc) return rc;
  return route_records(e, e->lists.cur.rec, e->lists.cur.fill, e->run.n_chunks, e->run.rw, splitters, nranks, d_send, capacity, counts, NULL, errbuf, errlen);
}

extern "C" int smg_engine_route_device(smg_engine *e, const uint64_t *splitters, int nranks, uint64_t *d_send, int64_t capacity,
                                       int64_t *d_counts, char *errbuf, size_t errlen)
{ int rc = route_check(e, nranks, d_counts, capacity, errbuf, errlen);
  if (rc) return rc;
  rc = route_records(e, e->lists.cur.rec, e->lists.cur.fill, e->run.n_chunks, e->run.rw, splitters, nranks, d_send, capacity, NULL, d_counts, errbuf, errlen);
  if (rc || !e->set.rp_want || !ran_fast(e)) return rc;
  // replay: the per-destination totals of a plain step are kept, those of a replayed step are put beside them -- the verdict
  // kernel (smg_engine_proof) compares the two: the caller splits its exchange by the RECORDED totals
  if (!e->router.rp_totals) HIPCHK(e->router.rp_totals.alloc(sizeof(u64) * 32));
  const bool rep = e->rp.active;
  if (rep && e->rp.nranks != nranks) { e->rp.routed = false; return SMG_OK; }
  HIPCHK(hipMemcpyAsync(e->router.rp_totals + (rep ? 16 : 0), d_counts, sizeof(u64) * nranks, hipMemcpyDeviceToDevice, e->stream));
  if (rep) e->rp.routed = true; else e->rp.nranks = nranks;
  return SMG_OK;
}

extern "C" int smg_engine_pass2(smg_engine *e, int64_t *d_plot, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!e->run.pass1_done || !d_plot) return fail(errbuf, errlen, SMG_EINVAL, "pass2 before pass1%s");
  HIPCHK(hipSetDevice(e->device));
  if (!ran_fast(e)) return counted_phase_pass2(e, d_plot, errbuf, errlen);
  return fast_pass2(e, d_plot, false, errbuf, errlen);
}

extern "C" int smg_engine_stats(smg_engine *e, smg_stats *stats)
{ if (!e || !stats) return SMG_EINVAL;
  if (e->run.lookup_pending)                 // look-ups of received requests were queued without a wait
    { hipSetDevice(e->device);
      if (hipEventSynchronize(e->ev[EV_LOOKUP_END]) == hipSuccess) e->st.ms_rclookup += ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
      e->run.lookup_pending = false;
    }
  if (e->st.ms_pass2 < 0)                // pass 2 of the phase API was queued without a wait
    { hipSetDevice(e->device);
      e->st.ms_pass2 = hipEventSynchronize(e->ev[EV_PASS2_END]) == hipSuccess ? ms_between(e, EV_PASS2_BEG, EV_PASS2_END) : 0;
    }
  *stats = e->st;
  return SMG_OK;
}
