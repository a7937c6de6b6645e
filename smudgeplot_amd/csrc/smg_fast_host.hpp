// smg_fast_host.hpp -- host side of the fast path (k <= 85) around its two passes: the kernel arguments (make_fast), the
// instantiations of kf_pass1_d (p1_kernel), the geometry of the candidate map and of the request filter, pass 1 from its plan
// (p1_plan, p1_form, list_capacity: pure functions, no device, no engine) through reserve and launch to the retry loop
// (fast_pass1), pass 2 and the resume of an out-of-core shard.  What lies between the passes is smg_fast_lookup.hpp.  Part of
// the one translation unit smg_hetmers.hip, included behind the engine struct.

// ---- fast path (k <= 85) --------------------------------------------------------------------------

static FastArgs make_fast(smg_engine *e)
{ FastArgs a;
  a.keys = e->tab.keys; a.cnt = e->tab.cnt; a.n = e->tab.n; a.g = e->tab.geo; a.dir = e->run.dir;
  a.code = e->deg;
  a.sig = (e->tab.W <= 2 && e->run.use_sig) ? e->sig : NULL;
  a.sigsh = 16 + e->run.dir.dsh;               // the 16 bits right below the directory's bucket bits
  a.bmap = e->run.bm_bits ? e->bmap : NULL;
  a.bmsh = 32 - e->run.bm_bits;
  a.bm2 = e->run.bm2;
  a.ow = e->run.one_way;
  return a;
}

// The instantiation of kf_pass1_d for a table (var: VAR of smg_pass1d.hpp; kf: 17 <= k <= 32).  The one place that names them: the
// occupancy query and the launch of fast_pass1 both go through it, so what is asked about is what is launched.  20 instantiations,
// none that no caller can select: the hot forms exist for key-only records, the two-way hot form of odd k (VAR = 6) where the
// two-bit map it needs does (k >= 24: one-word k-mers with KF, two-word k-mers).  NULL: no such instantiation.
static P1Kernel p1_kernel(int W, int rw, bool odd, bool kf, int var)
{
#define P1_K(W_, RW_, ODD_, KF_) do { \
    if constexpr ((RW_) == (W_)) \
      { if constexpr ((ODD_) && ((W_) == 2 || (KF_))) if (var == 6) return kf_pass1_d<W_, W_, ODD_, KF_, 6>; \
        if (var == 2) return kf_pass1_d<W_, W_, ODD_, KF_, 2>; \
      } \
    if (var == 1) return kf_pass1_d<W_, RW_, ODD_, KF_, 1>; \
    return NULL; } while (0)
#define P1_K2(RW_, ODD_) { if (kf) P1_K(1, RW_, ODD_, true); else P1_K(1, RW_, ODD_, false); }
  if (W == 2 && rw == 2) { if (odd) P1_K(2, 2, true, false); else P1_K(2, 2, false, false); }
  else if (W == 2)  { if (odd) P1_K(2, 3, true, false); else P1_K(2, 3, false, false); }
  else if (rw == 1) { if (odd) P1_K2(1, true) else P1_K2(1, false) }
  else              { if (odd) P1_K2(2, true) else P1_K2(2, false) }
#undef P1_K2
#undef P1_K
}

// 32-bit words of a block map of 2^bits ids (two-bit map, smg_fast.hpp: 64 bits per 32 ids)
static inline int64_t bm_words(int bits, int two_bit) { return (((1ll << bits) + 31) >> 5) << two_bit; }

// block ids of the request filter = the leading bm_id_bits(k) bits of a k-mer (a function of k alone, so that the
// maps of all the shards of a table line up): window blocks, coarsened to 2^30 ids (128 MB of bits) at most
// cap: 30 when the maps of several shards are exchanged (128 MB in total), 32 on one GPU, where the probes of the
// first 30 bits are LDS reads (smg_lookup.hpp) and a finer map only costs its memset; SMG_BM_BITS overrides (8..32).
// An id never runs past the k-mer (2k bits) nor past its leading 32 bits.
static int bm_id_bits(int kmer, int cap)
{ cap = (int) hook_int("SMG_BM_BITS", 8, 32, cap);
  int nbits = cap > 30 ? 2 * kmer : 2 * (kmer / 2);
  if (nbits > cap) nbits = cap;
  return nbits;
}

// records the request filter covers (k = 1 has no prefix bases to name a block by)
static bool filter_ok(int kmer, int W, int rw)
{ return kmer >= 2 && ((W == 1 && rw == 1) || (W == 2 && rw != 1) || (W == 3 && rw == 4)); }
static bool filter_ok(const smg_engine *e) { return filter_ok(e->tab.kmer, e->tab.W, e->run.rw); }

static GeoR p1_geor(int kmer, int W)
{ GeoR gr;
  const int p0 = kmer / 2, sbits = 2 * (kmer - p0);
  gr.k = kmer;
  gr.kshift = (W == 1 ? 64 : 128) - 2 * kmer;           // (W = 2, 33 <= k <= 64: 0 .. 62)
  gr.pshift = (W == 1 ? 32 : 64) - 2 * p0;              // (W = 2: p0 = 16 .. 32)
  gr.smask = sbits >= 64 ? ~0ull : ((1ull << sbits) - 1ull);
  gr.mshift = sbits - 2;
  return gr;
}

// ---- pass 1 of the fast path: decide (p1_plan, p1_form), size (p1_reserve), launch (p1_attempt), retry (fast_pass1) --------
// What a pass 1 is going to do, as a function of k, n, the proof, the caller and the test hooks: no device, no engine
// (smg_engine_pass1_plan hands it to the tests).  SMG_TWO_WAY, SMG_NO_FILTER, SMG_ONE_BIT_MAP, SMG_SIG and SMG_BM_BITS are read here.
struct P1Plan
{ int     kmer, W, rw;            // record = the complement k-mer (W words) [+ one word: count | has-hi-pair << 16]
  bool    emit_all, want_fp;      // exact proof: every entry sends; hash proof: the fingerprints
  bool    one_way;                // one request per complement class (smg_fast.hpp)
  bool    narrow, odd, kf;        // k <= 64: kf_pass1_d (blocked register scan); its template arguments ODD and KF (17 <= k <= 32)
  int     dir_per;  bool index_ok;          // entries per directory bucket (dir_geometry); the table's own index may be the directory
  int     bm_bits, bm2;           // the candidate map: id bits (0: none, nothing is filtered), two-bit
  bool    chain, use_sig;         // the look-up chain of smg_lookup.hpp; pass 1 writes signatures
  GeoR    gr;
  int64_t ntiles, want_rec, want_big, dwords;     // tiles; first guess of the request list (without the grid's slack) and of the
};                                                //   list of deferred entries; 32-bit words of their bit map

// one_way_ok: the caller looks this engine's requests up itself, with this engine's map (smg_engine_run): odd k <= 63 with key-only
// records under the hash proof then sends one request per complement class; the test hook SMG_TWO_WAY=1 keeps the two-way
// protocol.  The phase API never passes it: its requests leave the engine, and the sender is not local to the look-up.
static P1Plan p1_plan(int kmer, int64_t n, bool emit_all, bool with_meta, bool want_fp, bool one_way_ok, int bm_cap, bool no_filter)
{ P1Plan p = {};
  p.kmer = kmer; p.W = (kmer + 31) / 32; p.emit_all = emit_all; p.want_fp = want_fp;
  p.narrow = p.W <= 2; p.odd = (kmer & 1) != 0;
  // (two-word k-mers send key-only records for the hash proof as one-word ones do: 16 instead of 24 bytes for 21.6 % of
  //  the entries at k = 51; three-word k-mers go through the generic kernel, whose records always carry the count word)
  p.rw = p.W + ((with_meta || p.W > 2) ? 1 : 0);
  p.one_way = one_way_ok && p.odd && kmer >= 3 && kmer <= 63 && p.rw == p.W && want_fp && !emit_all && !test_hook("SMG_TWO_WAY");
  // (hash proof of one- and two-word k-mers: the table's own prefix index, when it came with one, is the directory)
  p.dir_per = (emit_all || p.W > 1) ? 8 : 64; p.index_ok = !emit_all && p.narrow;
  p.use_sig = p.narrow;
  // request filter: the candidate block map (an empty shard has one too -- all zero -- so that every rank of a
  // sharded run reports the same geometry and takes part in the exchange of the maps)
  if (filter_ok(kmer, p.W, p.rw) && !emit_all && !no_filter && !test_hook("SMG_NO_FILTER"))
    { p.bm_bits = bm_id_bits(kmer, bm_cap);
      // the look-up chain of smg_lookup.hpp: one- and two-word k-mers, key-only records, a map of >= 12 id bits
      p.chain = p.bm_bits >= 12 && p.narrow && p.rw == p.W;
      // ... with the two-bit map (smg_fast.hpp) when the k-mer has bits below the id to hash (a function of k and the
      // environment alone: every shard of a table decides the same)
      p.bm2 = (p.chain && kmer >= 24 && !test_hook("SMG_ONE_BIT_MAP")) ? 1 : 0;
      // Signatures (2 bytes per entry written by pass 1, so that a look-up bisects 2-byte instead of 8-byte words)
      // pay when most requests are looked up.  With the 32-bit two-bit map of a single-GPU run 1 request in 115
      // survives the filter: 3.9e6 look-ups at 2.5e9 entries, which can afford the k-mer lines of their bucket, while
      // the signatures cost pass 1 5 GB of stores and four instructions per entry.  SMG_SIG=0/1 overrides.
      if (p.chain && p.bm2 && p.bm_bits >= 32) p.use_sig = false;
    }
  if (p.narrow) p.use_sig = hook_int("SMG_SIG", HOOK_ANY, p.use_sig) != 0;
  p.gr = p1_geor(kmer, p.W);
  p.kf = p.W == 1 && p.gr.pshift < 32 && p.gr.kshift < 32;
  p.ntiles = p.narrow ? (n + D_OWN - 1) / D_OWN : (n + F_TILE - 1) / F_TILE;
  p.want_rec = emit_all ? n + n / 24 : p.one_way ? n / 8 : n / 4;      // (one-way requests: half the senders)
  p.want_big = n / 16 + 4096;               // deferred entries: 0.13 % of the diploid table, 0.4 % with 5 % repeats
  p.dwords = ((((n + 31) >> 5) + 2) + 3) & ~3ll;                       // (kf_bigfix reads the map four words at a time)
  return p;
}

// The form of kf_pass1_d (VAR of smg_pass1d.hpp), settled once dir_geometry has said whether the index serves.  The hot form:
// key-only records through the look-up chain with the two-bit map and the fingerprint, on a table that came with its index (no
// directory, no signatures); where k is odd it has the protocol compiled in, one-way (2) or two-way (6: the phase API, the hook
// SMG_TWO_WAY).  Everything else: the general form (1).  0: the generic kf_pass1 of three-word k-mers, or no launch at all.
static int p1_form(const P1Plan &p, bool dir_preset, int64_t n)
{ if (!p.narrow || n == 0) return 0;
  const bool hot = p.rw == p.W && dir_preset && !p.use_sig && p.bm2 && p.bm_bits && p.want_fp && !p.emit_all && p.chain;
  return !hot ? 1 : (p.odd && !p.one_way) ? 6 : 2;
}

// Chunks of the request list that pass 1 over `grid` workgroups is given for want_rec records (the capacity its kernels see).
// A chunk is closed as soon as the next tile's batch (<= one tile of records) does not fit, so chunks fill to >= 75 %: want_rec
// is sized for that.  Never below `have`, the chunks already allocated (an engine reused on the same table must not redo pass 1).
static unsigned list_capacity(int64_t want_rec, unsigned grid, bool chain, int64_t have)
{ unsigned maxc = (unsigned) ((want_rec + F_CH - 1) / F_CH);
  if (chain)
    { // look-up chain: owner w fills the slots w, w + G, w + 2G, .. (G = workgroups of this launch + those of kf_bigfix),
      // so the list must hold G times the chunks of the busiest owner -- pass 1 deals its tiles round-robin, the owners
      // are balanced to a few per cent -- and the slots of the kf_bigfix owners stay empty on a table without long blocks
      const int64_t G = (int64_t) grid + BF_MAXGRID;
      const int64_t per = ((int64_t) maxc + grid - 1) / grid + 2;
      if (per * G > (int64_t) maxc && per * G < 0x7FFFFFFFll) maxc = (unsigned) (per * G);
    }
  if (have > (int64_t) maxc && have < 0x7FFFFFFFll) maxc = (unsigned) have;
  return maxc;
}

extern "C" int smg_engine_pass1_plan(int kmer, int64_t nels, int symcheck, int own_lookups, int have_index, int bm_cap, int no_filter,
                                     int32_t out[12])
{ if (kmer < 1 || kmer > FAST_MAX_K || nels < 0 || !out || symcheck == SMG_SYM_NONE) return SMG_EINVAL;
  const bool exact = symcheck == SMG_SYM_EXACT, hash = symcheck == SMG_SYM_HASH;
  const P1Plan p = p1_plan(kmer, nels, exact, exact, hash, own_lookups && hash, bm_cap, no_filter != 0);
  const bool preset = p.index_ok && have_index && nels > 0;               // (dir_geometry)
  const int32_t v[12] = { p.rw, p.one_way, p.narrow, p.dir_per, preset, p.bm_bits, p.bm2, p.chain ? lookup_geo(p.bm_bits).nb : 0,
                          p.use_sig, p1_form(p, preset, nels), p.kf, p.W };
  memcpy(out, v, sizeof(v));
  return SMG_OK;
}

// everything pass 1 writes besides its lists, in the order the stream sees it: code bytes, directory, map, signatures; then
// the kernel and its grid, and the bit map of deferred entries.  n = 0: no launch follows.
static int p1_reserve(smg_engine *e, const P1Plan &p, P1Kernel *p1k, unsigned *grid_out, char *errbuf, size_t errlen)
{ int rc;
  const int64_t n = e->tab.n, pbytes = ((n + 15) & ~15ll) + 32;
  HIPCHK(e->deg.reserve(pbytes));
  if ((rc = dir_geometry(e, p.dir_per, errbuf, errlen, p.index_ok))) return rc;
  if (p.bm_bits)
    { const int64_t bytes = 4 * bm_words(p.bm_bits, p.bm2) + ((4 * D_BMW + 64) << p.bm2);
      HIPCHK(e->bmap.reserve(bytes));
      HIPCHK(hipMemsetAsync(e->bmap, 0, (size_t) bytes, e->stream));
    }
  if (p.use_sig) HIPCHK(e->sig.reserve(2 * pbytes));
  if (!e->run.dir_preset)
    HIPCHK(hipMemsetAsync(e->bstart, n > 0 ? 0xFF : 0, sizeof(uint32_t) * ((size_t) e->run.dir.nb + 2), e->stream));
  if (n == 0) return SMG_OK;
  e->run.p1_var = p1_form(p, e->run.dir_preset, n);
  unsigned grid = P1_GRID;
  if (p.narrow)
    { if (!(*p1k = p1_kernel(p.W, p.rw, p.odd, p.kf, e->run.p1_var))) return fail(errbuf, errlen, SMG_EINVAL, "pass 1: no kernel for this table%s");
      // persistent workgroups: exactly what is resident (a static tile stride must not have stragglers)
      if (e->p1.asked != *p1k)
        { int nb = 0;
          const hipError_t he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, *p1k, D_TPB, 0);
          if (he != hipSuccess || nb < 1) nb = 3;
          if (nb > 8) nb = 8;
          e->p1.resident = (unsigned) (nb * e->cus);
          e->p1.asked = *p1k;
        }
      grid = e->p1.resident;
    }
  if (grid > P1_MAXGRID) grid = P1_MAXGRID;
  if ((int64_t) grid > p.ntiles) grid = (unsigned) p.ntiles;
  // (tests: fewer workgroups, never more -- and the cached occupancy above stays what the device said.  The chunk slots of an
  //  owner are strided by the number of owners, grid + BF_MAXGRID, so with ONE workgroup the list below holds 513 times the chunks
  //  of that owner plus the usual slack: by this arithmetic ~5 GB for a table of 4e5 one-word entries, ~11 GB for 1e6 two-word ones,
  //  and the filtered list takes the same again.  Sized, not measured; a hook for small tables on a device with room to spare.)
  grid = hook_grid("SMG_P1_GRID", grid);
  if (p.narrow)
    { if ((int64_t) e->p1.dbits.bytes < p.dwords * 4) e->p1.dbits_dirty = true;               // (fresh memory)
      HIPCHK(e->p1.dbits.reserve(p.dwords * 4));
    }
  *grid_out = grid;
  return SMG_OK;
}

// ONE attempt, straight through: the request list for want_rec records and the list of deferred entries for want_big, the
// clears, pass 1 over `grid` workgroups, kf_collect + kf_bigfix.  *maxc, *bigcap: the capacities the kernels were given.
static int p1_attempt(smg_engine *e, const P1Plan &p, P1Kernel p1k, unsigned grid, int64_t want_rec, int64_t want_big,
                      unsigned *maxc_out, unsigned *bigcap_out, char *errbuf, size_t errlen)
{ RunState &r = e->run;
  const unsigned maxc = list_capacity(want_rec, grid, r.lg.nb != 0, e->lists.chunks(r.rw));
  HIPCHK(e->lists.reserve(e->lists.cur, maxc, r.rw));
  *maxc_out = r.max_chunks = maxc;
  if (p.narrow && e->p1.dbits_dirty)
    { HIPCHK(hipMemsetAsync(e->p1.dbits, 0, e->p1.dbits.bytes, e->stream)); e->p1.dbits_dirty = false; }
  FastArgs a = make_fast(e);
  if (r.lg.nb)
    { // owners of the request chunks: the workgroups of this launch, then those of kf_bigfix (rows zero unless it runs)
      HIPCHK(e->chain.whist.reserve((int64_t) (grid + BF_MAXGRID) * L_BK * 4));
      HIPCHK(hipMemsetAsync(e->chain.whist + (size_t) grid * L_BK, 0, sizeof(unsigned) * BF_MAXGRID * L_BK, e->stream));
      HIPCHK(hipMemsetAsync(e->lists.cur.fill, 0, (size_t) maxc * 4, e->stream));      // (a slot that stays empty has fill 0)
      r.nown = grid + BF_MAXGRID;
    }
  r.p1grid = grid;
  hipEventRecord(e->ev[EV_PASS1_BEG], e->stream);
  if (!p.narrow)
    with_words<3>(p.W, [&](auto w) { hipLaunchKernelGGL(kf_pass1<w()>, dim3(grid), dim3(F_TPB), 0, e->stream, a, e->bstart,
        e->lists.cur.rec, e->lists.cur.fill, maxc, (int) p.emit_all, (int) p.want_fp, e->p1.partials, &e->ctrl->fast, p.ntiles); });
  else
    { P1Hot hot;
      hot.keys = a.keys; hot.cnt = a.cnt; hot.n = a.n; hot.code = a.code; hot.sig = a.sig; hot.bstart = r.dir_preset ? (uint32_t *) NULL : e->bstart;
      hot.bmap = a.bmap; hot.b0 = r.dir.b0; hot.nb = r.dir.nb;
      hot.shifts = P1Hot::pack(r.dir.dsh, a.sigsh, a.bmsh, p.emit_all, p.want_fp, r.lg.nb, r.bm2 != 0, r.one_way != 0);
      hot.G = p.gr; hot.ntiles = p.ntiles;
      P1Cold &c = *e->p1.h_cold;
      c.req = e->lists.cur.rec; c.chunk_fill = e->lists.cur.fill; c.dbits = e->p1.dbits;
      e->p1.dbits_dirty = true;                                               // until kf_bigfix has cleared the bits again
      c.partials = e->p1.partials; c.ctl = &e->ctrl->fast; c.max_chunks = maxc; c.whist = e->chain.whist; c.owners = grid + BF_MAXGRID;
      HIPCHK(e->p1.tick.reserve((int64_t) D_NCLS * D_TICKW * 4));
      HIPCHK(hipMemsetAsync(e->p1.tick, 0, (size_t) D_NCLS * D_TICKW * 4, e->stream));
      c.tick = e->p1.tick;
      HIPCHK(hipMemcpyAsync(e->p1.cold, e->p1.h_cold, sizeof(P1Cold), hipMemcpyHostToDevice, e->stream));
      // (the hot forms take these for granted: what chose them is what the kernel argument says)
      if (r.p1_var != 1 && (hot.bstart != NULL || hot.sig != NULL || hot.bmap == NULL))
        return fail(errbuf, errlen, SMG_EINVAL, "pass 1: the hot form without its preconditions%s");
      hipLaunchKernelGGL(p1k, dim3(grid), dim3(D_TPB), 0, e->stream, hot, (const P1Cold *) e->p1.cold);
    }
  hipEventRecord(e->ev[EV_PASS1_END], e->stream);
  HIPCHK(hipGetLastError());
  if (p.want_fp)
    HIPCHK(hipMemcpyAsync(e->p1.h_partials, e->p1.partials, sizeof(u64) * 4 * grid, hipMemcpyDeviceToHost, e->stream));
  *bigcap_out = 0;
  if (!p.narrow) return SMG_OK;
  // exact redo of the deferred entries (a pair at distance 4..30, or a window block longer than the window): kf_collect compacts
  // the bit map pass 1 marked them in into a list (and clears it), kf_bigfix redoes the list.  Launched without waiting for pass 1's
  // control words (a list that overflowed is guarded on the device; the run is redone either way, as for too short a biglist).
  if (want_big < (int64_t) e->p1.biglist.bytes / 4) want_big = (int64_t) e->p1.biglist.bytes / 4;
  if (want_big > 0xFFFFFFF0ll) want_big = 0xFFFFFFF0ll;
  HIPCHK(e->p1.biglist.reserve(want_big * 4));
  HIPCHK(e->p1.farp.reserve(e->p1.biglist.bytes));
  const unsigned bigcap = (unsigned) (e->p1.biglist.bytes / 4 > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : e->p1.biglist.bytes / 4);
  const int64_t cb = (p.dwords / 4 + BF_TPB - 1) / BF_TPB;
  hipEventRecord(e->ev[EV_BIGFIX_BEG], e->stream);
  hipLaunchKernelGGL(kf_collect, dim3((unsigned) (cb > BF_MAXGRID ? BF_MAXGRID : cb)), dim3(BF_TPB), 0, e->stream, e->p1.dbits, p.dwords, e->p1.biglist, bigcap, &e->ctrl->fast.nbig);
  unsigned *const bf_hist = r.lg.nb ? e->chain.whist + (size_t) grid * L_BK : (unsigned *) NULL;
  with_bool(p.W == 2, [&](auto two_words) { with_bool(r.rw == p.W, [&](auto key_only)
    { hipLaunchKernelGGL((kf_bigfix<two_words() ? 2 : 1, (two_words() ? 2 : 1) + (key_only() ? 0 : 1)>), dim3(BF_MAXGRID), dim3(BF_TPB), 0, e->stream, a, e->p1.biglist,
          &e->ctrl->fast.nbig, bigcap, e->lists.cur.rec, e->lists.cur.fill, maxc, &e->ctrl->fast, bf_hist, grid, grid + BF_MAXGRID, r.lg.nb, e->p1.farp); }); });
  hipEventRecord(e->ev[EV_PASS1_END], e->stream);
  HIPCHK(hipGetLastError());
  *bigcap_out = bigcap;
  return SMG_OK;
}

// the table's fingerprints: XOR of the partial words of pass 1's workgroups (smg_device.hpp)
static void fold_fp(smg_engine *e, unsigned grid)
{ memset(e->run.fp, 0, sizeof(e->run.fp));
  for (unsigned b = 0; b < grid; b++)
    for (int q = 0; q < 4; q++) e->run.fp[q] ^= e->p1.h_partials[b * 4 + q];
}

// replay: a step of the phase API on the table of the step before (smg_engine_set_replay).  Everything is launched as ever, but
// nothing is read back here: the lists are as large as last time, the counts that later launches take from the host (requests,
// deferred entries) are the recorded step's -- they are functions of the table -- and the device checks all of it against the
// control words at the end of the step (k_proof_replay).
static int fast_pass1(smg_engine *e, int emit_all, int with_meta, int want_fp, char *errbuf, size_t errlen, bool replay = false,
                      bool one_way_ok = false)
{ int rc;
  begin_run(e, RUN_FAST);
  RunState &r = e->run;
  const P1Plan p = p1_plan(e->tab.kmer, e->tab.n, emit_all != 0, with_meta != 0, want_fp != 0, one_way_ok, e->set.bm_cap, e->set.no_filter);
  r.rw = r.p1_rw = p.rw; r.p1_w = p.W; r.one_way = p.one_way; r.use_sig = p.use_sig; r.bm_bits = p.bm_bits; r.bm2 = p.bm2;
  if (p.chain) r.lg = lookup_geo(p.bm_bits);
  HIPCHK(hipMemsetAsync(e->ctrl, 0, sizeof(Ctrl), e->stream));
  set_geo(e);
  P1Kernel p1k = NULL;
  unsigned grid = 0, maxc = 0, bigcap = 0;
  if ((rc = p1_reserve(e, p, &p1k, &grid, errbuf, errlen))) return rc;
  if (e->tab.n == 0) { r.pass1_done = true; return SMG_OK; }
  int64_t want_rec = p.want_rec + (int64_t) (grid + 16 + 256) * F_CH, want_big = p.want_big;
  const FastCtl &f = e->h_ctrl->fast;
  bool done = false;
  for (int attempt = 0; attempt < 5 && !done; attempt++)
    { if ((rc = p1_attempt(e, p, p1k, grid, want_rec, want_big, &maxc, &bigcap, errbuf, errlen))) return rc;
      if (replay) break;
      if ((rc = read_ctrl(e, errbuf, errlen))) return rc;
      e->p1.dbits_dirty = false;
      if (f.unsorted) return fail(errbuf, errlen, SMG_EFORMAT, "table entries are not strictly increasing%s");
      // each redo sizes its list from the count the failed attempt reported, so the second attempt fits
      if (p.narrow && f.nbig > bigcap)        // more deferred entries than the list holds (a repeat-dominated table)
        { want_big = (int64_t) f.nbig + (int64_t) f.nbig / 8 + 4096;
          e->p1.dbits_dirty = true;              // (the bits of the entries that did not fit are still set)
        }
      else if (f.n_chunks > maxc) want_rec = (int64_t) (f.n_chunks + 16 + 256) * F_CH;       // the request list outgrew its first guess
      else done = true;
      if (!done) HIPCHK(hipMemsetAsync(&e->ctrl->fast, 0, sizeof(FastCtl), e->stream));
    }
  // (a list that still overflows is a bug, and must not be read as a complete request list)
  if (!replay && (!done || f.n_chunks > r.max_chunks))
    return fail(errbuf, errlen, SMG_ENODEV, "pass 1: the request list overflowed its capacity on every attempt%s");
  // the counts: this step's, or (replay) the recorded step's -- the real ones are checked at the end of the step, the
  // fingerprints and the times are read then (smg_engine_replay_done)
  if (replay) e->rp.grid = grid;
  else { fold_fp(e, want_fp ? grid : 0); e->st.ms_pass1 = ms_between(e, EV_PASS1_BEG, EV_PASS1_END); }
  r.n_chunks = replay ? 1 : f.n_chunks;                 // (replay: > 0, "there are requests")
  e->st.nrequests = e->st.nemitted = replay ? e->rp.nreq : (int64_t) f.nreq;
  e->st.nbig = replay ? e->rp.nbig : p.narrow ? (int64_t) f.nbig : 0;
  e->st.ms_filter = 0;
  e->st.ms_bigfix = (!replay && p.narrow) ? ms_between(e, EV_BIGFIX_BEG, EV_PASS1_END) : 0;
  r.far_listed = p.narrow;
  r.pass1_done = true;
  return SMG_OK;
}

static int fast_pass2(smg_engine *e, int64_t *d_plot, bool with_sum, char *errbuf, size_t errlen)
{ HIPCHK(hipMemsetAsync(d_plot, 0, sizeof(int64_t) * SMG_PLOT_CELLS, e->stream));
  FastArgs a = make_fast(e);
  hipEventRecord(e->ev[EV_PASS2_BEG], e->stream);
  if (e->tab.n > 0)
    { int64_t nb = (e->tab.n + P2_TPB - 1) / P2_TPB;
      if (nb > P2_GRID) nb = P2_GRID;
      nb = hook_grid("SMG_P2_GRID", (unsigned) nb);
      with_words<3>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_pass2<w()>, dim3((unsigned) nb), dim3(P2_TPB), 0, e->stream, a, (u64 *) d_plot); });
      // entries whose unique partner is out of the code's reach: from the list of deferred entries that pass 1 of one-
      // and two-word k-mers leaves, else (three words: the generic pass 1) from a scan of the code bytes
      if (e->run.far_listed && e->tab.W <= 2)
        { const unsigned nl = (unsigned) e->st.nbig;
          unsigned fb = (nl + 255) / 256;
          if (fb > 4096) fb = 4096;
          if (nl)
            with_words<2>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_pass2_far<w()>, dim3(fb), dim3(256), 0, e->stream, a, (const uint32_t *) e->p1.biglist,
                (const uint32_t *) e->p1.farp, nl, (u64 *) d_plot); });
        }
      else
        { int64_t fb = ((e->tab.n + 15) / 16 + 255) / 256;
          if (fb > 4096) fb = 4096;
          with_words<3>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_pass2_farscan<w()>, dim3((unsigned) fb), dim3(256), 0, e->stream, a, (u64 *) d_plot); });
        }
    }
  hipEventRecord(e->ev[EV_PASS2_END], e->stream);
  HIPCHK(hipGetLastError());
  int rc = SMG_OK;
  e->st.path = 1; e->run.completed = true;
  if (!with_sum)                        // (phase API: no host wait here; smg_engine_stats reads the events once they have fired)
    { e->st.npairs = 0; e->st.ms_pass2 = -1.0; return SMG_OK; }
  rc = plot_sum(e, d_plot, errbuf, errlen);                         // (one more kernel and a host round trip)
  if (rc) return rc;
  e->st.ms_pass2 = ms_between(e, EV_PASS2_BEG, EV_PASS2_END);
  return SMG_OK;
}

// ---- out-of-core shards: take a shard up again after its keys were dropped (smg_multi.hpp, host_run_sequential) ------------
// The shard's k-mers and counts are back in the engine (decoded again from the table), `d_codes` are the code bytes its
// pass 1 left.  What the look-ups of the received requests and pass 2 need besides is the directory: the table's prefix
// index if it was handed over, else one pass of k_directory.  No candidate map, no signatures, no list of deferred entries
// (pass 2 finds the far partners by scanning the code bytes, as it does for three-word k-mers).
static int fast_resume(smg_engine *e, const uint8_t *d_codes, int with_meta, char *errbuf, size_t errlen)
{ int rc;
  HIPCHK(hipSetDevice(e->device));
  begin_run(e, RUN_FAST);
  HIPCHK(hipMemsetAsync(e->ctrl, 0, sizeof(Ctrl), e->stream));
  set_geo(e);
  HIPCHK(e->deg.reserve(((e->tab.n + 15) & ~15ll) + 32));
  if (e->tab.n > 0) HIPCHK(hipMemcpyAsync(e->deg, d_codes, (size_t) e->tab.n, hipMemcpyDeviceToDevice, e->stream));
  e->run.rw = e->tab.W + ((with_meta || e->tab.W > 2) ? 1 : 0);
  e->st.nrequests = 0; e->st.ms_rclookup = 0;
  if ((rc = dir_geometry(e, 8, errbuf, errlen, true))) return rc;
  if (!e->run.dir_preset)
    { HIPCHK(hipMemsetAsync(e->bstart, e->tab.n > 0 ? 0xFF : 0, sizeof(uint32_t) * ((size_t) e->run.dir.nb + 2), e->stream));
      if (e->tab.n > 0)
        { Tab t = make_tab(e);
          const unsigned nblk = (unsigned) ((e->tab.n + 1 + TPB - 1) / TPB);
          with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(k_directory<w()>, dim3(nblk), dim3(TPB), 0, e->stream, t, e->bstart, e->ctrl); });
          HIPCHK(hipGetLastError());
        }
    }
  e->run.pass1_done = true;
  return SMG_OK;
}
