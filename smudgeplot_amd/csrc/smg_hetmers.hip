// smg_hetmers.hip -- MI355X (gfx950) heterozygous k-mer pair engine: kernels + C ABI.
//
// What it computes (reference: src/lib/PloidyPlot.c, restated in SURVEY.md section 8a):
//   pairs   = {(x,y) in table : x,y differ at exactly one base, cnt_x+cnt_y <= 1000}
//   deg(x)  = number of pairs containing x   (uint8, wraps mod 256: PloidyPlot.c:163,535)
//   plot[cnt_x+cnt_y][min(cnt_x,cnt_y)] += 1 for pairs with deg(x) <= 1 and deg(y) <= 1
//
// How (NOT the reference's k-level 4-way merge recursion, PloidyPlot.c:454-700, 851-923):
//   * Window scan.  In the sorted table the partners of x at a position p >= p0 share the
//     first p0 bases with x, so they sit in x's "window block" -- a handful of neighbouring
//     entries.  One thread per entry walks its block and tests neighbours with
//     XOR / popcount; blocks longer than WIN_LIM entries switch to binary searches.
//   * Reverse-complement half-scan.  A conditioned table contains every k-mer together with
//     its reverse complement at the same count (Symmex; PloidyPlot.c:1395-1414), and the
//     complement maps a pair at position p onto a pair at position k-1-p.  So only the
//     suffix-side positions p >= ceil((k-1)/2) are scanned (tiny blocks), pairs at p > k-1-p
//     count twice, and   deg(x) = S_all(x) + S_hi(rc(x))   where S_all / S_hi are the
//     numbers of pairs of x at p >= p0 / at p > k-1-p.  The second term is delivered by one
//     "request" per entry that owns such a pair, looked up through a bucket directory.
//     The symmetry is PROVEN per run (exact look-up of every complement, or a 128-bit
//     multiset fingerprint); if it fails the general path below is taken.
//   * General path.  Positions p < p0 are resolved by directory look-ups of the 3 variants;
//     nothing is assumed about the table.  Slow, exact, used only for asymmetric input.
//
// All arithmetic is integer; results are bit-exact against the reference.
//
// This file: the engine struct, the fast path (k <= 85), the phase API of sharded runs, the run entry points and the C ABI.
// The other paths are headers of this one translation unit, included where they are needed: smg_decode.hpp (FastK records ->
// table), smg_counted.hpp (k > 85 and the general path), smg_condition.hpp (trim, symmetrise, close), smg_ingest.hpp, smg_multi.hpp.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "smg_hetmers.h"
#include "smg_device.hpp"
#include "smg_keysort.hpp"
#include "smg_fast.hpp"
#include "smg_pass1d.hpp"
#include "smg_lookup.hpp"

// The environment, in two classes:
//   documented modes    getenv(): SMG_VIRTUAL_SHARDS, SMG_SEQUENTIAL_SHARDS, SMG_SHARD_LIMIT, SMG_HBM_LIMIT, SMG_FORCE_MULTI, and for a
//                       table on the device SMG_DEVICE_SHARDS, SMG_DEVICE_SHARD_LIMIT (smg_hetmers.h);
//   test hooks          test_hook(): force, on a table of any size, a code path that the engine otherwise picks from the table's
//                       size, k or counts (the 30-bit exchanged map, the one-bit map of k < 24, kl_probe_x, the unfiltered chain,
//                       pass 1's own directory, ..) -- tests/test_gpu_parity.py drives every one of them against the oracle;
//                       SMG_TWO_WAY=1 keeps the two-way request protocol where one-way would be chosen (tests/test_one_way_gpu.py);
//                       SMG_P2_GRID=<g> (1 .. P2_GRID) and SMG_EXTRACT_GRID=<g> (1 .. EX_GRID) launch kf_pass2 / kf_extract with at
//                       most g workgroups, so that a table of 1e5 entries takes a workgroup through several tiles or rounds
//                       (tests/test_pass2_regimes_gpu.py); the tile sizes they are cut at are read from smg_engine_pass2_limits;
//                       SMG_P1_GRID=<g> (>= 1) launches pass 1 with at most g workgroups, so that one owner of the request list
//                       holds several batches of kl_part on a table of 4e5 entries (tests/test_lookup_regimes_gpu.py, with
//                       smg_engine_lookup_limits and smg_engine_lookup_state);
//                       SMG_FILTER_GRID=<g> (>= 1) launches kf_filter with at most g workgroups, so that one workgroup takes several
//                       chunks and splits its survivors across output chunks on a table of 1e4 entries
//                       (tests/test_wide_fast_path_gpu.py, with smg_engine_wide_limits);
//                       SMG_APPLY_SORT_MIN=<n> (>= SORT_MIN) sorts a key-only list of one-word k-mers from n records on, so that a
//                       list of a few thousand records -- sentinel words among them -- takes the sort branch of apply_sorted
//                       (tests/test_list_lookups_gpu.py, with smg_engine_list_limits and smg_engine_apply_state).
static inline const char *test_hook(const char *name) { return getenv(name); }

// host: f(std::true_type) or f(std::false_type) -- with_words (smg_device.hpp) for a template argument that is a bool
template <class F> static inline void with_bool(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

#define WIN_LIM   32          // window blocks up to this many entries are walked linearly
#define TPB       256

// ------------------------------------------------------------------------------------------
//  Device-resident run state
// ------------------------------------------------------------------------------------------

struct Ctrl                    // small control block in device memory, zeroed per run
{ u64      nreq;               // requests emitted (may exceed capacity => rerun)
  u64      missing;            // complements absent / wrong count
  u64      unsorted;           // order violations found while building the directory
  u64      fp[4];              // fingerprints: T (2 seeds), rc(T) (2 seeds)
  u64      plot_sum;           // total weight in the plot (kf_plot_sum)
  FastCtl  fast;               // control words of the fast path
};

struct Tab                     // kernel argument block (passed by value)
{ const u64      *keys;
  const uint16_t *cnt;
  uint8_t        *deg;
  int64_t         n;
  Geo             g;
  Dir             dir;
};

// ------------------------------------------------------------------------------------------
//  Host side
// ------------------------------------------------------------------------------------------

#define FAST_MAX_K   85        // above this a uint8 degree can wrap: counted path (v1 kernels)
#define P1_GRID      1280      // persistent workgroups of the generic kf_pass1<W> (5 per CU resident: LDS bound)
#define P1_MAXGRID   4096      // upper bound of any pass-1 grid (partial fingerprint sums)
#define BF_MAXGRID   512       // workgroups of kf_bigfix (1024 threads each: two per CU)
#define P2_GRID      512       // persistent workgroups of kf_pass2 (2 per CU: 43.7 KB plot tile + 32 KB queue each)
#define EX_GRID      2048      // workgroups of kf_extract at most

typedef void (*P1Kernel)(P1Hot, const P1Cold *);          // an instantiation of kf_pass1_d (p1_kernel)

// the timing events, in pairs around: decode or conditioning (the first also starts kf_collect + kf_bigfix, whose time ends with
// pass 1's), pass 1, the look-ups (filter included), pass 2, the whole run, the filter of a replayed step, extract;
// EV_PROBE_BEG sits between the partition and the probe of the look-up chain
enum Ev { EV_DECODE_BEG, EV_DECODE_END, EV_PASS1_BEG, EV_PASS1_END, EV_LOOKUP_BEG, EV_LOOKUP_END, EV_PASS2_BEG, EV_PASS2_END,
          EV_RUN_BEG, EV_RUN_END, EV_PROBE_BEG, EV_REPLAY_FILTER_BEG, EV_REPLAY_FILTER_END, EV_EXTRACT_BEG, EV_EXTRACT_END, EV_COUNT };

// The engine's scalar state, by lifetime.  Four groups, each reset in one place:
//   Settings    what the caller asked for: survives every table and every run
//   TableState  the bound table: table_changed()
//   RunState    what the last pass 1 decided and how far its run has got: begin_run(), which table_changed() calls as well
//   Replay      the record a replayed step of the phase API runs from (below)
struct Settings
{ bool no_filter;             // pass 1 builds no candidate map and nothing is filtered (out-of-core shards: smg_multi.hpp, host_run_sequential)
  int  bm_cap;                // id bits of the block map: 32 on one GPU, 30 when the maps of several shards are exchanged
  int  bm_want;               //   ... as asked for by smg_engine_set_blockmap_bits (0: default)
  bool rp_want;               // replayed steps asked for (smg_engine_set_replay)
};

struct TableState
{ int             kmer, W;
  int64_t         n;
  const u64      *keys;       // bound or owned
  const uint16_t *cnt;
  bool            have_ixdir; // ixdir holds this table's prefix index (smg_engine_set_prefix_index)
  bool            have_ends;  u64 end_first, end_last;     // leading words of the first and the last entry (read once)
  Geo             geo;        // (set_geo: a function of k)
};

enum RunKind { RUN_NONE, RUN_FAST, RUN_COUNTED, RUN_GENERAL };    // k <= 85 / k > 85 / every position, nothing assumed
// the request list before the filter: not looked at yet / req2 holds it bucketed on its leading 8 bits / left as it is /
// req2 holds it partitioned into the buckets of the look-up chain
enum Presort { PRESORT_NONE, PRESORT_BUCKETED, PRESORT_ASIS, PRESORT_CHAIN };
enum ProbeForm { PROBE_NONE = 0, PROBE_FUSED = 1, PROBE_X = 2, PROBE_LIST = 3 };   // kl_probe fused / kl_probe_x / kl_probe to a list (exported)
// the list route of the last apply (smg_engine_apply_state): the look-up kernel, what became of the holes of the chunk list
enum ApplyKernel { APPLY_NONE = 0, APPLY_PLAIN = 1, APPLY_INDEXED = 2, APPLY_SORTED = 3 };      // none / kf_apply / kf_apply_indexed / kf_apply_sorted
enum ApplyHoles { HOLES_NONE = 0, HOLES_SENTINELS = 1, HOLES_COMPACTED = 2 };                   // a flat list / kf_fill_holes / kf_compact
struct ApplyState
{ ApplyKernel kernel;
  bool        sorted;           // the list, or its (key, record number) pairs, went through a radix sort first
  ApplyHoles  holes;
  int64_t     covered;          // records (flat and compacted lists) or chunk slots (sentinels) the look-up kernel walked
  bool        sig;              // the look-ups bisected signatures (FastArgs::sig != NULL)
};

struct RunState
{ RunKind   kind;             // the path of the pass 1 that ran last on this table
  bool      pass1_done;       // ... and it left its requests to the phase calls (the one-shot counted and general runs never do)
  bool      completed;        // pass 2 has run: deg[] holds finished code bytes (fast) or degrees (counted, general)
  int       rw;               // 64-bit words per request record
  int       one_way;          // the requests are one-way (smg_fast.hpp): smg_engine_run only, never the phase API
  bool      use_sig;          // pass 1 writes the 2-byte look-up signatures (not worth their 5 GB when the filter leaves 1 request in 115)
  int       bm_bits, bm2;     // leading k-mer bits per block id of the candidate map (0: none built); a two-bit map (smg_fast.hpp)
  LookupGeo lg;               // the look-up chain (lg.nb = 0: not used)
  Dir       dir;  bool dir_preset;      // the directory; it is the table's own index (ixdir): pass 1 writes none
  bool      filtered;         // the request list has been filtered
  Presort   presorted;
  ApplyState ap;              // the list route of the last apply (fast_apply resets it)
  ProbeForm probe_form;  unsigned probe_part;   // the probe kernel of the filter / look-up, requests per ticket of kl_probe_x (else 0)
  bool      far_listed;       // biglist[0 .. st.nbig) holds pass 1's deferred entries: pass 2 finishes the far partners from it
  bool      lookup_pending;   // look-ups of received requests were queued without a host wait (their time is read later)
  unsigned  n_chunks, max_chunks;       // chunks of the request list in use; its capacity
  unsigned  p1grid, nown;     // workgroups of pass 1; owners of the request list (+ BF_MAXGRID for kf_bigfix):
                              //   owner w fills the chunk slots w, w + nown, w + 2 nown, ..
  int       p1_var, p1_w, p1_rw;        // VAR of kf_pass1_d (0: the wide or the counted kernels), W, RW (smg_engine_pass1_form)
  u64       fp[4];            // fingerprints of the table and of its complement
};

// Replay of the PHASE calls (sharded runs, smg_engine_set_replay): a step on a table whose last step went through pass1 ->
// filter (hash proof, look-up chain) is queued without a read-back -- the counts the host needs are last step's (functions
// of the table and of the exchanged maps), the device compares them with this step's and reports through smg_engine_proof.
// The record is dropped (have = false) when the table changes, by smg_engine_set_replay(0) and by smg_engine_replay_done(!ok).
struct Replay
{ bool     have, active;      // a record exists / the current step runs from it
  int64_t  nreq, nbig, nf_req;          // pass 1: requests, deferred entries; filter: requests kept
  unsigned nf_chunks, grid;   // filter: chunks of the kept list (the list the routing kernels walk); pass-1 grid (rows of `partials`)
  unsigned seen_chunks;       // chunks the plain step's filter filled (a replayed step walks that many + slack)
  int      nranks;  bool routed;        // router: ranks of the recorded totals (rp_totals); this step's are there to be compared
  int      bm_bits, sym;      // map geometry and proof the record belongs to
};

struct smg_engine
{ int          device;
  hipStream_t  stream;
  Settings     set;
  TableState   tab;
  RunState     run;
  Replay       rp;
  DevBuf<u64>  rp_totals;     // replay: per-destination totals of the recorded step (16 words) and of this step (16 more)
  // (every device allocation is a DevBuf: grown where it is used by reserve(), freed with the engine)
  DevBuf<u64>  own_keys;      // owned copies (decode path)
  DevBuf<uint16_t> own_cnt;
  DevBuf<uint8_t>  deg;       // degree bytes (counted path) / code bytes (fast path)
  DevBuf<uint16_t> sig;       // k <= 32: look-up signatures (2 bytes per entry)
  DevBuf<uint32_t> bstart;
  DevBuf<uint32_t> ixdir;     // the table's own FastK prefix index (2^24 + 1 bucket starts, relative to this shard) as directory
  DevBuf<u64>  req;
  DevBuf<u64>  req2;          // radix sort output
  Dev          sort_tmp;      // rocPRIM's scratch (with_scratch)
  DevBuf<u64>  dense;         // compacted requests
  DevBuf<uint32_t> chunk_off;
  DevBuf<uint32_t> skey[2];   // index sort of wide records: leading k-mer bits (in, out)
  DevBuf<uint32_t> sidx[2];   //                                  record numbers (in, out)
  DevBuf<uint32_t> dbits;     // deferred entries of kf_pass1_d: one bit per table entry; all zero between runs
  bool         dbits_dirty;   //   ... unless a run was abandoned between pass 1 and kf_bigfix
  DevBuf<uint32_t> biglist;   // the marked entries, compacted (kf_collect)
  DevBuf<unsigned> p1tick;    // tile tickets of kf_pass1_d
  DevBuf<unsigned> xtick;     // (bucket, part) tickets of kl_probe_x, one counter per XCD
  DevBuf<uint32_t> farp;      // beside it: the partner of a listed entry whose code is CODE_FAR (kf_bigfix -> kf_pass2_far)
  DevBuf<uint32_t> chunk_fill;
  DevBuf<uint32_t> bmap;      // candidate block map (request filter)
  DevBuf<u64>  reqf;          // filtered request chunks (swapped with req)
  DevBuf<uint32_t> chunk_fillf;
  DevBuf<uint32_t> route_cnt;
  DevBuf<u64>  route_off;
  DevBuf<u64>  partials;   // [P1_MAXGRID][4]
  DevBuf<unsigned> ghist;  // look-up chain: requests per bucket [L_BK], bucket cursor `bnext` behind it
  DevBuf<unsigned> whist;  //   requests per owner and bucket [owners][L_BK] (owner = a workgroup of pass 1 / kf_bigfix)
  DevBuf<u64>  boff;       //   bucket offsets [L_BK + 1] and scatter cursors [L_BK] behind them
  DevBuf<P1Cold> p1cold;   // rarely used arguments of kf_pass1_d (device copy)
  P1Cold      *h_p1cold;   // pinned staging
  DevBuf<u64>  d_split;
  DevBuf<Ctrl> ctrl;
  Ctrl        *h_ctrl;        // pinned mirror
  u64         *h_partials;    // pinned
  P1Kernel     p1_asked;      // the instantiation of kf_pass1_d whose resident workgroups were asked for last (NULL: none yet) ..
  unsigned     p1_resident;   //   .. and the answer
  smg_stats    st;
  int          cus;           // compute units of the device (256 where it does not say)
  hipEvent_t   ev[EV_COUNT];
  float        ms_extract;    // device time of the last extract launch
};

static int fail(char *errbuf, size_t errlen, int code, const char *fmt, const char *a = "")
{ if (errbuf && errlen) snprintf(errbuf, errlen, fmt, a);
  return code;
}

#define HIPCHK(call)                                                                         \
  do { hipError_t _e = (call);                                                               \
       if (_e != hipSuccess)                                                                 \
         return fail(errbuf, errlen, _e == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV,     \
                     "HIP error: %s (" #call ")", hipGetErrorString(_e)); } while (0)

static float ms_between(smg_engine *e, Ev a, Ev b)
{ float ms = 0;
  hipEventElapsedTime(&ms, e->ev[a], e->ev[b]);
  return ms;
}

extern "C" const char *smg_version(void) { return "smudgeplot_amd 0.4 (hetmers engine, gfx950)"; }

extern "C" int smg_device_count(void)
{ int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" smg_engine *smg_engine_create(int device, void *stream, char *errbuf, size_t errlen)
{ int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    { fail(errbuf, errlen, SMG_ENODEV, "no HIP device available (this engine has no CPU fallback)%s");
      return NULL;
    }
  if (device < 0 || device >= n)
    { fail(errbuf, errlen, SMG_EINVAL, "device ordinal out of range%s"); return NULL; }
  if (hipSetDevice(device) != hipSuccess)
    { fail(errbuf, errlen, SMG_ENODEV, "cannot select HIP device%s"); return NULL; }
  smg_engine *e = new (std::nothrow) smg_engine();
  if (!e) { fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s"); return NULL; }
  e->device = device;
  e->stream = (hipStream_t) stream;
  e->set.bm_cap = 30;
  if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || e->cus < 1) e->cus = 256;
  for (int i = 0; i < EV_COUNT; i++) hipEventCreate(&e->ev[i]);
  if (e->ctrl.alloc(sizeof(Ctrl)) != hipSuccess
      || hipHostMalloc(&e->h_ctrl, sizeof(Ctrl)) != hipSuccess
      || e->partials.alloc(sizeof(u64) * 4 * (P1_MAXGRID + 1)) != hipSuccess      // (+ a row for the proof words)
      || hipHostMalloc(&e->h_partials, sizeof(u64) * 4 * P1_MAXGRID) != hipSuccess
      || e->d_split.alloc(sizeof(u64) * 16 * 4) != hipSuccess
      || e->p1cold.alloc(sizeof(P1Cold)) != hipSuccess
      || e->ghist.alloc(sizeof(unsigned) * (L_BK + 4)) != hipSuccess
      || e->boff.alloc(sizeof(u64) * (2 * L_BK + 4)) != hipSuccess
      || hipHostMalloc(&e->h_p1cold, sizeof(P1Cold)) != hipSuccess)
    { fail(errbuf, errlen, SMG_ENOMEM, "cannot allocate the control block%s");
      smg_engine_destroy(e); return NULL;
    }
  return e;
}

extern "C" void smg_engine_destroy(smg_engine *e)
{ if (!e) return;
  hipSetDevice(e->device);
  hipStreamSynchronize(e->stream);
  hipHostFree(e->h_ctrl); hipHostFree(e->h_partials); hipHostFree(e->h_p1cold);
  for (int i = 0; i < EV_COUNT; i++) hipEventDestroy(e->ev[i]);
  delete e;                                  // (frees every device buffer)
}

// which pass 1 the engine's byte array, lists and map belong to (ran_fast: with its requests there for the phase calls)
static inline bool ran_fast(const smg_engine *e)    { return e->run.kind == RUN_FAST && e->run.pass1_done; }
static inline bool ran_counted(const smg_engine *e) { return e->run.kind == RUN_COUNTED; }
static inline bool ran_general(const smg_engine *e) { return e->run.kind == RUN_GENERAL; }
static inline bool has_chain(const smg_engine *e)   { return ran_fast(e) && e->run.lg.nb > 0; }

// a pass 1 of `kind` starts (RUN_NONE: none has run on this table): nothing an earlier run decided or reached is left
static void begin_run(smg_engine *e, RunKind kind)
{ e->run = RunState{};
  e->run.kind = kind;
}

// the engine's table has n entries now and is another table: what a run, the prefix index and the ends said is gone
static void table_changed(smg_engine *e, int64_t n)
{ e->tab.n = n;
  e->tab.have_ixdir = false; e->tab.have_ends = false;
  begin_run(e, RUN_NONE);
  e->st.nels = n;
}

static int set_table(smg_engine *e, int kmer, int64_t nels, char *errbuf, size_t errlen)
{ if (kmer < 1 || kmer > SMG_MAX_KMER)
    return fail(errbuf, errlen, SMG_EINVAL, "k-mer length out of range (1..128)%s");
  if (nels < 0 || nels >= 0xFFFFFFF0ll)
    return fail(errbuf, errlen, SMG_EINVAL, "table shard too large (entries per GPU must be < 2^32-16)%s");
  e->tab.kmer = kmer;
  e->tab.W = (kmer + 31) / 32;
  memset(&e->st, 0, sizeof(e->st));
  table_changed(e, nels);
  e->rp.have = false; e->rp.active = false;
  e->st.key_words = e->tab.W;
  return SMG_OK;
}

static void set_geo(smg_engine *e)
{ Geo &g = e->tab.geo;
  g.k = e->tab.kmer;
  // first scanned position p0 = ceil((k-1)/2) = k/2 (integer division) for both parities: on
  // the symmetric path positions below it are the mirror images of the scanned ones, on the
  // general path they are resolved by directory look-ups
  g.p0 = e->tab.kmer / 2;
  g.pw = g.p0 >> 5;
  const int r = g.p0 & 31;
  g.pmask = r ? ~0ull << (64 - 2 * r) : 0ull;
  g.mid = (e->tab.kmer & 1) ? (e->tab.kmer - 1) / 2 : -1;
  g.wrap = e->tab.kmer > FAST_MAX_K;
}

extern "C" int smg_engine_bind(smg_engine *e, int kmer, int64_t nels, const uint64_t *d_keys,
                               const uint16_t *d_counts, char *errbuf, size_t errlen)
{ if (!e) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");
  if (nels > 0 && (!d_keys || !d_counts)) return fail(errbuf, errlen, SMG_EINVAL, "null table pointer%s");
  if (((uintptr_t) d_keys & 15) || ((uintptr_t) d_counts & 7))
    return fail(errbuf, errlen, SMG_EINVAL, "table pointers must be aligned (k-mers 16 bytes, counts 8 bytes)%s");
  HIPCHK(hipSetDevice(e->device));
  int rc = set_table(e, kmer, nels, errbuf, errlen);
  if (rc) return rc;
  e->tab.keys = (const u64 *) d_keys;
  e->tab.cnt = d_counts;
  return SMG_OK;
}

#include "smg_decode.hpp"

static int read_ctrl(smg_engine *e, char *errbuf, size_t errlen)
{ HIPCHK(hipMemcpyAsync(e->h_ctrl, e->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return SMG_OK;
}

// directory geometry over the first key word: `per` .. 2 `per` entries per bucket.  8 (one 128-byte line of k-mers) where
// every entry is looked up (exact proof, counted and general paths); 64 for the hash proof, whose filter leaves a few
// million look-ups: their bisection still stays inside one or two lines of signatures, while pass 1 writes -- and every
// run clears -- an eighth of the directory (1 GB -> 128 MB at 2.5e9 entries: -0.5 ms per run).
static int dir_geometry(smg_engine *e, int per, char *errbuf, size_t errlen, bool index_ok = false)
{ e->run.dir_preset = false;
  if (index_ok && e->tab.have_ixdir && e->tab.n > 0)
    { e->run.dir.bstart = e->ixdir; e->run.dir.b0 = 0; e->run.dir.dsh = 32 - IXDIR_BITS; e->run.dir.nb = 1u << IXDIR_BITS;
      e->run.dir_preset = true;
      return SMG_OK;
    }
  u64 first = 0, last = 0;
  if (e->tab.n > 0 && !e->tab.have_ends)      // (read once per bound table: a host round trip)
    { HIPCHK(hipMemcpyAsync(&e->tab.end_first, e->tab.keys, 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipMemcpyAsync(&e->tab.end_last, e->tab.keys + (size_t) (e->tab.n - 1) * e->tab.W, 8, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      e->tab.have_ends = true;
    }
  if (e->tab.n > 0) { first = e->tab.end_first; last = e->tab.end_last; }
  if (last < first) return fail(errbuf, errlen, SMG_EFORMAT, "table entries are not strictly increasing%s");
  int bits = 4;
  { const char *v = test_hook("SMG_DIR_PER"); if (v && atoi(v) >= 1) per = atoi(v); }       // tuning override
  while (bits < 30 && (1ll << (bits + 1)) <= e->tab.n / per) bits++;
  const uint32_t hf = (uint32_t) (first >> 32), hl = (uint32_t) (last >> 32);
  int dsh = 0;
  while (dsh < 31 && ((hl >> dsh) - (hf >> dsh)) >= (1u << bits)) dsh++;
  e->run.dir.b0 = hf >> dsh;
  e->run.dir.dsh = dsh;
  e->run.dir.nb = (hl >> dsh) - (hf >> dsh) + 1;
  HIPCHK(e->bstart.reserve((int64_t) sizeof(uint32_t) * ((int64_t) e->run.dir.nb + 2)));
  e->run.dir.bstart = e->bstart;
  return SMG_OK;
}

static int plot_sum(smg_engine *e, int64_t *d_plot, char *errbuf, size_t errlen)
{ HIPCHK(hipMemsetAsync(&e->ctrl->plot_sum, 0, sizeof(u64), e->stream));
  hipLaunchKernelGGL(kf_plot_sum, dim3(64), dim3(1024), 0, e->stream, (const u64 *) d_plot, &e->ctrl->plot_sum);
  int rc = read_ctrl(e, errbuf, errlen);
  if (rc) return rc;
  e->st.npairs = (int64_t) e->h_ctrl->plot_sum;
  return SMG_OK;
}

#include "smg_counted.hpp"

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
{ { const char *v = test_hook("SMG_BM_BITS"); if (v && atoi(v) >= 8 && atoi(v) <= 32) cap = atoi(v); }
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
  { const char *v = test_hook("SMG_SIG"); if (v && p.narrow) p.use_sig = atoi(v) != 0; }
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
      if (e->p1_asked != *p1k)
        { int nb = 0;
          const hipError_t he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, *p1k, D_TPB, 0);
          if (he != hipSuccess || nb < 1) nb = 3;
          if (nb > 8) nb = 8;
          e->p1_resident = (unsigned) (nb * e->cus);
          e->p1_asked = *p1k;
        }
      grid = e->p1_resident;
    }
  if (grid > P1_MAXGRID) grid = P1_MAXGRID;
  if ((int64_t) grid > p.ntiles) grid = (unsigned) p.ntiles;
  // (tests: fewer workgroups, never more -- and the cached occupancy above stays what the device said.  The chunk slots of an
  //  owner are strided by the number of owners, grid + BF_MAXGRID, so with ONE workgroup the list below holds 513 times the chunks
  //  of that owner plus the usual slack: by this arithmetic ~5 GB for a table of 4e5 one-word entries, ~11 GB for 1e6 two-word ones,
  //  and the filtered list takes the same again.  Sized, not measured; a hook for small tables on a device with room to spare.)
  { const char *v = test_hook("SMG_P1_GRID"); if (v && atoi(v) >= 1 && (unsigned) atoi(v) < grid) grid = (unsigned) atoi(v); }
  if (p.narrow)
    { if ((int64_t) e->dbits.bytes < p.dwords * 4) e->dbits_dirty = true;               // (fresh memory)
      HIPCHK(e->dbits.reserve(p.dwords * 4));
    }
  *grid_out = grid;
  return SMG_OK;
}

// ONE attempt, straight through: the request list for want_rec records and the list of deferred entries for want_big, the
// clears, pass 1 over `grid` workgroups, kf_collect + kf_bigfix.  *maxc, *bigcap: the capacities the kernels were given.
static int p1_attempt(smg_engine *e, const P1Plan &p, P1Kernel p1k, unsigned grid, int64_t want_rec, int64_t want_big,
                      unsigned *maxc_out, unsigned *bigcap_out, char *errbuf, size_t errlen)
{ RunState &r = e->run;
  // a chunk is closed as soon as the next tile's batch (<= one tile of records) does not fit, so chunks fill to >= 75 %: size
  // the list for that, and never below what is already allocated (an engine reused on the same table must not redo pass 1)
  unsigned maxc = (unsigned) ((want_rec + F_CH - 1) / F_CH);
  if (r.lg.nb)
    { // look-up chain: owner w fills the slots w, w + G, w + 2G, .. (G = workgroups of this launch + those of kf_bigfix),
      // so the list must hold G times the chunks of the busiest owner -- pass 1 deals its tiles round-robin, the owners
      // are balanced to a few per cent -- and the slots of the kf_bigfix owners stay empty on a table without long blocks
      const int64_t G = (int64_t) grid + BF_MAXGRID;
      const int64_t per = ((int64_t) maxc + grid - 1) / grid + 2;
      if (per * G > (int64_t) maxc && per * G < 0x7FFFFFFFll) maxc = (unsigned) (per * G);
    }
  { const int64_t have = (int64_t) e->req.bytes / ((int64_t) F_CH * (int64_t) sizeof(u64) * r.rw);
    if (e->req && have > (int64_t) maxc && have < 0x7FFFFFFFll) maxc = (unsigned) have;
  }
  HIPCHK(e->req.reserve((int64_t) maxc * F_CH * (int64_t) sizeof(u64) * r.rw));
  HIPCHK(e->chunk_fill.reserve((int64_t) maxc * 4 + 4));
  *maxc_out = r.max_chunks = maxc;
  if (p.narrow && e->dbits_dirty)
    { HIPCHK(hipMemsetAsync(e->dbits, 0, e->dbits.bytes, e->stream)); e->dbits_dirty = false; }
  FastArgs a = make_fast(e);
  if (r.lg.nb)
    { // owners of the request chunks: the workgroups of this launch, then those of kf_bigfix (rows zero unless it runs)
      HIPCHK(e->whist.reserve((int64_t) (grid + BF_MAXGRID) * L_BK * 4));
      HIPCHK(hipMemsetAsync(e->whist + (size_t) grid * L_BK, 0, sizeof(unsigned) * BF_MAXGRID * L_BK, e->stream));
      HIPCHK(hipMemsetAsync(e->chunk_fill, 0, (size_t) maxc * 4, e->stream));      // (a slot that stays empty has fill 0)
      r.nown = grid + BF_MAXGRID;
    }
  r.p1grid = grid;
  hipEventRecord(e->ev[EV_PASS1_BEG], e->stream);
  if (!p.narrow)
    with_words<3>(p.W, [&](auto w) { hipLaunchKernelGGL(kf_pass1<w()>, dim3(grid), dim3(F_TPB), 0, e->stream, a, e->bstart,
        e->req, e->chunk_fill, maxc, (int) p.emit_all, (int) p.want_fp, e->partials, &e->ctrl->fast, p.ntiles); });
  else
    { P1Hot hot;
      hot.keys = a.keys; hot.cnt = a.cnt; hot.n = a.n; hot.code = a.code; hot.sig = a.sig; hot.bstart = r.dir_preset ? (uint32_t *) NULL : e->bstart;
      hot.bmap = a.bmap; hot.b0 = r.dir.b0; hot.nb = r.dir.nb;
      hot.shifts = P1Hot::pack(r.dir.dsh, a.sigsh, a.bmsh, p.emit_all, p.want_fp, r.lg.nb, r.bm2 != 0, r.one_way != 0);
      hot.G = p.gr; hot.ntiles = p.ntiles;
      P1Cold &c = *e->h_p1cold;
      c.req = e->req; c.chunk_fill = e->chunk_fill; c.dbits = e->dbits;
      e->dbits_dirty = true;                                               // until kf_bigfix has cleared the bits again
      c.partials = e->partials; c.ctl = &e->ctrl->fast; c.max_chunks = maxc; c.whist = e->whist; c.owners = grid + BF_MAXGRID;
      HIPCHK(e->p1tick.reserve((int64_t) D_NCLS * D_TICKW * 4));
      HIPCHK(hipMemsetAsync(e->p1tick, 0, (size_t) D_NCLS * D_TICKW * 4, e->stream));
      c.tick = e->p1tick;
      HIPCHK(hipMemcpyAsync(e->p1cold, e->h_p1cold, sizeof(P1Cold), hipMemcpyHostToDevice, e->stream));
      // (the hot forms take these for granted: what chose them is what the kernel argument says)
      if (r.p1_var != 1 && (hot.bstart != NULL || hot.sig != NULL || hot.bmap == NULL))
        return fail(errbuf, errlen, SMG_EINVAL, "pass 1: the hot form without its preconditions%s");
      hipLaunchKernelGGL(p1k, dim3(grid), dim3(D_TPB), 0, e->stream, hot, (const P1Cold *) e->p1cold);
    }
  hipEventRecord(e->ev[EV_PASS1_END], e->stream);
  HIPCHK(hipGetLastError());
  if (p.want_fp)
    HIPCHK(hipMemcpyAsync(e->h_partials, e->partials, sizeof(u64) * 4 * grid, hipMemcpyDeviceToHost, e->stream));
  *bigcap_out = 0;
  if (!p.narrow) return SMG_OK;
  // exact redo of the deferred entries (a pair at distance 4..30, or a window block longer than the window): kf_collect compacts
  // the bit map pass 1 marked them in into a list (and clears it), kf_bigfix redoes the list.  Launched without waiting for pass 1's
  // control words (a list that overflowed is guarded on the device; the run is redone either way, as for too short a biglist).
  if (want_big < (int64_t) e->biglist.bytes / 4) want_big = (int64_t) e->biglist.bytes / 4;
  if (want_big > 0xFFFFFFF0ll) want_big = 0xFFFFFFF0ll;
  HIPCHK(e->biglist.reserve(want_big * 4));
  HIPCHK(e->farp.reserve(e->biglist.bytes));
  const unsigned bigcap = (unsigned) (e->biglist.bytes / 4 > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : e->biglist.bytes / 4);
  const int64_t cb = (p.dwords / 4 + BF_TPB - 1) / BF_TPB;
  hipEventRecord(e->ev[EV_DECODE_BEG], e->stream);
  hipLaunchKernelGGL(kf_collect, dim3((unsigned) (cb > BF_MAXGRID ? BF_MAXGRID : cb)), dim3(BF_TPB), 0, e->stream, e->dbits, p.dwords, e->biglist, bigcap, &e->ctrl->fast.nbig);
  unsigned *const bf_hist = r.lg.nb ? e->whist + (size_t) grid * L_BK : (unsigned *) NULL;
  with_bool(p.W == 2, [&](auto two_words) { with_bool(r.rw == p.W, [&](auto key_only)
    { hipLaunchKernelGGL((kf_bigfix<two_words() ? 2 : 1, (two_words() ? 2 : 1) + (key_only() ? 0 : 1)>), dim3(BF_MAXGRID), dim3(BF_TPB), 0, e->stream, a, e->biglist,
          &e->ctrl->fast.nbig, bigcap, e->req, e->chunk_fill, maxc, &e->ctrl->fast, bf_hist, grid, grid + BF_MAXGRID, r.lg.nb, e->farp); }); });
  hipEventRecord(e->ev[EV_PASS1_END], e->stream);
  HIPCHK(hipGetLastError());
  *bigcap_out = bigcap;
  return SMG_OK;
}

// the table's fingerprints: XOR of the partial words of pass 1's workgroups (smg_device.hpp)
static void fold_fp(smg_engine *e, unsigned grid)
{ memset(e->run.fp, 0, sizeof(e->run.fp));
  for (unsigned b = 0; b < grid; b++)
    for (int q = 0; q < 4; q++) e->run.fp[q] ^= e->h_partials[b * 4 + q];
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
      e->dbits_dirty = false;
      if (f.unsorted) return fail(errbuf, errlen, SMG_EFORMAT, "table entries are not strictly increasing%s");
      // each redo sizes its list from the count the failed attempt reported, so the second attempt fits
      if (p.narrow && f.nbig > bigcap)        // more deferred entries than the list holds (a repeat-dominated table)
        { want_big = (int64_t) f.nbig + (int64_t) f.nbig / 8 + 4096;
          e->dbits_dirty = true;              // (the bits of the entries that did not fit are still set)
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
  e->st.ms_bigfix = (!replay && p.narrow) ? ms_between(e, EV_DECODE_BEG, EV_PASS1_END) : 0;
  r.far_listed = p.narrow;
  r.pass1_done = true;
  return SMG_OK;
}

// key-only records of one-word k-mers: radix sort on the leading 32 bits, then look up in order.
// rocPRIM's mid-size (merge sort) variant returned garbage with a partial bit range on gfx950 /
// ROCm 7.2, so Onesweep is forced (MergeSortLimit = 0) and small batches are not sorted at all
// (their look-ups are too few to matter).  SMG_VERIFY_SORT=1 checks every sort (order + checksums).
#define SORT_MIN 4096
#define APPLY_SORT_MIN  (1 << 21)     // apply_sorted: key-only lists of one-word k-mers are sorted from here on (SMG_APPLY_SORT_MIN)
#define FILTER_SORT_MIN (1 << 22)     // filter_presort: chunk slots from which a key-only list is bucketed first (SMG_FILTER_SORT_MIN)
typedef rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                   rocprim::default_config, 0> smg_sort_config;

// sort nsort keys and look them up in that order; holes != 0: the list contains sentinel words (kf_fill_holes)
static int apply_sorted(smg_engine *e, const u64 *keys_in, int64_t nsort, int holes, char *errbuf, size_t errlen)
{ if (nsort <= 0) return SMG_OK;
  FastArgs a = make_fast(e);
  int64_t nb = (nsort + F_TPB - 1) / F_TPB;
  if (nb > 16384) nb = 16384;
  const u64 *src = keys_in;
  // (a short list -- what one rank of eight receives -- is looked up as it comes: the sort is eight launches, ~90 us, to put
  //  a few hundred thousand look-ups in order, which take 70 us either way)
  int64_t sort_min = APPLY_SORT_MIN;
  { const char *v = test_hook("SMG_APPLY_SORT_MIN"); if (v) sort_min = atoll(v); if (sort_min < SORT_MIN) sort_min = SORT_MIN; }
  e->run.ap.kernel = APPLY_SORTED; e->run.ap.sorted = nsort >= sort_min; e->run.ap.covered = nsort; e->run.ap.sig = a.sig != NULL;
  if (nsort >= sort_min)
    { HIPCHK(e->req2.reserve(nsort * (int64_t) sizeof(u64)));
      const unsigned lobit = 40;             // sort on bits [lobit, 64) of the k-mer
      HIPCHK(with_scratch(e->sort_tmp, [&](void *tmp, size_t &bytes)
        { return rocprim::radix_sort_keys<smg_sort_config>(tmp, bytes, (u64 *) keys_in, (u64 *) e->req2, (size_t) nsort, lobit, 64u, e->stream); }));
      src = e->req2;
      if (test_hook("SMG_VERIFY_SORT"))
        { DevBuf<u64> d_chk; u64 h[4];
          HIPCHK(d_chk.alloc(32));
          HIPCHK(hipMemsetAsync(d_chk, 0, 32, e->stream));
          hipLaunchKernelGGL(kf_check_sorted, dim3((unsigned) nb), dim3(F_TPB), 0, e->stream, keys_in, e->req2, nsort, (int) lobit, d_chk);
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
// that order (small batches are looked up as they come)
static int apply_indexed(smg_engine *e, const u64 *rec, int64_t n, int check_count, char *errbuf, size_t errlen)
{ if (n <= 0) return SMG_OK;
  FastArgs a = make_fast(e);
  int64_t nb = (n + F_TPB - 1) / F_TPB;
  if (nb > 16384) nb = 16384;
  e->run.ap.covered = n; e->run.ap.sig = a.sig != NULL;
  if (n < SORT_MIN || n >= 0xFFFFFFF0ll)
    { e->run.ap.kernel = APPLY_PLAIN; e->run.ap.sorted = false;
      with_words<3>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_apply<w()>, dim3((unsigned) (nb > 8192 ? 8192 : nb)), dim3(F_TPB), 0, e->stream, a, rec,
          (const uint32_t *) NULL, n, check_count, &e->ctrl->fast, e->run.rw); });
      return SMG_OK;
    }
  e->run.ap.kernel = APPLY_INDEXED; e->run.ap.sorted = true;
  for (int q = 0; q < 2; q++)
    { HIPCHK(e->skey[q].reserve(n * 4 + 16));
      HIPCHK(e->sidx[q].reserve(n * 4 + 16));
    }
  hipLaunchKernelGGL(kf_sortkey, dim3((unsigned) nb), dim3(F_TPB), 0, e->stream, rec, e->run.rw, n, e->skey[0], e->sidx[0]);
  uint32_t *const ki = e->skey[0], *const ko = e->skey[1], *const vi = e->sidx[0], *const vo = e->sidx[1];
  HIPCHK(with_scratch(e->sort_tmp, [&](void *tmp, size_t &bytes)
    { return rocprim::radix_sort_pairs<smg_sort_config>(tmp, bytes, ki, ko, vi, vo, (size_t) n, 8u, 32u, e->stream); }));
  with_words<3>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_apply_indexed<w()>, dim3((unsigned) nb), dim3(F_TPB), 0, e->stream, a, rec, e->sidx[1], n,
      check_count, &e->ctrl->fast, e->run.rw); });
  return SMG_OK;
}

// first half of the request filter, which does not need the map (a sharded run overlaps it with the exchange of the
// block maps): long key-only lists are bucketed on their leading 8 bits.  The probes of the 128 MB map are random
// 64-byte fetches otherwise (7 ms for the 4.4e8 requests of the 1 Gbp table); one radix pass (holes of the chunk
// array as sentinels, as for the look-ups) keeps the map words that the resident workgroups probe inside the L2s.
static int filter_presort(smg_engine *e, char *errbuf, size_t errlen)
{ hipEventRecord(e->ev[EV_LOOKUP_BEG], e->stream);                      // start of the filter's time
  if (e->run.lg.nb)
    { // smg_lookup.hpp: bucket offsets from pass 1's histogram, one-pass partition into the dense array req2
      const int64_t nreq = e->st.nrequests;
      HIPCHK(e->req2.reserve((nreq > 0 ? nreq : 1) * (int64_t) sizeof(u64) * e->run.rw));
      const int nbk = 1 << e->run.lg.nb;
      // bucket sizes = column sums of the owners' histogram rows -> bucket offsets -> first slot of every owner in every bucket
      hipLaunchKernelGGL(kl_tot, dim3(L_BK / LW_BPW), dim3(LW_SL * LW_BPW), 0, e->stream, (const unsigned *) e->whist, e->run.nown, e->ghist);
      hipLaunchKernelGGL(kl_scan, dim3(1), dim3(L_BK), 0, e->stream, e->ghist, nbk, e->boff, e->boff + L_BK + 2, e->ghist + L_BK);
      hipLaunchKernelGGL(kl_woff, dim3(L_BK / LW_BPW), dim3(LW_SL * LW_BPW), 0, e->stream, e->whist, e->run.nown, (const u64 *) e->boff);
      if (e->run.n_chunks)
        with_words<2>(e->run.rw, [&](auto rw) { hipLaunchKernelGGL(kl_part<rw()>, dim3(e->run.nown), dim3(PT_TPB), 0, e->stream, e->req, e->chunk_fill, e->run.nown,
            (const unsigned *) e->whist, e->run.max_chunks, e->run.lg.nb, e->req2); });
      HIPCHK(hipGetLastError());
      e->run.presorted = PRESORT_CHAIN;
      return SMG_OK;
    }
  e->run.presorted = PRESORT_ASIS;
  const int64_t nslots = (int64_t) e->run.n_chunks * F_CH;
  int64_t sort_min = FILTER_SORT_MIN;       // below this the probes are too few to matter
  { const char *v = test_hook("SMG_FILTER_SORT_MIN"); if (v) sort_min = atoll(v); if (sort_min < SORT_MIN) sort_min = SORT_MIN; }
  if (!(e->run.rw == 1 && nslots >= sort_min && e->tab.kmer < 32)) return SMG_OK;
  hipLaunchKernelGGL(kf_fill_holes, dim3(e->run.n_chunks), dim3(F_TPB), 0, e->stream, e->req, e->chunk_fill);
  HIPCHK(e->req2.reserve(nslots * (int64_t) sizeof(u64)));
  HIPCHK(with_scratch(e->sort_tmp, [&](void *tmp, size_t &bytes)
    { return rocprim::radix_sort_keys<smg_sort_config>(tmp, bytes, (u64 *) e->req, (u64 *) e->req2, (size_t) nslots, 56u, 64u, e->stream); }));
  e->run.presorted = PRESORT_BUCKETED;
  return SMG_OK;
}

// smg_lookup.hpp: filter the partitioned requests against `map`; list = false: look the survivors up at once
static int lookup_probe(smg_engine *e, const uint32_t *map, bool list, unsigned maxout, char *errbuf, size_t errlen)
{ const bool two = e->run.bm2 != 0;                             // (a map that came from outside was built by the same rule)
  unsigned grid = (unsigned) e->cus;
  const unsigned nbk = 1u << e->run.lg.nb;
  FastArgs a = make_fast(e);
  // The fused probe + look-up of a single shard has two forms.  kl_probe (a bucket per workgroup, the bucket's map folded
  // into LDS) is the faster one on a table without long window blocks: 2.5 against 2.7 ms at 2.5e9 entries.  kl_probe_x
  // (XCD by XCD straight from the full-resolution map, small independent workgroups) does not care how long a look-up
  // takes: with 5 % repeats in the genome the survivors' look-ups bisect directory buckets of thousands of k-mers, the
  // sixteen waves of a kl_probe workgroup wait for each other at every bucket, and it takes 4.5 ms against 2.9.  The
  // share of deferred entries that pass 1 reported tells the two kinds of table apart (0.13 % / 0.39 % in the two
  // bench workloads); SMG_PROBE_X=0/1 overrides.
  { const char *px = test_hook("SMG_PROBE_X");
    // ... and so does the share of entries that sent a request: 17.5 % on the diploid tables, a third on the polyploid ones, where
    // one request in seven survives the filter (2.5e7 look-ups at 6.4e8 entries) and kl_probe_x is 7-8 % ahead as well
    // (a one-way run sends one request per complement class: half the share says the same about the table)
    const int64_t share = e->run.one_way ? 14 : 28;
    const bool auto_x = (e->st.nbig > 0 && e->st.nbig * 400 > e->tab.n) || e->st.nemitted * 100 > e->tab.n * share;
    if (!list && e->run.lg.nb >= 3 && (px ? atoi(px) != 0 : auto_x))
      { HIPCHK(e->xtick.reserve((int64_t) PX_NXCD * PX_TICKW * 4));
        HIPCHK(hipMemsetAsync(e->xtick, 0, (size_t) PX_NXCD * PX_TICKW * 4, e->stream));
        // tickets of 2048 requests where many requests survive (polyploid tables: one in seven, all real hits -- half as many
        // buckets in flight per XCD keep more of a bucket's k-mer lines in reach: -0.25 ms on the hexaploid table), 4096 where the
        // kernel is mostly streaming (a table with repeats: 1 request in 50 survives, and a ticket's fixed cost shows: +0.5 ms at 2048)
        unsigned part = e->st.nemitted * 100 > e->tab.n * share ? PX_PART : 2 * PX_PART;
        if (test_hook("SMG_PX_ONE_XCC")) part |= 0x80000000u;                      // (tests: every workgroup claims XCD 0)
        const unsigned xg = grid * PX_WGS;
        with_bool(two, [&](auto t) { with_words<2>(e->run.rw, [&](auto rw)
          { hipLaunchKernelGGL((kl_probe_x<t(), rw()>), dim3(xg), dim3(PX_TPB), 0, e->stream, a, (const u64 *) e->req2,
                               (const u64 *) e->boff, map, e->run.lg, e->xtick, &e->ctrl->fast, part); }); });
        HIPCHK(hipGetLastError());
        e->run.probe_form = PROBE_X; e->run.probe_part = part & 0x7FFFFFFFu;
        return SMG_OK;
      }
  }
  if (grid > nbk) grid = nbk;
  u64 *const out = list ? (u64 *) e->reqf : (u64 *) NULL;                  // (the fused form keeps no survivor list)
  uint32_t *const fill = list ? (uint32_t *) e->chunk_fillf : (uint32_t *) NULL;
  with_bool(list, [&](auto l) { with_bool(two, [&](auto t) { with_words<2>(e->run.rw, [&](auto rw)
    { hipLaunchKernelGGL((kl_probe<l(), t(), rw()>), dim3(grid), dim3(PB_TPB), 0, e->stream, a, (const u64 *) e->req2, (const u64 *) e->boff,
                         map, e->run.lg, e->ghist + L_BK, out, fill, list ? maxout : 0u, &e->ctrl->fast); }); }); });
  HIPCHK(hipGetLastError());
  e->run.probe_form = list ? PROBE_LIST : PROBE_FUSED; e->run.probe_part = 0;
  return SMG_OK;
}

// drop the requests whose target window block holds no candidate (kf_filter); map = NULL: this engine's own map
static int fast_filter(smg_engine *e, const uint32_t *map, char *errbuf, size_t errlen)
{ int rc;
  if (!filter_ok(e) || e->run.n_chunks == 0) return SMG_OK;
  if (!map) map = e->run.bm_bits ? e->bmap : NULL;
  if (!map) return SMG_OK;
  const int nbits = bm_id_bits(e->tab.kmer, e->set.bm_cap);
  // two workgroups per CU, chunks dealt round-robin: the chunks in flight then span one or two of the 256 sorted
  // buckets, i.e. <= 1 MB of the map (measured: 512 workgroups 3.0 ms, 256 / 1024 / 2048 workgroups 3.4-3.7 ms)
  unsigned grid = 2u * (unsigned) e->cus;
  if (grid > e->run.n_chunks) grid = e->run.n_chunks;
  { const char *v = test_hook("SMG_FILTER_GRID"); if (v && atoi(v) >= 1 && (unsigned) atoi(v) < grid) grid = (unsigned) atoi(v); }
  unsigned maxout = e->run.n_chunks + grid + 16;
  if (e->run.lg.nb)
    { // kl_probe: every wave of every workgroup (one per CU, lookup_probe) fills chunks of its own, each to the brim
      // but for the < 64 records that did not fit: size the list from the launch and the request count, not from 256 CUs
      const int64_t need = (int64_t) e->cus * PB_WAVES + e->st.nrequests / (F_CH - 63) + 16;
      maxout = need < 0x7FFFFFFFll ? (unsigned) need : 0x7FFFFFFFu;
      if (maxout < e->run.n_chunks + 16) maxout = e->run.n_chunks + 16;
    }
  // (the two chunk lists swap roles after every filter: keep them the same size, or pass 1 would reallocate)
  { int64_t want = (int64_t) maxout * F_CH * (int64_t) sizeof(u64) * e->run.rw, wantf = (int64_t) maxout * 4 + 4;
    if (want < (int64_t) e->req.bytes) want = (int64_t) e->req.bytes;
    if (wantf < (int64_t) e->chunk_fill.bytes) wantf = (int64_t) e->chunk_fill.bytes;
    HIPCHK(e->reqf.reserve(want));
    HIPCHK(e->chunk_fillf.reserve(wantf));
  }
  if (e->rp.active)
    { // replayed step: WHICH chunks the waves of the probe kernel fill is decided by an atomic counter, and how many by the
      // way the buckets fall to the workgroups -- so the routing kernels walk the whole list, and a chunk nobody opened must
      // read as empty
      hipEventRecord(e->ev[EV_REPLAY_FILTER_BEG], e->stream);
      // (as many chunks as the recorded step's filter filled, and some: the device checks that this step stayed inside)
      if (e->rp.seen_chunks + 64u < maxout) maxout = e->rp.seen_chunks + 64u;
      HIPCHK(hipMemsetAsync(e->chunk_fillf, 0, (size_t) maxout * 4, e->stream));
    }
  if (!e->run.presorted && (rc = filter_presort(e, errbuf, errlen))) return rc;
  const int64_t nslots = (int64_t) e->run.n_chunks * F_CH;
  if (e->run.presorted == PRESORT_CHAIN)
    { if ((rc = lookup_probe(e, map, true, maxout, errbuf, errlen))) return rc; }
  else if (e->run.presorted == PRESORT_BUCKETED)
    hipLaunchKernelGGL(kf_filter<1>, dim3(grid), dim3(F_TPB), 0, e->stream, e->req2, (const uint32_t *) NULL, e->run.n_chunks, nslots,
                       map, 64 - nbits, e->reqf, e->chunk_fillf, maxout, &e->ctrl->fast);
  else
    with_words<4>(e->run.rw, [&](auto rw) { hipLaunchKernelGGL(kf_filter<rw()>, dim3(grid), dim3(F_TPB), 0, e->stream, e->req, e->chunk_fill, e->run.n_chunks, (int64_t) 0,
        map, 64 - nbits, e->reqf, e->chunk_fillf, maxout, &e->ctrl->fast); });
  hipEventRecord(e->ev[EV_LOOKUP_END], e->stream);
  HIPCHK(hipGetLastError());
  if (e->rp.active)
    { // replayed step: the kept list is as long as last time (the device checks it: smg_engine_proof) -- nothing is read
      hipEventRecord(e->ev[EV_REPLAY_FILTER_END], e->stream);
      e->rp.nf_chunks = maxout;             // (the device checks that the probe kernel stayed inside the list)
    }
  else
    { if ((rc = read_ctrl(e, errbuf, errlen))) return rc;
      if (e->h_ctrl->fast.nf_chunks > maxout) return fail(errbuf, errlen, SMG_ENODEV, "request filter overflowed its chunk list%s");
    }
  e->req.swap(e->reqf); e->chunk_fill.swap(e->chunk_fillf);
  if (e->rp.active)
    { e->run.n_chunks = e->rp.nf_chunks; e->st.nrequests = e->rp.nf_req; e->run.filtered = true;
      return SMG_OK;
    }
  e->run.n_chunks = e->h_ctrl->fast.nf_chunks;
  e->st.nrequests = (int64_t) e->h_ctrl->fast.nf_req;
  e->run.filtered = true;
  e->st.ms_filter = ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
  e->st.ms_rclookup += e->st.ms_filter;
  // what a replayed step on this table may take for granted (key-only records through the look-up chain, k <= 64)
  e->rp.have = e->set.rp_want && e->run.presorted == PRESORT_CHAIN && e->tab.W <= 2 && e->run.rw == e->tab.W;
  if (e->rp.have)
    { e->rp.nreq = e->st.nemitted; e->rp.nbig = e->st.nbig; e->rp.nf_req = e->st.nrequests; e->rp.bm_bits = e->run.bm_bits;
      e->rp.seen_chunks = e->run.n_chunks; e->rp.nranks = 0;
    }
  return SMG_OK;
}

// squeeze the request chunks (ragged fills) into the dense array e->dense: exclusive scan of the fills + one copy
static int compact_chunks(smg_engine *e, int64_t nreq, char *errbuf, size_t errlen)
{ HIPCHK(e->dense.reserve(nreq * (int64_t) sizeof(u64) * e->run.rw));
  HIPCHK(e->chunk_off.reserve((int64_t) e->run.n_chunks * 4 + 4));
  HIPCHK(with_scratch(e->sort_tmp, [&](void *tmp, size_t &bytes)
    { return rocprim::exclusive_scan(tmp, bytes, (uint32_t *) e->chunk_fill, (uint32_t *) e->chunk_off, 0u, (size_t) e->run.n_chunks,
                                     rocprim::plus<uint32_t>(), e->stream); }));
  hipLaunchKernelGGL(kf_compact, dim3(e->run.n_chunks), dim3(F_TPB), 0, e->stream, e->req, e->chunk_fill, e->chunk_off, e->run.rw, e->dense);
  return SMG_OK;
}

// look-ups of this engine's own request chunks (flat = NULL; filtered first if a block map was built) or of a flat
// array of received records
static int fast_apply(smg_engine *e, const u64 *flat, int64_t nflat, int check_count, int64_t *missing,
                      char *errbuf, size_t errlen)
{ int rc = SMG_OK;
  e->run.ap = ApplyState{};
  if (!flat && e->run.lg.nb && e->run.bm_bits && !e->run.filtered)
    { // own requests, own map: partition, then filter and look-ups in one kernel (no survivor list, no sort)
      if (e->run.n_chunks == 0 || e->st.nrequests == 0) { if (missing) *missing = 0; return SMG_OK; }
      if (!e->run.presorted && (rc = filter_presort(e, errbuf, errlen))) return rc;
      hipEventRecord(e->ev[EV_PROBE_BEG], e->stream);
      if ((rc = lookup_probe(e, e->bmap, false, 0u, errbuf, errlen))) return rc;
      hipEventRecord(e->ev[EV_LOOKUP_END], e->stream);
      if ((rc = read_ctrl(e, errbuf, errlen))) return rc;
      e->st.ms_filter = ms_between(e, EV_LOOKUP_BEG, EV_PROBE_BEG);       // scan + partition
      e->st.ms_rclookup += ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
      e->st.nrequests = (int64_t) e->h_ctrl->fast.nf_req;
      e->run.filtered = true;
      e->run.n_chunks = 0;                                            // nothing left to route or to look up
      if (missing) *missing = e->h_ctrl->fast.missing;
      return SMG_OK;
    }
  if (!flat && e->run.bm_bits && !e->run.filtered && (rc = fast_filter(e, NULL, errbuf, errlen))) return rc;
  hipEventRecord(e->ev[EV_LOOKUP_BEG], e->stream);
  const bool keys_only = e->tab.W == 1 && e->run.rw == 1;
  const int64_t nreq = e->st.nrequests;
  if (flat)
    { if (nflat > 0) rc = keys_only ? apply_sorted(e, flat, nflat, 0, errbuf, errlen) : apply_indexed(e, flat, nflat, check_count, errbuf, errlen); }
  else if (nreq > 0 && e->run.n_chunks > 0)
    { const int64_t nslots = (int64_t) e->run.n_chunks * F_CH;
      if (keys_only && nslots <= nreq + nreq / 8 && nslots >= SORT_MIN && e->tab.kmer < 32)
        { // nearly every chunk is full (pass 1 and the filter split their batches): sort the chunk array as it is,
          // holes as sentinels behind the requests, instead of compacting it first
          hipLaunchKernelGGL(kf_fill_holes, dim3(e->run.n_chunks), dim3(F_TPB), 0, e->stream, e->req, e->chunk_fill);
          rc = apply_sorted(e, e->req, nslots, 1, errbuf, errlen);
          e->run.ap.holes = HOLES_SENTINELS;
        }
      else
        { // ragged chunks, k = 32 (the all-T k-mer equals the sentinel) or records with a count/flag word
          // (W > 1, exact proof): compact, then sorted (keys) or index-sorted (records) look-ups
          if ((rc = compact_chunks(e, nreq, errbuf, errlen))) return rc;
          rc = keys_only ? apply_sorted(e, e->dense, nreq, 0, errbuf, errlen) : apply_indexed(e, e->dense, nreq, check_count, errbuf, errlen);
          e->run.ap.holes = HOLES_COMPACTED;
        }
    }
  if (rc) return rc;
  hipEventRecord(e->ev[EV_LOOKUP_END], e->stream);
  HIPCHK(hipGetLastError());
  if (!missing && flat)                   // (sharded run: the count of missing complements stays on the device -- smg_engine_proof)
    { e->run.lookup_pending = true; return SMG_OK; }
  rc = read_ctrl(e, errbuf, errlen);
  if (rc) return rc;
  e->st.ms_rclookup += ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
  if (missing) *missing = e->h_ctrl->fast.missing;
  return SMG_OK;
}

static int fast_pass2(smg_engine *e, int64_t *d_plot, bool with_sum, char *errbuf, size_t errlen)
{ HIPCHK(hipMemsetAsync(d_plot, 0, sizeof(int64_t) * SMG_PLOT_CELLS, e->stream));
  FastArgs a = make_fast(e);
  hipEventRecord(e->ev[EV_PASS2_BEG], e->stream);
  if (e->tab.n > 0)
    { int64_t nb = (e->tab.n + P2_TPB - 1) / P2_TPB;
      if (nb > P2_GRID) nb = P2_GRID;
      { const char *v = test_hook("SMG_P2_GRID"); if (v && atoi(v) >= 1 && atoi(v) <= P2_GRID && atoi(v) < nb) nb = atoi(v); }
      with_words<3>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_pass2<w()>, dim3((unsigned) nb), dim3(P2_TPB), 0, e->stream, a, (u64 *) d_plot); });
      // entries whose unique partner is out of the code's reach: from the list of deferred entries that pass 1 of one-
      // and two-word k-mers leaves, else (three words: the generic pass 1) from a scan of the code bytes
      if (e->run.far_listed && e->tab.W <= 2)
        { const unsigned nl = (unsigned) e->st.nbig;
          unsigned fb = (nl + 255) / 256;
          if (fb > 4096) fb = 4096;
          if (nl)
            with_words<2>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_pass2_far<w()>, dim3(fb), dim3(256), 0, e->stream, a, (const uint32_t *) e->biglist,
                (const uint32_t *) e->farp, nl, (u64 *) d_plot); });
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

// ---- public phase API (sharded runs) ------------------------------------------------------------
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
  if (!ok) { e->rp.have = false; e->dbits_dirty = true; e->run.lookup_pending = false; return SMG_OK; }
  int rc = read_ctrl(e, errbuf, errlen);
  if (rc) return rc;
  e->dbits_dirty = false;
  fold_fp(e, e->rp.grid);
  e->st.ms_pass1 = ms_between(e, EV_PASS1_BEG, EV_PASS1_END);
  e->st.ms_bigfix = ms_between(e, EV_DECODE_BEG, EV_PASS1_END);
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
      x.totals = e->rp.routed ? e->rp_totals : (const u64 *) NULL; x.nranks = e->rp.nranks;     // (not routed: nothing to vouch for the split)
      hipLaunchKernelGGL(k_proof_replay, dim3(1), dim3(64), 0, e->stream, (const Ctrl *) e->ctrl, (const u64 *) e->partials, x, d_dst);
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
  u64 *tmp = e->partials + (size_t) 4 * P1_MAXGRID;           // (the row behind the workgroups' partial sums)
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
  if (!ran_fast(e)) return counted_phase_apply(e, e->req, e->st.nrequests, missing, errbuf, errlen);
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
static int route_records(smg_engine *e, const u64 *req, const uint32_t *chunk_fill, unsigned nc, int rw,
                         const uint64_t *splitters, int nranks, uint64_t *d_send, int64_t capacity, int64_t *counts,
                         char *errbuf, size_t errlen, int64_t *d_counts = NULL /* device: the totals stay there, no host wait */)
{ if (counts) for (int r = 0; r < nranks; r++) counts[r] = 0;
  if (nc == 0)
    { if (d_counts) HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * nranks, e->stream));
      return SMG_OK;
    }
  if (nranks > 1)
    HIPCHK(hipMemcpyAsync(e->d_split, splitters, sizeof(u64) * (nranks - 1) * e->tab.W,
                          hipMemcpyHostToDevice, e->stream));
  HIPCHK(e->route_cnt.reserve((int64_t) nc * nranks * 4));
  HIPCHK(e->route_off.reserve(((int64_t) nc * nranks + 16) * 8));
  u64 *totals = e->route_off + (size_t) nc * nranks;           // [nranks], behind the offsets
  with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_route_count<w()>, dim3(nc), dim3(F_TPB), 0, e->stream, req,
      chunk_fill, rw, e->d_split, nranks, e->route_cnt); });
  // offsets and scatter follow on the device; the host only learns the totals (what the exchange needs): ONE round trip
  hipLaunchKernelGGL(kf_route_offsets, dim3(nranks), dim3(1024), 0, e->stream, (const uint32_t *) e->route_cnt, nc, nranks, e->route_off, totals);
  with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_route_scatter<w()>, dim3(nc), dim3(F_TPB), 0, e->stream, req,
      chunk_fill, rw, e->d_split, nranks, (const u64 *) e->route_off, (const u64 *) totals, (u64 *) d_send,
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

extern "C" int smg_engine_route(smg_engine *e, const uint64_t *splitters, int nranks,
                                uint64_t *d_send, int64_t capacity, int64_t *counts,
                                char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!counts || nranks < 1 || nranks > 16)
    return fail(errbuf, errlen, SMG_EINVAL, "bad route arguments (1..16 ranks)%s");
  if (!e->run.pass1_done) return fail(errbuf, errlen, SMG_EINVAL, "route before pass1%s");
  if (e->run.one_way) return fail(errbuf, errlen, SMG_EINVAL, "one-way requests cannot be routed: their senders are local to this engine%s");
  HIPCHK(hipSetDevice(e->device));
  if (e->st.nrequests > capacity) return fail(errbuf, errlen, SMG_EINVAL, "send buffer too small%s");
  return route_records(e, e->req, e->chunk_fill, e->run.n_chunks, e->run.rw, splitters, nranks, d_send, capacity, counts, errbuf, errlen);
}

extern "C" int smg_engine_route_device(smg_engine *e, const uint64_t *splitters, int nranks, uint64_t *d_send, int64_t capacity,
                                       int64_t *d_counts, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (!d_counts || nranks < 1 || nranks > 16)
    return fail(errbuf, errlen, SMG_EINVAL, "bad route arguments (1..16 ranks)%s");
  if (!e->run.pass1_done) return fail(errbuf, errlen, SMG_EINVAL, "route before pass1%s");
  if (e->run.one_way) return fail(errbuf, errlen, SMG_EINVAL, "one-way requests cannot be routed: their senders are local to this engine%s");
  HIPCHK(hipSetDevice(e->device));
  if (e->st.nrequests > capacity) return fail(errbuf, errlen, SMG_EINVAL, "send buffer too small%s");
  int rc = route_records(e, e->req, e->chunk_fill, e->run.n_chunks, e->run.rw, splitters, nranks, d_send, capacity, NULL, errbuf, errlen, d_counts);
  if (rc || !e->set.rp_want || !ran_fast(e)) return rc;
  // replay: the per-destination totals of a plain step are kept, those of a replayed step are put beside them -- the verdict
  // kernel (smg_engine_proof) compares the two: the caller splits its exchange by the RECORDED totals
  if (!e->rp_totals) HIPCHK(e->rp_totals.alloc(sizeof(u64) * 32));
  const bool rep = e->rp.active;
  if (rep && e->rp.nranks != nranks) { e->rp.routed = false; return SMG_OK; }
  HIPCHK(hipMemcpyAsync(e->rp_totals + (rep ? 16 : 0), d_counts, sizeof(u64) * nranks, hipMemcpyDeviceToDevice, e->stream));
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

extern "C" int smg_engine_run(smg_engine *e, int symcheck, int64_t *d_plot, smg_stats *stats,
                              char *errbuf, size_t errlen)
{ if (!e || !d_plot) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  HIPCHK(hipSetDevice(e->device));
  int rc;
  hipEventRecord(e->ev[EV_RUN_BEG], e->stream);
  e->st.ms_pass1 = e->st.ms_rclookup = e->st.ms_pass2 = 0;
  bool symmetric = false;
  if (symcheck != SMG_SYM_NONE && e->tab.kmer <= FAST_MAX_K)
    { // hash : requests from the entries that own a hi-side pair; closure proven by the fingerprint
      // exact: EVERY entry sends (rc(kmer), count) and the look-up compares the count -- the same records the
      //        sharded protocol exchanges, index-sorted look-ups (kf_apply_indexed)
      const int exact = symcheck == SMG_SYM_EXACT;
      e->set.bm_cap = 32;
      // (Rounds 3-5 queued a re-run on the same table from the counts of the run before -- "run_speculative", one host wait
      //  instead of four.  Measured twice without a gain, 17.94 against 17.7-18.0 ms per step, profiles/r05_lookup_experiments.txt:
      //  taken out in round 6.  The one mechanism of that kind left is the replayed step of the phase API, for sharded runs.)
      rc = fast_pass1(e, exact, exact, symcheck == SMG_SYM_HASH, errbuf, errlen, false, symcheck == SMG_SYM_HASH);
      if (rc) return rc;
      int64_t missing = 0;
      if ((rc = fast_apply(e, NULL, 0, exact, &missing, errbuf, errlen))) return rc;
      symmetric = (missing == 0);
      if (symmetric && symcheck == SMG_SYM_HASH)
        symmetric = e->run.fp[0] == e->run.fp[2] && e->run.fp[1] == e->run.fp[3];
      if (symmetric && (rc = fast_pass2(e, d_plot, true, errbuf, errlen))) return rc;
    }
  else if (symcheck != SMG_SYM_NONE)
    { if ((rc = counted_symmetric(e, symcheck, d_plot, &symmetric, errbuf, errlen))) return rc; }
  if (!symmetric && (rc = run_general(e, d_plot, errbuf, errlen))) return rc;
  hipEventRecord(e->ev[EV_RUN_END], e->stream);
  HIPCHK(hipStreamSynchronize(e->stream));
  e->st.ms_total = ms_between(e, EV_RUN_BEG, EV_RUN_END);
  if (stats) *stats = e->st;
  return SMG_OK;
}

#include "smg_condition.hpp"

// ---- extract: the unique pairs of the labelled pixels (next row of the scope table: extract_kmer_pairs) ------

// d_set: the shard set of a general run over virtual shards (smg_multi.hpp), NULL otherwise
static int engine_extract(smg_engine *e, const uint16_t *d_labels, uint64_t *d_out, int64_t capacity, int64_t *nrec,
                          const TabSet *d_set, char *errbuf, size_t errlen)
{ if (!e || !d_labels || !nrec) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  const bool general = ran_general(e);        // the table failed the proof: all positions
  const bool counted = ran_counted(e);        // k > 85: degrees instead of code bytes
  if (!e->run.completed)
    return fail(errbuf, errlen, SMG_EINVAL, "extract needs a completed run on the engine's current table%s");
  HIPCHK(hipSetDevice(e->device));
  u64 *d_total = &e->ctrl->plot_sum;
  HIPCHK(hipMemsetAsync(d_total, 0, sizeof(u64), e->stream));
  hipEventRecord(e->ev[EV_EXTRACT_BEG], e->stream);
  if (e->tab.n > 0 && general)
    { Tab t = make_tab(e);
      const unsigned nblk = (unsigned) ((e->tab.n + TPB - 1) / TPB);
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(k_extract_general<w()>, dim3(nblk), dim3(TPB), 0, e->stream, t, d_labels, (u64 *) d_out,
          (u64) (d_out ? capacity : 0), d_total, d_set); });
    }
  else if (e->tab.n > 0 && counted)
    { Tab t = make_tab(e);
      const unsigned nblk = (unsigned) ((e->tab.n + TPB - 1) / TPB);
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(k_extract<w()>, dim3(nblk), dim3(TPB), 0, e->stream, t, d_labels, (u64 *) d_out,
          (u64) (d_out ? capacity : 0), d_total); });
    }
  else if (e->tab.n > 0)
    { FastArgs a = make_fast(e);
      int64_t nb = (e->tab.n + F_TPB - 1) / F_TPB;
      if (nb > EX_GRID) nb = EX_GRID;
      { const char *v = test_hook("SMG_EXTRACT_GRID"); if (v && atoi(v) >= 1 && atoi(v) <= EX_GRID && atoi(v) < nb) nb = atoi(v); }
      with_words<3>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kf_extract<w()>, dim3((unsigned) nb), dim3(F_TPB), 0, e->stream, a, d_labels,
          (u64 *) d_out, (u64) (d_out ? capacity : 0), d_total); });
    }
  hipEventRecord(e->ev[EV_EXTRACT_END], e->stream);
  HIPCHK(hipGetLastError());
  int rc = read_ctrl(e, errbuf, errlen);
  if (rc) return rc;
  e->ms_extract = ms_between(e, EV_EXTRACT_BEG, EV_EXTRACT_END);
  *nrec = (int64_t) e->h_ctrl->plot_sum;
  return SMG_OK;
}

extern "C" int smg_engine_extract(smg_engine *e, const uint16_t *d_labels, uint64_t *d_out, int64_t capacity,
                                  int64_t *nrec, char *errbuf, size_t errlen)
{ return engine_extract(e, d_labels, d_out, capacity, nrec, NULL, errbuf, errlen); }

extern "C" void smg_engine_pass2_limits(int32_t out[8])
{ const int32_t v[8] = { P2_TILE, P2_QCAP, P2_FAR, P2_SMAX, P2_GRID, EX_STAGE, F_TPB, EX_GRID };
  memcpy(out, v, sizeof(v));
}

extern "C" void smg_engine_lookup_limits(int32_t out[12])
{ const int32_t v[12] = { F_CH, PT_LDSREC, PT_LDSREC / 2, PB_WAVES * 64 * PB_PER, PB_WQ, PX_PART, PX_TPB / 64 * 64 * PX_PER,
                          L_NB_MAX, L_SLICE_LG, BF_MAXGRID, LW_SL, LW_UNR };
  memcpy(out, v, sizeof(v));
}

extern "C" void smg_engine_pass1_limits(int32_t out[4])
{ const int32_t v[4] = { D_OWN, D_LEAD, D_SLOTS, D_WIN };
  memcpy(out, v, sizeof(v));
}

extern "C" void smg_engine_wide_limits(int32_t out[8])
{ const int32_t v[8] = { F_TILE, F_HALO, F_CH, F_FSTAGE, SORT_MIN, CODE_REACH, BB_LIN, BB_STEP };
  memcpy(out, v, sizeof(v));
}

extern "C" void smg_engine_list_limits(int32_t out[4])
{ const int32_t v[4] = { SORT_MIN, APPLY_SORT_MIN, FILTER_SORT_MIN, F_CH };
  memcpy(out, v, sizeof(v));
}

extern "C" int smg_engine_apply_state(smg_engine *e, int64_t out[6])
{ if (!e || !out) return SMG_EINVAL;
  const ApplyState &ap = e->run.ap;
  out[0] = ap.kernel; out[1] = ap.sorted; out[2] = ap.holes; out[3] = ap.covered; out[4] = ap.sig; out[5] = e->run.presorted;
  return SMG_OK;
}

extern "C" int smg_engine_lookup_state(smg_engine *e, int64_t out[10])
{ if (!e || !out) return SMG_EINVAL;
  const bool chain = has_chain(e);
  out[0] = e->run.pass1_done ? e->run.bm_bits : 0; out[1] = chain ? e->run.lg.nb : 0; out[2] = e->run.bm2; out[3] = e->run.one_way; out[4] = e->run.rw;
  const bool fast = ran_fast(e);                                 // (three-word k-mers run pass 1 in chunks too, without the chain)
  out[5] = fast ? e->run.p1grid : 0; out[6] = chain ? e->run.nown : 0;
  out[7] = fast ? (int64_t) e->h_ctrl->fast.n_chunks : 0;        // (pass 1's counter: the filter counts in nf_chunks)
  out[8] = e->run.probe_form; out[9] = e->run.probe_part;
  return SMG_OK;
}

extern "C" int smg_engine_pass1_form(smg_engine *e, int32_t out[4])
{ if (!e || !out) return SMG_EINVAL;
  const bool ran = ran_fast(e);
  out[0] = ran ? e->run.p1_var : 0; out[1] = ran ? e->run.p1_w : 0; out[2] = ran ? e->run.p1_rw : 0;
  out[3] = 0;                                // (no launch is an INNER-only grid)
  return SMG_OK;
}

#include "smg_ingest.hpp"
#include "smg_shards.hpp"
#include "smg_multi.hpp"

// ---- one-shot host entry ----------------------------------------------------------------------

#define SECS(a, b) ((double) ((b).tv_sec - (a).tv_sec) + 1e-9 * (double) ((b).tv_nsec - (a).tv_nsec))

// the table in core on one device: ingest, condition or take the index, run, and -- labels != NULL -- the extract leg.
// w0: when the call began (the wall-time line of the verbose output).
static int host_run_core(const smg_table_source *tv, const smg_opts *opts, int64_t *plot, smg_stats *stats, const uint16_t *labels,
                         uint64_t **records, int64_t *nrec, int *rec_words, const struct timespec &w0, char *errbuf, size_t errlen)
{ const int device = opts ? opts->device : 0;
  const int symcheck = opts ? opts->symcheck : SMG_SYM_EXACT;
  const int pbyte = ((tv->kmer + 3) >> 2) + 2 - tv->ibyte;
  struct timespec w1, w2;
  EngineOwner eng;                           // (in front of the buffers: destroyed after them)
  smg_engine *e = eng.create(device, errbuf, errlen);
  if (!e) return SMG_ENODEV;
  clock_gettime(CLOCK_MONOTONIC, &w1);       // (the first HIP call of the process: runtime start-up + code object load)
  int rc = SMG_OK;
  DevBuf<int64_t> d_index, d_plot;
  const size_t ixbytes = sizeof(int64_t) << (8 * tv->ibyte);
  double h2d_s = 0, alloc_s = 0, cond_s = 0, run_s = 0, out_s = 0;
  if (d_index.alloc(ixbytes) != hipSuccess || d_plot.alloc(sizeof(int64_t) * SMG_PLOT_CELLS) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory for the table%s");
  // the index goes first (asynchronously from pageable memory: staged by the runtime); the records stream behind it,
  // piece by piece through a pinned ring, and every piece is decoded on the device as soon as its copy has landed
  if (hipMemcpyAsync(d_index, tv->prefix_index, ixbytes, hipMemcpyHostToDevice, e->stream) != hipSuccess
      || hipEventRecord(e->ev[EV_DECODE_BEG], e->stream) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENODEV, "host to device copy failed%s");
  if ((rc = ingest_range(e, tv, 0, tv->nels, d_index, device, tv->host_threads, &h2d_s, e->ev[EV_DECODE_BEG], errbuf, errlen))) return rc;
  clock_gettime(CLOCK_MONOTONIC, &w2);
  alloc_s = SECS(w1, w2) - h2d_s;            // (the engine's table is allocated inside ingest_range, in front of the first copy)
  if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(errbuf, errlen, SMG_ENODEV, "host to device copy failed%s");
  clock_gettime(CLOCK_MONOTONIC, &w1);
  if (opts && opts->condition)
    rc = smg_engine_condition(e, opts->ethresh, opts->condition & SMG_COND_TRIM, opts->condition & SMG_COND_SYMM, NULL, errbuf, errlen);
  else rc = smg_engine_set_prefix_index(e, d_index, tv->ibyte, 0, errbuf, errlen);   // the table's index = its directory
  if (rc) return rc;
  clock_gettime(CLOCK_MONOTONIC, &w2); cond_s = SECS(w1, w2);
  if ((rc = smg_engine_run(e, symcheck, d_plot, NULL, errbuf, errlen))) return rc;
  clock_gettime(CLOCK_MONOTONIC, &w1); run_s = SECS(w2, w1);
  if (hipMemcpy(plot, d_plot, sizeof(int64_t) * SMG_PLOT_CELLS, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENODEV, "device to host copy failed%s");
  if (labels)
    { // one launch: the number of records is known, it is the plot's weight on the labelled pixels
      DevBuf<uint16_t> d_labels;
      std::vector<uint64_t> rec;
      if ((rc = upload_labels(labels, d_labels, errbuf, errlen))) return rc;
      if ((rc = extract_to_host(e, d_labels, NULL, pair_weight(labels, plot), rec, errbuf, errlen))) return rc;
      if ((rc = records_to_caller(rec, e->tab.W + 1, labels, plot, records, nrec, rec_words, errbuf, errlen))) return rc;
    }
  clock_gettime(CLOCK_MONOTONIC, &w2); out_s = SECS(w1, w2);
  e->st.ms_h2d = h2d_s * 1e3;
  if (stats) *stats = e->st;
  if (opts && opts->verbose)
    { fprintf(stderr, "  [smg] n=%lld k=%d path=%s  read+h2d+decode %.2f ms (%.1f GB/s, %d readers; the decode of a piece runs behind its copy), "
              "pass1 %.2f, rc-lookup %.2f, pass2 %.2f, total(device) %.2f ms => %.3g k-mers/s\n",
              (long long) e->st.nels, tv->kmer, e->st.path == 1 ? "rc-half-scan" : "general",
              e->st.ms_h2d, h2d_s > 0 ? (double) tv->nels * pbyte / h2d_s / 1e9 : 0.0, tv->host_threads > 0 ? tv->host_threads : 4,
              e->st.ms_pass1, e->st.ms_rclookup, e->st.ms_pass2,
              e->st.ms_total, e->st.ms_total > 0 ? e->st.nels / (e->st.ms_total * 1e-3) : 0.0);
      if (labels)
        fprintf(stderr, "  [smg] extract %.2f ms (device), %lld records\n", e->ms_extract, (long long) *nrec);
      // where the wall time of this call went (the process adds its own start-up, the table probe and the .smu writer)
      fprintf(stderr, "  [smg] wall %.1f ms: runtime start-up + code object %.1f, allocations + index %.1f, read+h2d+decode %.1f, "
              "conditioning %.1f, passes + host round trips %.1f, results %.1f\n",
              SECS(w0, w2) * 1e3, (SECS(w0, w2) - alloc_s - h2d_s - cond_s - run_s - out_s) * 1e3, alloc_s * 1e3, h2d_s * 1e3,
              cond_s * 1e3, run_s * 1e3, out_s * 1e3);
    }
  return SMG_OK;
}

// ---- one-shot host entry ----------------------------------------------------------------------
// validate, plan (run_mode_plan, smg_shards.hpp), dispatch to the shard drivers (smg_multi.hpp) -- or run in core.
// labels == NULL: hetmers.  labels != NULL: additionally the extract leg; *records receives a malloc'ed
// array of *nrec records of (words + 1) uint64 each.
static int host_run(const smg_table_source *tv, const smg_opts *opts, int64_t *plot, smg_stats *stats,
                    const uint16_t *labels, uint64_t **records, int64_t *nrec, int *rec_words,
                    char *errbuf, size_t errlen)
{ if (!tv || !plot || !tv->read) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  struct timespec w0;
  clock_gettime(CLOCK_MONOTONIC, &w0);       // (the first HIP call of the process -- the plan's free-memory query -- starts the runtime)
  const int verbose = opts ? opts->verbose : 0;
  if (tv->ibyte < 1 || tv->ibyte > 3) return fail(errbuf, errlen, SMG_EINVAL, "ibyte must be 1, 2 or 3%s");
  if (((tv->kmer + 3) >> 2) + 2 - tv->ibyte < 3) return fail(errbuf, errlen, SMG_EINVAL, "k-mer shorter than the index prefix%s");
  int64_t sum = 0;
  for (int p = 0; p < tv->nparts; p++) sum += tv->part_nels[p];
  if (sum != tv->nels) return fail(errbuf, errlen, SMG_EFORMAT, "part sizes do not add up to nels%s");
  RunMode m;
  int rc = run_mode_plan(tv->kmer, tv->nels, opts ? opts->ngpus : 0, opts ? opts->condition : 0, opts ? opts->symcheck : SMG_SYM_EXACT,
                         opts ? opts->device : 0, 0, &m, errbuf, errlen);
  if (verbose && m.cut_by_limit)
    fprintf(stderr, "  [smg] %lld entries%s: %d prefix shards on one device\n", (long long) tv->nels,
            opts && (opts->condition & SMG_COND_SYMM) ? " before the table is symmetrised" : "", m.cut_by_limit);
  if (rc) return rc;
  if (m.mode == SMG_MODE_CORE) return host_run_core(tv, opts, plot, stats, labels, records, nrec, rec_words, w0, errbuf, errlen);
  smg_opts o; memset(&o, 0, sizeof(o));
  if (opts) o = *opts; else o.symcheck = SMG_SYM_HASH;
  if (m.mode == SMG_MODE_SEQUENTIAL)
    { if (verbose) fprintf(stderr, "  [smg] %lld entries do not fit the device together: %d prefix shards one after the other\n",
                           (long long) tv->nels, m.count);
      return host_run_sequential(tv, &o, m.count, plot, stats, errbuf, errlen, labels, records, nrec, rec_words);
    }
  rc = host_run_multi(tv, &o, m.count, m.mode == SMG_MODE_VIRTUAL, plot, stats, errbuf, errlen, labels, records, nrec, rec_words);
  // a table that fails the symmetry proof: shards on ONE device run the general path together (smg_multi.hpp,
  // TabSet); several real GPUs hand the table to one of them, which can hold it as long as it has < 2^32 entries
  if (rc != SMG_ENOTSYM) return rc;
  if (tv->nels >= SMG_ONE_SHARD_MAX)
    return fail(errbuf, errlen, SMG_ENOTSYM, "the table is not closed under reverse complement and has more than 2^32 entries: "
                "the general path for such a table runs on one device (unset SMUDGEPLOT_GPUS), or condition the table%s");
  if (verbose) fprintf(stderr, "  [smg] the table is not closed under reverse complement: general path on one GPU\n");
  return host_run_core(tv, opts, plot, stats, labels, records, nrec, rec_words, w0, errbuf, errlen);
}
#undef SECS

extern "C" int smg_hetmers_run(const smg_table_view *tv, const smg_opts *opts, int64_t *plot,
                               smg_stats *stats, char *errbuf, size_t errlen)
{ if (!tv) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  ViewCtx vc; smg_table_source src;
  view_source(tv, &vc, &src);
  return host_run(&src, opts, plot, stats, NULL, NULL, NULL, NULL, errbuf, errlen);
}

extern "C" int smg_hetmers_run_source(const smg_table_source *src, const smg_opts *opts, int64_t *plot,
                                      smg_stats *stats, char *errbuf, size_t errlen)
{ return host_run(src, opts, plot, stats, NULL, NULL, NULL, NULL, errbuf, errlen); }

// ---- one-shot entry: a table that is already on the device -> plot ------------------------------------------------------
// What smg_hetmers_run does behind its ingest, for the table the k-mer counter left in device memory (smg_count.h, the
// _device entries): bind, trim, close, run.  One device; in core, or -- a canonical table whose closure is beyond one engine
// or does not fit -- in prefix shards of the closed table one after the other (device_run_sequential, smg_multi.hpp).
// 1: a canonical table is closed by smg_engine_close_canonical, any other by the generic closure (same table either way).
// profiles/reads_to_smu.md: at 1e8 entries the merge takes 17.0 against 24.0 ms at k = 31 and 27.4 against 43.1 ms at k = 51;
// at 1e6 entries it is 0.1 - 0.2 ms behind.  0 takes the generic closure always.
#define RUN_DEVICE_CLOSE_BY_MERGE 1

extern "C" int smg_hetmers_run_device(int kmer, int64_t nels, const uint64_t *d_keys, const uint16_t *d_counts, const smg_opts *opts,
                                      int64_t *plot, smg_stats *stats, char *errbuf, size_t errlen)
{ if (!plot) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  const int device = opts ? opts->device : 0;
  const int symcheck = opts ? opts->symcheck : SMG_SYM_HASH;
  const int cond = opts ? opts->condition : 0;
  if (opts && opts->ngpus > 1)
    return fail(errbuf, errlen, SMG_EINVAL, "a table that is already on one device runs on that device only (ngpus > 1)%s");
  if (kmer < 1 || kmer > SMG_MAX_KMER) return fail(errbuf, errlen, SMG_EINVAL, "k-mer length out of range (1..128)%s");
  if (nels < 0) return fail(errbuf, errlen, SMG_EINVAL, "negative number of entries%s");
  // in core -- the closed table next to the lists of a run, or next to the buffers of its own closure -- or, where that is
  // refused and the table is to be closed, in prefix shards of the closed table one after the other (run_device_plan)
  RunMode mode;
  int rc = run_device_plan(kmer, nels, 0, cond, symcheck, device, 0, true, &mode, errbuf, errlen);
  if (rc) return rc;
  if (mode.mode == SMG_MODE_SEQUENTIAL)
    { smg_opts o = *opts;
      bool not_canonical = false;
      rc = device_run_sequential(kmer, nels, (const u64 *) d_keys, d_counts, &o, mode.count, plot, stats, &not_canonical, errbuf, errlen);
      if (!not_canonical) return rc;
      // not canonical: the generic closure, which runs in core or not at all -- as ever, whatever the hooks say
      if ((rc = run_device_plan(kmer, nels, 0, cond, symcheck, device, 0, false, &mode, errbuf, errlen))) return rc;
      if (mode.mode != SMG_MODE_CORE)
        return fail(errbuf, errlen, SMG_ENOMEM, mode.cut_by_limit ? "more than 2^32 - 32 entries in the closed table: one engine does not address them%s"
                    : "the table does not fit the device in core, and it is not canonical: no prefix shards%s", DEVICE_TWO_STEP);
    }
  EngineOwner eng;                           // (in front of the buffer: destroyed after it)
  smg_engine *e = eng.create(device, errbuf, errlen);
  if (!e) return SMG_ENODEV;
  DevBuf<int64_t> d_plot;
  if (d_plot.alloc(sizeof(int64_t) * SMG_PLOT_CELLS) != hipSuccess) return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory for the plot%s");
  if ((rc = smg_engine_bind(e, kmer, nels, d_keys, d_counts, errbuf, errlen))) return rc;
  if ((cond & SMG_COND_TRIM) && (rc = smg_engine_condition(e, opts->ethresh, 1, 0, NULL, errbuf, errlen))) return rc;
  if (cond & SMG_COND_SYMM)
    { bool generic = !RUN_DEVICE_CLOSE_BY_MERGE;
      if (!generic) rc = close_canonical(e, NULL, &generic, errbuf, errlen);     // (not canonical: left as it was, the generic closure takes it)
      if (generic) rc = smg_engine_condition(e, 0, 0, 1, NULL, errbuf, errlen);
      if (rc) return rc;
    }
  if ((rc = smg_engine_run(e, symcheck, d_plot, NULL, errbuf, errlen))) return rc;
  if (hipMemcpy(plot, d_plot, sizeof(int64_t) * SMG_PLOT_CELLS, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENODEV, "device to host copy failed%s");
  if (stats) *stats = e->st;
  if (opts && opts->verbose)
    fprintf(stderr, "  [smg] n=%lld k=%d path=%s  conditioning %.2f ms, pass1 %.2f, rc-lookup %.2f, pass2 %.2f, total(device) %.2f ms\n",
            (long long) e->st.nels, kmer, e->st.path == 1 ? "rc-half-scan" : "general", e->st.ms_decode, e->st.ms_pass1,
            e->st.ms_rclookup, e->st.ms_pass2, e->st.ms_total);
  return SMG_OK;
}

extern "C" int smg_hetmers_extract(const smg_table_view *tv, const smg_opts *opts, const uint16_t *labels,
                                   int64_t *plot, uint64_t **records, int64_t *nrec, int *rec_words,
                                   smg_stats *stats, char *errbuf, size_t errlen)
{ if (!labels || !records || !nrec || !rec_words) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  *records = NULL; *nrec = 0; *rec_words = 0;
  if (!tv) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  ViewCtx vc; smg_table_source src;
  view_source(tv, &vc, &src);
  return host_run(&src, opts, plot, stats, labels, records, nrec, rec_words, errbuf, errlen);
}

extern "C" void smg_free(void *p) { free(p); }

// ---- stand-alone conditioning: host table in, conditioned host table out (third "next" row of the scope table) ----
extern "C" int smg_condition_table(const smg_table_view *tv, const smg_opts *opts, uint64_t **keys_out,
                                   uint16_t **counts_out, int64_t *nels_out, int *words_out,
                                   char *errbuf, size_t errlen)
{ if (!tv || !opts || !keys_out || !counts_out || !nels_out || !words_out)
    return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  *keys_out = NULL; *counts_out = NULL; *nels_out = 0; *words_out = 0;
  if (tv->ibyte < 1 || tv->ibyte > 3) return fail(errbuf, errlen, SMG_EINVAL, "ibyte must be 1, 2 or 3%s");
  if (((tv->kmer + 3) >> 2) + 2 - tv->ibyte < 3) return fail(errbuf, errlen, SMG_EINVAL, "k-mer shorter than the index prefix%s");
  EngineOwner eng;                           // (in front of the buffer: destroyed after it)
  smg_engine *e = eng.create(opts->device, errbuf, errlen);
  if (!e) return SMG_ENODEV;
  int rc;
  DevBuf<int64_t> d_index;
  ViewCtx vc; smg_table_source src;
  view_source(tv, &vc, &src);
  if ((rc = upload_index(&src, d_index, "the table", errbuf, errlen))) return rc;
  if ((rc = ingest_range(e, &src, 0, tv->nels, d_index, opts->device, ING_VIEW_READERS, NULL, NULL, errbuf, errlen))) return rc;
  if (opts->condition
      && (rc = smg_engine_condition(e, opts->ethresh, opts->condition & SMG_COND_TRIM, opts->condition & SMG_COND_SYMM,
                                    NULL, errbuf, errlen)))
    return rc;
  // (the two arrays go to the caller, who releases them with smg_free: malloc)
  const int64_t n = e->tab.n;
  uint64_t *hk = (uint64_t *) malloc(sizeof(uint64_t) * (size_t) (n > 0 ? n : 1) * e->tab.W);
  uint16_t *hc = (uint16_t *) malloc(sizeof(uint16_t) * (size_t) (n > 0 ? n : 1));
  if (!hk || !hc) rc = fail(errbuf, errlen, SMG_ENOMEM, "out of host memory for the conditioned table%s");
  else if (n > 0 && (hipMemcpy(hk, e->tab.keys, sizeof(uint64_t) * (size_t) n * e->tab.W, hipMemcpyDeviceToHost) != hipSuccess
                     || hipMemcpy(hc, e->tab.cnt, sizeof(uint16_t) * (size_t) n, hipMemcpyDeviceToHost) != hipSuccess))
    rc = fail(errbuf, errlen, SMG_ENODEV, "device to host copy failed%s");
  if (rc) { free(hk); free(hc); return rc; }
  *keys_out = hk; *counts_out = hc; *nels_out = n; *words_out = e->tab.W;
  return SMG_OK;
}

