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
// This file: the engine struct with the parts that own its buffers, create / destroy / bind, the directory geometry, the run entry
// points, extract and the exports of limits and state.  Everything else is a header of this one translation unit, included where
// it is needed: smg_decode.hpp (FastK records -> table), smg_counted.hpp (k > 85 and the general path), smg_fast_host.hpp (k <= 85:
// pass 1 from plan to retry, pass 2, resume), smg_fast_lookup.hpp (k <= 85: what lies between the passes -- the plans of presort,
// filter, probe and apply, and the launches that carry them out), smg_phase.hpp (the phase API of sharded runs, replay, the block
// map calls), smg_condition.hpp (trim, symmetrise, close), smg_ingest.hpp, smg_shards.hpp, smg_multi.hpp.

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
//                       (tests/test_list_lookups_gpu.py, with smg_engine_list_limits and smg_engine_apply_state);
//                       SMG_FILTER_SORT_MIN=<n> (>= SORT_MIN) buckets a key-only list in front of the filter from n chunk slots on;
//                       SMG_PROBE_X=0/1 and SMG_PX_ONE_XCC choose the probe kernel of a single shard and its tickets.
//                       Where they are read: SMG_DIR_PER in dir_geometry; SMG_TWO_WAY, SMG_NO_FILTER, SMG_ONE_BIT_MAP, SMG_SIG and
//                       SMG_BM_BITS in p1_plan, SMG_P1_GRID in p1_reserve, SMG_P2_GRID in fast_pass2 (smg_fast_host.hpp);
//                       SMG_FILTER_SORT_MIN, SMG_FILTER_GRID, SMG_PROBE_X, SMG_PX_ONE_XCC and SMG_APPLY_SORT_MIN in the plans of
//                       smg_fast_lookup.hpp (smg_engine_lookup_plan hands them to tests/test_lookup_plan_host.py),
//                       SMG_VERIFY_SORT (every sort of apply_sorted is checked) in apply_plan; SMG_EXTRACT_GRID in
//                       engine_extract; SMG_NO_INDEX_DIR in smg_decode.hpp.
static inline const char *test_hook(const char *name) { return getenv(name); }
// a hook that is an integer: its value where lo <= value <= hi, any other value is ignored (dflt)
#define HOOK_ANY INT64_MIN, INT64_MAX
static inline int64_t hook_int(const char *name, int64_t lo, int64_t hi, int64_t dflt)
{ const char *v = test_hook(name);
  const int64_t x = v ? atoll(v) : 0;
  return v && x >= lo && x <= hi ? x : dflt;
}
// a *_GRID hook: fewer workgroups, never more
static inline unsigned hook_grid(const char *name, unsigned grid) { return grid > 1 ? (unsigned) hook_int(name, 1, (int64_t) grid - 1, grid) : grid; }

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

// the timing events, in pairs around: decode or conditioning, pass 1, the look-ups (filter included), pass 2, the whole run, the
// filter of a replayed step, extract; EV_PROBE_BEG sits between the partition and the probe of the look-up chain, EV_BIGFIX_BEG
// in front of kf_collect + kf_bigfix, whose time ends with pass 1's
enum Ev { EV_DECODE_BEG, EV_DECODE_END, EV_PASS1_BEG, EV_PASS1_END, EV_LOOKUP_BEG, EV_LOOKUP_END, EV_PASS2_BEG, EV_PASS2_END,
          EV_RUN_BEG, EV_RUN_END, EV_PROBE_BEG, EV_REPLAY_FILTER_BEG, EV_REPLAY_FILTER_END, EV_EXTRACT_BEG, EV_EXTRACT_END,
          EV_BIGFIX_BEG, EV_COUNT };

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

// pinned host memory that frees itself: what DevBuf (smg_keysort.hpp) is for device memory
template <class T> struct Pinned
{ T *p = nullptr;
  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  ~Pinned() { if (p) (void) hipHostFree(p); }
  hipError_t alloc(size_t bytes) { return hipHostMalloc((void **) &p, bytes); }
  operator T *() const { return p; }
  T *operator->() const { return p; }
};

// The parts of the engine that own the buffers of ONE stage each.  Every device allocation is a DevBuf: grown where it is used by
// reserve(), freed with the engine; init() makes the allocations of fixed size when the engine is created.
struct Pass1Part
{ DevBuf<uint32_t> dbits;     // deferred entries of kf_pass1_d: one bit per table entry; all zero between runs
  bool         dbits_dirty;   //   ... unless a run was abandoned between pass 1 and kf_bigfix
  DevBuf<uint32_t> biglist;   // the marked entries, compacted (kf_collect)
  DevBuf<uint32_t> farp;      // beside it: the partner of a listed entry whose code is CODE_FAR (kf_bigfix -> kf_pass2_far)
  DevBuf<unsigned> tick;      // tile tickets of kf_pass1_d
  DevBuf<P1Cold> cold;        // rarely used arguments of kf_pass1_d (device copy)
  Pinned<P1Cold> h_cold;      //   ... and their pinned staging
  DevBuf<u64>  partials;      // fingerprint words of the workgroups [P1_MAXGRID][4], and a row for the proof words
  Pinned<u64>  h_partials;
  P1Kernel     asked;         // the instantiation of kf_pass1_d whose resident workgroups were asked for last (NULL: none yet) ..
  unsigned     resident;      //   .. and the answer
  hipError_t init()
  { hipError_t he = partials.alloc(sizeof(u64) * 4 * (P1_MAXGRID + 1));
    if (he == hipSuccess) he = h_partials.alloc(sizeof(u64) * 4 * P1_MAXGRID);
    if (he == hipSuccess) he = cold.alloc(sizeof(P1Cold));
    return he == hipSuccess ? h_cold.alloc(sizeof(P1Cold)) : he;
  }
};

struct ChainPart              // the look-up chain (smg_lookup.hpp)
{ DevBuf<unsigned> ghist;     // requests per bucket [L_BK], bucket cursor `bnext` behind it
  DevBuf<unsigned> whist;     // requests per owner and bucket [owners][L_BK] (owner = a workgroup of pass 1 / kf_bigfix)
  DevBuf<u64>  boff;          // bucket offsets [L_BK + 1] and scatter cursors [L_BK] behind them
  DevBuf<unsigned> xtick;     // (bucket, part) tickets of kl_probe_x, one counter per XCD
  hipError_t init()
  { const hipError_t he = ghist.alloc(sizeof(unsigned) * (L_BK + 4));
    return he == hipSuccess ? boff.alloc(sizeof(u64) * (2 * L_BK + 4)) : he;
  }
};

struct SortedPart             // look-ups in sorted order
{ DevBuf<u64>  req2;          // radix sort output; the request list bucketed or partitioned in front of the filter (Presort)
  DevBuf<u64>  dense;         // compacted requests
  DevBuf<uint32_t> chunk_off;
  DevBuf<uint32_t> skey[2];   // index sort of wide records: leading k-mer bits (in, out)
  DevBuf<uint32_t> sidx[2];   //                                  record numbers (in, out)
};

struct RouterPart
{ DevBuf<u64>  d_split;       // the splitters of up to 16 ranks
  DevBuf<uint32_t> route_cnt;
  DevBuf<u64>  route_off;
  DevBuf<u64>  rp_totals;     // replay: per-destination totals of the recorded step (16 words) and of this step (16 more)
  hipError_t init() { return d_split.alloc(sizeof(u64) * 16 * 4); }
};

// The two request lists: records in chunks of F_CH, `fill` records in each.  Pass 1 (and kf_bigfix) fill `cur`; the filter reads
// `cur`, writes what it keeps to `kept`, and the two swap, so that `cur` is always the list the router and the look-ups walk.
// Invariant: a list is never smaller than the other one was when it was sized, and no allocation shrinks -- so from the second
// filter on the same table both hold the same, and no step allocates.  The counts (chunks in use, the capacity the kernels were
// given, the owners) are RunState's: begin_run resets them, the buffers outlive a run.  The counted path (k > 85,
// smg_counted.hpp) keeps ONE flat list in cur.rec and presents it to the router as full chunks through cur.fill.
struct RequestLists
{ struct List { DevBuf<u64> rec; DevBuf<uint32_t> fill; };
  List cur, kept;
  // chunks of rw-word records that the current list's allocation holds
  int64_t chunks(int rw) const { return (int64_t) cur.rec.bytes / ((int64_t) F_CH * (int64_t) sizeof(u64) * rw); }
  // the one place a list is sized: room for `chunks` chunks of rw-word records, and never less than the other list has
  hipError_t reserve(List &l, unsigned chunks, int rw)
  { const List &o = &l == &cur ? kept : cur;
    size_t rec_bytes = (size_t) chunks * F_CH * sizeof(u64) * rw, fill_bytes = (size_t) chunks * 4 + 4;
    if (rec_bytes < o.rec.bytes) rec_bytes = o.rec.bytes;
    if (fill_bytes < o.fill.bytes) fill_bytes = o.fill.bytes;
    const hipError_t he = l.rec.reserve(rec_bytes);
    return he == hipSuccess ? l.fill.reserve(fill_bytes) : he;
  }
  hipError_t reserve_flat(int64_t records, int rw) { return cur.rec.reserve((size_t) records * sizeof(u64) * rw); }     // (counted path)
  hipError_t reserve_fills(int64_t chunks) { return cur.fill.reserve((size_t) chunks * 4 + 4); }                      // (counted path)
  void swap() { cur.rec.swap(kept.rec); cur.fill.swap(kept.fill); }
};

struct smg_engine
{ int          device;
  hipStream_t  stream;
  Settings     set;
  TableState   tab;
  RunState     run;
  Replay       rp;
  // table-level state
  DevBuf<u64>  own_keys;      // owned copies (decode path)
  DevBuf<uint16_t> own_cnt;
  DevBuf<uint8_t>  deg;       // degree bytes (counted path) / code bytes (fast path)
  DevBuf<uint16_t> sig;       // k <= 32: look-up signatures (2 bytes per entry)
  DevBuf<uint32_t> bstart;
  DevBuf<uint32_t> ixdir;     // the table's own FastK prefix index (2^24 + 1 bucket starts, relative to this shard) as directory
  DevBuf<uint32_t> bmap;      // candidate block map (request filter)
  DevBuf<Ctrl> ctrl;
  Pinned<Ctrl> h_ctrl;        // pinned mirror
  Dev          sort_tmp;      // rocPRIM's scratch (with_scratch), shared by every stage
  // the stages
  Pass1Part    p1;
  RequestLists lists;
  ChainPart    chain;
  SortedPart   srt;
  RouterPart   router;
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
  if (e->ctrl.alloc(sizeof(Ctrl)) != hipSuccess || e->h_ctrl.alloc(sizeof(Ctrl)) != hipSuccess
      || e->p1.init() != hipSuccess || e->router.init() != hipSuccess || e->chain.init() != hipSuccess)
    { fail(errbuf, errlen, SMG_ENOMEM, "cannot allocate the control block%s");
      smg_engine_destroy(e); return NULL;
    }
  return e;
}

extern "C" void smg_engine_destroy(smg_engine *e)
{ if (!e) return;
  hipSetDevice(e->device);
  hipStreamSynchronize(e->stream);
  for (int i = 0; i < EV_COUNT; i++) hipEventDestroy(e->ev[i]);
  delete e;                                  // (frees every device buffer and the pinned host memory)
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
  per = (int) hook_int("SMG_DIR_PER", 1, 0x7FFFFFFF, per);                                  // tuning override
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

#include "smg_fast_host.hpp"
#include "smg_fast_lookup.hpp"
#include "smg_phase.hpp"

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
      nb = hook_grid("SMG_EXTRACT_GRID", (unsigned) nb);
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

