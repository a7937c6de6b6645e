// smg_multi.hpp -- several GPUs of one node behind the C ABI (smg_opts.ngpus > 1): what the `hetmers`
// executable uses when SMUDGEPLOT_GPUS=N is set, so that the unchanged `smudgeplot hetmers` CLI scales
// over the node.  Included at the end of smg_hetmers.hip (uses the engine's internals).
//
// One host thread per GPU, each with its own engine.  The conditioned table is cut into contiguous PREFIX
// shards on window-block boundaries (every scanned position is shard local; the reference's analogue is
// the prefix-subtree task list of small_window, PloidyPlot.c:1040-1084).  Exchanges:
//   1. complement requests: grouped by destination on the device (smg_engine_route), then one
//      send/recv pair per peer inside ONE RCCL group call (an all-to-all over the xGMI links);
//   2. ONE ncclAllReduce(SUM, int64[1001*501]) of the per-GPU histograms.
// The symmetry proof (missing counts + fingerprint residues) is a few words per GPU and is reduced on the
// host: all ranks live in one process.
//
// RCCL is resolved with dlopen at the first multi-GPU call: the single-GPU path (and a process that
// already carries another RCCL, e.g. PyTorch's) never loads it.
//
// Virtual shards (run_mode_plan, smg_shards.hpp): N shards on ONE device, the exchanges done with device-to-device copies
// and a host-side sum -- exercises the cutting, the ranged decode, the routing and the proof on a 1-GPU box.
// The multi-process equivalent (one process per GPU, torch.distributed) is smudgeplot_amd/sharded.py.

#pragma once
#include <atomic>
#include <memory>
#include <pthread.h>
#include <dlfcn.h>
#include <rccl/rccl.h>          // types and enums only: the functions are looked up at run time

struct RcclApi
{ void *lib;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *);
  ncclResult_t (*CommDestroy)(ncclComm_t);
  ncclResult_t (*GroupStart)(void);
  ncclResult_t (*GroupEnd)(void);
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
  const char  *(*GetErrorString)(ncclResult_t);
};

static bool rccl_load(RcclApi *a, char *errbuf, size_t errlen)
{ memset(a, 0, sizeof(*a));
  const char *names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so" };
  // an RCCL that the process has loaded already (a Python caller's torch brings its own) is the one to use: two copies of the
  // library in one process take each other's state down at exit ("double free or corruption" after an otherwise clean run)
  for (unsigned i = 0; i < 2 && !a->lib; i++) a->lib = dlopen(names[i], RTLD_NOW | RTLD_NOLOAD);
  // (RTLD_LOCAL: this copy's symbols are reached through dlsym alone -- with RTLD_GLOBAL a torch that loads ITS librccl later
  //  binds part of it to this one)
  for (unsigned i = 0; i < sizeof(names) / sizeof(names[0]) && !a->lib; i++) a->lib = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
  if (!a->lib) { fail(errbuf, errlen, SMG_ENODEV, "cannot load RCCL (librccl.so) for the multi-GPU run%s"); return false; }
#define SYM(field, name) *(void **) (&a->field) = dlsym(a->lib, name); if (!a->field) { fail(errbuf, errlen, SMG_ENODEV, "RCCL symbol missing: %s", name); return false; }
  SYM(CommInitAll, "ncclCommInitAll") SYM(CommDestroy, "ncclCommDestroy") SYM(GroupStart, "ncclGroupStart")
  SYM(GroupEnd, "ncclGroupEnd") SYM(Send, "ncclSend") SYM(Recv, "ncclRecv") SYM(AllReduce, "ncclAllReduce")
  SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
  return true;
}

// what rank r publishes: written by r alone, read by the others after a barrier
struct RankPub
{ u64      first[4] = { ~0ull, ~0ull, ~0ull, ~0ull };   // first k-mer the shard can hold (all ones: nothing is left for it)
  int64_t  nshard = 0;                                   // entries of the shard
  int64_t  counts[SMG_MAXGPU] = {};                      // records grouped for rank d, of the exchange under way
  const uint64_t *send = NULL;                           // ... and where they are (device memory of r: Rank::send)
  const uint32_t *bmap = NULL;                           // candidate block map of the shard (request filter), bm_bits = 0: none
  int      bm_bits = 0;
  int64_t  missing = 0;                                  // proof words
  u64      fp[4] = { 0, 0, 0, 0 };
  std::vector<int64_t> symm_hist;                        // symmetrise: entries / complements per leading `symm_bits` bits
  const int64_t *h_plot = NULL;                          // virtual mode: the shard's histogram on the host (Rank::h_plot)
  Tab      tab = {};                                     // general path over virtual shards: the shard's table
  smg_stats st = {};
  int      rc = SMG_OK;                                  // the rank's first error ...
  char     err[256] = "";                                // ... and its message
  std::vector<uint64_t> rec;                             // extract leg: records of the shard
};

struct MultiCtx
{ int  n = 0;                               // shards == threads
  bool virt = false;                        // all shards on one device, no RCCL
  int  devs[SMG_MAXGPU] = {};
  const smg_table_source *tv = NULL;
  int  symcheck = 0, condition = 0, ethresh = 0, W = 0, io_threads = 0, symm_bits = 0;
  int64_t cut[SMG_MAXGPU + 1] = {};         // entry ranges of the shards in the input table
  pthread_barrier_t bar;
  pthread_mutex_t big_mu;                   // virtual shards: the sort of the symmetrise step runs one shard at a time
  bool have_sync = false, have_comm = false;
  std::atomic<int> failed { 0 };            // some rank has failed: raised by Rank::step, read by Rank::ok and multi_agree
  RcclApi  api = {};
  ncclComm_t comm[SMG_MAXGPU] = {};
  RankPub  pub[SMG_MAXGPU];
  const TabSet *d_set = NULL;               // general path over virtual shards: the shards' tables, published by rank 0 (Rank::d_set)
  int      general = 0;                     // 1: the table failed the proof and the shards ran the general path together (rank 0 says)
  int64_t *plot = NULL;                     // result (host), written by rank 0
  const uint16_t *labels = NULL;            // extract leg (or NULL): labels of the annotated pixels (host, SMG_PLOT_CELLS)
  MultiCtx() = default;
  MultiCtx(const MultiCtx &) = delete;
  ~MultiCtx()
  { if (have_comm) for (int r = 0; r < n; r++) api.CommDestroy(comm[r]);
    if (have_sync) { pthread_barrier_destroy(&bar); pthread_mutex_destroy(&big_mu); }
  }
};

// Every rank takes part in a collective (or in the peer copies of the virtual mode) or none does: the failure flag is
// read between two barriers, where nobody writes it, so all ranks see the same value.  (A rank that failed after
// the previous barrier would otherwise skip its ncclSend/ncclRecv while its peers block in theirs for ever.)
static bool multi_agree(MultiCtx *c)
{ pthread_barrier_wait(&c->bar);
  const bool ok = !c->failed.load();
  pthread_barrier_wait(&c->bar);
  return ok;
}

__global__ void km_or_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, int64_t n)
{ for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
    dst[i] |= src[i];
}

// request filter across shards: OR the word ranges that the k-mer ranges of the shards cover (neighbours share their
// boundary word) into one map on this shard's device, then drop the requests whose target block holds no candidate
static int multi_filter(MultiCtx *c, int r, smg_engine *e, const u64 *splitters, char *eb, size_t el)
{ const int n = c->n, bits = c->pub[r].bm_bits;
  for (int s = 0; s < n; s++) if (c->pub[s].bm_bits != bits) return SMG_OK;       // (cannot happen: a function of k and the proof)
  if (!bits) return SMG_OK;
  const int two = e->run.bm2;                            // 64-bit map words (two-bit map): twice the 32-bit words per id range
  const int64_t nwords = bm_words(bits, two);
  int64_t wlo[SMG_MAXGPU], wlen[SMG_MAXGPU], width = 1;
  for (int s = 0; s < n; s++)
    { const u64 a = s == 0 ? 0 : splitters[(size_t) (s - 1) * c->W] >> (64 - bits);
      const u64 b = s == n - 1 ? (1ull << bits) - 1 : splitters[(size_t) s * c->W] >> (64 - bits);
      wlo[s] = (int64_t) (a >> 5) << two;
      wlen[s] = (((int64_t) (b >> 5) << two) - wlo[s]) + (1 << two);
      if (wlen[s] < 1) wlen[s] = 1;
      if (wlen[s] > width) width = wlen[s];
    }
  DevBuf<uint32_t> full, tmp;
  int rc = SMG_OK;
  if (full.alloc((size_t) nwords * 4) != hipSuccess || tmp.alloc((size_t) width * 4) != hipSuccess)
    rc = fail(eb, el, SMG_ENOMEM, "out of device memory for the block map exchange%s");
  if (rc == SMG_OK && hipMemsetAsync(full, 0, (size_t) nwords * 4, e->stream) != hipSuccess) rc = fail(eb, el, SMG_ENODEV, "memset failed%s");
  for (int s = 0; s < n && rc == SMG_OK; s++)
    { const uint32_t *src = c->pub[s].bmap + wlo[s];
      hipError_t he = c->virt || c->devs[s] == c->devs[r]
                        ? hipMemcpyAsync(tmp, src, (size_t) wlen[s] * 4, hipMemcpyDeviceToDevice, e->stream)
                        : hipMemcpyPeerAsync(tmp, c->devs[r], src, c->devs[s], (size_t) wlen[s] * 4, e->stream);
      if (he != hipSuccess) { rc = fail(eb, el, SMG_ENODEV, "block map copy failed: %s", hipGetErrorString(he)); break; }
      unsigned nb = (unsigned) ((wlen[s] + 255) / 256);
      if (nb > 4096) nb = 4096;
      hipLaunchKernelGGL(km_or_words, dim3(nb), dim3(256), 0, e->stream, full + wlo[s], tmp.as<uint32_t>(), wlen[s]);
    }
  if (rc == SMG_OK) rc = smg_engine_filter(e, full, NULL, eb, el);
  hipStreamSynchronize(e->stream);                       // (the two maps are freed on return)
  return rc;
}

// records of `rw` words: what rank s grouped for rank r in pub[s].send (pub[s].counts, destination-major) -> recv of rank r.
// Call behind multi_agree(): every rank takes part.
static int multi_exchange(MultiCtx *c, int r, smg_engine *e, uint64_t *recv, int rw, const char *what, char *eb, size_t el)
{ const int n = c->n;
  if (c->virt)
    { const int64_t *counts[SMG_MAXGPU]; const uint64_t *send[SMG_MAXGPU];
      for (int s = 0; s < n; s++) { counts[s] = c->pub[s].counts; send[s] = c->pub[s].send; }
      return gather_received(counts, n, r, send, rw, recv) ? SMG_OK : fail(eb, el, SMG_ENODEV, "device to device copy failed (%s)", what);
    }
  const RankPub &me = c->pub[r];
  ncclResult_t nr = c->api.GroupStart();
  int64_t soff = 0, roff = 0;
  for (int p = 0; p < n && nr == ncclSuccess; p++)
    { const int64_t out = me.counts[p], in = c->pub[p].counts[r];
      if (out) nr = c->api.Send(me.send + soff * rw, (size_t) out * rw, ncclUint64, p, c->comm[r], e->stream);
      if (nr == ncclSuccess && in) nr = c->api.Recv(recv + roff * rw, (size_t) in * rw, ncclUint64, p, c->comm[r], e->stream);
      soff += out; roff += in;
    }
  const ncclResult_t ne = c->api.GroupEnd();
  if (nr == ncclSuccess) nr = ne;
  if (nr != ncclSuccess || hipStreamSynchronize(e->stream) != hipSuccess)
    return fail(eb, el, SMG_ENODEV, "RCCL exchange failed: %s", nr != ncclSuccess ? c->api.GetErrorString(nr) : "stream error");
  return SMG_OK;
}

// ---- one rank ---------------------------------------------------------------------------------------------------------------
// A rank runs every step the same way: `if (ok()) step(f(..))`.  ok() reads the flag that all ranks share, step() records
// this rank's first error and raises the flag, fail() does the same with a message of this file.
//
// THE BARRIER RULE.  Every rank crosses the same barriers in the same order on every path, failed or not: a phase has
// no return in front of a barrier, and what decides whether a barrier is reached at all (symmetrise or not, the verdict behind
// C1) is the same on every rank.  A collective or a peer copy happens only behind multi_agree(), where all ranks have read
// the same flag.  The barriers, in order, and the phase that crosses them:
//   close_across_shards   S1 histograms published, S2 splitters published, S3 counts known, S4 (agree) exchange,
//                         S5 peers have copied                                           [only where the table is symmetrised]
//   pass1_and_route       A shards ready, A2 splitters final, A3 block maps complete, B all counts known
//   exchange_and_apply    B2 (agree) exchange, C proof words published
//   verdict               C1 (agree) verdict known to all
//   second_pass           G1 directories built, G2 shard set published, G3 all degrees final   [only on the general path]
//   reduce                C2 (agree) reduction, D histograms ready
//   take_down             E done with the histograms and the shard set
// What peers read of a rank -- send, h_plot, the shard set; the block map is the engine's -- is owned by that rank and
// released explicitly at the barrier named beside it, not at the end of a scope.
namespace {       // (Rank and its phases are this file's own: no symbols)
struct Rank
{ MultiCtx *const c;
  const int r;
  RankPub &me;
  char *const eb; const size_t el;          // me.err
  EngineOwner eng;                          // (in front of the buffers: destroyed after them)
  smg_engine *e = NULL;
  DevBuf<int64_t>  d_plot;
  DevBuf<uint64_t> send;                    // read by the peers between S3 and S5, and between B and C
  DevBuf<uint64_t> recv;
  DevBuf<TabSet>   d_set;                   // rank 0, general path: read by all ranks until E
  std::vector<int64_t> h_plot;              // virtual mode: read by rank 0 between D and E
  u64 splitters[SMG_MAXGPU * 4];
  int rw = 0;
  int64_t nrecv = 0;
  bool general = false;

  Rank(MultiCtx *ctx, int rank) : c(ctx), r(rank), me(ctx->pub[rank]), eb(ctx->pub[rank].err), el(sizeof(ctx->pub[rank].err)) { }
  bool ok() const { return !c->failed.load(); }
  void step(int rc) { if (rc == SMG_OK) return; if (me.rc == SMG_OK) me.rc = rc; c->failed.store(1); }
  void fail(int code, const char *msg) { step(::fail(eb, el, code, "%s", msg)); }
  void barrier() { pthread_barrier_wait(&c->bar); }
  void splitters_from_first() { for (int s = 1; s < c->n; s++) memcpy(splitters + (size_t) (s - 1) * c->W, c->pub[s].first, sizeof(u64) * c->W); }
  void alloc_records(DevBuf<uint64_t> &buf, int64_t nrec, int words, const char *msg)
  { if (ok() && buf.alloc(sizeof(uint64_t) * (size_t) (nrec > 0 ? nrec : 1) * words) != hipSuccess) fail(SMG_ENOMEM, msg); }

  void load_shard();
  void close_across_shards();
  void pass1_and_route();
  void exchange_and_apply();
  bool verdict();
  void second_pass(bool go);
  void reduce();
  void extract();
  void take_down();
};

// phase 1: the shard on the device -- ingest, index, trim
void Rank::load_shard()
{ const smg_table_source *tv = c->tv;
  const int64_t lo = c->cut[r], hi = c->cut[r + 1];
  DevBuf<int64_t> d_index;
  if (hipSetDevice(c->devs[r]) != hipSuccess) fail(SMG_ENODEV, "cannot select HIP device");
  if (ok() && !(e = eng.create(c->devs[r], eb, el))) step(SMG_ENODEV);
  if (ok() && !c->virt && c->n >= 8) smg_engine_set_blockmap_bits(e, 29);     // (the exchanged map: see TorchEngine.pass1 in sharded.py)
  if (ok()) step(upload_index(tv, d_index, "the table shard", eb, el));
  if (ok() && d_plot.alloc(sizeof(int64_t) * SMG_PLOT_CELLS) != hipSuccess) fail(SMG_ENOMEM, "out of device memory for the table shard");
  if (ok()) step(ingest_range(e, tv, lo, hi, d_index, c->devs[r], c->io_threads, NULL, NULL, eb, el));
  // a shard that is taken as it is keeps the table's prefix index as its look-up directory (bucket starts relative to entry lo)
  if (ok() && !c->condition) step(smg_engine_set_prefix_index(e, d_index, tv->ibyte, lo, eb, el));
  if (ok() && !c->condition && hipStreamSynchronize(e->stream) != hipSuccess) fail(SMG_ENODEV, "index conversion failed");
  d_index.reset();
  if (ok() && (c->condition & SMG_COND_TRIM)) { int64_t nn = 0; step(smg_engine_condition(e, c->ethresh, 1, 0, &nn, eb, el)); }
  if (ok() && !(c->condition & SMG_COND_SYMM))
    { me.nshard = e->tab.n;
      if (e->tab.n > 0 && hipMemcpy(me.first, e->tab.keys, sizeof(u64) * c->W, hipMemcpyDeviceToHost) != hipSuccess)
        fail(SMG_ENODEV, "device to host copy failed");
    }
}

// phase 2: close the table under reverse complement ACROSS the shards (Symmex, PloidyPlot.c:1395-1414)
void Rank::close_across_shards()
{ const int n = c->n, W = c->W, bits = c->symm_bits, nbin = 1 << bits, rw2 = W + 1;
  // S1: shape of the closed table -> balanced splitters on a boundary of `symm_bits` leading bits
  me.symm_hist.assign((size_t) 2 * nbin, 0);
  if (ok()) step(smg_engine_symm_hist(e, bits, me.symm_hist.data(), eb, el));
  barrier();                                                                             // S1: histograms published
  if (ok() && r == 0)
    { std::vector<int64_t> hist((size_t) 2 * nbin, 0);
      for (int s = 0; s < n; s++) for (int b = 0; b < 2 * nbin; b++) hist[(size_t) b] += c->pub[s].symm_hist[(size_t) b];
      balanced_splitters(hist.data(), nbin, bits, n, W, splitters);
      for (int s = 0; s < n; s++)
        { memset(c->pub[s].first, 0, sizeof(c->pub[s].first));
          if (s > 0) memcpy(c->pub[s].first, splitters + (size_t) (s - 1) * W, sizeof(u64) * W);
        }
    }
  barrier();                                                                             // S2: splitters published
  std::vector<int64_t>().swap(me.symm_hist);
  splitters_from_first();
  // S3: two records per entry (itself, its complement), grouped by destination
  const int64_t n2 = ok() ? 2 * e->tab.n : 0;
  alloc_records(send, n2, rw2, "out of device memory while symmetrising");
  me.send = send;
  if (ok()) step(smg_engine_symm_route(e, (const uint64_t *) splitters, n, send, n2, me.counts, eb, el));
  barrier();                                                                             // S3: counts known
  nrecv = 0;
  if (ok()) for (int s = 0; s < n; s++) nrecv += c->pub[s].counts[r];
  alloc_records(recv, nrecv, rw2, "out of device memory while symmetrising");
  if (multi_agree(c)) step(multi_exchange(c, r, e, recv, rw2, "symmetrise", eb, el));     // S4: all in, or all out
  barrier();                                                                             // S5: peers have copied
  send.reset(); me.send = NULL;
  if (ok())
    { int64_t nn = 0;
      if (c->virt) pthread_mutex_lock(&c->big_mu);
      step(smg_engine_symm_finish(e, recv, nrecv, &nn, eb, el));
      if (c->virt) pthread_mutex_unlock(&c->big_mu);
    }
  recv.reset();
  if (ok()) me.nshard = e->tab.n;                                                        // (splitters = first[])
}

// phase 3: pass 1, the candidate map published, the requests filtered against all maps and grouped by destination
void Rank::pass1_and_route()
{ const int n = c->n;
  barrier();                                                                             // A: shards ready, first k-mers published
  if (ok() && r == 0 && !(c->condition & SMG_COND_SYMM))
    for (int s = n - 2; s >= 0; s--)              // an empty shard inherits its successor's first k-mer
      if (c->pub[s].nshard == 0) memcpy(c->pub[s].first, c->pub[s + 1].first, sizeof(c->pub[s].first));
  barrier();                                                                             // A2: splitters final
  if (ok())
    { splitters_from_first();
      step(smg_engine_pass1(e, c->symcheck, eb, el));
    }
  if (ok() && e->run.bm_bits) { me.bmap = e->bmap; me.bm_bits = e->run.bm_bits; hipStreamSynchronize(e->stream); }
  barrier();                                                                             // A3: block maps complete
  if (ok()) step(multi_filter(c, r, e, splitters, eb, el));
  int64_t nreq = 0;
  if (ok()) { nreq = smg_engine_nreq(e); rw = smg_engine_record_words(e); }
  alloc_records(send, nreq, rw, "out of device memory for the request exchange");
  me.send = send;
  if (ok()) step(smg_engine_route(e, (const uint64_t *) splitters, n, send, nreq, me.counts, eb, el));
  barrier();                                                                             // B: all counts known
}

// phase 4: the requests to the shards that hold their targets, the look-ups, the proof words
void Rank::exchange_and_apply()
{ nrecv = 0;
  if (ok()) for (int s = 0; s < c->n; s++) nrecv += c->pub[s].counts[r];
  alloc_records(recv, nrecv, rw, "out of device memory for the request exchange");
  if (multi_agree(c)) step(multi_exchange(c, r, e, recv, rw, "requests", eb, el));       // B2: all in, or all out
  if (ok()) step(smg_engine_apply(e, recv, nrecv, &me.missing, eb, el));
  if (ok()) smg_engine_symhash(e, (uint64_t *) me.fp, eb, el);
  barrier();                                                                             // C: proof words published
  send.reset(); me.send = NULL;                   // peers have copied what they needed
  recv.reset();
}

// phase 5: the symmetry proof, reduced on the host -- every rank computes the same verdict from the same published words
bool Rank::verdict()
{ if (ok())
    { int64_t miss = 0; u64 f[4] = { 0, 0, 0, 0 };
      for (int s = 0; s < c->n; s++) { miss += c->pub[s].missing; for (int q = 0; q < 4; q++) f[q] ^= c->pub[s].fp[q]; }
      const bool closed = proof_holds(c->symcheck, miss, f);
      if (!closed && c->virt) { general = true; if (r == 0) c->general = 1; }
      else if (!closed)
        fail(SMG_ENOTSYM, "the table is not closed under reverse complement with equal counts: "
                          "a multi-GPU run needs a conditioned table (use one GPU for this one)");
    }
  return multi_agree(c);                                                                 // C1: verdict known to all
}

// phase 6: pass 2 -- or, for a table that failed the proof, the general path.  The reference answers for ANY sorted table
// (it only spot-checks the symmetry, PloidyPlot.c:1199-1229): so do the shards of one device, together -- both passes over
// all k positions, a prefix-side partner looked up in whichever shard holds it (TabSet).  Several real GPUs hand such a table
// to one GPU instead (host_run).
void Rank::second_pass(bool go)
{ if (go && general)                              // (`go` and `general` are the same on every rank: so are the barriers)
    { if (ok()) step(general_shard_prepare(e, &me.tab, eb, el));
      barrier();                                                                         // G1: directories built
      if (ok() && r == 0)
        { TabSet hs; memset(&hs, 0, sizeof(hs));
          hs.ns = c->n;
          for (int s = 0; s < c->n; s++)
            { hs.shard[s] = c->pub[s].tab;
              for (int w = 0; w < 4; w++) hs.first[s][w] = w < c->W ? c->pub[s].first[w] : 0;
            }
          if (d_set.alloc(sizeof(TabSet)) != hipSuccess || hipMemcpy(d_set, &hs, sizeof(TabSet), hipMemcpyHostToDevice) != hipSuccess)
            fail(SMG_ENOMEM, "out of device memory for the shard set");
          c->d_set = d_set;
        }
      barrier();                                                                         // G2: shard set published
      if (ok()) step(general_shard_pass(e, c->d_set, 1, d_plot, eb, el));
      barrier();                                                                         // G3: all degrees final
      if (ok()) step(general_shard_pass(e, c->d_set, 2, d_plot, eb, el));
      // (the set stays until barrier E: the extract leg looks partners up through it too)
    }
  else if (go && ok()) step(smg_engine_pass2(e, d_plot, eb, el));
}

// phase 7: the histograms of the shards, summed
void Rank::reduce()
{ const bool go = multi_agree(c);                                                        // C2: all in, or all out
  if (go && c->virt)
    { h_plot.resize(SMG_PLOT_CELLS);
      me.h_plot = h_plot.data();
      if (hipMemcpy(h_plot.data(), d_plot, sizeof(int64_t) * SMG_PLOT_CELLS, hipMemcpyDeviceToHost) != hipSuccess)
        fail(SMG_ENODEV, "device to host copy failed");
    }
  else if (go)
    { const ncclResult_t nr = c->api.AllReduce(d_plot, d_plot, SMG_PLOT_CELLS, ncclInt64, ncclSum, c->comm[r], e->stream);
      if (nr != ncclSuccess || hipStreamSynchronize(e->stream) != hipSuccess)
        step(::fail(eb, el, SMG_ENODEV, "RCCL all-reduce of the histograms failed: %s", nr != ncclSuccess ? c->api.GetErrorString(nr) : "stream error"));
      if (ok() && r == 0 && hipMemcpy(c->plot, d_plot, sizeof(int64_t) * SMG_PLOT_CELLS, hipMemcpyDeviceToHost) != hipSuccess)
        fail(SMG_ENODEV, "device to host copy failed");
    }
  if (e) me.st = e->st;
  barrier();                                                                             // D: histograms ready
  if (ok() && c->virt && r == 0)
    for (int cell = 0; cell < SMG_PLOT_CELLS; cell++)
      { int64_t v = 0;
        for (int s = 0; s < c->n; s++) v += c->pub[s].h_plot[cell];
        c->plot[cell] = v;
      }
}

// phase 8: the extract leg (PloidyList.c:1207-1583 has no size limit either): every shard lists the pairs behind the labelled
// pixels among ITS entries -- the two members of a pair share a window block, hence a shard -- the host concatenates
void Rank::extract()
{ DevBuf<uint16_t> d_labels;
  if (ok() && c->labels) step(upload_labels(c->labels, d_labels, eb, el));
  // (general path: a prefix-side partner may live in another shard)
  if (ok() && c->labels) step(extract_to_host(e, d_labels, general ? c->d_set : NULL, -1, me.rec, eb, el));
}

// phase 9: what the peers read goes when they are done with it, the engine last
void Rank::take_down()
{ barrier();                                                                             // E: done with h_plot and the shard set
  d_set.reset();
  std::vector<int64_t>().swap(h_plot); me.h_plot = NULL;
  d_plot.reset();
}
}       // namespace

struct MultiArg { MultiCtx *c; int r; };

static void *multi_worker(void *argp)
{ const MultiArg *arg = (const MultiArg *) argp;
  Rank rank(arg->c, arg->r);
  rank.load_shard();                                                     // 1
  if (arg->c->condition & SMG_COND_SYMM) rank.close_across_shards();     // 2   S1 S2 S3 S4 S5
  rank.pass1_and_route();                                                // 3   A A2 A3 B
  rank.exchange_and_apply();                                             // 4   B2 C
  const bool go = rank.verdict();                                        // 5   C1
  rank.second_pass(go);                                                  // 6   (G1 G2 G3)
  rank.reduce();                                                         // 7   C2 D
  rank.extract();                                                        // 8
  rank.take_down();                                                      // 9   E
  return NULL;
}

// the team: one thread per shard, this one for shard 0.  The first error among the ranks, named by its device.
static int multi_run_team(MultiCtx *c, char *errbuf, size_t errlen)
{ pthread_t th[SMG_MAXGPU];
  MultiArg args[SMG_MAXGPU];
  for (int r = 0; r < c->n; r++) { args[r].c = c; args[r].r = r; }
  int started = 0;
  for (int r = 1; r < c->n; r++)
    if (pthread_create(&th[r], NULL, multi_worker, &args[r]) == 0) started++;
  if (started != c->n - 1)
    { // cannot run with a partial team: the barrier would never release.  Nothing else has started waiting
      // on it yet only if NO thread was created; otherwise this process cannot recover cleanly.
      if (started) { fprintf(stderr, "smg_hetmers: fatal: partial thread team\n"); abort(); }
      return fail(errbuf, errlen, SMG_ENOMEM, "cannot create the per-GPU host threads%s");
    }
  multi_worker(&args[0]);
  for (int r = 1; r < c->n; r++) pthread_join(th[r], NULL);
  for (int r = 0; r < c->n; r++)
    if (c->pub[r].rc != SMG_OK)
      { if (errbuf && errlen) snprintf(errbuf, errlen, "GPU %d: %s", c->devs[r], c->pub[r].err);
        return c->pub[r].rc;
      }
  return SMG_OK;
}

// sums over the shards, the slowest shard's time of each step, the wall time of the whole run
static void multi_stats(const MultiCtx *c, const smg_opts *opts, float wall, smg_stats *stats)
{ smg_stats st; memset(&st, 0, sizeof(st));
  st.path = c->general ? 2 : 1; st.key_words = c->W;
  for (int r = 0; r < c->n; r++)
    { const smg_stats &s = c->pub[r].st;
      st.nels += s.nels; st.nrequests += s.nrequests; st.nemitted += s.nemitted;
      if (s.ms_decode > st.ms_decode) st.ms_decode = s.ms_decode;
      if (s.ms_pass1 > st.ms_pass1) st.ms_pass1 = s.ms_pass1;
      if (s.ms_rclookup > st.ms_rclookup) st.ms_rclookup = s.ms_rclookup;
      if (s.ms_pass2 > st.ms_pass2) st.ms_pass2 = s.ms_pass2;
    }
  for (int cell = 0; cell < SMG_PLOT_CELLS; cell++) st.npairs += c->plot[cell];
  st.ms_total = wall;                  // H2D + decode + both passes + exchanges, all shards
  if (stats) *stats = st;
  if (opts->verbose)
    fprintf(stderr, "  [smg] n=%lld k=%d gpus=%d%s  decode %.2f ms, pass1 %.2f, exchange+rc-lookup %.2f, pass2 %.2f "
            "(slowest shard each), wall incl. H2D %.2f ms\n", (long long) st.nels, c->tv->kmer, c->n,
            c->virt ? " (virtual shards on one device)" : "", st.ms_decode, st.ms_pass1, st.ms_rclookup, st.ms_pass2, wall);
}

// ngpus shards at once: on as many devices (RCCL), or -- virt -- all on opts->device
static int host_run_multi(const smg_table_source *tv, const smg_opts *opts, int ngpus, bool virt, int64_t *plot,
                          smg_stats *stats, char *errbuf, size_t errlen, const uint16_t *labels = NULL,
                          uint64_t **records = NULL, int64_t *nrec = NULL, int *rec_words = NULL)
{ std::unique_ptr<MultiCtx> ctx(new (std::nothrow) MultiCtx());
  MultiCtx *c = ctx.get();
  if (!c) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s");
  c->n = ngpus; c->tv = tv; c->symcheck = opts->symcheck == SMG_SYM_NONE ? SMG_SYM_HASH : opts->symcheck;
  c->condition = opts->condition; c->ethresh = opts->ethresh;
  c->W = (tv->kmer + 31) / 32;
  c->plot = plot;
  c->labels = labels;
  c->virt = virt;
  c->io_threads = (tv->host_threads > 0 ? tv->host_threads : 4) / ngpus;
  if (c->io_threads < 2) c->io_threads = 2;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(errbuf, errlen, SMG_ENODEV, "no HIP device available (this engine has no CPU fallback)%s");
  for (int r = 0; r < ngpus; r++) c->devs[r] = c->virt ? opts->device : opts->device + r;
  if (!c->virt && opts->device + ngpus > ndev)
    return fail(errbuf, errlen, SMG_EINVAL, "fewer HIP devices than SMUDGEPLOT_GPUS asks for%s");
  if (!c->virt)
    { if (!rccl_load(&c->api, errbuf, errlen)) return SMG_ENODEV;
      const ncclResult_t nr = c->api.CommInitAll(c->comm, ngpus, c->devs);
      if (nr != ncclSuccess) return fail(errbuf, errlen, SMG_ENODEV, "ncclCommInitAll failed: %s", c->api.GetErrorString(nr));
      c->have_comm = true;
    }
  multi_cuts(tv, ngpus, c->cut);
  c->symm_bits = symm_split_bits(tv->kmer);
  pthread_mutex_init(&c->big_mu, NULL);
  pthread_barrier_init(&c->bar, NULL, (unsigned) ngpus);
  c->have_sync = true;
  hipEvent_t t0, t1;
  hipSetDevice(c->devs[0]);
  hipEventCreate(&t0); hipEventCreate(&t1);
  hipEventRecord(t0, 0);
  int rc = multi_run_team(c, errbuf, errlen);
  hipSetDevice(c->devs[0]);
  hipEventRecord(t1, 0); hipEventSynchronize(t1);
  float wall = 0; hipEventElapsedTime(&wall, t0, t1);
  hipEventDestroy(t0); hipEventDestroy(t1);
  if (rc == SMG_OK) multi_stats(c, opts, wall, stats);
  if (rc == SMG_OK && labels)
    { // the shards' records, one after the other
      std::vector<uint64_t> all;
      for (int r = 0; r < ngpus; r++) all.insert(all.end(), c->pub[r].rec.begin(), c->pub[r].rec.end());
      rc = records_to_caller(all, c->W + 1, labels, plot, records, nrec, rec_words, errbuf, errlen);
    }
  return rc;
}

// ---- out of core: prefix shards ONE AFTER THE OTHER on one device ---------------------------------------------------------
// The reference streams a table of any size from disk (small_recursion loads a subtree into its cache when it fits and
// falls back to the streaming twins when it does not, PloidyPlot.c:931-1038); the virtual shards above must all be
// resident together.  Here a table whose shards do not fit together is slow instead of an error: what has to outlive a
// shard between its two passes is its code bytes (1 byte per entry) and its requests (8 bytes for ~17 % of the entries,
// grouped by destination shard) -- not its k-mers.
//   round 1, shard by shard: read + decode, pass 1 (no candidate map: the filter would need the maps of the shards that have
//            not been read yet), requests grouped by destination, code bytes and requests kept, k-mers dropped;
//   round 2, shard by shard: read + decode again (the reference reads its table ~2 (BLEVEL + 1) times), code bytes back, look-ups
//            of all requests that name this shard, pass 2 into the one histogram.
// Symmetry proof as everywhere: XOR of the shards' fingerprints, no look-up may miss.  A table that fails it is refused with a
// precise message (condition the table with smg_condition first).  Round 6: a table that still has to be conditioned is -- shard by
// shard, host_condition_sequential below -- and k > 85 takes the same two rounds with the counted kernels (counted_resume).
// The extract leg runs per shard in round 2 (the two members of a pair share a shard).
// A RAW table out of core (round 6): Logex 'A[e-]' + Symmex (PloidyPlot.c:1381-1414) shard by shard.  The conditioned table
// never exists on the device as a whole -- and not on disk either (the reference writes .trim / .symx tables into the working
// directory): its prefix shards are left in HOST memory (8 W + 2 bytes per entry), from where the two rounds of the run
// below take them instead of reading and decoding part files.
//   sweep 1  every piece of the input: read + decode, trim, histogram of the entries AND their complements per leading 12 bits
//            -> splitters that cut the CLOSED table into n shards of equal size (the rule of the in-core protocol, host_run_multi);
//   sweep 2  every piece again: trim, one record per entry and per complement grouped by destination shard (symm_route),
//            copied out to the destination's list on the host (2 (W + 1) words per kept entry, for the length of this sweep);
//   then     every destination: its records back to the device, sort + dedupe (symm_finish), the shard's k-mers and counts
//            out to the host.
// Trim only: one sweep, the pieces are the shards.
struct HostShard { std::vector<u64> keys; std::vector<uint16_t> cnt; int64_t n = 0; };

static int host_condition_sequential(const smg_table_source *tv, const smg_opts *opts, int n, smg_engine *e, const int64_t *d_index,
                                     std::vector<HostShard> &out, std::vector<u64> &splitters, int verbose, char *errbuf, size_t errlen)
{ const int W = (tv->kmer + 31) / 32, rw = W + 1;
  const bool trim = (opts->condition & SMG_COND_TRIM) != 0, symm = (opts->condition & SMG_COND_SYMM) != 0;
  std::vector<int64_t> cut((size_t) n + 1);
  multi_cuts(tv, n, cut.data());
  int rc = SMG_OK;
  out.assign((size_t) n, HostShard());
  splitters.assign((size_t) (n > 1 ? n - 1 : 1) * W, 0);
  auto load = [&](int s) -> int            // piece s of the input in the engine, trimmed
  { int r = ingest_range(e, tv, cut[s], cut[s + 1], d_index, opts->device, tv->host_threads, NULL, NULL, errbuf, errlen);
    if (r) return r;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(errbuf, errlen, SMG_ENODEV, "decode failed%s");
    if (trim) { int64_t nn = 0; if ((r = smg_engine_condition(e, opts->ethresh, 1, 0, &nn, errbuf, errlen))) return r; }
    return SMG_OK;
  };
  auto take = [&](int d) -> int            // the engine's table -> shard d on the host
  { HostShard &h = out[(size_t) d];
    h.n = e->tab.n;
    h.keys.resize((size_t) (e->tab.n > 0 ? e->tab.n : 0) * W); h.cnt.resize((size_t) (e->tab.n > 0 ? e->tab.n : 0));
    if (e->tab.n > 0 && (hipMemcpy(h.keys.data(), e->tab.keys, sizeof(u64) * (size_t) e->tab.n * W, hipMemcpyDeviceToHost) != hipSuccess
                     || hipMemcpy(h.cnt.data(), e->tab.cnt, sizeof(uint16_t) * (size_t) e->tab.n, hipMemcpyDeviceToHost) != hipSuccess))
      return fail(errbuf, errlen, SMG_ENODEV, "device to host copy failed%s");
    return SMG_OK;
  };
  if (!symm)
    { for (int s = 0; s < n && rc == SMG_OK; s++) { if ((rc = load(s)) == SMG_OK) rc = take(s); }
      index_splitters(tv, cut.data(), n, W, splitters.data());       // (the pieces are the shards, as for a conditioned table)
      return rc;
    }
  const int bits = symm_split_bits(tv->kmer), nbin = 1 << bits;
  std::vector<int64_t> hist((size_t) 2 * nbin, 0), one((size_t) 2 * nbin, 0);
  for (int s = 0; s < n && rc == SMG_OK; s++)                                  // sweep 1
    { if ((rc = load(s))) break;
      if ((rc = smg_engine_symm_hist(e, bits, one.data(), errbuf, errlen))) break;
      for (int b = 0; b < 2 * nbin; b++) hist[(size_t) b] += one[(size_t) b];
    }
  if (rc) return rc;
  if (balanced_splitters(hist.data(), nbin, bits, n, W, splitters.data()) / n >= SMG_ONE_SHARD_MAX)
    return fail(errbuf, errlen, SMG_EINVAL, "out of core: a shard of the closed table would hold more than 2^32 entries (more shards are needed)%s");
  std::vector<std::vector<u64> > rec((size_t) n);
  std::vector<int64_t> counts((size_t) n);
  DevBuf<uint64_t> send, recv;
  for (int s = 0; s < n && rc == SMG_OK; s++)                                  // sweep 2
    { if ((rc = load(s))) break;
      const int64_t n2 = 2 * e->tab.n;
      if (send.alloc(sizeof(uint64_t) * (size_t) (n2 > 0 ? n2 : 1) * rw) != hipSuccess)
        return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory while symmetrising%s");
      rc = smg_engine_symm_route(e, (const uint64_t *) splitters.data(), n, send, n2, counts.data(), errbuf, errlen);
      int64_t off = 0;
      for (int d = 0; d < n && rc == SMG_OK; d++)
        { const size_t at = rec[(size_t) d].size(), words = (size_t) counts[(size_t) d] * rw;
          rec[(size_t) d].resize(at + words);
          if (words && hipMemcpy(rec[(size_t) d].data() + at, send + (size_t) off * rw, sizeof(uint64_t) * words, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(errbuf, errlen, SMG_ENODEV, "device to host copy failed%s");
          off += counts[(size_t) d];
        }
      send.reset();
    }
  for (int d = 0; d < n && rc == SMG_OK; d++)                                  // every destination: sort + dedupe, out to the host
    { const int64_t nrecv = (int64_t) (rec[(size_t) d].size() / (size_t) rw);
      if (recv.alloc(sizeof(uint64_t) * (size_t) (nrecv > 0 ? nrecv : 1) * rw) != hipSuccess)
        return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory while symmetrising%s");
      if (nrecv && hipMemcpy(recv, rec[(size_t) d].data(), sizeof(uint64_t) * (size_t) nrecv * rw, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(errbuf, errlen, SMG_ENODEV, "host to device copy failed%s");
      std::vector<u64>().swap(rec[(size_t) d]);
      int64_t nn = 0;
      if (rc == SMG_OK) rc = smg_engine_symm_finish(e, recv, nrecv, &nn, errbuf, errlen);
      recv.reset();
      if (rc == SMG_OK) rc = take(d);
    }
  if (rc == SMG_OK && verbose)
    { int64_t tot = 0; for (int d = 0; d < n; d++) tot += out[(size_t) d].n;
      fprintf(stderr, "  [smg] conditioned out of core: %lld -> %lld k-mers in %d prefix shards kept in host memory (%s%s)\n", (long long) tv->nels,
              (long long) tot, n, trim ? "trimmed, " : "", "closed under reverse complement");
    }
  return rc;
}

// One out-of-core run: what stays from shard to shard and between the two rounds.
struct SeqRun
{ const smg_table_source *tv; const smg_opts *opts;
  const int n, W, symcheck;
  const bool raw;                            // the shards come out of host_condition_sequential (host memory), not out of the part files
  int64_t *plot; const uint16_t *labels;
  char *eb; size_t el;
  EngineOwner eng;                           // (in front of the buffers: destroyed after them)
  smg_engine *e = NULL;
  std::vector<HostShard> hshard;
  std::vector<int64_t> cut, counts, nreq;    // counts[src * n + dst], records
  std::vector<u64> splitters;
  std::vector<DevBuf<uint8_t> > codes;       // what a shard leaves behind for its second round: a byte per entry ..
  std::vector<DevBuf<uint64_t> > send;       // .. and, for the shards they name, its requests grouped by destination
  DevBuf<int64_t> d_index, d_plot;
  DevBuf<uint16_t> d_labels;
  std::vector<int64_t> h_plot;
  std::vector<uint64_t> xrec;                // extract leg: handed out only if the whole table proves closed
  int rw;
  // a third source of shards: the canonical table C that is already on the device (device_run_sequential).  Shard sh is the
  // closure of C inside its key range, built in each of the two rounds with room for dev_cap[sh] complements
  const u64 *dev_keys = NULL; const uint16_t *dev_cnt = NULL;
  int64_t dev_n = -1;                        // >= 0: this source
  std::vector<int64_t> dev_cap;
  float ms_close = 0;                        // device time of the range closures, both rounds
  int64_t missing = 0, nels = 0, nemit = 0;
  u64 fp[4] = { 0, 0, 0, 0 };
  float ms_p1 = 0, ms_look = 0, ms_p2 = 0;

  SeqRun(const smg_table_source *t, const smg_opts *o, int nshards, int64_t *p, const uint16_t *l, char *errbuf, size_t errlen)
    : tv(t), opts(o), n(nshards), W((t->kmer + 31) / 32), symcheck(o->symcheck == SMG_SYM_NONE ? SMG_SYM_HASH : o->symcheck),
      raw(o->condition != 0), plot(p), labels(l), eb(errbuf), el(errlen), cut((size_t) nshards + 1), counts((size_t) nshards * nshards, 0),
      nreq((size_t) nshards, 0), splitters((size_t) (nshards > 1 ? nshards - 1 : 1) * W, 0), codes((size_t) nshards), send((size_t) nshards),
      h_plot(SMG_PLOT_CELLS), rw(W) { }
};

// shard sh in the engine: a conditioned shard from host memory (it has no prefix index: pass 1 / k_directory build a
// directory), the closure of its key range of a canonical table on the device (no prefix index either), or its range of the
// part files, read and decoded
static int seq_load(SeqRun &s, int sh)
{ smg_engine *e = s.e;
  const smg_table_source *tv = s.tv;
  int rc;
  if (s.dev_n >= 0)
    { const uint64_t *lo = sh > 0 ? (const uint64_t *) &s.splitters[(size_t) (sh - 1) * s.W] : NULL;
      const uint64_t *hi = sh + 1 < s.n ? (const uint64_t *) &s.splitters[(size_t) sh * s.W] : NULL;
      bool not_canonical;
      e->own_keys.reset(); e->own_cnt.reset();           // (the shard before this one goes first: one shard at a time)
      e->tab.keys = NULL; e->tab.cnt = NULL;
      table_changed(e, 0);
      rc = close_canonical_range(e, tv->kmer, s.dev_n, s.dev_keys, s.dev_cnt, lo, hi, s.dev_cap[(size_t) sh], NULL, &not_canonical, s.eb, s.el);
      if (rc == SMG_OK) s.ms_close += (float) e->st.ms_decode;
      return rc;
    }
  if (s.raw)
    { const HostShard &h = s.hshard[(size_t) sh];
      if ((rc = decode_begin(e, tv->kmer, tv->ibyte, h.n, s.eb, s.el))) return rc;
      if (h.n > 0 && (hipMemcpy(e->own_keys, h.keys.data(), sizeof(u64) * (size_t) h.n * s.W, hipMemcpyHostToDevice) != hipSuccess
                      || hipMemcpy(e->own_cnt, h.cnt.data(), sizeof(uint16_t) * (size_t) h.n, hipMemcpyHostToDevice) != hipSuccess))
        return fail(s.eb, s.el, SMG_ENODEV, "host to device copy failed%s");
    }
  else
    { const int64_t lo = s.cut[sh];
      if ((rc = ingest_range(e, tv, lo, s.cut[sh + 1], s.d_index, s.opts->device, tv->host_threads, NULL, NULL, s.eb, s.el))) return rc;
      if ((rc = smg_engine_set_prefix_index(e, s.d_index, tv->ibyte, lo, s.eb, s.el))) return rc;
    }
  if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(s.eb, s.el, SMG_ENODEV, "decode failed%s");
  return SMG_OK;
}

// round 1 of shard sh: pass 1, its requests grouped by destination and its code bytes kept, its k-mers dropped
static int seq_round1(SeqRun &s, int sh)
{ smg_engine *e = s.e;
  int rc = seq_load(s, sh);
  if (rc) return rc;
  const int64_t ns = e->tab.n;
  e->set.bm_want = 32;
  if ((rc = smg_engine_pass1(e, s.symcheck, s.eb, s.el))) return rc;
  s.rw = smg_engine_record_words(e);
  s.nreq[sh] = smg_engine_nreq(e);
  if (s.send[sh].alloc(sizeof(uint64_t) * (size_t) (s.nreq[sh] > 0 ? s.nreq[sh] : 1) * s.rw) != hipSuccess
      || s.codes[sh].alloc((size_t) (ns > 0 ? ns : 1)) != hipSuccess)
    return fail(s.eb, s.el, SMG_ENOMEM, "out of device memory for what a shard leaves behind (1 byte per entry and its requests)%s");
  if ((rc = smg_engine_route(e, (const uint64_t *) s.splitters.data(), s.n, s.send[sh], s.nreq[sh], &s.counts[(size_t) sh * s.n], s.eb, s.el))) return rc;
  if (ns > 0 && hipMemcpy(s.codes[sh], e->deg, (size_t) ns, hipMemcpyDeviceToDevice) != hipSuccess) return fail(s.eb, s.el, SMG_ENODEV, "device copy failed%s");
  for (int q = 0; q < 4; q++) s.fp[q] ^= e->run.fp[q];
  s.ms_p1 += e->st.ms_pass1; s.nels += ns; s.nemit += e->st.nemitted;
  return SMG_OK;
}

// round 2 of shard sh: its code bytes back, the look-ups of all requests that name it, pass 2 into the one histogram, and
// -- the two members of a pair share a window block, hence a shard -- its part of the extract leg
static int seq_round2(SeqRun &s, int sh)
{ smg_engine *e = s.e;
  const int n = s.n;
  int rc = seq_load(s, sh);
  if (rc) return rc;
  // (k > 85: the counted kernels in the same steps -- what stays between the rounds is the degree byte)
  if ((rc = s.tv->kmer > FAST_MAX_K ? counted_resume(e, s.codes[sh], s.eb, s.el)
                                    : fast_resume(e, s.codes[sh], s.symcheck == SMG_SYM_EXACT, s.eb, s.el))) return rc;
  const int64_t *counts[SMG_MAXGPU]; const uint64_t *send[SMG_MAXGPU];
  for (int t = 0; t < n; t++) { counts[t] = &s.counts[(size_t) t * n]; send[t] = s.send[t]; }
  const int64_t nrecv = received_total(counts, n, sh);
  DevBuf<uint64_t> recv;
  if (recv.alloc(sizeof(uint64_t) * (size_t) (nrecv > 0 ? nrecv : 1) * s.rw) != hipSuccess)
    return fail(s.eb, s.el, SMG_ENOMEM, "out of device memory for a shard's requests%s");
  if (!gather_received(counts, n, sh, send, s.rw, recv)) return fail(s.eb, s.el, SMG_ENODEV, "device copy failed%s");
  int64_t miss = 0;
  if ((rc = smg_engine_apply(e, recv, nrecv, &miss, s.eb, s.el))) return rc;
  s.missing += miss;
  recv.reset();
  s.codes[sh].reset();
  if ((rc = smg_engine_pass2(e, s.d_plot, s.eb, s.el))) return rc;
  if (hipMemcpy(s.h_plot.data(), s.d_plot, sizeof(int64_t) * SMG_PLOT_CELLS, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(s.eb, s.el, SMG_ENODEV, "device to host copy failed%s");
  for (int cell = 0; cell < SMG_PLOT_CELLS; cell++) s.plot[cell] += s.h_plot[(size_t) cell];
  if (s.labels && !s.d_labels && (rc = upload_labels(s.labels, s.d_labels, s.eb, s.el))) return rc;
  if (s.labels && (rc = extract_to_host(e, s.d_labels, NULL, -1, s.xrec, s.eb, s.el))) return rc;
  smg_stats st2; smg_engine_stats(e, &st2);
  s.ms_look += st2.ms_rclookup; s.ms_p2 += st2.ms_pass2 > 0 ? st2.ms_pass2 : 0;
  return SMG_OK;
}

// the verdict over all shards, and what the caller gets
static int seq_result(SeqRun &s, const struct timespec &w0, smg_stats *stats, uint64_t **records, int64_t *nrec_out, int *rec_words)
{ if (!proof_holds(s.symcheck, s.missing, s.fp))
    return fail(s.eb, s.el, SMG_ENOTSYM, "the table is not closed under reverse complement with equal counts, and it does not fit the "
                "device in one piece: condition it first (smg_condition)%s");
  int rc;
  if (s.labels && (rc = records_to_caller(s.xrec, s.W + 1, s.labels, s.plot, records, nrec_out, rec_words, s.eb, s.el))) return rc;
  struct timespec w1;
  clock_gettime(CLOCK_MONOTONIC, &w1);
  smg_stats st; memset(&st, 0, sizeof(st));
  st.path = 1; st.key_words = s.W; st.nels = s.nels; st.nemitted = s.nemit; st.nrequests = s.nemit;
  st.ms_pass1 = s.ms_p1; st.ms_rclookup = s.ms_look; st.ms_pass2 = s.ms_p2;
  st.ms_total = (float) (((double) (w1.tv_sec - w0.tv_sec) + 1e-9 * (double) (w1.tv_nsec - w0.tv_nsec)) * 1e3);
  for (int cell = 0; cell < SMG_PLOT_CELLS; cell++) st.npairs += s.plot[cell];
  if (stats) *stats = st;
  if (s.opts->verbose)
    fprintf(stderr, "  [smg] n=%lld k=%d out of core: %d prefix shards one after the other, the table read twice; pass1 %.2f ms, "
            "rc-lookup %.2f, pass2 %.2f (sums over the shards), wall incl. both reads %.2f ms\n",
            (long long) s.nels, s.tv->kmer, s.n, s.ms_p1, s.ms_look, s.ms_p2, st.ms_total);
  return SMG_OK;
}

// nshards (2 .. 16, run_mode_plan) prefix shards one after the other on opts->device
static int host_run_sequential(const smg_table_source *tv, const smg_opts *opts, int nshards, int64_t *plot, smg_stats *stats,
                               char *errbuf, size_t errlen, const uint16_t *labels = NULL, uint64_t **records = NULL,
                               int64_t *nrec_out = NULL, int *rec_words = NULL)
{ SeqRun s(tv, opts, nshards, plot, labels, errbuf, errlen);
  const int n = s.n;
  multi_cuts(tv, n, s.cut.data());
  for (int sh = 0; sh < n; sh++)          // (a forced shard count -- SMG_SEQUENTIAL_SHARDS -- may leave a shard too large to index)
    if (s.cut[sh + 1] - s.cut[sh] >= SMG_ONE_SHARD_MAX)
      return fail(errbuf, errlen, SMG_EINVAL, "out of core: a shard of more than 2^32 entries (more shards are needed)%s");
  if (!s.raw) index_splitters(tv, s.cut.data(), n, s.W, s.splitters.data());
  if (!(s.e = s.eng.create(opts->device, errbuf, errlen))) return SMG_ENODEV;
  s.e->set.no_filter = true;                  // (k <= 85: no candidate map out of core -- the filter would need the maps of the shards not read yet)
  struct timespec w0;
  clock_gettime(CLOCK_MONOTONIC, &w0);
  int rc = upload_index(tv, s.d_index, "the table index", errbuf, errlen);
  if (rc) return rc;
  if (s.d_plot.alloc(sizeof(int64_t) * SMG_PLOT_CELLS) != hipSuccess) return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory for the table index%s");
  memset(plot, 0, sizeof(int64_t) * SMG_PLOT_CELLS);
  if (s.raw && (rc = host_condition_sequential(tv, opts, n, s.e, s.d_index, s.hshard, s.splitters, opts->verbose, errbuf, errlen))) return rc;
  for (int sh = 0; sh < n; sh++) if ((rc = seq_round1(s, sh))) return rc;
  for (int sh = 0; sh < n; sh++) if ((rc = seq_round2(s, sh))) return rc;
  return seq_result(s, w0, stats, records, nrec_out, rec_words);
}

// ---- a canonical table that is ALREADY ON THE DEVICE, in prefix shards of its closure one after the other --------------------
// What smg_hetmers_run_device does where the closed table is beyond one engine or does not fit in core (run_device_plan).
// The table C is trimmed once, up front, into an engine of its own that only holds it.  The 12-bit histogram of its entries
// and complements cuts the CLOSED table into shards of equal size (balanced_splitters); the histogram also gives every
// shard's size -- one at or above the shard limit raises the number of shards, up to 16 -- and the room its complements need.
// Then the two rounds of SeqRun, every shard built from C by close_canonical_range in each of them: nothing is written to
// disk, nothing leaves the device, and what is allocated beside C is one shard, the code bytes and the requests.
// *not_canonical: the table is not canonical (SMG_EINVAL, nothing has run): the caller takes the generic closure in core.
static int device_run_sequential(int kmer, int64_t nels, const u64 *d_keys, const uint16_t *d_cnt, const smg_opts *opts, int nshards,
                                 int64_t *plot, smg_stats *stats, bool *not_canonical, char *errbuf, size_t errlen)
{ *not_canonical = false;
  const int W = (kmer + 31) / 32, bits = symm_split_bits(kmer), nbin = 1 << bits;
  struct timespec w0;
  clock_gettime(CLOCK_MONOTONIC, &w0);
  EngineOwner holder;                        // (in front of the run: destroyed after it)
  smg_engine *te = holder.create(opts->device, errbuf, errlen);
  if (!te) return SMG_ENODEV;
  int rc;
  if ((rc = smg_engine_bind(te, kmer, nels, (const uint64_t *) d_keys, d_cnt, errbuf, errlen))) return rc;
  if ((opts->condition & SMG_COND_TRIM) && (rc = smg_engine_condition(te, opts->ethresh, 1, 0, NULL, errbuf, errlen))) return rc;
  const int64_t n = te->tab.n;
  { // canonical or not: the selection pass over an empty range keeps nothing and looks at every entry
    const uint64_t zero[4] = { 0, 0, 0, 0 };
    Dev rk, rcnt;
    int64_t m, a0, a1;
    if ((rc = range_select(te, kmer, n, te->tab.keys, te->tab.cnt, zero, zero, 0, rk, rcnt, &m, not_canonical, &a0, &a1, errbuf, errlen))) return rc;
    if (*not_canonical) return fail(errbuf, errlen, SMG_EINVAL, "table is not canonical%s");
  }
  std::vector<int64_t> hist((size_t) 2 * nbin, 0), cap;
  std::vector<u64> splitters;
  if ((rc = symm_hist_of(te, te->tab.keys, n, kmer, bits, hist.data(), errbuf, errlen))) return rc;
  const int64_t limit = device_shard_limit(true);
  int q = nshards;
  for (;; q++)
    { splitters.assign((size_t) (q - 1) * W, 0);
      cap.assign((size_t) q, 0);
      balanced_splitters(hist.data(), nbin, bits, q, W, splitters.data());
      int worst = 0;
      int64_t worst_size = -1;
      for (int sh = 0; sh < q; sh++)
        { int b0, b1;
          int64_t size = 0;
          range_bins(sh > 0 ? (const uint64_t *) &splitters[(size_t) (sh - 1) * W] : NULL,
                     sh + 1 < q ? (const uint64_t *) &splitters[(size_t) sh * W] : NULL, W, bits, &b0, &b1);
          for (int b = b0; b < b1; b++) { size += hist[(size_t) b] + hist[(size_t) nbin + b]; cap[(size_t) sh] += hist[(size_t) nbin + b]; }
          if (size > worst_size) { worst_size = size; worst = sh; }
        }
      if (worst_size < limit) break;
      if (q == SMG_MAXGPU)
        { if (errbuf && errlen)
            snprintf(errbuf, errlen, "prefix shard %d of %d of the closed table would hold %lld entries, one engine addresses fewer than %lld%s",
                     worst, q, (long long) worst_size, (long long) limit, DEVICE_TWO_STEP);
          return SMG_ENOMEM;
        }
    }
  if (opts->verbose)
    fprintf(stderr, "  [smg] %lld entries on the device%s: the closed table in %d prefix shards one after the other, every shard closed "
            "from the table on the device in each of the two rounds\n", (long long) n, (opts->condition & SMG_COND_TRIM) ? " after trimming" : "", q);
  smg_table_source tv; memset(&tv, 0, sizeof(tv));
  tv.kmer = kmer; tv.nels = n; tv.ibyte = 3;
  SeqRun s(&tv, opts, q, plot, NULL, errbuf, errlen);
  s.dev_keys = te->tab.keys; s.dev_cnt = te->tab.cnt; s.dev_n = n;
  s.dev_cap = cap;
  s.splitters = splitters;
  if (s.splitters.empty()) s.splitters.assign((size_t) W, 0);
  if (!(s.e = s.eng.create(opts->device, errbuf, errlen))) return SMG_ENODEV;
  s.e->set.no_filter = true;                  // (no candidate map: the filter would need the maps of the shards not built yet)
  if (s.d_plot.alloc(sizeof(int64_t) * SMG_PLOT_CELLS) != hipSuccess) return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory for the plot%s");
  memset(plot, 0, sizeof(int64_t) * SMG_PLOT_CELLS);
  for (int sh = 0; sh < q; sh++) if ((rc = seq_round1(s, sh))) return rc;
  for (int sh = 0; sh < q; sh++) if ((rc = seq_round2(s, sh))) return rc;
  if ((rc = seq_result(s, w0, stats, NULL, NULL, NULL))) return rc;
  if (stats) stats->ms_decode = s.ms_close;     // (conditioning, as in core: here the range closures of both rounds)
  if (opts->verbose) fprintf(stderr, "  [smg] range closures of the %d shards, both rounds: %.2f ms on the device\n", q, s.ms_close);
  return SMG_OK;
}
