// smg_count.hip -- k-mer counter for one MI355X (gfx950, wave64): FASTA / FASTQ / unaligned BAM in, canonical k-mer table out.
//
// What FastK does in front of `hetmers`, on the device (include/smg_count.h is the contract):
//   host    reader threads (one file each) strip records to sequence bytes, one separator byte between records, into
//           pinned blocks; the consumer copies them into the batch buffer on the device
//   batch   kc_extract<W>  bases -> canonical k-mers (left aligned, W = ceil(k/32) words), compacted
//           rocPRIM radix sort (W = 1: the keys themselves; W > 1: word by word, least significant first)
//           kc_flag_heads + scan + kc_runs + kc_run_counts: (k-mer, uint32 count) per distinct k-mer of the batch
//   merge   the batch list and the running distinct list are both duplicate free: after sorting their concatenation
//           a k-mer occurs at most twice and kc_merge_write adds the right-hand neighbour (uint32, saturating)
//   finish  kc_finish_flag (histogram, trim flag) + scan + kc_finish_compact (k-mers, uint16 counts clamped to 32767)
//   A block-gzipped (BGZF) file goes the same way: its reader thread copies whole members to the device, inf_members
//           inflates them one per wave and checks their CRC-32, and the text comes back to the same parser
//   A BAM file is a BGZF file whose text begins BAM\1: the reader thread frames its records on the host (fixed fields only)
//           and bam_unpack turns their 4-bit sequences into stripped bytes where the inflate kernel left the text; those
//           come back into the same ring.  Its bound is that of a BGZF file (the text), an over-estimate of its bases by
//           1.5 or more: it may be counted by key range where one pass would have done, with the same result
// A batch boundary never loses or doubles a window: a piece that does not continue the byte in front of it in the
// batch buffer is preceded by a separator and the last k-1 bytes of its file's stream (no whole window fits in those).
//
// Where one merge cannot be guaranteed to hold the distinct k-mers of the input, the run is partitioned by key range:
//   pack    kc_pack  every batch of bytes -> 3 bits per position (2-bit codes, validity) appended to a resident store
//   plan    kc_bins<false>  windows per bin of the leading 12 bits of the canonical k-mer; smg_count_plan cuts the 4096
//           bins into contiguous ranges whose windows (an upper bound of their distinct k-mers) stay within one sorted
//           batch or, where a single bin is larger than that, within one merge.  Only where a single bin is larger than
//           one merge: kc_bins<true>  the windows of that bin by their next 12 bits, and smg_count_plan_fine cuts the
//           whole bins and the 4096 sub-bins of every such bin, so that a range is an interval of the leading 24 bits
//   range   kc_extract_store<W, 12>  the store -> canonical k-mers of ONE range, the key buffer filled across the store
//           and sorted when full; then batch / merge / finish as above, the kept entries appended to the output table
//           (kc_extract_store<W, 24>: the same for a range with an end inside a split bin, its filter on 24 bits)
// Every instance of a k-mer lies in one range, so ranges in ascending order give the sorted table.
//
// The output table is host arrays, or (the _device entries) two whole allocations in device memory, which the caller
// hands to smg_engine_bind / smg_hetmers_run_device and frees; the kept entries of every range are appended to it.
//
// Where what is:
//   smg_count_kernels.hpp  all kc_* device code.  Earlier records (profiles/*.md) name kernels that have since been merged:
//                          kc_extract_packed<W> is kc_extract_store<W, 12>, kc_extract_fine<W> is kc_extract_store<W, 24>,
//                          kc_bins is kc_bins<false>, kc_subbins is kc_bins<true>, kc_bin / kc_bin24 are kc_bin<12> / kc_bin<24>
//   smg_count_reader.hpp   host only: the FASTA / FASTQ parser, the reader threads and their ring of blocks (read_files), the
//                          members of a BGZF file (bgzf_walk, bgzf_feed) and the Inflater they are handed to
//   smg_inflate.hpp        DEFLATE, one BGZF member per wave: inf_members and the decoder it shares with the host check
//   smg_bam.hpp            BAM: the framer of the records (host), bam_unpack and the tile logic it shares with the host check
//   smg_count_plan.hpp     host only: the memory plan, how buffers grow, the cuts of the key ranges
//   smg_count_parts.hpp    the parts of the device driver, each owning its buffers: Run (what they share), Batch, Distinct,
//                          Store, Table
//   this file              the driver itself (Counter: set-up, flush, the ranges, finish), the entry points and the C ABI

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <rocprim/rocprim.hpp>

#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "smg_count.h"
#include "smg_device.hpp"
#include "smg_keysort.hpp"
#include "smg_count_kernels.hpp"
#include "smg_count_reader.hpp"
#include "smg_count_plan.hpp"
#include "smg_count_parts.hpp"
#include "smg_inflate.hpp"
#include "smg_bam.hpp"

// where a run puts its results (the arguments of the C ABI)
struct Out
{ uint64_t **keys; uint16_t **counts; int64_t *nels; int *key_words; uint64_t *hist; smg_count_stats *stats; smg_count_parts *parts;
  bool dev_out;                                                // the table stays in device memory
};

struct Counter
{ Run x;
  Batch batch{ x };
  Distinct list{ x };
  Store store{ x };
  std::unique_ptr<Table> table;
  DevBuf<unsigned long long> dh;                               // the histogram of the counts, summed over the ranges
  bool parted = false;                                         // the batches are packed and counted by key range in finish()
  int req_parts = 0;

  // argument checks, the device, the memory plan (smg_count_plan.hpp), then the allocations it asks for
  int init(const smg_count_opts *o, const Out &io, int64_t bound, int nfiles, char *errbuf, size_t errlen)
  { x.errbuf = errbuf; x.errlen = errlen;
    if (io.parts)
      { if (io.parts->partitions < 0 || io.parts->partitions > SMG_COUNT_BINS)
          return fail(errbuf, errlen, SMG_EINVAL, "partitions = %d is out of range 0 .. %d", io.parts->partitions, SMG_COUNT_BINS);
        if (io.parts->max_entries < 0) return fail(errbuf, errlen, SMG_EINVAL, "max_entries = %lld is negative", (long long) io.parts->max_entries);
        req_parts = io.parts->partitions; list.max_entries = io.parts->max_entries;
      }
    x.pt.used = 1;
    x.k = o->kmer; x.t = o->minval; x.W = count_words(x.k);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
      return fail(errbuf, errlen, SMG_ENODEV, "no HIP device: the k-mer counter has no CPU fallback%s", "");
    if (o->device < 0 || o->device >= ndev) return fail(errbuf, errlen, SMG_EINVAL, "device %d of %d", o->device, ndev);
    DCHK(hipSetDevice(o->device));
    size_t free_b = 0;
    RCHK(x.free_bytes(&free_b));
    const char *hook = getenv("SMG_COUNT_BATCH_BASES");
    int64_t cap = 0, store_cap = 0;
    int32_t ranges = 0;
    RCHK(memory_plan(x.k, free_b, bound, req_parts, list.max_entries, hook ? atoll(hook) : 0, &cap, &ranges, &store_cap, errbuf, errlen));
    parted = ranges != 0;
    DCHK(hipStreamCreate(&x.stream));
    DCHK(hipEventCreate(&x.ev0));
    DCHK(hipEventCreate(&x.ev1));
    RCHK(batch.init(cap, nfiles));
    if (parted) RCHK(store.init(store_cap));
    if (io.dev_out) table.reset(new DeviceTable(x)); else table.reset(new HostTable(x));
    return 0;
  }

  int add(const uint8_t *p, int64_t n, int file) { return batch.add(p, n, file, [&] { return flush(); }); }

  // the batch buffer -> (k-mer, count) runs -> merged into the distinct list (a partitioned run packs it instead)
  int flush()
  { if (parted) return store.pack(batch);
    const int64_t n = batch.take();
    if (n < x.k) return 0;
    x.st.batches++;
    int64_t nwin = 0;
    RCHK(batch.extract(n, &nwin));
    return nwin ? list.count_keys(batch, nwin) : 0;
  }

  // histogram, clamp and trim of the distinct list, which is final; its kept entries go behind the output table
  int finish_range()
  { const int64_t nd = list.nd;
    int64_t kept = 0;
    DevBuf<uint32_t> ff, fp;
    DevBuf<u64> ok;
    DevBuf<uint16_t> oc;
    x.tic();
    if (nd > 0)
      { RCHK(x.alloc(ff, sizeof(uint32_t) * (size_t) nd)); RCHK(x.alloc(fp, sizeof(uint32_t) * (size_t) nd));
        LAUNCH(kc_finish_flag, ngrid(nblk(nd)), list.dc, nd, (unsigned) x.t, dh, ff);
        DCHK(scan_flags(ff, fp, nd, x.stream, x.tmp, &kept));
        RCHK(x.alloc(ok, sizeof(u64) * (size_t) kept * x.W)); RCHK(x.alloc(oc, sizeof(uint16_t) * (size_t) kept));
        LAUNCH_W(kc_finish_compact, nblk(nd), list.dk, list.dc, ff, fp, nd, ok, oc);
        DCHK(hipGetLastError());
      }
    RCHK(x.toc(&x.st.ms_finish));
    x.st.distinct += nd;
    x.st.kept += kept;
    RCHK(table->append(ok, oc, kept));
    list.clear();
    return 0;
  }

  // Entries one merge is guaranteed to hold, now that the store and the batch buffers are allocated: the smaller of the
  // uint32 limit of the scans and what is free, priced as merge() prices it (less a reserve for the sort's scratch).
  int merge_budget(int64_t *budget)
  { size_t free_b = 0;
    RCHK(x.free_bytes(&free_b));
    const size_t reserve = (size_t) 320 << 20;
    int64_t b = free_b > reserve ? (int64_t) ((free_b - reserve) / merge_price(x.W)) : 0;
    if (b > 0xFFFFFFEFll) b = 0xFFFFFFEFll;
    if (list.max_entries && b > list.max_entries) b = list.max_entries;
    if (b < 1)
      return fail(x.errbuf, x.errlen, SMG_ENOMEM, "no device memory is left for a merge: %.3f GB are free next to the packed input (%.3f GB) "
                  "and the batch buffers", (double) free_b * 1e-9, (double) x.pt.store_bytes * 1e-9);
    *budget = b;
    return 0;
  }

  // The cuts, from the bin histogram.  Automatic mode: ranges of one sorted batch each, which never merge (an extra pass
  // over the store costs less than the merge it saves, profiles/count_partitioned.md); where a single bin is above a
  // batch, the merge limit is the budget; where a single bin is above that as well, every such bin is split on its next 12
  // bits (one kc_bins<true> pass over the store each) and the flat plan over whole bins and sub-bins makes the cuts.
  int plan_ranges(RangePlan &rp)
  { int64_t budget = 0;
    RCHK(merge_budget(&budget));
    int rc = SMG_ENOMEM;
    if (req_parts == 0 && batch.cap < budget) rc = plan(rp.bins.data(), batch.cap, 0, rp.cuts.data(), &rp.nranges, x.errbuf, x.errlen);
    if (rc == SMG_ENOMEM) rc = plan(rp.bins.data(), budget, req_parts, rp.cuts.data(), &rp.nranges, x.errbuf, x.errlen);
    if (rc != SMG_ENOMEM)
      { for (int r = 0; r <= rp.nranges && rc == 0; r++) rp.cuts[(size_t) r] <<= SMG_COUNT_BIN_BITS;
        return rc;
      }
    uint64_t total = 0;
    for (int b = 0; b < SMG_COUNT_BINS; b++)
      { total += rp.bins[(size_t) b];
        if (rp.bins[(size_t) b] > (uint64_t) budget) rp.split.push_back(b);
      }
    rp.sub.assign(rp.split.size() * SMG_COUNT_BINS, 0);
    for (size_t s = 0; s < rp.split.size(); s++) RCHK(store.histogram<true>((unsigned) rp.split[s], rp.sub.data() + s * SMG_COUNT_BINS));
    uint64_t room = 2 * (total / (uint64_t) budget) + 5;       // (two neighbouring ranges of a greedy plan hold more than the budget)
    if (room > (uint64_t) SMG_COUNT_FINE_BINS + 1) room = (uint64_t) SMG_COUNT_FINE_BINS + 1;
    rp.cuts.assign((size_t) room, 0);
    return plan_fine(rp.bins.data(), rp.split.data(), (int32_t) rp.split.size(), rp.sub.data(), budget, rp.cuts.data(), (int64_t) room, &rp.nranges,
                     x.errbuf, x.errlen);
  }

  // range r of the plan: its windows from the store into the key buffer, sorted and merged whenever the buffer is full
  int count_range(const RangePlan &rp, int r)
  { const int64_t cap = batch.cap;
    const unsigned lo = (unsigned) rp.cuts[(size_t) r], hi = (unsigned) rp.cuts[(size_t) r + 1];
    const bool fine = ((lo | hi) & (SMG_COUNT_BINS - 1u)) != 0;          // an end inside a split bin: the filter is on 24 bits,
    const unsigned flo = fine ? lo : lo >> SMG_COUNT_BIN_BITS, fhi = fine ? hi : hi >> SMG_COUNT_BIN_BITS;      // else on 12
    int64_t left = rp.below(hi) - rp.below(lo);                // windows of the range not yet in the key buffer
    if (left == 0) return 0;
    int64_t p = 0, have = 0;                                   // next store position, keys in the buffer
    DCHK(hipMemsetAsync(batch.ctr.p, 0, 16, x.stream));
    while (left > 0 && p < store.n)
      { // a span of s positions holds at most s windows: all that is left of the store if the rest of the range fits
        const int64_t room = cap - have;
        const int64_t p1 = left <= room ? store.n : (p + room < store.n ? p + room : store.n);
        const unsigned ntiles = (unsigned) ((p1 - 1) / KC_TILE - p / KC_TILE + 1);
        x.tic();
        with_words<4>(x.W, [&](auto w)
          { const auto kern = fine ? kc_extract_store<w(), SMG_COUNT_FINE_BITS> : kc_extract_store<w(), SMG_COUNT_BIN_BITS>;
            LAUNCH(kern, ntiles, store.code, store.val, store.n, p, p1, x.k, flo, fhi, batch.ka, (unsigned long long) cap, batch.ctr);
          });
        DCHK(hipGetLastError());
        unsigned long long now = 0;
        DCHK(hipMemcpyAsync(&now, batch.ctr.p, 8, hipMemcpyDeviceToHost, x.stream));
        RCHK(x.toc(&x.st.ms_extract));
        if ((int64_t) now > cap || (int64_t) now - have > left)
          return fail(x.errbuf, x.errlen, SMG_ENODEV, "internal error: %llu keys of range %d in a buffer of %lld, %lld were left",
                      now, r, (long long) cap, (long long) left);
        left -= (int64_t) now - have;
        have = (int64_t) now;
        p = p1;
        if (left > 0 && cap - have < (cap / 8 > 1 ? cap / 8 : 1))           // full (or nearly): sort it
          { x.st.batches++;
            RCHK(list.count_keys(batch, have));
            have = 0;
            DCHK(hipMemsetAsync(batch.ctr.p, 0, 16, x.stream));
          }
      }
    if (left != 0) return fail(x.errbuf, x.errlen, SMG_ENODEV, "internal error: %lld windows of range %d were not found again", (long long) left, r);
    if (have > 0) { x.st.batches++; RCHK(list.count_keys(batch, have)); }
    return finish_range();
  }

  // the ranges of a partitioned run, in ascending order
  int run_ranges()
  { const double t0 = now_ms();
    RangePlan rp;
    RCHK(store.histogram<false>(0u, rp.bins.data()));
    RCHK(plan_ranges(rp));
    x.pt.used = rp.nranges;
    x.pt.split = (int32_t) rp.split.size();
    x.pt.ms_plan = now_ms() - t0;
    rp.index();
    for (int r = 0; r < rp.nranges; r++) RCHK(count_range(rp, r));
    return 0;
  }

  // the last batch, then histogram, clamp, trim; the table goes to the caller
  int finish(const Out &io)
  { RCHK(flush());
    batch.seq.reset();
    RCHK(x.alloc(dh, sizeof(uint64_t) * SMG_COUNT_HIST));
    DCHK(hipMemsetAsync(dh.p, 0, sizeof(uint64_t) * SMG_COUNT_HIST, x.stream));
    if (parted) RCHK(run_ranges());
    batch.drop_keys(); store.drop();
    if (!table->any) RCHK(finish_range());                     // one pass; or no range held a window: a valid empty table
    if (io.hist) DCHK(hipMemcpy(io.hist, dh.p, sizeof(uint64_t) * SMG_COUNT_HIST, hipMemcpyDeviceToHost));
    RCHK(table->release(io.keys, io.counts, io.nels));
    *io.key_words = x.W;
    if (io.parts)
      { io.parts->used = x.pt.used; io.parts->store_bytes = x.pt.store_bytes; io.parts->ms_pack = x.pt.ms_pack; io.parts->ms_plan = x.pt.ms_plan;
        io.parts->split = x.pt.split;
      }
    return 0;
  }
};

// ---------------------------------------------------------------------------------------------------------------
//  the Inflater of the device: one per reader thread, on a stream of its own
// ---------------------------------------------------------------------------------------------------------------

static_assert(sizeof(InfBlock) == sizeof(BgzfBlock) && sizeof(BgzfBlock) == 20, "the kernel reads the reader's blocks as they are");

#define BAM_SLAB     ((size_t) 32 << 20)                       // output bytes of one launch of bam_unpack (a multiple of BAM_TILE)
#define BAM_MAX_DESC (BGZF_TEXT / 36 + 1)                      // records that begin in the text of one call: 36 bytes each at least
static_assert(BAM_SLAB % BAM_TILE == 0, "a slab is whole tiles");

struct DeviceInflater : Inflater
{ int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint8_t *h_text = nullptr, *d_chunk = nullptr, *d_text = nullptr;
  uint32_t *h_status = nullptr, *d_status = nullptr;
  InfBlock *d_blk = nullptr;
  double ms_kernel = 0;
  int64_t launches = 0;
  // the second step, for BAM: set up by the first piece that needs it (a file shows that it is BAM only in its text)
  size_t text_n = 0;                                           // text bytes of the last inflate call
  BamDesc *h_desc = nullptr, *d_desc = nullptr;
  uint8_t *h_out = nullptr, *d_out = nullptr;
  double ms_unpack = 0, ms_out_d2h = 0;                        // bam_unpack alone (HIP events); the copies of its output (host clock)
  struct BamNote { std::string path; int64_t records, bases; double ms[4]; };     // ms: as smg_count_bam_report gives them
  std::vector<BamNote> bam_files;
  double mark_inflate = 0, mark_unpack = 0, mark_d2h = 0;

  // pinned and device memory for a chunk, its blocks, their text and statuses; 0 or the HIP error
  hipError_t init(int dev)
  { device = dev;
    hipError_t e;
    if ((e = hipSetDevice(dev)) != hipSuccess) return e;
    if ((e = hipStreamCreate(&stream)) != hipSuccess) return e;
    if ((e = hipEventCreate(&ev0)) != hipSuccess || (e = hipEventCreate(&ev1)) != hipSuccess) return e;
    if ((e = hipHostMalloc((void **) &chunk, SMG_COUNT_BGZF_CHUNK, hipHostMallocDefault)) != hipSuccess) return e;
    if ((e = hipHostMalloc((void **) &blk, sizeof(BgzfBlock) * BGZF_MAX_BLOCKS, hipHostMallocDefault)) != hipSuccess) return e;
    if ((e = hipHostMalloc((void **) &h_text, BGZF_TEXT, hipHostMallocDefault)) != hipSuccess) return e;
    if ((e = hipHostMalloc((void **) &h_status, sizeof(uint32_t) * BGZF_MAX_BLOCKS, hipHostMallocDefault)) != hipSuccess) return e;
    if ((e = hipMalloc((void **) &d_chunk, SMG_COUNT_BGZF_CHUNK)) != hipSuccess) return e;
    if ((e = hipMalloc((void **) &d_blk, sizeof(InfBlock) * BGZF_MAX_BLOCKS)) != hipSuccess) return e;
    if ((e = hipMalloc((void **) &d_text, BGZF_TEXT)) != hipSuccess) return e;
    return hipMalloc((void **) &d_status, sizeof(uint32_t) * BGZF_MAX_BLOCKS);
  }
  ~DeviceInflater() override
  { (void) hipFree(d_out); (void) hipFree(d_desc); (void) hipHostFree(h_out); (void) hipHostFree(h_desc);
    (void) hipFree(d_status); (void) hipFree(d_text); (void) hipFree(d_blk); (void) hipFree(d_chunk);
    (void) hipHostFree(h_status); (void) hipHostFree(h_text); (void) hipHostFree(blk); (void) hipHostFree(chunk);
    if (ev0) (void) hipEventDestroy(ev0);
    if (ev1) (void) hipEventDestroy(ev1);
    if (stream) (void) hipStreamDestroy(stream);
  }

  const char *reason(int status) const override { return inflate_reason(status); }

  // H2D of the members, the kernel, D2H of statuses and text.  The reader has bounded every block: its payload lies
  // in the chunk, its text in BGZF_TEXT bytes, and the kernel stays inside both whatever the payload says.
  int inflate(int n, const uint8_t **text, int *bad, char *errbuf, size_t errlen) override
  { size_t in_end = 0, out_end = 0;
    for (int i = 0; i < n; i++)
      { const size_t ie = (size_t) blk[i].in_off + blk[i].clen, oe = (size_t) blk[i].out_off + blk[i].isize;
        if (ie > in_end) in_end = ie;
        if (oe > out_end) out_end = oe;
      }
    if (n < 1 || n > BGZF_MAX_BLOCKS || in_end > (size_t) SMG_COUNT_BGZF_CHUNK || out_end > BGZF_TEXT)
      return fail(errbuf, errlen, SMG_EINVAL, "internal error: %d BGZF blocks of %zu bytes with %zu bytes of text in one launch", n, in_end, out_end);
#define ICHK(call) do { const hipError_t _e = (call); if (_e != hipSuccess) \
      return fail(errbuf, errlen, _e == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV, "HIP error: %s (%s)", hipGetErrorString(_e), #call); } while (0)
    float ms = 0;
    ICHK(hipSetDevice(device));                                // (a reader thread has not chosen its device yet)
    ICHK(hipMemcpyAsync(d_chunk, chunk, in_end, hipMemcpyHostToDevice, stream));
    ICHK(hipMemcpyAsync(d_blk, blk, sizeof(InfBlock) * (size_t) n, hipMemcpyHostToDevice, stream));
    ICHK(hipEventRecord(ev0, stream));
    hipLaunchKernelGGL(inf_members, dim3((unsigned) n), dim3(64), 0, stream, d_chunk, d_blk, n, d_text, d_status);
    ICHK(hipGetLastError());
    ICHK(hipEventRecord(ev1, stream));
    ICHK(hipMemcpyAsync(h_status, d_status, sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost, stream));
    if (out_end) ICHK(hipMemcpyAsync(h_text, d_text, out_end, hipMemcpyDeviceToHost, stream));
    ICHK(hipStreamSynchronize(stream));
    ICHK(hipEventElapsedTime(&ms, ev0, ev1));
    ms_kernel += ms; launches++;
    text_n = 0;
    for (int i = 0; i < n; i++)
      if (h_status[i] != INF_OK) { *bad = i; return h_status[i] < INF_NSTATUS ? (int) h_status[i] : INF_NSTATUS; }
    *text = h_text;
    text_n = out_end;
    return 0;
  }

  void mark() override { mark_inflate = ms_kernel; mark_unpack = ms_unpack; mark_d2h = ms_out_d2h; }
  void note_bam(const char *path, const BamFramer &fr) override
  { bam_files.push_back(BamNote{ path, fr.records, fr.bases, { fr.ms_feed, ms_kernel - mark_inflate, ms_unpack - mark_unpack, ms_out_d2h - mark_d2h } }); }

  // H2D of the descriptors, then BAM_SLAB bytes of output at a time: bam_unpack over their tiles, D2H into pinned memory,
  // the sink.  The descriptors are checked against the text and the output here, and the kernel stays inside both anyway.
  int unpack(const BamDesc *d, size_t nd, size_t out_len, Sink &sink, char *errbuf, size_t errlen) override
  { if (nd > BAM_MAX_DESC || out_len > 0xFFFFFFFFu - 2 * BAM_SLAB || !bam_desc_ok(d, nd, text_n, out_len))
      return fail(errbuf, errlen, SMG_EINVAL, "internal error: %zu BAM records with %zu bases do not describe a text of %zu bytes", nd, out_len, text_n);
    if (out_len == 0) return 0;
    ICHK(hipSetDevice(device));
    if (!d_out)
      { ICHK(hipHostMalloc((void **) &h_desc, sizeof(BamDesc) * BAM_MAX_DESC, hipHostMallocDefault));
        ICHK(hipHostMalloc((void **) &h_out, BAM_SLAB, hipHostMallocDefault));
        ICHK(hipMalloc((void **) &d_desc, sizeof(BamDesc) * BAM_MAX_DESC));
        ICHK(hipMalloc((void **) &d_out, BAM_SLAB));
      }
    memcpy(h_desc, d, sizeof(BamDesc) * nd);
    ICHK(hipMemcpyAsync(d_desc, h_desc, sizeof(BamDesc) * nd, hipMemcpyHostToDevice, stream));
    for (size_t base = 0; base < out_len; base += BAM_SLAB)
      { const size_t len = out_len - base < BAM_SLAB ? out_len - base : BAM_SLAB;
        float ms = 0;
        ICHK(hipEventRecord(ev0, stream));
        hipLaunchKernelGGL(bam_unpack, dim3((unsigned) ((len + BAM_TILE - 1) / BAM_TILE)), dim3(BAM_LANES), 0, stream, d_text, (uint32_t) text_n,
                           d_desc, (uint32_t) nd, d_out, (uint32_t) base, (uint32_t) len);
        ICHK(hipGetLastError());
        ICHK(hipEventRecord(ev1, stream));
        ICHK(hipStreamSynchronize(stream));
        ICHK(hipEventElapsedTime(&ms, ev0, ev1));
        ms_unpack += ms;
        const double t0 = now_ms();
        ICHK(hipMemcpyAsync(h_out, d_out, len, hipMemcpyDeviceToHost, stream));
        ICHK(hipStreamSynchronize(stream));
        ms_out_d2h += now_ms() - t0;
        if (!sink.put(h_out, len)) return 1;
      }
    return 0;
  }
#undef ICHK
};

// a device inflater, or the error: the device is checked as Counter::init checks it
static int new_inflater(int device, std::unique_ptr<DeviceInflater> &out, char *errbuf, size_t errlen)
{ int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(errbuf, errlen, SMG_ENODEV, "no HIP device: the k-mer counter has no CPU fallback%s", "");
  if (device < 0 || device >= ndev) return fail(errbuf, errlen, SMG_EINVAL, "device %d of %d", device, ndev);
  out.reset(new DeviceInflater());
  const hipError_t e = out->init(device);
  if (e != hipSuccess)
    return fail(errbuf, errlen, e == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV, "cannot set up the BGZF inflater: %s", hipGetErrorString(e));
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
//  entry points
// ---------------------------------------------------------------------------------------------------------------

static int check_opts(const smg_count_opts *o, char *errbuf, size_t errlen)
{ if (!o) return fail(errbuf, errlen, SMG_EINVAL, "null options%s", "");
  if (o->kmer < SMG_COUNT_MIN_KMER || o->kmer > SMG_MAX_KMER)
    return fail(errbuf, errlen, SMG_EINVAL, "k = %d is out of range: the table has a 3-byte prefix index, so k must be %d .. %d",
                o->kmer, SMG_COUNT_MIN_KMER, SMG_MAX_KMER);
  if (o->minval < 1 || o->minval > SMG_COUNT_MAX_COUNT)
    return fail(errbuf, errlen, SMG_EINVAL, "count threshold %d is out of range 1 .. %d", o->minval, SMG_COUNT_MAX_COUNT);
  return 0;
}

// One run.  input_ok: the caller's check of its own arguments; survey(&bound): refuses what cannot be read before the
// device is touched and bounds the sequence bytes of the input; feed(counter, &t_read): adds all of it, sets st.bases and
// the time (now_ms) at which the last of it was read.
template <class Survey, class Feed>
static int count_run(const smg_count_opts *opts, const Out &io, bool input_ok, int nfiles, Survey &&survey, Feed &&feed, char *errbuf, size_t errlen)
{ const double t0 = now_ms();
  RCHK(check_opts(opts, errbuf, errlen));
  if (!input_ok || !io.keys || !io.counts || !io.nels || !io.key_words) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  int64_t bound = 0;
  RCHK(survey(&bound));
  Counter c;
  RCHK(c.init(opts, io, bound, nfiles, errbuf, errlen));
  double t_read = t0;
  RCHK(feed(c, &t_read));
  c.x.st.ms_read = t_read - t0;
  RCHK(c.finish(io));
  c.x.st.ms_wall = now_ms() - t0;
  if (io.stats) *io.stats = c.x.st;
  return 0;
}

#define RING_BLOCK ((size_t) 8 << 20)

// what the last call of this process that reads BAM (a counting call or smg_count_bam_strip) read from its BAM files, for the
// report of the executable and of tools/count_time.py (smg_count_bam_report)
static std::mutex bam_seen_m;
static std::vector<DeviceInflater::BamNote> bam_seen;

// (the inflaters of the reader threads that meet a BGZF file are set up by the survey, before Counter::init reads the
//  free device memory, so that the plan sees what is left)
static int count_files(const char *const *paths, int npaths, const smg_count_opts *opts, const Out &io, char *errbuf, size_t errlen)
{ std::vector<std::unique_ptr<DeviceInflater>> own;
  std::vector<Inflater *> infl;
  struct Seen                                                  // (the BAM files of this call, for smg_count_bam_report)
  { std::vector<std::unique_ptr<DeviceInflater>> &own;
    ~Seen()
    { std::lock_guard<std::mutex> lk(bam_seen_m);
      bam_seen.clear();
      try { for (auto &i : own) if (i) bam_seen.insert(bam_seen.end(), i->bam_files.begin(), i->bam_files.end()); }
      catch (...) { bam_seen.clear(); }                        // (out of memory: no report)
    }
  } seen{ own };
  return count_run(opts, io, paths && npaths >= 1, npaths,
    [&](int64_t *bound)
      { std::vector<char> bgzf;
        RCHK(survey_files(paths, npaths, opts->kmer, bound, errbuf, errlen, &bgzf));
        const int nthr = reader_threads(opts->host_threads, npaths);
        own.resize((size_t) nthr); infl.assign((size_t) nthr, nullptr);
        for (int f = 0; f < npaths; f++)
          if (bgzf[(size_t) f] && !own[(size_t) (f % nthr)])
            { RCHK(new_inflater(opts->device, own[(size_t) (f % nthr)], errbuf, errlen));
              infl[(size_t) (f % nthr)] = own[(size_t) (f % nthr)].get();
            }
        return 0;
      },
    [&](Counter &c, double *t_read)
      { const int nthr = reader_threads(opts->host_threads, npaths);
        std::vector<uint8_t *> pinned;
        struct Unpin { std::vector<uint8_t *> &v; ~Unpin() { for (uint8_t *p : v) (void) hipHostFree(p); } } unpin{ pinned };
        pinned.reserve((size_t) (2 * nthr + 2));
        for (int b = 0; b < 2 * nthr + 2; b++)
          { uint8_t *p = nullptr;
            if (hipHostMalloc((void **) &p, RING_BLOCK, hipHostMallocDefault) != hipSuccess)
              return fail(errbuf, errlen, SMG_ENOMEM, "cannot pin %zu bytes of host memory", RING_BLOCK);
            pinned.push_back(p);
          }
        return read_files(paths, npaths, nthr, pinned.data(), (int) pinned.size(), RING_BLOCK,
                          [&](const uint8_t *p, int64_t n, int file) { return c.add(p, n, file); }, &c.x.st.bases, t_read, errbuf, errlen,
                          infl.data());
      }, errbuf, errlen);
}

static int count_bases(const uint8_t *seq, int64_t n, const smg_count_opts *opts, const Out &io, char *errbuf, size_t errlen)
{ return count_run(opts, io, n >= 0 && (n == 0 || seq), 1,
    [&](int64_t *bound) { *bound = n; return 0; },
    [&](Counter &c, double *t_read)
      { const int64_t piece = (int64_t) 256 << 20;
        for (int64_t o = 0; o < n; o += piece) RCHK(c.add(seq + o, n - o < piece ? n - o : piece, 0));
        c.x.st.bases = n;
        *t_read = now_ms();
        return 0;
      }, errbuf, errlen);
}

// members and text bytes of a BGZF file; what is not BGZF is refused with the words of the counting calls
static int bgzf_scan(const char *path, int64_t *blocks, int64_t *text_bytes, char *errbuf, size_t errlen)
{ if (!path || !blocks || !text_bytes) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  uint8_t magic[2] = { 0, 0 };
  const ssize_t got = pread(fd, magic, 2, 0);
  int rc = bgzf_probe(fd, path, errbuf, errlen);
  if (rc == 1)
    rc = got == 2 && magic[0] == 0x1f && magic[1] == 0x8b
           ? fail(errbuf, errlen, SMG_EINVAL, "%s is gzip compressed: compressed input is not supported, decompress it first", path)
           : fail(errbuf, errlen, SMG_EINVAL, "%s is not BGZF: it does not begin with a gzip header", path);
  else if (rc == 0) rc = bgzf_walk(fd, path, blocks, text_bytes, errbuf, errlen);
  close(fd);
  return rc;
}

static int bgzf_inflate(const char *path, int32_t device, uint8_t **text, int64_t *n, double *ms_kernel, char *errbuf, size_t errlen)
{ if (!text || !n) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  int64_t blocks = 0, bytes = 0;
  RCHK(bgzf_scan(path, &blocks, &bytes, errbuf, errlen));
  std::unique_ptr<DeviceInflater> infl;
  RCHK(new_inflater(device, infl, errbuf, errlen));
  struct Fd { int fd; ~Fd() { if (fd >= 0) close(fd); } } f{ open(path, O_RDONLY) };
  if (f.fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  std::unique_ptr<uint8_t, void (*)(void *)> buf((uint8_t *) malloc((size_t) bytes + 1), free);
  if (!buf) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s", "");
  int64_t have = 0;
  RCHK(bgzf_feed(f.fd, path, *infl, [&](const uint8_t *t, size_t m)
    { if (have + (int64_t) m > bytes) return fail(errbuf, errlen, SMG_EFORMAT, "%s changed while it was read", path);
      memcpy(buf.get() + have, t, m); have += (int64_t) m;
      return 0;
    }, errbuf, errlen));
  *text = buf.release(); *n = have;
  if (ms_kernel) *ms_kernel = infl->ms_kernel;
  return 0;
}

// the stripped stream of inflated BAM text, every record by the host routine; pieces of `piece` bytes (0: one piece)
static int bam_text(const uint8_t *text, int64_t n, int64_t piece, uint8_t **seq, int64_t *nseq, char *errbuf, size_t errlen)
{ if (n < 0 || (n && !text) || piece < 0 || !seq || !nseq) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  BamFramer fr;
  fr.all_host = true;
  GrowSink sink;
  const int64_t step = piece ? piece : (n < (int64_t) BAM_MAX_PIECE ? n : (int64_t) BAM_MAX_PIECE);
  for (int64_t o = 0; o < n; o += step)
    { RCHK(fr.feed(text + o, (size_t) (n - o < step ? n - o : step), "<text>", errbuf, errlen));
      if (!fr.head.empty()) sink.put(fr.head.data(), fr.head.size());
    }
  RCHK(fr.finish("<text>", errbuf, errlen));
  if (!sink.p) sink.p = (uint8_t *) malloc(1);
  if (!sink.p) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s", "");
  *seq = sink.p; *nseq = (int64_t) sink.len;
  sink.p = nullptr;
  return 0;
}

// the stripped stream of a BAM file by the route of the counting calls
static int bam_strip(const char *path, int32_t device, uint8_t **seq, int64_t *nseq, int64_t *records, double *ms_kernel, char *errbuf, size_t errlen)
{ if (!seq || !nseq) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  int64_t blocks = 0, bytes = 0;
  RCHK(bgzf_scan(path, &blocks, &bytes, errbuf, errlen));
  std::unique_ptr<DeviceInflater> infl;
  RCHK(new_inflater(device, infl, errbuf, errlen));
  struct Fd { int fd; ~Fd() { if (fd >= 0) close(fd); } } f{ open(path, O_RDONLY) };
  if (f.fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  GrowSink sink;
  BamFramer fr;
  bool any = false;
  infl->mark();
  RCHK(bgzf_feed(f.fd, path, *infl, [&](const uint8_t *t, size_t m)
    { if (!any && m)
        { if (!is_bam_text(t, m)) return fail(errbuf, errlen, SMG_EINVAL, "%s is not BAM: its text does not begin with the magic BAM\\1", path);
          any = true;
        }
      return bam_piece(fr, t, m, path, *infl, sink, errbuf, errlen);
    }, errbuf, errlen));
  if (!any) return fail(errbuf, errlen, SMG_EINVAL, "%s is not BAM: it has no text", path);
  RCHK(fr.finish(path, errbuf, errlen));
  if (!sink.p) sink.p = (uint8_t *) malloc(1);
  if (!sink.p) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s", "");
  *seq = sink.p; *nseq = (int64_t) sink.len;
  sink.p = nullptr;
  if (records) *records = fr.records;
  if (ms_kernel) *ms_kernel = infl->ms_unpack;
  infl->note_bam(path, fr);
  std::lock_guard<std::mutex> lk(bam_seen_m);
  bam_seen = infl->bam_files;
  return 0;
}

static int bam_report(const char *path, int64_t *records, int64_t *bases, double *ms)
{ if (!path || !records || !bases) return SMG_EINVAL;
  std::lock_guard<std::mutex> lk(bam_seen_m);
  for (const DeviceInflater::BamNote &b : bam_seen)
    if (b.path == path)
      { *records = b.records; *bases = b.bases;
        if (ms) memcpy(ms, b.ms, sizeof(b.ms));
        return 0;
      }
  return SMG_EINVAL;
}

// ---------------------------------------------------------------------------------------------------------------
//  C ABI: no C++ exception crosses it
// ---------------------------------------------------------------------------------------------------------------

#define GUARD(expr) \
  try { return (expr); } \
  catch (const std::bad_alloc &) { return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s", ""); } \
  catch (const std::exception &x) { return fail(errbuf, errlen, SMG_ENODEV, "internal error: %s", x.what()); } \
  catch (...) { return fail(errbuf, errlen, SMG_ENODEV, "internal error%s", ""); }

#define TABLE_OUT uint64_t **keys, uint16_t **counts, int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen
#define OUT(parts, dev) Out{ keys, counts, nels, key_words, hist, stats, parts, dev }

extern "C" int smg_count_files(const char *const *paths, int npaths, const smg_count_opts *opts, TABLE_OUT)
{ GUARD(count_files(paths, npaths, opts, OUT(nullptr, false), errbuf, errlen)) }

extern "C" int smg_count_bases(const uint8_t *seq, int64_t n, const smg_count_opts *opts, TABLE_OUT)
{ GUARD(count_bases(seq, n, opts, OUT(nullptr, false), errbuf, errlen)) }

extern "C" int smg_count_files_parts(const char *const *paths, int npaths, const smg_count_opts *opts, smg_count_parts *parts, TABLE_OUT)
{ GUARD(count_files(paths, npaths, opts, OUT(parts, false), errbuf, errlen)) }

extern "C" int smg_count_bases_parts(const uint8_t *seq, int64_t n, const smg_count_opts *opts, smg_count_parts *parts, TABLE_OUT)
{ GUARD(count_bases(seq, n, opts, OUT(parts, false), errbuf, errlen)) }

extern "C" int smg_count_files_device(const char *const *paths, int npaths, const smg_count_opts *opts, smg_count_parts *parts, TABLE_OUT)
{ GUARD(count_files(paths, npaths, opts, OUT(parts, true), errbuf, errlen)) }

extern "C" int smg_count_bases_device(const uint8_t *seq, int64_t n, const smg_count_opts *opts, smg_count_parts *parts, TABLE_OUT)
{ GUARD(count_bases(seq, n, opts, OUT(parts, true), errbuf, errlen)) }

extern "C" void smg_count_device_free(void *d) { if (d) (void) hipFree(d); }

extern "C" int smg_count_plan(const uint64_t *windows, int64_t budget, int32_t partitions, int32_t *cuts, int32_t *nranges, char *errbuf,
                              size_t errlen)
{ GUARD(plan(windows, budget, partitions, cuts, nranges, errbuf, errlen)) }

extern "C" int smg_count_plan_fine(const uint64_t *windows, const int32_t *split, int32_t nsplit, const uint64_t *sub, int64_t budget,
                                   int32_t *cuts, int64_t cuts_cap, int32_t *nranges, char *errbuf, size_t errlen)
{ GUARD(plan_fine(windows, split, nsplit, sub, budget, cuts, cuts_cap, nranges, errbuf, errlen)) }

extern "C" int smg_count_memory_plan(int32_t kmer, uint64_t free_bytes, int64_t bound, int32_t partitions, int64_t max_entries, int64_t batch_bases,
                                     int64_t *cap, int32_t *parted, int64_t *store_cap, char *errbuf, size_t errlen)
{ GUARD(memory_plan(kmer, (size_t) free_bytes, bound, partitions, max_entries, batch_bases, cap, parted, store_cap, errbuf, errlen)) }

extern "C" int smg_count_parse(const char *path, uint8_t **seq, int64_t *n, char *errbuf, size_t errlen)
{ GUARD(parse_path(path, seq, n, errbuf, errlen)) }

extern "C" int smg_count_bgzf_scan(const char *path, int64_t *blocks, int64_t *text_bytes, char *errbuf, size_t errlen)
{ GUARD(bgzf_scan(path, blocks, text_bytes, errbuf, errlen)) }

extern "C" int smg_count_bgzf_inflate(const char *path, int32_t device, uint8_t **text, int64_t *n, double *ms_kernel, char *errbuf, size_t errlen)
{ GUARD(bgzf_inflate(path, device, text, n, ms_kernel, errbuf, errlen)) }

extern "C" int smg_count_bam_text(const uint8_t *text, int64_t n, int64_t piece, uint8_t **seq, int64_t *nseq, char *errbuf, size_t errlen)
{ GUARD(bam_text(text, n, piece, seq, nseq, errbuf, errlen)) }

extern "C" int smg_count_bam_strip(const char *path, int32_t device, uint8_t **seq, int64_t *nseq, int64_t *records, double *ms_kernel,
                                   char *errbuf, size_t errlen)
{ GUARD(bam_strip(path, device, seq, nseq, records, ms_kernel, errbuf, errlen)) }

extern "C" int smg_count_bam_report(const char *path, int64_t *records, int64_t *bases, double *ms)
{ try { return bam_report(path, records, bases, ms); } catch (...) { return SMG_ENOMEM; } }

extern "C" void smg_count_free(void *p) { free(p); }

extern "C" const char *smg_count_version(void) { return "smudgeplot_amd 0.5 (k-mer counter, gfx950)"; }
