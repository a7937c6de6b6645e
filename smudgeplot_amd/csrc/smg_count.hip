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
// A call that opted in (smg_count_opts.dump) reads k-mers that another tool has counted: text dumps, one line per k-mer.
//   host    the reader threads route the text as above and cut it into blocks of whole lines (DumpCutter, smg_dump.hpp)
//   batch   kd_lines<W>  the lines of the batch -> (canonical k-mer, uint32 count), the first bad line by atomicMin
//           pair sort, kc_flag_heads + scan, kd_run_sums + kd_run_clamp: one saturating sum per distinct k-mer of the batch
//   merge, finish  as above.  One pass only: the packed store is a store of reads
//
// An input may be a stream (standard input as "-", a FIFO, /dev/fd/N): opened once by the survey, told by its first bytes as a
// file is, and read forward only by the same reader thread, inflater and kernels.  A call with a stream has no bound on its
// input: stream_plan (smg_count_plan.hpp) plans it in the place of memory_plan, and the packed store grows as the stream goes on.
//
// The output table is host arrays, or (the _device entries) two whole allocations in device memory, which the caller
// hands to smg_engine_bind / smg_hetmers_run_device and frees; the kept entries of every range are appended to it.
//
// Where what is:
//   smg_count_kernels.hpp  all kc_* device code.  Earlier records (profiles/*.md) name kernels that have since been merged:
//                          kc_extract_packed<W> is kc_extract_store<W, 12>, kc_extract_fine<W> is kc_extract_store<W, 24>,
//                          kc_bins is kc_bins<false>, kc_subbins is kc_bins<true>, kc_bin / kc_bin24 are kc_bin<12> / kc_bin<24>
//   smg_count_reader.hpp   host only: the FASTA / FASTQ parser, what a file is by its first bytes (file_kind), the members of
//                          a BGZF file (bgzf_walk, bgzf_feed) and the Inflater they are handed to, the routing of one file
//                          (parse_file) and what it gives back (FileRead), the reader threads and their ring (read_files)
//   smg_inflate.hpp        DEFLATE, one BGZF member per wave: inf_members and the decoder it shares with the host check
//   smg_gzip.hpp           plain gzip, for a call that opted in: block finder, marker decoder, resolver and exact decoder (one text
//                          for the kernels and the host twin), the chain that builds the index of a file and the pass over it
//   smg_bam.hpp            BAM: the framer of the records (host), bam_unpack and the tile logic it shares with the host check
//   smg_count_plan.hpp     host only: the memory plan, how buffers grow, the cuts of the key ranges
//   smg_count_parts.hpp    the parts of the device driver, each owning its buffers: Run (what they share), Batch, Distinct,
//                          Store, Table; the one HIP check (DCHK), the device check, pinned memory that frees itself
//   smg_count_inflater.hpp the device stage of compressed input, a part like those: DeviceInflater (inflate, unpack), one per
//                          reader thread (with the gzip engine and the indexes of its gzip files), and the BGZF file a one-file
//                          route opens for an inflater of its own
//   smg_dump.hpp           k-mer dumps, host and device: the line decoder (one text for kd_lines and the host twin), the cutter
//                          that hands whole lines on, the twin itself
//   smg_count_dump.hpp     kd_lines, kd_run_sums, kd_run_clamp and the part that runs them: DumpFeed
//   this file              the driver itself (Counter: set-up, flush, the ranges, finish), the entry points (count_files,
//                          count_bases, the one-file routes, the report of the BAM files of the last call) and the C ABI

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
#include "smg_count_inflater.hpp"
#include "smg_count_dump.hpp"

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
  DumpFeed dump{ x, batch };                                   // (allocates only in a run over dumps)
  bool dumps = false;                                          // the input is k-mer dumps: lines, not windows
  std::unique_ptr<Table> table;
  DevBuf<unsigned long long> dh;                               // the histogram of the counts, summed over the ranges
  bool parted = false;                                         // the batches are packed and counted by key range in finish()
  int req_parts = 0;

  // argument checks, the device, the memory plan (smg_count_plan.hpp), then the allocations it asks for.  streams: the
  // call reads at least one stream, so bound covers its regular files only and the plan is stream_plan's: with no stream
  // in the call memory_plan decides, as it always did
  int init(const smg_count_opts *o, const Out &io, int64_t bound, int nfiles, char *errbuf, size_t errlen, const char *const *dump_paths = nullptr,
           bool streams = false)
  { x.errbuf = errbuf; x.errlen = errlen;
    dumps = dump_paths != nullptr;
    if (dumps && io.parts && io.parts->partitions > 1)
      return fail(errbuf, errlen, SMG_EINVAL, "partitions = %d with the dump option: k-mer dumps are counted in one pass (the packed store "
                  "is a store of reads), partitions must be 0 or 1", io.parts->partitions);
    if (io.parts)
      { if (io.parts->partitions < 0 || io.parts->partitions > SMG_COUNT_BINS)
          return fail(errbuf, errlen, SMG_EINVAL, "partitions = %d is out of range 0 .. %d", io.parts->partitions, SMG_COUNT_BINS);
        if (io.parts->max_entries < 0) return fail(errbuf, errlen, SMG_EINVAL, "max_entries = %lld is negative", (long long) io.parts->max_entries);
        req_parts = io.parts->partitions; list.max_entries = io.parts->max_entries;
      }
    x.pt.used = 1;
    x.k = o->kmer; x.t = o->minval; x.W = count_words(x.k);
    RCHK(check_device(o->device, errbuf, errlen));
    DCHK(hipSetDevice(o->device));
    size_t free_b = 0;
    RCHK(x.free_bytes(&free_b));
    const char *hook = getenv("SMG_COUNT_BATCH_BASES");
    int64_t cap = 0, store_cap = 0;
    int32_t ranges = 0;
    const char *store_hook = getenv("SMG_COUNT_STREAM_STORE");
    if (dumps) RCHK(dump_plan(free_b, bound, nfiles, hook ? atoll(hook) : 0, streams, &cap));
    else if (streams)
      RCHK(stream_plan(x.k, free_b, bound, req_parts, list.max_entries, hook ? atoll(hook) : 0, store_hook && atoll(store_hook) > 0 ? atoll(store_hook) : 0,
                       &cap, &ranges, &store_cap, errbuf, errlen));
    else RCHK(memory_plan(x.k, free_b, bound, req_parts, list.max_entries, hook ? atoll(hook) : 0, &cap, &ranges, &store_cap, errbuf, errlen));
    parted = ranges != 0;
    store.open_ended = streams;
    DCHK(hipStreamCreate(&x.stream));
    DCHK(hipEventCreate(&x.ev0));
    DCHK(hipEventCreate(&x.ev1));
    RCHK(batch.init(cap, nfiles));
    if (parted) RCHK(store.init(store_cap));
    if (dumps) RCHK(dump.init(dump_paths, nfiles));
    if (io.dev_out) table.reset(new DeviceTable(x)); else table.reset(new HostTable(x));
    return 0;
  }

  // The plan of a run over dumps, before the first allocation.  bound: the text bytes of the files at most, so lines =
  // bound / (k + 3) + one per file bounds the lines, the records and every merge.  The batch is what smg_count_memory_plan
  // gives a single pass over that many bytes (the hook: text bytes), at least one longest line; then the one merge that may
  // hold every line must fit next to it, or the call is refused here.  With a stream in the call (streams) nothing bounds the
  // lines: the batch is that of one pass of stream_plan, and what does not fit is refused by the merge that meets it.
  int dump_plan(size_t free_b, int64_t bound, int nfiles, int64_t hook, bool streams, int64_t *cap)
  { int32_t ranges = 0;
    int64_t store_cap = 0;
    if (streams) RCHK(stream_plan(x.k, free_b, bound, 1, 0, hook, 0, cap, &ranges, &store_cap, x.errbuf, x.errlen));
    else RCHK(memory_plan(x.k, free_b, bound, 1, 0, hook, cap, &ranges, &store_cap, x.errbuf, x.errlen));
    if (*cap < SMG_COUNT_DUMP_LINE) *cap = SMG_COUNT_DUMP_LINE;
    if (streams) return 0;
    const int64_t lines = bound / (x.k + 3) + nfiles;
    if (lines >= 0xFFFFFFF0ll)
      return fail(x.errbuf, x.errlen, SMG_ENOMEM, "dumps of %lld text bytes may hold %lld lines of %d bases, one merge holds 2^32 - 16 entries: "
                  "k-mer dumps are counted in one pass", (long long) bound, (long long) lines, x.k);
    const size_t want = (size_t) (*cap * batch_price(x.W)) + dump_price(*cap, x.k) + (size_t) lines * merge_price(x.W) + CP_RESERVE;
    if (want > free_b)
      return fail(x.errbuf, x.errlen, SMG_ENOMEM, "dumps of %lld text bytes may hold %lld lines of %d bases: a batch of %lld bytes and one merge "
                  "of that many entries need %.3f GB, %.3f GB of device memory are free, and k-mer dumps are counted in one pass",
                  (long long) bound, (long long) lines, x.k, (long long) *cap, (double) want * 1e-9, (double) free_b * 1e-9);
    return 0;
  }

  int add(const uint8_t *p, int64_t n, int file)
  { if (dumps) return dump.add(p, n, file, [&] { return flush(); });
    return batch.add(p, n, file, [&] { return flush(); });
  }

  // the batch buffer -> (k-mer, count) runs -> merged into the distinct list (a partitioned run packs it instead)
  int flush()
  { if (parted) return store.pack(batch);
    const int64_t n = batch.take();
    if (dumps)
      { int64_t nl = 0;
        if (n == 0) return 0;
        x.st.batches++;
        RCHK(dump.extract(n, &nl));
        return nl ? dump.count(list, nl) : 0;
      }
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
    if (dumps) x.st.bases = x.st.windows * x.k;
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

// One run.  input_ok: the caller's check of its own arguments; survey(&bound, &streams): refuses what cannot be read before
// the device is touched and bounds the sequence bytes of the input (*streams: of its regular files only, there are streams
// among the inputs); feed(counter, &t_read): adds all of it, sets st.bases and
// the time (now_ms) at which the last of it was read.
template <class Survey, class Feed>
static int count_run(const smg_count_opts *opts, const Out &io, bool input_ok, int nfiles, Survey &&survey, Feed &&feed, char *errbuf, size_t errlen,
                     const char *const *dump_paths = nullptr)
{ const double t0 = now_ms();
  RCHK(check_opts(opts, errbuf, errlen));
  if (!input_ok || !io.keys || !io.counts || !io.nels || !io.key_words) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  int64_t bound = 0;
  bool streams = false;
  RCHK(survey(&bound, &streams));
  Counter c;
  RCHK(c.init(opts, io, bound, nfiles, errbuf, errlen, dump_paths, streams));
  double t_read = t0;
  RCHK(feed(c, &t_read));
  c.x.st.ms_read = t_read - t0;
  RCHK(c.finish(io));
  c.x.st.ms_wall = now_ms() - t0;
  if (io.stats) *io.stats = c.x.st;
  return 0;
}

#define RING_BLOCK ((size_t) 8 << 20)

// What the last call of this process that reads BAM (a counting call over files or smg_count_bam_strip) read from the BAM
// files it read to their end, for the report of the executable and of tools/count_time.py (smg_count_bam_report).
struct BamSeen { std::string path; FileRead read; };
static std::mutex bam_seen_m;
static std::vector<BamSeen> bam_seen;

// the one way that table is written: the BAM files among paths[f] with files[f], thread by thread as nthr readers took them
static void publish_bam(const char *const *paths, const std::vector<FileRead> &files, int nthr)
{ std::lock_guard<std::mutex> lk(bam_seen_m);
  bam_seen.clear();
  try
    { for (int j = 0; j < nthr; j++)
        for (size_t f = (size_t) j; f < files.size(); f += (size_t) nthr)
          if (files[f].route == ROUTE_BAM) bam_seen.push_back(BamSeen{ paths[f], files[f] });
    }
  catch (...) { bam_seen.clear(); }                            // (out of memory: no report)
}

static int bam_report(const char *path, int64_t *records, int64_t *bases, double *ms)
{ if (!path || !records || !bases) return SMG_EINVAL;
  std::lock_guard<std::mutex> lk(bam_seen_m);
  for (const BamSeen &b : bam_seen)
    if (b.path == path)
      { *records = b.read.records; *bases = b.read.bases;
        if (ms) { ms[0] = b.read.ms_frame; ms[1] = b.read.dev.inflate; ms[2] = b.read.dev.unpack; ms[3] = b.read.dev.d2h; }
        return 0;
      }
  return SMG_EINVAL;
}

// What the last call of this process that reads plain gzip read of every such file (smg_count_gzip_report): a counting call
// that opted in, smg_count_gzip_inflate, smg_count_gzip_text_host.
struct GzSeen { std::string path; int64_t members, text, spans, linked, repaired; double ms[3]; };
static std::mutex gz_seen_m;
static std::vector<GzSeen> gz_seen;

static void publish_gzip(const char *path, const GzIndex *ix, bool more = false)
{ std::lock_guard<std::mutex> lk(gz_seen_m);
  if (!more) gz_seen.clear();
  try { if (ix) gz_seen.push_back(GzSeen{ path, (int64_t) ix->mem.size(), ix->text, ix->spans, ix->linked, ix->repaired, { ix->ms[0], ix->ms[1], ix->ms[2] } }); }
  catch (...) { gz_seen.clear(); }
}

static int gzip_report(const char *path, int64_t *members, int64_t *text_bytes, int64_t *spans, int64_t *linked, int64_t *repaired, double *ms)
{ if (!path || !members || !text_bytes || !spans || !linked || !repaired) return SMG_EINVAL;
  std::lock_guard<std::mutex> lk(gz_seen_m);
  for (const GzSeen &g : gz_seen)
    if (g.path == path)
      { *members = g.members; *text_bytes = g.text; *spans = g.spans; *linked = g.linked; *repaired = g.repaired;
        if (ms) { ms[0] = g.ms[0]; ms[1] = g.ms[1]; ms[2] = g.ms[2]; }
        return 0;
      }
  return SMG_EINVAL;
}

// (the inflaters of the reader threads that meet a BGZF file are set up by the survey, before Counter::init reads the
//  free device memory, so that the plan sees what is left; the indexes of the plain gzip files of a call that opted in are
//  built there too, once every file of the call has been looked at: they give the text bytes the bound needs)
struct Inputs
{ std::vector<std::unique_ptr<DeviceInflater>> own;
  std::vector<Inflater *> infl;
  int nthr = 1;
  std::vector<std::unique_ptr<Taken>> taken;                   // per path: the stream the survey opened, for its reader thread
  bool streams = false;                                        // there is one: the bound is that of the regular files only

  // what survey_files refuses and bounds; then the reader threads, an inflater for each that meets a compressed file, and the
  // indexes of the plain gzip files.  A call over dumps: a plain file that does not begin with a base is refused here too,
  // before the device is touched (the text of a compressed one is first seen by its reader thread, which says the same).
  // A stream is opened here, once, and told by the bytes taken from it, which decide all this as those of a file do.
  int survey(const char *const *paths, int npaths, const smg_count_opts *opts, int64_t *bound, char *errbuf, size_t errlen)
  { std::vector<char> bgzf;
    RCHK(survey_files(paths, npaths, opts->kmer, bound, errbuf, errlen, &bgzf, opts->gzip != 0, &taken));
    for (const std::unique_ptr<Taken> &t : taken) streams = streams || t;
    for (int f = 0; f < npaths && opts->dump; f++)
      if (bgzf[(size_t) f] == FILE_PLAIN)
        { uint8_t first = 0;
          bool any = false;
          struct NoSink { bool put(const uint8_t *, size_t) { return true; } size_t room() const { return (size_t) -1; } bool cut() { return true; } } none;
          if (taken[(size_t) f])
            { any = taken[(size_t) f]->src.take(1) >= 1;
              if (any) first = taken[(size_t) f]->src.taken()[0];
            }
          else
            { const Fd fd(paths[f]);
              any = fd.fd >= 0 && pread(fd.fd, &first, 1, 0) == 1;
            }
          if (any) RCHK(DumpCutter<NoSink>(none).feed(&first, 1, paths[f], errbuf, errlen));
        }
    nthr = reader_threads(opts->host_threads, npaths);
    own.resize((size_t) nthr); infl.assign((size_t) nthr, nullptr);
    for (int f = 0; f < npaths; f++)
      if (bgzf[(size_t) f] && !own[(size_t) (f % nthr)])
        { RCHK(new_inflater(opts->device, own[(size_t) (f % nthr)], errbuf, errlen));
          infl[(size_t) (f % nthr)] = own[(size_t) (f % nthr)].get();
        }
    for (int f = 0; f < npaths; f++)
      if (bgzf[(size_t) f] == FILE_GZIP)
        { const Fd fd(paths[f]);
          int64_t text = 0;
          if (fd.fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", paths[f]);
          RCHK(own[(size_t) (f % nthr)]->gzip_survey(fd.fd, paths[f], 0, &text, errbuf, errlen));
          *bound += text;
        }
    return 0;
  }
};

static int count_files(const char *const *paths, int npaths, const smg_count_opts *opts, const Out &io, char *errbuf, size_t errlen)
{ Inputs in;
  std::vector<std::unique_ptr<DeviceInflater>> &own = in.own;
  std::vector<Inflater *> &infl = in.infl;
  int &nthr = in.nthr;
  const bool dumps = opts && opts->dump != 0;
  publish_bam(paths, std::vector<FileRead>(), 1);              // (whatever becomes of this call, the report of an earlier one is gone)
  publish_gzip(nullptr, nullptr);
  const auto report_gzip = [&]
    { for (const std::unique_ptr<DeviceInflater> &d : own)
        if (d) for (const auto &g : d->gz_index) publish_gzip(g.first.c_str(), &g.second, true);
    };
  const int rc = count_run(opts, io, paths && npaths >= 1, npaths,
    [&](int64_t *bound, bool *streams)
      { const int rc = in.survey(paths, npaths, opts, bound, errbuf, errlen);
        *streams = in.streams;
        return rc;
      },
    [&](Counter &c, double *t_read)
      { std::vector<Pinned<uint8_t>> pinned((size_t) (2 * nthr + 2));
        std::vector<uint8_t *> blocks;
        for (Pinned<uint8_t> &b : pinned)
          { if (b.alloc(RING_BLOCK) != hipSuccess) return fail(errbuf, errlen, SMG_ENOMEM, "cannot pin %zu bytes of host memory", RING_BLOCK);
            blocks.push_back(b);
          }
        std::vector<FileRead> files;
        const int rc = read_files(paths, npaths, nthr, blocks.data(), (int) blocks.size(), RING_BLOCK,
                                  [&](const uint8_t *p, int64_t n, int file) { return c.add(p, n, file); }, &c.x.st.bases, t_read, &files,
                                  errbuf, errlen, infl.data(), dumps, in.taken.data());
        publish_bam(paths, files, nthr);                       // (after an error too: the files read to their end before it)
        return rc;
      }, errbuf, errlen, dumps ? paths : nullptr);
  report_gzip();
  return rc;
}

static int count_bases(const uint8_t *seq, int64_t n, const smg_count_opts *opts, const Out &io, char *errbuf, size_t errlen)
{ if (opts && opts->dump) return fail(errbuf, errlen, SMG_EINVAL, "the dump option reads files: a buffer of sequence bytes is no k-mer dump%s", "");
  return count_run(opts, io, n >= 0 && (n == 0 || seq), 1,
    [&](int64_t *bound, bool *) { *bound = n; return 0; },
    [&](Counter &c, double *t_read)
      { const int64_t piece = (int64_t) 256 << 20;
        for (int64_t o = 0; o < n; o += piece) RCHK(c.add(seq + o, n - o < piece ? n - o : piece, 0));
        c.x.st.bases = n;
        *t_read = now_ms();
        return 0;
      }, errbuf, errlen);
}

// the text of a whole BGZF file, inflated as the counting calls inflate it
static int bgzf_inflate(const char *path, int32_t device, uint8_t **text, int64_t *n, double *ms_kernel, char *errbuf, size_t errlen)
{ if (!text || !n) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  BgzfInput in;
  RCHK(in.open(path, device, errbuf, errlen));
  GrowSink sink;
  sink.reserve((size_t) in.text_bytes + 1);
  RCHK(bgzf_feed(in.src, path, *in.infl, [&](const uint8_t *t, size_t m)
    { if ((int64_t) (sink.len + m) > in.text_bytes) return fail(errbuf, errlen, SMG_EFORMAT, "%s changed while it was read", path);
      sink.put(t, m);
      return 0;
    }, errbuf, errlen));
  if (ms_kernel) *ms_kernel = in.infl->ms.inflate;
  return sink.hand_over(text, n, errbuf, errlen);
}

// what a one-file gzip route is given: a gzip file (BGZF is one), opened
static int gzip_open(const char *path, std::unique_ptr<Fd> &file, char *errbuf, size_t errlen)
{ if (!path) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  RCHK(refuse_stream(path, errbuf, errlen));
  file.reset(new Fd(path));
  if (file->fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  Source src(file->fd, false);
  const int kind = file_kind(src, path, errbuf, errlen, true);
  if (kind < 0) return kind;
  if (kind == FILE_PLAIN) return fail(errbuf, errlen, SMG_EINVAL, "%s is not gzip: it does not begin with a gzip header", path);
  return 0;
}

// the text of a whole gzip file by the route of the counting calls: the index, then the exact decoder over it
static int gzip_inflate(const char *path, int32_t device, int64_t span_bytes, uint8_t **text, int64_t *n, double *ms_kernel, char *errbuf, size_t errlen)
{ if (!text || !n) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  publish_gzip(nullptr, nullptr);
  std::unique_ptr<Fd> file;
  RCHK(gzip_open(path, file, errbuf, errlen));
  std::unique_ptr<DeviceInflater> infl;
  RCHK(new_inflater(device, infl, errbuf, errlen));
  int64_t bytes = 0;
  RCHK(infl->gzip_survey(file->fd, path, span_bytes, &bytes, errbuf, errlen));
  GrowSink sink;
  sink.reserve((size_t) bytes + 1);
  RCHK(infl->gzip_text(file->fd, path, [&](const uint8_t *t, size_t m)
    { if ((int64_t) (sink.len + m) > bytes) return fail(errbuf, errlen, SMG_EFORMAT, "%s changed while it was read", path);
      sink.put(t, m);
      return 0;
    }, errbuf, errlen));
  const GzIndex &ix = infl->gz_index[path];
  if (ms_kernel) { ms_kernel[0] = ix.ms[0]; ms_kernel[1] = ix.ms[1]; ms_kernel[2] = ix.ms[2]; }
  publish_gzip(path, &ix);
  return sink.hand_over(text, n, errbuf, errlen);
}

// the same by the host twin: finder, marker decoder, chain, resolver and exact decoder as one lane (a test twin, no fallback)
static int gzip_text_host(const char *path, int64_t span_bytes, uint8_t **text, int64_t *n, char *errbuf, size_t errlen)
{ if (!text || !n) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  publish_gzip(nullptr, nullptr);
  std::unique_ptr<Fd> file;
  RCHK(gzip_open(path, file, errbuf, errlen));
  uint32_t span = 0;
  RCHK(gz_span(span_bytes, &span, errbuf, errlen));
  GzHostEngine e;
  GzIndex ix;
  std::vector<uint8_t> bytes;
  RCHK(gz_text_host(file->fd, path, span, BGZF_TEXT, GZ_MAX_PIECE, e, ix, bytes, errbuf, errlen));
  GrowSink sink;
  sink.reserve(bytes.size() + 1);
  sink.put(bytes.data(), bytes.size());
  publish_gzip(path, &ix);
  return sink.hand_over(text, n, errbuf, errlen);
}

// the records of a dump go to the caller as malloc'ed arrays (one element where there is none)
static int dump_hand_over(const std::vector<uint64_t> &k, const std::vector<uint32_t> &c, int W, uint64_t **keys, uint32_t **counts, int64_t *n,
                          int *key_words, char *errbuf, size_t errlen)
{ uint64_t *ok = (uint64_t *) malloc(sizeof(uint64_t) * (k.empty() ? 1 : k.size()));
  uint32_t *oc = (uint32_t *) malloc(sizeof(uint32_t) * (c.empty() ? 1 : c.size()));
  if (!ok || !oc) { free(ok); free(oc); return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s", ""); }
  if (!k.empty()) memcpy(ok, k.data(), sizeof(uint64_t) * k.size());
  if (!c.empty()) memcpy(oc, c.data(), sizeof(uint32_t) * c.size());
  *keys = ok; *counts = oc; *n = (int64_t) c.size(); *key_words = W;
  return 0;
}

static int dump_args(const char *path, int32_t kmer, const void *keys, const void *counts, const void *n, const void *key_words,
                     char *errbuf, size_t errlen)
{ if (!path || !keys || !counts || !n || !key_words) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  smg_count_opts o;
  memset(&o, 0, sizeof(o));
  o.kmer = kmer; o.minval = 1;
  return check_opts(&o, errbuf, errlen);
}

// the records of a plain dump by the host twin (DumpHost, smg_dump.hpp): cutter and line decoder, no device
static int dump_parse(const char *path, int32_t kmer, uint64_t **keys, uint32_t **counts, int64_t *n, int *key_words, char *errbuf, size_t errlen)
{ RCHK(dump_args(path, kmer, keys, counts, n, key_words, errbuf, errlen));
  Taken f(path);
  if (f.file.fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  const int kind = file_kind(f.src, path, errbuf, errlen);
  if (kind < 0) return kind;
  if (kind != FILE_PLAIN)
    return fail(errbuf, errlen, SMG_EINVAL, "%s is BGZF compressed: this call has no device to inflate it on, use one of the counting calls "
                "or smg_count_dump_records", path);
  DumpHost host(kmer);
  DumpCutter<DumpHost> cut(host);
  std::vector<uint8_t> buf((size_t) 4 << 20);
  int rc = 0;
  for (;;)
    { const ssize_t got = f.src.get(buf.data(), buf.size());
      if (got < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
      if (got == 0) { rc = cut.finish(); break; }
      if ((rc = cut.feed(buf.data(), (size_t) got, path, errbuf, errlen)) != 0) break;
    }
  if (rc < 0) return rc;
  if (host.bad) return dump_bad_line(errbuf, errlen, path, host.bad_off, host.bad, kmer);
  return dump_hand_over(host.keys, host.counts, host.W, keys, counts, n, key_words, errbuf, errlen);
}

// the same records as kd_lines emits them, by the route of the counting calls: survey, reader thread, ring, feeder, batches
static int dump_records(const char *path, int32_t kmer, int32_t device, int32_t gzip, uint64_t **keys, uint32_t **counts, int64_t *n,
                        int *key_words, double *ms_kernel, char *errbuf, size_t errlen)
{ RCHK(dump_args(path, kmer, keys, counts, n, key_words, errbuf, errlen));
  publish_gzip(nullptr, nullptr);
  smg_count_opts o;
  memset(&o, 0, sizeof(o));
  o.kmer = kmer; o.minval = 1; o.device = device; o.host_threads = 1; o.gzip = gzip; o.dump = 1;
  Inputs in;
  int64_t bound = 0;
  RCHK(in.survey(&path, 1, &o, &bound, errbuf, errlen));
  Counter c;                                                   // (its batch and feeder; nothing is sorted or merged)
  const Out none{ nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false };
  RCHK(c.init(&o, none, bound, 1, errbuf, errlen, &path, in.streams));
  Run &x = c.x;
  std::vector<uint64_t> hk;
  std::vector<uint32_t> hc;
  const auto flush = [&]
    { const int64_t len = c.batch.take();
      int64_t nl = 0;
      if (len == 0) return 0;
      RCHK(c.dump.extract(len, &nl));
      const size_t at = hc.size();
      hk.resize((at + (size_t) nl) * (size_t) x.W); hc.resize(at + (size_t) nl);
      if (nl)
        { DCHK(hipMemcpy(hk.data() + at * (size_t) x.W, c.batch.ka.p, sizeof(uint64_t) * (size_t) nl * (size_t) x.W, hipMemcpyDeviceToHost));
          DCHK(hipMemcpy(hc.data() + at, c.dump.ca.p, sizeof(uint32_t) * (size_t) nl, hipMemcpyDeviceToHost));
        }
      return 0;
    };
  std::vector<Pinned<uint8_t>> pinned(4);
  std::vector<uint8_t *> blocks;
  for (Pinned<uint8_t> &b : pinned)
    { if (b.alloc(RING_BLOCK) != hipSuccess) return fail(errbuf, errlen, SMG_ENOMEM, "cannot pin %zu bytes of host memory", RING_BLOCK);
      blocks.push_back(b);
    }
  std::vector<FileRead> files;
  int64_t bases = 0;
  double t_read = 0;
  RCHK(read_files(&path, 1, 1, blocks.data(), (int) blocks.size(), RING_BLOCK,
                  [&](const uint8_t *p, int64_t m, int file) { return c.dump.add(p, m, file, flush); }, &bases, &t_read, &files, errbuf, errlen,
                  in.infl.data(), true, in.taken.data()));
  RCHK(flush());
  for (const std::unique_ptr<DeviceInflater> &d : in.own)
    if (d) for (const auto &g : d->gz_index) publish_gzip(g.first.c_str(), &g.second, true);
  if (ms_kernel) *ms_kernel = c.dump.ms_lines;
  return dump_hand_over(hk, hc, x.W, keys, counts, n, key_words, errbuf, errlen);
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
  return sink.hand_over(seq, nseq, errbuf, errlen);
}

// the stripped stream of a BAM file by the route of the counting calls
static int bam_strip(const char *path, int32_t device, uint8_t **seq, int64_t *nseq, int64_t *records, double *ms_kernel, char *errbuf, size_t errlen)
{ if (!seq || !nseq) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  BgzfInput in;
  RCHK(in.open(path, device, errbuf, errlen));
  GrowSink sink;
  BamFramer fr;
  bool any = false;
  RCHK(bgzf_feed(in.src, path, *in.infl, [&](const uint8_t *t, size_t m)
    { if (!any && m)
        { if (!is_bam_text(t, m)) return fail(errbuf, errlen, SMG_EINVAL, "%s is not BAM: its text does not begin with the magic BAM\\1", path);
          any = true;
        }
      return bam_piece(fr, t, m, path, *in.infl, sink, errbuf, errlen);
    }, errbuf, errlen));
  if (!any) return fail(errbuf, errlen, SMG_EINVAL, "%s is not BAM: it has no text", path);
  RCHK(fr.finish(path, errbuf, errlen));
  RCHK(sink.hand_over(seq, nseq, errbuf, errlen));
  if (records) *records = fr.records;
  if (ms_kernel) *ms_kernel = in.infl->ms.unpack;
  publish_bam(&path, { bam_read(fr, in.infl->times()) }, 1);
  return 0;
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

extern "C" int smg_count_stream_plan(int32_t kmer, uint64_t free_bytes, int64_t known_bound, int32_t partitions, int64_t max_entries,
                                     int64_t batch_bases, int64_t store_bases, int64_t *cap, int32_t *parted, int64_t *store_cap, char *errbuf,
                                     size_t errlen)
{ GUARD(stream_plan(kmer, (size_t) free_bytes, known_bound, partitions, max_entries, batch_bases, store_bases, cap, parted, store_cap, errbuf, errlen)) }

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

extern "C" int smg_count_gzip_inflate(const char *path, int32_t device, int64_t span_bytes, uint8_t **text, int64_t *n, double *ms_kernel,
                                      char *errbuf, size_t errlen)
{ GUARD(gzip_inflate(path, device, span_bytes, text, n, ms_kernel, errbuf, errlen)) }

extern "C" int smg_count_gzip_text_host(const char *path, int64_t span_bytes, uint8_t **text, int64_t *n, char *errbuf, size_t errlen)
{ GUARD(gzip_text_host(path, span_bytes, text, n, errbuf, errlen)) }

extern "C" int smg_count_gzip_report(const char *path, int64_t *members, int64_t *text_bytes, int64_t *spans, int64_t *linked, int64_t *repaired,
                                     double *ms)
{ try { return gzip_report(path, members, text_bytes, spans, linked, repaired, ms); } catch (...) { return SMG_ENOMEM; } }

extern "C" int smg_count_dump_parse(const char *path, int32_t kmer, uint64_t **keys, uint32_t **counts, int64_t *n, int *key_words,
                                    char *errbuf, size_t errlen)
{ GUARD(dump_parse(path, kmer, keys, counts, n, key_words, errbuf, errlen)) }

extern "C" int smg_count_dump_records(const char *path, int32_t kmer, int32_t device, int32_t gzip, uint64_t **keys, uint32_t **counts, int64_t *n,
                                      int *key_words, double *ms_kernel, char *errbuf, size_t errlen)
{ GUARD(dump_records(path, kmer, device, gzip, keys, counts, n, key_words, ms_kernel, errbuf, errlen)) }

extern "C" void smg_count_free(void *p) { free(p); }

extern "C" const char *smg_count_version(void) { return "smudgeplot_amd 0.5 (k-mer counter, gfx950)"; }
