// smg_count_plan.hpp -- every decision of the k-mer counter that is arithmetic: how the device memory is shared out, how
// a buffer grows, where the key ranges of a partitioned run are cut (smg_count.hip holds the map of the whole counter).
// Host only, no HIP; nothing here touches the device or reads the environment.

#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "smg_count.h"
#include "smg_count_err.hpp"

#define CP_TILE 4096                     // the store is sized in whole tiles of the kernels that read it (KC_TILE)

// ---- memory -------------------------------------------------------------------------------------------------------

static inline int     count_words(int k) { return (k + 31) / 32; }
// bytes per position of a batch: the sequence, two key buffers, flags, positions, run starts, the word sort's scratch
static inline int64_t batch_price(int W) { return 1 + 16 * W + 12 + (W > 1 ? 24 : 0); }
// bytes per entry of a merge of the distinct list
static inline size_t  merge_price(int W) { return 3 * (sizeof(uint64_t) * W + sizeof(uint32_t)) + 8 + (W > 1 ? 24 : 0); }

#define CP_RESERVE ((size_t) 64 << 20)   // left free by every plan, for what the runtime and the sorts take

// positions a batch holds when `avail` bytes are there to share between the batch and the merges; hook > 0 (the test hook
// SMG_COUNT_BATCH_BASES) names the bases of a batch instead
static inline int64_t batch_cap(size_t avail, int k, int64_t bound, int64_t hook)
{ int64_t c = (int64_t) (avail / 3) / batch_price(count_words(k));
  if (c > ((int64_t) 1 << 30)) c = (int64_t) 1 << 30;
  if (hook > 0) c = hook + k;
  if (c > bound + k + 1) c = bound + k + 1;
  if (c < k + 1) c = k + 1;
  return c;
}

// The capacity a buffer of `cap` units grows to when `need` are wanted: by half, or to the need where that is more, in
// whole multiples of `unit`.  The packed store, the device table and the host table all grow by this rule.
static inline int64_t grown_cap(int64_t cap, int64_t need, int64_t unit)
{ int64_t nc = cap + cap / 2;
  if (nc < need) nc = need;
  if (nc < 1) nc = 1;
  return (nc + unit - 1) / unit * unit;
}

// Memory plan, before the first allocation: a third of what is free goes to the batch, the rest is left to the distinct
// list and its merge.  `bound` is the most sequence the input can hold, hence a bound on its windows and its distinct
// k-mers: where a merge of that many entries fits next to the batch (and within max_entries, if that is set), the run is
// one pass; otherwise, or when the caller asks for ranges (partitions > 1), the batches are packed into a store that comes
// off the top at 3 bits per position, and the batch is sized again from what is left.  *cap = positions of a batch,
// *parted = 1 for a store and ranges, *store_cap = positions of the store (a multiple of CP_TILE; 0 for one pass).
static inline int memory_plan(int k, size_t free_b, int64_t bound, int32_t partitions, int64_t max_entries, int64_t hook, int64_t *cap,
                              int32_t *parted, int64_t *store_cap, char *errbuf, size_t errlen)
{ if (!cap || !parted || !store_cap || k < SMG_COUNT_MIN_KMER || k > SMG_MAX_KMER || bound < 0 || partitions < 0 || partitions > SMG_COUNT_BINS ||
      max_entries < 0)
    return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  const int W = count_words(k);
  const int64_t per = batch_price(W);
  int64_t c = batch_cap(free_b, k, bound, hook);
  *cap = 0; *store_cap = 0;
  *parted = partitions > 1;
  if (partitions == 0)
    { const bool fits = bound < 0xFFFFFFF0ll && (size_t) (c * per) + (size_t) bound * merge_price(W) + CP_RESERVE <= free_b;
      *parted = !(fits && (max_entries == 0 || bound <= max_entries));
    }
  if (*parted)
    { *store_cap = ((bound + bound / 32 + ((int64_t) 1 << 16)) + CP_TILE - 1) / CP_TILE * CP_TILE;
      const size_t need = (size_t) *store_cap / 8 * 3;
      if (need + CP_RESERVE > free_b)
        return fail(errbuf, errlen, SMG_ENOMEM, "the packed input does not fit the device: a store of %lld positions needs %.3f GB, "
                    "%.3f GB of device memory are free", (long long) *store_cap, (double) need * 1e-9, (double) free_b * 1e-9);
      free_b -= need;
      c = batch_cap(free_b, k, bound, hook);
    }
  if (c * per > (int64_t) free_b)
    return fail(errbuf, errlen, SMG_ENOMEM, "a batch of %lld bases needs %.3f GB, %.3f GB of device memory are free",
                (long long) c, (double) (c * per) * 1e-9, (double) free_b * 1e-9);
  *cap = c;
  return 0;
}

// The plan of a call that reads a stream, whose length nobody knows: there is no bound.  known_bound bounds the regular
// files of the call only.  partitions == 1 is one pass with the batch of memory_plan, never clamped to the input; what
// memory_plan guarantees in advance is left to the check that every merge makes (it refuses, with its figures, a distinct
// list that does not fit).  Any other value, 0 included, packs the batches into a store and counts by key range, which is
// defined to give what one pass gives.  The store begins with store_bases positions (the test hook SMG_COUNT_STREAM_STORE)
// or, where that is 0, CP_STREAM_STORE of them -- 2^30, 384 MiB, 0.14 % of an MI355X -- or what memory_plan
// gives a store for known_bound where that is more; in whole tiles, as memory_plan rounds.  From there it grows by half
// (grown_cap) as the stream goes on.  max_entries is checked and otherwise left to the merges and the plan of the ranges.
#define CP_STREAM_STORE ((int64_t) 1 << 30)
#define CP_NO_BOUND     (INT64_MAX - 2 * SMG_MAX_KMER)         // a bound that clamps no batch
static inline int64_t store_tiles(int64_t positions) { return (positions + CP_TILE - 1) / CP_TILE * CP_TILE; }

static inline int stream_plan(int k, size_t free_b, int64_t known_bound, int32_t partitions, int64_t max_entries, int64_t hook, int64_t store_bases,
                              int64_t *cap, int32_t *parted, int64_t *store_cap, char *errbuf, size_t errlen)
{ if (!cap || !parted || !store_cap || k < SMG_COUNT_MIN_KMER || k > SMG_MAX_KMER || known_bound < 0 || partitions < 0 ||
      partitions > SMG_COUNT_BINS || max_entries < 0 || store_bases < 0 || store_bases > ((int64_t) 1 << 50))
    return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  *cap = 0; *store_cap = 0;
  *parted = partitions != 1;
  if (*parted)
    { const int64_t known = known_bound + known_bound / 32 + ((int64_t) 1 << 16);
      *store_cap = store_tiles(store_bases ? store_bases : (known > CP_STREAM_STORE ? known : CP_STREAM_STORE));
      const size_t need = (size_t) *store_cap / 8 * 3;
      if (need + CP_RESERVE > free_b)
        return fail(errbuf, errlen, SMG_ENOMEM, "the packed input does not fit the device: a first store of %lld positions needs %.3f GB, "
                    "%.3f GB of device memory are free", (long long) *store_cap, (double) need * 1e-9, (double) free_b * 1e-9);
      free_b -= need;
    }
  const int64_t c = batch_cap(free_b, k, CP_NO_BOUND, hook);
  if (c * batch_price(count_words(k)) > (int64_t) free_b)
    return fail(errbuf, errlen, SMG_ENOMEM, "a batch of %lld bases needs %.3f GB, %.3f GB of device memory are free",
                (long long) c, (double) (c * batch_price(count_words(k))) * 1e-9, (double) free_b * 1e-9);
  *cap = c;
  return 0;
}

// ---- key ranges ---------------------------------------------------------------------------------------------------

#define CP_BIN_BASES (SMG_COUNT_BIN_BITS / 2)

static inline void lead_bases(char *out, unsigned v, int bases)
{ for (int j = 0; j < bases; j++) out[j] = "acgt"[(v >> (2 * (bases - 1 - j))) & 3];
  out[bases] = 0;
}

// The cuts of a partitioned run.  Greedy over the bins: a range takes bins while its windows stay within the budget, which
// gives the fewest contiguous ranges; the windows of a range bound its distinct k-mers and every merge of it, so a plan
// made this way cannot overflow.  A requested number of ranges gets cuts at the equal shares of the windows instead,
// moved where needed so that every range has a bin.
static inline int plan(const uint64_t *windows, int64_t budget, int32_t partitions, int32_t *cuts, int32_t *nranges, char *errbuf, size_t errlen)
{ if (!windows || !cuts || !nranges) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  if (partitions < 0 || partitions > SMG_COUNT_BINS)
    return fail(errbuf, errlen, SMG_EINVAL, "partitions = %d is out of range 0 .. %d", partitions, SMG_COUNT_BINS);
  int32_t n = 0;
  cuts[0] = 0;
  if (partitions == 0)
    { if (budget < 1) return fail(errbuf, errlen, SMG_EINVAL, "budget = %lld is not positive", (long long) budget);
      uint64_t sum = 0;
      for (int b = 0; b < SMG_COUNT_BINS; b++)
        { if (windows[b] > (uint64_t) budget)
            { char lead[CP_BIN_BASES + 1];
              lead_bases(lead, (unsigned) b, CP_BIN_BASES);
              return fail(errbuf, errlen, SMG_ENOMEM, "bin %d (canonical k-mers that begin with %s) holds %llu windows, one merge holds %lld "
                          "entries: a single bin cannot be split", b, lead, (unsigned long long) windows[b], (long long) budget);
            }
          if (sum + windows[b] > (uint64_t) budget) { cuts[++n] = b; sum = 0; }
          sum += windows[b];
        }
      cuts[++n] = SMG_COUNT_BINS;
    }
  else
    { uint64_t total = 0, cum = 0;
      for (int b = 0; b < SMG_COUNT_BINS; b++) total += windows[b];
      int b = 0;
      for (int j = 1; j < partitions; j++)                         // cut j: the first bin boundary with j / P of the windows below it
        { const uint64_t want = (uint64_t) (((unsigned __int128) total * (unsigned) j + (unsigned) partitions - 1) / (unsigned) partitions);
          while (b < SMG_COUNT_BINS && cum < want) cum += windows[b++];
          int c = b;
          if (c <= cuts[j - 1]) c = cuts[j - 1] + 1;
          if (c > SMG_COUNT_BINS - (partitions - j)) c = SMG_COUNT_BINS - (partitions - j);
          while (b < c) cum += windows[b++];
          cuts[j] = c;
        }
      n = partitions;
      cuts[n] = SMG_COUNT_BINS;
    }
  *nranges = n;
  return 0;
}

// The cuts where `plan` refuses a bin: the same greedy rule over one ascending sequence of units, a bin that is not split
// or one of the 4096 sub-bins of a bin that is.  What is left to refuse is a single sub-bin above the budget.
static inline int plan_fine(const uint64_t *windows, const int32_t *split, int32_t nsplit, const uint64_t *sub, int64_t budget, int32_t *cuts,
                            int64_t cuts_cap, int32_t *nranges, char *errbuf, size_t errlen)
{ if (!windows || !cuts || !nranges || cuts_cap < 2 || nsplit < 0 || nsplit > SMG_COUNT_BINS || (nsplit > 0 && (!split || !sub)))
    return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  if (budget < 1) return fail(errbuf, errlen, SMG_EINVAL, "budget = %lld is not positive", (long long) budget);
  for (int s = 0; s < nsplit; s++)
    { const int b = split[s];
      if (b < 0 || b >= SMG_COUNT_BINS || (s > 0 && b <= split[s - 1]))
        return fail(errbuf, errlen, SMG_EINVAL, "split bins must be ascending values 0 .. %d (entry %d is %d)", SMG_COUNT_BINS - 1, s, b);
      uint64_t sum = 0;
      for (int j = 0; j < SMG_COUNT_BINS; j++) sum += sub[(size_t) s * SMG_COUNT_BINS + j];
      if (sum != windows[b])
        return fail(errbuf, errlen, SMG_EINVAL, "bin %d holds %llu windows, its sub-bins %llu", b, (unsigned long long) windows[b],
                    (unsigned long long) sum);
    }
  int64_t n = 0;
  uint64_t sum = 0;
  int s = 0;
  cuts[0] = 0;
  for (int b = 0; b < SMG_COUNT_BINS; b++)
    { const bool is_split = s < nsplit && split[s] == b;
      if (!is_split && windows[b] > (uint64_t) budget)
        return fail(errbuf, errlen, SMG_EINVAL, "bin %d holds %llu windows, one merge holds %lld entries, and it is not among the bins to split",
                    b, (unsigned long long) windows[b], (long long) budget);
      for (int j = 0; j < (is_split ? SMG_COUNT_BINS : 1); j++)
        { const uint64_t w = is_split ? sub[(size_t) s * SMG_COUNT_BINS + j] : windows[b];
          if (w > (uint64_t) budget)
            { char lead[CP_BIN_BASES + 1], lead2[2 * CP_BIN_BASES + 1];
              lead_bases(lead, (unsigned) b, CP_BIN_BASES);
              lead_bases(lead2, ((unsigned) b << SMG_COUNT_BIN_BITS) | (unsigned) j, 2 * CP_BIN_BASES);
              return fail(errbuf, errlen, SMG_ENOMEM, "bin %d (canonical k-mers that begin with %s) holds %llu windows, one merge holds %lld "
                          "entries: its sub-bin %d (canonical k-mers that begin with %s) holds %llu windows, and a bin of the leading %d bits "
                          "cannot be split", b, lead, (unsigned long long) windows[b], (long long) budget, j, lead2, (unsigned long long) w,
                          SMG_COUNT_FINE_BITS);
            }
          if (sum + w > (uint64_t) budget)
            { if (n + 3 > cuts_cap) return fail(errbuf, errlen, SMG_EINVAL, "more ranges than the %lld cuts there is room for", (long long) cuts_cap);
              cuts[++n] = (int32_t) (((unsigned) b << SMG_COUNT_BIN_BITS) | (unsigned) j);
              sum = 0;
            }
          sum += w;
        }
      if (is_split) s++;
    }
  cuts[++n] = SMG_COUNT_FINE_BINS;
  *nranges = (int32_t) n;
  return 0;
}

// The ranges of one partitioned run.  bins: windows per bin of the leading 12 bits; split: the bins that alone are above
// the budget (ascending), sub: their 4096 sub-bin windows each; cuts[0 .. nranges]: values of the leading 24 bits, a
// multiple of 4096 wherever the cut lies between whole bins.
struct RangePlan
{ std::vector<uint64_t> bins = std::vector<uint64_t>(SMG_COUNT_BINS, 0), sub;
  std::vector<int32_t> cuts = std::vector<int32_t>(SMG_COUNT_BINS + 1, 0), split;
  int32_t nranges = 1;
  std::vector<int64_t> cum;                                    // windows in front of every bin, once the bins are final

  void index()
  { cum.assign(SMG_COUNT_BINS + 1, 0);
    for (int b = 0; b < SMG_COUNT_BINS; b++) cum[(size_t) b + 1] = cum[(size_t) b] + (int64_t) bins[(size_t) b];
  }

  // windows below a cut: whole bins in front of it, and inside a split bin the sub-bins in front of it
  int64_t below(unsigned x) const
  { const unsigned b = x >> SMG_COUNT_BIN_BITS, j = x & (SMG_COUNT_BINS - 1u);
    int64_t n = cum[b];
    if (j)
      { size_t s = 0;
        while (s + 1 < split.size() && (unsigned) split[s] != b) s++;
        for (unsigned i = 0; i < j; i++) n += (int64_t) sub[s * SMG_COUNT_BINS + i];
      }
    return n;
  }
};
