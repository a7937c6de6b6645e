// smg_count_dump.hpp -- k-mer dumps on the device: the lines of a batch of text -> (canonical k-mer, count) records ->
// one saturating sum per distinct k-mer, handed to Distinct::merge (smg_count.hip holds the map of the whole counter).
//   kd_lines<W>     the front half of kc_extract (16 bytes per thread into the two LDS bit streams) with the raw bytes kept
//                   beside them; every line start of the tile is decoded by dump_line (smg_dump.hpp, the text the host twin
//                   compiles) over the LDS accessor, the good ones go out as kc_emit puts windows out, the first bad one of
//                   the batch is left in one 64-bit word by atomicMin
//   kd_run_sums<W>  after the pair sort (Distinct::sort_entries), kc_flag_heads and scan_flags: the head of every run writes
//                   its k-mer, every wave adds the counts of its part of a run to the run's 64-bit sum (a segmented shuffle
//                   scan, one atomic per wave and run: a run may be longer than a workgroup's share and than 65535, and
//                   2^32 addends of 2^32 - 1 do not wrap 64 bits)
//   kd_run_clamp    the sums, saturated to the uint32 counts that Distinct::merge takes
// and DumpFeed, the part that owns the count buffers, feeds the batch buffer with whole lines and maps a bad line back to its
// file and offset.  Batch::add, with its k-1 tails and separators, is for reads and is not used here.
// A kernel of our own and not rocprim::reduce_by_key: the keys are W words wide and the heads are flagged and scanned by the
// kernels the counter has anyway; what it costs is in profiles/count_dump.md.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "smg_count.h"
#include "smg_device.hpp"
#include "smg_count_kernels.hpp"
#include "smg_count_parts.hpp"
#include "smg_dump.hpp"

// The halo behind a tile: a line that starts on the last byte of the tile is read to its end, SMG_COUNT_DUMP_LINE - 1 bytes on.
// 192 and not 160: the chunks of a tile are then a multiple of 4, which the validity stream's 16-bit stores (^ 3) want.
#define KD_HALO   192
#define KD_CHUNKS ((KC_TILE + KD_HALO) / 16)
static_assert(KD_HALO >= SMG_COUNT_DUMP_LINE && KD_CHUNKS % 4 == 0, "the halo holds a longest line, the chunks fill whole words");
static_assert(SMG_COUNT_DUMP_LINE == SMG_MAX_KMER + 1 + 20 + 2, "the longest line");

// the accessor of dump_line over the LDS of a tile: positions are those of the tile, -1 is the byte in front of it
struct KdTile
{ const u64 *s_code, *s_val;
  const uint8_t *s_raw;                                        // byte p of the tile at s_raw[16 + p]
  SMG_DEV unsigned byte(int64_t p) const { return s_raw[16 + (int) p]; }
  SMG_DEV bool bases(int64_t p, int k) const { return kc_window(s_val, (int) p, k); }
  SMG_DEV u64 take64(int64_t bit) const { return kc_take64(s_code, (int) bit); }
  template <int W> SMG_DEV void revcomp(const uint64_t *x, int k, uint64_t *r) const
  { Key<W> a;
#pragma unroll
    for (int w = 0; w < W; w++) a.w[w] = x[w];
    const Key<W> b = ::revcomp<W>(a, k);
#pragma unroll
    for (int w = 0; w < W; w++) r[w] = b.w[w];
  }
};

// One workgroup per tile of KC_TILE text bytes, one byte in front and KD_HALO behind.  Position p starts a line when the
// byte in front of it is '\n' or p is the first byte of the batch; the tile that holds a line's first byte owns the line.
// The predicate (dump_line says DUMP_OK) is complete before the ballot; the records go out in position order behind one
// atomic per workgroup, 8 W + 4 bytes each.  A bad line writes nothing: (batch position << 8 | reason) goes into *bad by
// atomicMin, so the first bad line of the batch is what the host reads.
template <int W> __global__ void __launch_bounds__(KC_TPB)
kd_lines(const uint8_t *__restrict__ seq, int64_t n, int k, u64 *__restrict__ keys, uint32_t *__restrict__ cnt, unsigned long long limit,
         unsigned long long *__restrict__ nout, unsigned long long *__restrict__ bad)
{ __shared__ u64 s_code[KD_CHUNKS / 2 + 2];
  __shared__ u64 s_val[KD_CHUNKS / 4 + 2];
  __shared__ uint4 s_raw4[KD_CHUNKS + 1];
  __shared__ unsigned s_cnt[64];
  __shared__ unsigned long long s_base;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t tile0 = (int64_t) blockIdx.x * KC_TILE;
  unsigned *c32 = reinterpret_cast<unsigned *>(s_code);
  uint16_t *v16 = reinterpret_cast<uint16_t *>(s_val);
  uint8_t *s_raw = reinterpret_cast<uint8_t *>(s_raw4);

  if (t < 4) c32[(KD_CHUNKS + t) ^ 1] = 0;
  if (t < 8) v16[(KD_CHUNKS + t) ^ 3] = 0;
  if (t == 8) s_raw[15] = tile0 ? seq[tile0 - 1] : (uint8_t) '\n';
  for (int c = t; c < KD_CHUNKS; c += KC_TPB)
    { const uint4 v = kc_load16(seq, tile0 + 16 * (int64_t) c, n);
      unsigned code = 0, valid = 0;
      kc_code4(v.x, code, valid); kc_code4(v.y, code, valid); kc_code4(v.z, code, valid); kc_code4(v.w, code, valid);
      c32[c ^ 1] = code;
      v16[c ^ 3] = (uint16_t) valid;
      s_raw4[c + 1] = v;
    }
  __syncthreads();
  const KdTile tile{ s_code, s_val, s_raw };

  unsigned mine = 0;
  unsigned long long worst = ~0ull;
#pragma unroll 1
  for (int j = 0; j < KC_TILE / KC_TPB; j++)
    { const int p = j * KC_TPB + t;
      bool ok = false;
      if (tile0 + p < n && dump_starts(tile, p, false))
        { uint64_t key[W];
          uint32_t c;
          int len;
          const int r = dump_line<W>(tile, p, k, key, &c, &len);
          ok = r == DUMP_OK;
          if (!ok)
            { const unsigned long long w = ((unsigned long long) (tile0 + p) << 8) | (unsigned) r;
              if (w < worst) worst = w;
            }
        }
      const unsigned long long bal = __ballot(ok);
      if (lane == 0) s_cnt[j * 4 + wave] = (unsigned) __popcll(bal);
      mine |= (unsigned) ok << j;
    }
  if (worst != ~0ull) atomicMin(bad, worst);
  __syncthreads();
  if (wave == 0)
    { const unsigned own = s_cnt[lane];
      unsigned inc = own;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1)
        { const unsigned up = __shfl_up(inc, o, 64);
          if (lane >= o) inc += up;
        }
      s_cnt[lane] = inc - own;
      if (lane == 63) s_base = inc ? atomicAdd(nout, (unsigned long long) inc) : 0ull;
    }
  __syncthreads();
  const unsigned long long base = s_base;
#pragma unroll 1
  for (int j = 0; j < KC_TILE / KC_TPB; j++)                   // (the trip count is uniform: every lane meets every ballot)
    { const bool ok = (mine >> j) & 1u;
      const unsigned long long bal = __ballot(ok);
      if (ok)
        { const int p = j * KC_TPB + t;
          const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned) (bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) bal, 0u));
          uint64_t key[W];
          uint32_t c = 0;
          int len;
          (void) dump_line<W>(tile, p, k, key, &c, &len);       // (decoded again: cheaper than 16 counts kept per thread)
          const unsigned long long q = base + s_cnt[j * 4 + wave] + rank;
          if (q < limit)                                       // (never false: a batch of n bytes holds at most n / (k + 3) lines)
            { u64 *o = keys + (size_t) q * W;
#pragma unroll
              for (int w = 0; w < W; w++) o[w] = key[w];
              cnt[q] = c;
            }
        }
    }
}

// Sorted (k-mer, count) records, the head flags of their runs and the exclusive scan of the flags (run of entry i:
// pos[i] + flag[i] - 1): ukeys[run] = the k-mer, sums[run] += the counts (zeroed by the host).
template <int W> __global__ void __launch_bounds__(KC_TPB)
kd_run_sums(const u64 *__restrict__ keys, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
            int64_t n, int64_t nruns, u64 *__restrict__ ukeys, unsigned long long *__restrict__ sums)
{ const int64_t i = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = i < n;
  const uint32_t f = in ? flag[i] : 0u;
  const uint32_t q = in ? pos[i] + f - 1u : 0xFFFFFFFFu;        // (beyond n: a run of its own that nobody writes)
  unsigned long long v = in ? cnt[i] : 0u;
  if (in && f && (int64_t) q < nruns)
    { const Key<W> x = load_key<W>(keys, i);
#pragma unroll
      for (int w = 0; w < W; w++) ukeys[(size_t) q * W + w] = x.w[w];
    }
  // runs are contiguous: after the step of width o, v is the sum over [lane, lane + 2 o) as far as the lane's run reaches
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
    { const unsigned long long v2 = __shfl_down(v, o, 64);
      const uint32_t q2 = __shfl_down(q, o, 64);
      if (lane + o < 64 && q2 == q) v += v2;
    }
  const uint32_t ql = __shfl_up(q, 1, 64);
  if (in && (lane == 0 || ql != q) && (int64_t) q < nruns) atomicAdd(&sums[q], v);
}

__global__ void __launch_bounds__(KC_TPB)
kd_run_clamp(const unsigned long long *__restrict__ sums, int64_t nruns, uint32_t *__restrict__ cnt)
{ const int64_t j = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  if (j < nruns) cnt[j] = sums[j] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) sums[j];
}

// bytes per text byte of a batch that a dump needs on top of batch_price: two count buffers and the sums, per line
static inline int64_t dump_lines_of(int64_t bytes, int k) { return bytes / (k + 3) + 1; }
static inline size_t  dump_price(int64_t cap, int k) { return (size_t) dump_lines_of(cap, k) * 16 + 8; }

// The feeder of a dump run: whole lines into the batch buffer, the table of the pieces that lie there, the buffers of the
// counts, and the two steps of a batch.
struct DumpFeed
{ Run &x;
  Batch &b;
  struct Piece { int64_t at, len; int file; int64_t off; };   // batch position, bytes, file, offset in the file's text
  std::vector<Piece> pieces;
  std::vector<int64_t> off;                                    // per file: text bytes handed over
  const char *const *paths = nullptr;
  int64_t max_lines = 0;
  double ms_lines = 0;                                         // HIP-event time of kd_lines
  DevBuf<uint32_t> ca, cb;                                     // the counts of a batch and the other half of their sort
  DevBuf<unsigned long long> sums, bad;
  DumpFeed(Run &r, Batch &batch) : x(r), b(batch) {}

  int init(const char *const *p, int nfiles)
  { paths = p;
    off.assign((size_t) (nfiles > 0 ? nfiles : 1), 0);
    max_lines = dump_lines_of(b.cap, x.k);
    RCHK(x.alloc(ca, sizeof(uint32_t) * (size_t) max_lines));
    RCHK(x.alloc(cb, sizeof(uint32_t) * (size_t) max_lines));
    RCHK(x.alloc(sums, sizeof(unsigned long long) * (size_t) max_lines));
    return x.alloc(bad, 8);
  }

  // whole lines of one file's text, in order; a piece that does not fit is cut behind the last line that does
  template <class Flush> int add(const uint8_t *p, int64_t n, int file, Flush &&flush)
  { while (n > 0)
      { const int64_t room = b.cap - b.fill;
        int64_t m = n;
        if (m > room)
          { const uint8_t *q = room > 0 ? (const uint8_t *) memrchr(p, '\n', (size_t) room) : nullptr;
            if (!q)
              { if (b.fill > 0) { RCHK(flush()); continue; }
                // a line longer than a whole batch (SMG_COUNT_DUMP_LINE bytes at least): it cannot be legal, and every line of
                // this file in front of it has passed the kernel
                uint64_t key[4]; uint32_t c; int len;
                const int r = dump_line_w(x.W, DumpText{ p, n }, 0, x.k, key, &c, &len);
                if (r != DUMP_OK) return dump_bad_line(x.errbuf, x.errlen, paths[file], off[(size_t) file], r, x.k);
                return fail(x.errbuf, x.errlen, SMG_ENODEV, "internal error: a dump line of %d bytes in a batch of %lld", len, (long long) b.cap);
              }
            m = (int64_t) (q - p) + 1;
          }
        DCHK(hipMemcpy(b.seq + b.fill, p, (size_t) m, hipMemcpyHostToDevice));
        pieces.push_back(Piece{ b.fill, m, file, off[(size_t) file] });
        b.fill += m; off[(size_t) file] += m;
        p += m; n -= m;
      }
    return 0;
  }

  // the n bytes of the batch buffer -> the records of their lines in (b.ka, ca); or the first bad line, by file and offset
  int extract(int64_t n, int64_t *nlines)
  { x.tic();
    DCHK(hipMemsetAsync(b.ctr.p, 0, 16, x.stream));
    DCHK(hipMemsetAsync(bad.p, 0xFF, 8, x.stream));
    const unsigned ntiles = (unsigned) ((n + KC_TILE - 1) / KC_TILE);
    LAUNCH_W(kd_lines, ntiles, b.seq, n, x.k, b.ka, ca, (unsigned long long) max_lines, b.ctr, bad);
    DCHK(hipGetLastError());
    unsigned long long got = 0, worst = 0;
    DCHK(hipMemcpyAsync(&got, b.ctr.p, 8, hipMemcpyDeviceToHost, x.stream));
    DCHK(hipMemcpyAsync(&worst, bad.p, 8, hipMemcpyDeviceToHost, x.stream));
    double ms = 0;
    RCHK(x.toc(&ms));
    x.st.ms_extract += ms; ms_lines += ms;
    if (worst != ~0ull)
      { const int64_t at = (int64_t) (worst >> 8);
        for (const Piece &pc : pieces)
          if (at >= pc.at && at < pc.at + pc.len)
            return dump_bad_line(x.errbuf, x.errlen, paths[pc.file], pc.off + (at - pc.at), (int) (worst & 0xFF), x.k);
        return fail(x.errbuf, x.errlen, SMG_ENODEV, "internal error: a bad dump line at batch position %lld, which no piece holds", (long long) at);
      }
    pieces.clear();
    if ((int64_t) got > max_lines) return fail(x.errbuf, x.errlen, SMG_ENODEV, "internal error: %llu lines from %lld bytes", got, (long long) n);
    *nlines = (int64_t) got;
    return 0;
  }

  // the records of a batch -> pair-sorted -> one saturating sum per run -> merged into the list
  int count(Distinct &list, int64_t nl)
  { x.st.windows += nl;
    u64 *sk = nullptr; uint32_t *sc = nullptr;
    x.tic();
    RCHK(list.sort_entries(b.ka, b.kb, ca, cb, nl, &sk, &sc));
    RCHK(x.toc(&x.st.ms_sort));
    u64 *uk = sk == b.ka ? b.kb : b.ka;
    int64_t nruns = 0;
    x.tic();
    LAUNCH_W(kc_flag_heads, nblk(nl), sk, nl, b.flag);
    DCHK(scan_flags(b.flag, b.pos, nl, x.stream, x.tmp, &nruns));
    if (nruns > 0)
      { DCHK(hipMemsetAsync(sums.p, 0, sizeof(unsigned long long) * (size_t) nruns, x.stream));
        LAUNCH_W(kd_run_sums, nblk(nl), sk, sc, b.flag, b.pos, nl, nruns, uk, sums);
        uint32_t *rc = b.flag;                                 // (the flags are spent: the counts of the runs take their place)
        LAUNCH(kd_run_clamp, nblk(nruns), sums, nruns, rc);
        DCHK(hipGetLastError());
        RCHK(list.merge(uk, rc, nruns));
      }
    return x.toc(&x.st.ms_reduce);
  }
};
