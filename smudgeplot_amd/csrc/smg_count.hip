// smg_count.hip -- k-mer counter for one MI355X (gfx950, wave64): FASTA / FASTQ in, canonical k-mer table out.
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
// A batch boundary never loses or doubles a window: a piece that does not continue the byte in front of it in the
// batch buffer is preceded by a separator and the last k-1 bytes of its file's stream (no whole window fits in those).
//
// Where one merge cannot be guaranteed to hold the distinct k-mers of the input, the run is partitioned by key range:
//   pack    kc_pack  every batch of bytes -> 3 bits per position (2-bit codes, validity) appended to a resident store
//   plan    kc_bins  windows per bin of the leading 12 bits of the canonical k-mer; smg_count_plan cuts the 4096 bins
//           into contiguous ranges whose windows (an upper bound of their distinct k-mers) stay within one sorted
//           batch or, where a single bin is larger than that, within one merge.  Only where a single bin is larger than
//           one merge: kc_subbins  the windows of that bin by their next 12 bits, and smg_count_plan_fine cuts the
//           whole bins and the 4096 sub-bins of every such bin, so that a range is an interval of the leading 24 bits
//   range   kc_extract_packed<W>  the store -> canonical k-mers of ONE range, the key buffer filled across the store
//           and sorted when full; then batch / merge / finish as above, the kept entries appended to the host table
//           (kc_extract_fine<W>: the same for a range with an end inside a split bin, its filter on 24 bits)
// Every instance of a k-mer lies in one range, so ranges in ascending order give the sorted table.
//
// The _device entries leave the table where it was made: the kept entries of a range are appended to a table in device
// memory instead (two whole allocations, which the caller hands to smg_engine_bind / smg_hetmers_run_device and frees).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <rocprim/rocprim.hpp>

#include <fcntl.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "smg_count.h"
#include "smg_device.hpp"
#include "smg_keysort.hpp"

#define KC_TPB   256
#define KC_TILE  4096                    // positions per workgroup: 16 bytes per thread
#define KC_HALO  128                     // >= SMG_MAX_KMER - 1, a multiple of 16
#define KC_CHUNKS ((KC_TILE + KC_HALO) / 16)
#define KC_HBINS 8192                    // counts below this go through per-workgroup LDS bins

// ---------------------------------------------------------------------------------------------------------------
//  device code
// ---------------------------------------------------------------------------------------------------------------

// 64 bits of a big-endian bit stream kept in 64-bit words, from bit `pos` on (reads s[pos/64] and the word behind it)
SMG_DEV u64 kc_take64(const u64 *s, int pos)
{ const int q = pos >> 6, sh = pos & 63;
  const u64 a = s[q], b = s[q + 1];
  return sh ? (a << sh) | (b >> (64 - sh)) : a;
}

// four sequence bytes -> 2-bit codes (first byte in the top bits of an 8-bit group) and one validity bit each
SMG_DEV void kc_code4(unsigned v, unsigned &code, unsigned &valid)
{
#pragma unroll
  for (int j = 0; j < 4; j++)
    { const unsigned b = (v >> (8 * j)) & 0xFFu, u = b & 0xDFu;
      const unsigned ok = (u == 'A') | (u == 'C') | (u == 'G') | (u == 'T');
      code = (code << 2) | ((((b >> 1) & 3u) ^ ((b >> 2) & 1u)) & (0u - ok));   // a c g t -> 0 1 2 3 (ktab.pack_bases)
      valid = (valid << 1) | ok;
    }
}

template <int W> SMG_DEV bool kc_all_ones(const Key<W> &x)
{ bool e = true;
#pragma unroll
  for (int w = 0; w < W; w++) e &= (x.w[w] == ~0ull);
  return e;
}

// The leading SMG_COUNT_BIN_BITS bits of the canonical k-mer of the window at position p of the LDS code stream:
// top(min(x, rc x)) = min(top x, top rc x), and top rc x is the complement of the window's last bases in reverse
// order, so two short reads of the stream give the bin and the k-mer itself is never built.
#define KC_BIN_BASES (SMG_COUNT_BIN_BITS / 2)
SMG_DEV unsigned kc_bin(const u64 *s_code, int p, int k)
{ const unsigned f = (unsigned) (kc_take64(s_code, 2 * p) >> (64 - SMG_COUNT_BIN_BITS));
  const u64 l = kc_take64(s_code, 2 * (p + k - KC_BIN_BASES)) & (~0ull << (64 - SMG_COUNT_BIN_BITS));
  const unsigned r = (unsigned) rev2_comp_word(l) & (SMG_COUNT_BINS - 1u);
  return f < r ? f : r;
}

// The same for the leading SMG_COUNT_FINE_BITS bits, twelve bases: kc_bin24 >> 12 is kc_bin.  k >= 13, so both reads stay
// inside the window; at k = 13 the first and the last twelve bases overlap in all but one base.
#define KC_FINE_BASES (SMG_COUNT_FINE_BITS / 2)
SMG_DEV unsigned kc_bin24(const u64 *s_code, int p, int k)
{ const unsigned f = (unsigned) (kc_take64(s_code, 2 * p) >> (64 - SMG_COUNT_FINE_BITS));
  const u64 l = kc_take64(s_code, 2 * (p + k - KC_FINE_BASES)) & (~0ull << (64 - SMG_COUNT_FINE_BITS));
  const unsigned r = (unsigned) rev2_comp_word(l) & (SMG_COUNT_FINE_BINS - 1u);
  return f < r ? f : r;
}

// does a window of k valid bases start at position p of the LDS validity stream?
SMG_DEV bool kc_window(const u64 *s_val, int p, int k)
{ const u64 x0 = kc_take64(s_val, p);
  if (k <= 64) return (~x0 >> (64 - k)) == 0;
  const u64 x1 = kc_take64(s_val, p + 64);
  return (x0 == ~0ull) & ((~x1 >> (128 - k)) == 0);
}

// The back half of both extract kernels.  The two LDS bit streams of a tile (2-bit codes, validity; both big endian so
// that one funnel shift serves both) are in place.  Position p of the tile starts a window when the k validity bits
// from p on are all set, its global position lies in [p0, p1) and, with BITS = 12 or 24 (0: no filter), the leading BITS
// bits of its canonical k-mer (kc_bin, kc_bin24) lie in [lo, hi): the predicate is complete BEFORE the ballot, so a rejected window never
// builds, reverse-complements or compares its k-mer.  The canonical k-mers go out in position order behind ONE atomic per workgroup (64 ballot
// counts, scanned by the first wavefront): 8 W bytes out per accepted window.
template <int W, int BITS> SMG_DEV void
kc_emit(const u64 *s_code, const u64 *s_val, unsigned *s_cnt, unsigned long long *s_base, int64_t tile0, int64_t p0, int64_t p1, int k,
        unsigned lo, unsigned hi, u64 *__restrict__ out, unsigned long long limit, unsigned long long *__restrict__ nout)
{ const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // which of this thread's 16 positions (p = j * 256 + t: neighbouring lanes, neighbouring windows) start a window
  unsigned mine = 0;
#pragma unroll
  for (int j = 0; j < KC_TILE / KC_TPB; j++)
    { const int p = j * KC_TPB + t;
      bool ok = (tile0 + p >= p0) & (tile0 + p < p1);
      ok &= kc_window(s_val, p, k);
      if constexpr (BITS != 0)
        { const unsigned b = BITS == SMG_COUNT_BIN_BITS ? kc_bin(s_code, p, k) : kc_bin24(s_code, p, k);   // (garbage where ok is false: ANDed away)
          ok &= (b >= lo) & (b < hi);
        }
      const unsigned long long bal = __ballot(ok);
      if (lane == 0) s_cnt[j * 4 + wave] = (unsigned) __popcll(bal);
      mine |= (unsigned) ok << j;
    }
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
      if (lane == 63) *s_base = inc ? atomicAdd(nout, (unsigned long long) inc) : 0ull;
    }
  __syncthreads();
  const unsigned long long base = *s_base;
  const int rem = 2 * k - 64 * (W - 1);                      // bits of the last word that belong to the k-mer
  const u64 lastmask = ~0ull << (64 - rem);
  for (int j = 0; j < KC_TILE / KC_TPB; j++)                 // (the trip count is uniform: every lane meets every ballot)
    { const bool ok = (mine >> j) & 1u;
      const unsigned long long bal = __ballot(ok);
      if (ok)
        { const int p = j * KC_TPB + t;
          const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned) (bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) bal, 0u));
          Key<W> x;
#pragma unroll
          for (int w = 0; w < W; w++) x.w[w] = kc_take64(s_code, 2 * p + 64 * w);
          x.w[W - 1] &= lastmask;
          const Key<W> r = revcomp<W>(x, k);
          const bool lt = key_lt<W>(r, x);
          const unsigned long long q = base + s_cnt[j * 4 + wave] + rank;
          u64 *o = out + (size_t) q * W;
          if (q < limit)                                       // (never false: the host sizes the span; it reads *nout and would say so)
            {
#pragma unroll
              for (int w = 0; w < W; w++) o[w] = lt ? r.w[w] : x.w[w];
            }
        }
    }
}

// One workgroup per tile of KC_TILE sequence bytes plus a halo of k-1.  The bytes are coded into the two LDS bit streams,
// kc_emit does the rest: 1 byte in per position, 8 W bytes out per window.
template <int W> __global__ void __launch_bounds__(KC_TPB)
kc_extract(const uint8_t *__restrict__ seq, int64_t n, int k, u64 *__restrict__ out, unsigned long long *__restrict__ nout)
{ __shared__ u64 s_code[KC_CHUNKS / 2 + 2];
  __shared__ u64 s_val[KC_CHUNKS / 4 + 2];
  __shared__ unsigned s_cnt[64];
  __shared__ unsigned long long s_base;
  const int t = threadIdx.x;
  const int64_t tile0 = (int64_t) blockIdx.x * KC_TILE;
  unsigned *c32 = reinterpret_cast<unsigned *>(s_code);
  uint16_t *v16 = reinterpret_cast<uint16_t *>(s_val);

  if (t < 4) c32[(KC_CHUNKS + t) ^ 1] = 0;
  if (t < 8) v16[(KC_CHUNKS + t) ^ 3] = 0;
  for (int c = t; c < KC_CHUNKS; c += KC_TPB)
    { const int64_t g = tile0 + 16 * (int64_t) c;
      uint4 v = make_uint4(0, 0, 0, 0);                      // (byte 0 is no base: past the end nothing is valid)
      if (g + 16 <= n) v = *reinterpret_cast<const uint4 *>(seq + g);
      else if (g < n)
        { unsigned d[4] = { 0, 0, 0, 0 };
          for (int b = 0; b < 16 && g + b < n; b++) d[b >> 2] |= (unsigned) seq[g + b] << (8 * (b & 3));
          v = make_uint4(d[0], d[1], d[2], d[3]);
        }
      unsigned code = 0, valid = 0;
      kc_code4(v.x, code, valid); kc_code4(v.y, code, valid); kc_code4(v.z, code, valid); kc_code4(v.w, code, valid);
      c32[c ^ 1] = code;                                     // (^1, ^3: the first chunk of a 64-bit word in its top bits)
      v16[c ^ 3] = (uint16_t) valid;
    }
  __syncthreads();
  kc_emit<W, 0>(s_code, s_val, s_cnt, &s_base, tile0, 0, n - k + 1, k, 0u, 0u, out, (unsigned long long) n, nout);
}

// ---- the resident store of a partitioned run: the two bit streams of kc_extract's LDS, kept in device memory -----------
// code[p / 32] holds position p in bits 63 - 2 (p % 32) and the one below, val[p / 64] in bit 63 - p % 64.  Batches are
// appended at multiples of 64 positions; the filler in between is invalid, like a separator.

// One thread per 64 positions of a batch: four 16-byte loads in, one 16-byte and one 8-byte store out (3 bits a base).
// at = the store position the batch goes to (a multiple of 64); npad = n rounded up to 64.
__global__ void __launch_bounds__(KC_TPB)
kc_pack(const uint8_t *__restrict__ seq, int64_t n, int64_t npad, int64_t at, u64 *__restrict__ code, u64 *__restrict__ val)
{ const int64_t i = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  if (64 * i >= npad) return;
  unsigned cw[4], vw[4];
#pragma unroll
  for (int c = 0; c < 4; c++)
    { const int64_t g = 64 * i + 16 * c;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (g + 16 <= n) v = *reinterpret_cast<const uint4 *>(seq + g);
      else if (g < n)
        { unsigned d[4] = { 0, 0, 0, 0 };
          for (int b = 0; b < 16 && g + b < n; b++) d[b >> 2] |= (unsigned) seq[g + b] << (8 * (b & 3));
          v = make_uint4(d[0], d[1], d[2], d[3]);
        }
      unsigned co = 0, va = 0;
      kc_code4(v.x, co, va); kc_code4(v.y, co, va); kc_code4(v.z, co, va); kc_code4(v.w, co, va);
      cw[c] = co; vw[c] = va;
    }
  const int64_t q = at / 64 + i;
  ulonglong2 cc;
  cc.x = ((u64) cw[0] << 32) | cw[1];
  cc.y = ((u64) cw[2] << 32) | cw[3];
  *reinterpret_cast<ulonglong2 *>(code + 2 * q) = cc;
  val[q] = ((u64) vw[0] << 48) | ((u64) vw[1] << 32) | ((u64) vw[2] << 16) | vw[3];
}

// the tile at position tile0 (a multiple of KC_TILE) and its halo from the store into the LDS streams; npos = positions
// in the store (a multiple of 64), beyond them nothing is valid
SMG_DEV void kc_load_tile(const u64 *__restrict__ code, const u64 *__restrict__ val, int64_t npos, int64_t tile0, u64 *s_code, u64 *s_val)
{ const int t = threadIdx.x;
  const int NC = KC_CHUNKS / 2 + 2, NV = KC_CHUNKS / 4 + 2;
  if (t < NC)
    { const int64_t g = tile0 / 32 + t;
      s_code[t] = (t < NC - 2 && g < npos / 32) ? code[g] : 0ull;
    }
  else if (t < NC + NV)
    { const int v = t - NC;
      const int64_t g = tile0 / 64 + v;
      s_val[v] = (v < NV - 2 && g < npos / 64) ? val[g] : 0ull;
    }
}

// windows per bin of the leading bits of the canonical k-mer: LDS bins, flushed once per workgroup (grid-stride over tiles)
__global__ void __launch_bounds__(KC_TPB)
kc_bins(const u64 *__restrict__ code, const u64 *__restrict__ val, int64_t npos, int k, unsigned long long *__restrict__ bins)
{ __shared__ u64 s_code[KC_CHUNKS / 2 + 2];
  __shared__ u64 s_val[KC_CHUNKS / 4 + 2];
  __shared__ unsigned h[SMG_COUNT_BINS];
  const int t = threadIdx.x;
  for (int b = t; b < SMG_COUNT_BINS; b += KC_TPB) h[b] = 0;
  const int64_t ntiles = (npos + KC_TILE - 1) / KC_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)     // (at most 2^32 / KC_TILE tiles per workgroup: host)
    { __syncthreads();
      kc_load_tile(code, val, npos, tile * KC_TILE, s_code, s_val);
      __syncthreads();
#pragma unroll 4
      for (int j = 0; j < KC_TILE / KC_TPB; j++)
        { const int p = j * KC_TPB + t;
          if (kc_window(s_val, p, k)) atomicAdd(&h[kc_bin(s_code, p, k)], 1u);
        }
    }
  __syncthreads();
  for (int b = t; b < SMG_COUNT_BINS; b += KC_TPB)
    if (h[b]) atomicAdd(&bins[b], (unsigned long long) h[b]);
}

// kc_bins restricted to ONE bin: the windows whose leading 12 bits are `bin`, counted by their next 12 bits.  Launched once
// per bin that is above one merge, which is rare: the 4096 LDS bins, the grid-stride and the single flush are kc_bins'.
__global__ void __launch_bounds__(KC_TPB)
kc_subbins(const u64 *__restrict__ code, const u64 *__restrict__ val, int64_t npos, int k, unsigned bin, unsigned long long *__restrict__ sub)
{ __shared__ u64 s_code[KC_CHUNKS / 2 + 2];
  __shared__ u64 s_val[KC_CHUNKS / 4 + 2];
  __shared__ unsigned h[SMG_COUNT_BINS];
  const int t = threadIdx.x;
  for (int b = t; b < SMG_COUNT_BINS; b += KC_TPB) h[b] = 0;
  const int64_t ntiles = (npos + KC_TILE - 1) / KC_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
    { __syncthreads();
      kc_load_tile(code, val, npos, tile * KC_TILE, s_code, s_val);
      __syncthreads();
#pragma unroll 4
      for (int j = 0; j < KC_TILE / KC_TPB; j++)
        { const int p = j * KC_TPB + t;
          if (kc_window(s_val, p, k))
            { const unsigned f = kc_bin24(s_code, p, k);
              if ((f >> SMG_COUNT_BIN_BITS) == bin) atomicAdd(&h[f & (SMG_COUNT_BINS - 1u)], 1u);
            }
        }
    }
  __syncthreads();
  for (int b = t; b < SMG_COUNT_BINS; b += KC_TPB)
    if (h[b]) atomicAdd(&sub[b], (unsigned long long) h[b]);
}

// kc_extract with its front half replaced by loads of the two streams from the store: the windows that start in
// [p0, p1) and whose bin lies in [lo, hi).  The grid starts at the tile that holds p0; 0.375 bytes in per position.
template <int W> __global__ void __launch_bounds__(KC_TPB)
kc_extract_packed(const u64 *__restrict__ code, const u64 *__restrict__ val, int64_t npos, int64_t p0, int64_t p1, int k,
                  unsigned lo, unsigned hi, u64 *__restrict__ out, unsigned long long limit, unsigned long long *__restrict__ nout)
{ __shared__ u64 s_code[KC_CHUNKS / 2 + 2];
  __shared__ u64 s_val[KC_CHUNKS / 4 + 2];
  __shared__ unsigned s_cnt[64];
  __shared__ unsigned long long s_base;
  const int64_t tile0 = (p0 / KC_TILE + blockIdx.x) * KC_TILE;
  kc_load_tile(code, val, npos, tile0, s_code, s_val);
  __syncthreads();
  kc_emit<W, SMG_COUNT_BIN_BITS>(s_code, s_val, s_cnt, &s_base, tile0, p0, p1, k, lo, hi, out, limit, nout);
}

// The same with lo and hi on the leading 24 bits, for a range with an end inside a split bin.  A kernel of its own and
// not a run-time switch in kc_extract_packed: a range of whole 12-bit bins keeps the pass it had, which is bound by what
// it does per position (profiles/count_partitioned.md).
template <int W> __global__ void __launch_bounds__(KC_TPB)
kc_extract_fine(const u64 *__restrict__ code, const u64 *__restrict__ val, int64_t npos, int64_t p0, int64_t p1, int k,
                unsigned lo, unsigned hi, u64 *__restrict__ out, unsigned long long limit, unsigned long long *__restrict__ nout)
{ __shared__ u64 s_code[KC_CHUNKS / 2 + 2];
  __shared__ u64 s_val[KC_CHUNKS / 4 + 2];
  __shared__ unsigned s_cnt[64];
  __shared__ unsigned long long s_base;
  const int64_t tile0 = (p0 / KC_TILE + blockIdx.x) * KC_TILE;
  kc_load_tile(code, val, npos, tile0, s_code, s_val);
  __syncthreads();
  kc_emit<W, SMG_COUNT_FINE_BITS>(s_code, s_val, s_cnt, &s_base, tile0, p0, p1, k, lo, hi, out, limit, nout);
}

template <int W> __global__ void __launch_bounds__(KC_TPB)
kc_gather_entries(const u64 *__restrict__ keys, const uint32_t *__restrict__ val, const uint32_t *__restrict__ perm, int64_t n,
                  u64 *__restrict__ okeys, uint32_t *__restrict__ oval)
{ const int64_t i = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = perm[i];
  const Key<W> x = load_key<W>(keys, s);
#pragma unroll
  for (int w = 0; w < W; w++) okeys[(size_t) i * W + w] = x.w[w];
  if (val) oval[i] = val[s];
}

// head flags on sorted keys; an all-ones key is no k-mer (never canonical: the complement of t..t is a..a, pad bits are 0)
template <int W> __global__ void __launch_bounds__(KC_TPB)
kc_flag_heads(const u64 *__restrict__ keys, int64_t n, uint32_t *__restrict__ flag)
{ const int64_t i = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  if (i >= n) return;
  const Key<W> x = load_key<W>(keys, i);
  bool head = !kc_all_ones<W>(x);
  if (head && i > 0) head = !key_eq<W>(x, load_key<W>(keys, i - 1));
  flag[i] = head;
}

// run j starts at start[j]; start[number of runs] = number of k-mers
template <int W> __global__ void __launch_bounds__(KC_TPB)
kc_runs(const u64 *__restrict__ keys, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t n,
        u64 *__restrict__ ukeys, uint32_t *__restrict__ start)
{ const int64_t i = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  if (i >= n) return;
  const Key<W> x = load_key<W>(keys, i);
  if (kc_all_ones<W>(x)) return;
  const uint32_t f = flag[i], q = pos[i];
  if (f)
    {
#pragma unroll
      for (int w = 0; w < W; w++) ukeys[(size_t) q * W + w] = x.w[w];
      start[q] = (uint32_t) i;
    }
  if (i == n - 1 || kc_all_ones<W>(load_key<W>(keys, i + 1))) start[q + f] = (uint32_t) (i + 1);
}

__global__ void __launch_bounds__(KC_TPB)
kc_run_counts(const uint32_t *__restrict__ start, int64_t nruns, uint32_t *__restrict__ cnt)
{ const int64_t j = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  if (j < nruns) cnt[j] = start[j + 1] - start[j];
}

// both merged lists were duplicate free: a k-mer occurs once or twice, the head takes its right-hand neighbour's count
template <int W> __global__ void __launch_bounds__(KC_TPB)
kc_merge_write(const u64 *__restrict__ keys, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ flag,
               const uint32_t *__restrict__ pos, int64_t n, u64 *__restrict__ okeys, uint32_t *__restrict__ ocnt)
{ const int64_t i = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const Key<W> x = load_key<W>(keys, i);
  uint32_t c = cnt[i];
  if (i + 1 < n && key_eq<W>(x, load_key<W>(keys, i + 1)))
    { const uint32_t s = c + cnt[i + 1];
      c = s < c ? 0xFFFFFFFFu : s;
    }
  const uint32_t q = pos[i];
#pragma unroll
  for (int w = 0; w < W; w++) okeys[(size_t) q * W + w] = x.w[w];
  ocnt[q] = c;
}

// histogram of the clamped counts (LDS bins below KC_HBINS, flushed once per workgroup; the rare larger counts go
// straight to the global bins) and the trim flag
__global__ void __launch_bounds__(KC_TPB)
kc_finish_flag(const uint32_t *__restrict__ cnt, int64_t n, unsigned t, unsigned long long *__restrict__ hist, uint32_t *__restrict__ flag)
{ __shared__ unsigned h[KC_HBINS];
  for (int b = threadIdx.x; b < KC_HBINS; b += KC_TPB) h[b] = 0;
  __syncthreads();
  for (int64_t i = (int64_t) blockIdx.x * KC_TPB + threadIdx.x; i < n; i += (int64_t) gridDim.x * KC_TPB)
    { unsigned c = cnt[i];
      if (c > SMG_COUNT_MAX_COUNT) c = SMG_COUNT_MAX_COUNT;
      flag[i] = c >= t;
      if (c < KC_HBINS) atomicAdd(&h[c], 1u); else atomicAdd(&hist[c], 1ull);
    }
  __syncthreads();
  for (int b = threadIdx.x; b < KC_HBINS; b += KC_TPB)
    if (h[b]) atomicAdd(&hist[b], (unsigned long long) h[b]);
}

template <int W> __global__ void __launch_bounds__(KC_TPB)
kc_finish_compact(const u64 *__restrict__ keys, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ flag,
                  const uint32_t *__restrict__ pos, int64_t n, u64 *__restrict__ okeys, uint16_t *__restrict__ ocnt)
{ const int64_t i = (int64_t) blockIdx.x * KC_TPB + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const Key<W> x = load_key<W>(keys, i);
  const uint32_t q = pos[i], c = cnt[i];
#pragma unroll
  for (int w = 0; w < W; w++) okeys[(size_t) q * W + w] = x.w[w];
  ocnt[q] = (uint16_t) (c > SMG_COUNT_MAX_COUNT ? SMG_COUNT_MAX_COUNT : c);
}

// ---------------------------------------------------------------------------------------------------------------
//  host: errors, parser
// ---------------------------------------------------------------------------------------------------------------

static int fail(char *errbuf, size_t errlen, int code, const char *fmt, ...)
{ if (errbuf && errlen)
    { va_list ap;
      va_start(ap, fmt);
      vsnprintf(errbuf, errlen, fmt, ap);
      va_end(ap);
    }
  return code;
}

static double now_ms()
{ return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Sink
{ virtual bool put(const uint8_t *p, size_t n) = 0;          // false: the consumer gave up
  virtual ~Sink() {}
};

// Line-wise state machine over the bytes of one file, fed in arbitrary pieces.  A '\r' is dropped only in front of a
// '\n' or at the end of the file; anywhere else it is a byte like any other (and ends a stretch).
struct Parser
{ Sink &out;
  int fmt = 0, phase = 0, kind = 0;                           // fmt 1 FASTA, 2 FASTQ; kind 0 skip, 1 sequence, 2 blank
  bool bol = true, first = true, pending_cr = false, started = false;
  int64_t bases = 0;
  explicit Parser(Sink &s) : out(s) {}

  bool emit(const uint8_t *p, size_t n) { bases += (int64_t) n; return n == 0 || out.put(p, n); }
  bool record() { const uint8_t sep = SMG_COUNT_SEPARATOR; const bool ok = first || out.put(&sep, 1); first = false; return ok; }

  // 0 ok, 1 the consumer gave up, SMG_EINVAL with a message
  int feed(const uint8_t *p, size_t n, const char *path, char *errbuf, size_t errlen)
  { size_t i = 0;
    if (n == 0) return 0;
    if (!started)
      { started = true;
        if (p[0] == 0x1f && (n < 2 || p[1] == 0x8b))
          return fail(errbuf, errlen, SMG_EINVAL, "%s is gzip compressed: compressed input is not supported, decompress it first", path);
        if (p[0] == '>') fmt = 1;
        else if (p[0] == '@') fmt = 2;
        else return fail(errbuf, errlen, SMG_EINVAL, "%s is neither FASTA nor FASTQ (first byte 0x%02x)", path, p[0]);
      }
    if (pending_cr)
      { const uint8_t cr = '\r';
        pending_cr = false;
        if (p[0] != '\n' && !emit(&cr, 1)) return 1;
      }
    while (i < n)
      { if (bol)
          { const uint8_t c = p[i];
            bol = false;
            if (fmt == 1)
              { kind = c != '>';
                if (c == '>' && !record()) return 1;
              }
            else if (phase == 0)
              { kind = (c == '\n' || c == '\r') ? 2 : 0;     // (blank lines between records are passed over)
                if (kind == 0 && !record()) return 1;
              }
            else kind = phase == 1;
          }
        const uint8_t *nl = (const uint8_t *) memchr(p + i, '\n', n - i);
        const size_t end = nl ? (size_t) (nl - p) : n;
        if (kind == 1)
          { size_t e = end;
            if (e > i && p[e - 1] == '\r') { e--; if (!nl) pending_cr = true; }
            if (!emit(p + i, e - i)) return 1;
          }
        if (nl)
          { bol = true;
            if (fmt == 2 && kind != 2) phase = (phase + 1) & 3;
            i = end + 1;
          }
        else i = n;
      }
    return 0;
  }
};

static int parse_fd(int fd, const char *path, Sink &sink, int64_t *bases, char *errbuf, size_t errlen)
{ std::vector<uint8_t> buf((size_t) 4 << 20);
  Parser ps(sink);
  for (;;)
    { const ssize_t got = read(fd, buf.data(), buf.size());
      if (got < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
      if (got == 0) break;
      const int rc = ps.feed(buf.data(), (size_t) got, path, errbuf, errlen);
      if (rc) return rc;
    }
  if (bases) *bases = ps.bases;
  return 0;
}

struct GrowSink : Sink
{ uint8_t *p = nullptr; size_t len = 0, cap = 0;
  bool put(const uint8_t *s, size_t n) override
  { if (len + n > cap)
      { size_t nc = cap ? cap * 2 : (size_t) 1 << 16;
        while (nc < len + n) nc *= 2;
        uint8_t *q = (uint8_t *) realloc(p, nc);
        if (!q) throw std::bad_alloc();
        p = q; cap = nc;
      }
    memcpy(p + len, s, n); len += n;
    return true;
  }
  ~GrowSink() override { free(p); }
};

// ---------------------------------------------------------------------------------------------------------------
//  host: the device side of a run
// ---------------------------------------------------------------------------------------------------------------

#define DCHK(call) do { hipError_t _e = (call); if (_e != hipSuccess) \
    return fail(errbuf, errlen, _e == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV, "HIP error: %s (" #call ")", hipGetErrorString(_e)); } while (0)
#define RCHK(call) do { const int _rc = (call); if (_rc) return _rc; } while (0)

static unsigned nblk(int64_t n) { return (unsigned) ((n + KC_TPB - 1) / KC_TPB); }

struct Counter
{ int k = 0, W = 1, t = 1;
  char *errbuf = nullptr; size_t errlen = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int64_t cap = 0;                                             // bytes of sequence a batch holds
  int64_t fill = 0;                                            // bytes in the batch buffer
  int last_file = -1;                                          // the file whose stream ends at `fill`
  std::vector<std::vector<uint8_t>> tails;                     // per file: the last k-1 bytes handed over
  Dev seq, ka, kb, flag, pos, start, tmp, ctr, dk, dc;         // tmp: the grow-only rocPRIM scratch; dk, dc: the running distinct list (k-mers, uint32 counts)
  int64_t nd = 0;
  smg_count_stats st;
  // a partitioned run: the packed input (positions; store_n is a multiple of 64), the bins, the host table so far
  bool parted = false;
  int req_parts = 0;
  int64_t max_entries = 0;
  Dev scode, sval, dh;
  int64_t store_cap = 0, store_n = 0;
  smg_count_parts pt;
  uint64_t *hk = nullptr; uint16_t *hc = nullptr;
  int64_t hn = 0, hcap = 0;
  // the _device entries: the table so far stays in device memory (tk, tc: whole allocations of tcap entries, tn in use)
  bool dev_out = false;
  Dev tk, tc;
  int64_t tn = 0, tcap = 0;

  ~Counter()
  { free(hk); free(hc);
    if (ev0) (void) hipEventDestroy(ev0);
    if (ev1) (void) hipEventDestroy(ev1);
    if (stream) (void) hipStreamDestroy(stream);
  }

  int alloc(Dev &d, size_t bytes)
  { const hipError_t e = d.alloc(bytes);
    if (e != hipSuccess)
      return fail(errbuf, errlen, e == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV,
                  "cannot allocate %.3f GB of device memory: %s", (double) bytes * 1e-9, hipGetErrorString(e));
    return 0;
  }

  void tic() { (void) hipEventRecord(ev0, stream); }
  int toc(double *acc)
  { float ms = 0;
    DCHK(hipEventRecord(ev1, stream));
    DCHK(hipEventSynchronize(ev1));
    DCHK(hipEventElapsedTime(&ms, ev0, ev1));
    *acc += ms;
    return 0;
  }

  size_t merge_price() const { return 3 * (sizeof(u64) * W + sizeof(uint32_t)) + 8 + (W > 1 ? 24 : 0); }   // bytes per merged entry

  // positions a batch holds when `avail` bytes are there to share between the batch and the merges
  int64_t batch_cap(size_t avail, int64_t per, int64_t bound) const
  { int64_t c = (int64_t) (avail / 3) / per;
    if (c > ((int64_t) 1 << 30)) c = (int64_t) 1 << 30;
    const char *hook = getenv("SMG_COUNT_BATCH_BASES");
    if (hook && atoll(hook) > 0) c = atoll(hook) + k;
    if (c > bound + k + 1) c = bound + k + 1;
    if (c < k + 1) c = k + 1;
    return c;
  }

  // Memory plan, before the first allocation: a third of what is free goes to the batch (sequence, two key buffers,
  // flags, positions, run starts, and the word sort's scratch for W > 1), the rest is left to the distinct list and
  // its merge.  `bound` is the most sequence the input can hold, hence a bound on its windows and its distinct k-mers:
  // where a merge of that many entries fits next to the batch, the run is one pass; otherwise (or when the caller asks
  // for ranges) the batches are packed into a store that comes off the top, and the ranges are planned in finish().
  int init(const smg_count_opts *o, const smg_count_parts *parts, int64_t bound, int nfiles, char *eb, size_t el)
  { errbuf = eb; errlen = el;
    memset(&st, 0, sizeof(st));
    memset(&pt, 0, sizeof(pt));
    if (parts)
      { if (parts->partitions < 0 || parts->partitions > SMG_COUNT_BINS)
          return fail(errbuf, errlen, SMG_EINVAL, "partitions = %d is out of range 0 .. %d", parts->partitions, SMG_COUNT_BINS);
        if (parts->max_entries < 0) return fail(errbuf, errlen, SMG_EINVAL, "max_entries = %lld is negative", (long long) parts->max_entries);
        req_parts = parts->partitions; max_entries = parts->max_entries;
      }
    pt.used = 1;
    k = o->kmer; t = o->minval; W = (k + 31) / 32;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
      return fail(errbuf, errlen, SMG_ENODEV, "no HIP device: the k-mer counter has no CPU fallback%s", "");
    if (o->device < 0 || o->device >= ndev) return fail(errbuf, errlen, SMG_EINVAL, "device %d of %d", o->device, ndev);
    DCHK(hipSetDevice(o->device));
    size_t free_b = 0, total_b = 0;
    DCHK(hipMemGetInfo(&free_b, &total_b));
    const int64_t per = 1 + 16 * W + 12 + (W > 1 ? 24 : 0);
    int64_t c = batch_cap(free_b, per, bound);
    parted = req_parts > 1;
    if (req_parts == 0)
      { const bool fits = bound < 0xFFFFFFF0ll &&
                          (size_t) (c * per) + (size_t) bound * merge_price() + ((size_t) 64 << 20) <= free_b;
        parted = !(fits && (max_entries == 0 || bound <= max_entries));
      }
    if (parted)
      { store_cap = ((bound + bound / 32 + ((int64_t) 1 << 16)) + KC_TILE - 1) / KC_TILE * KC_TILE;
        const size_t need = (size_t) store_cap / 8 * 3;
        if (need + ((size_t) 64 << 20) > free_b)
          return fail(errbuf, errlen, SMG_ENOMEM, "the packed input does not fit the device: a store of %lld positions needs %.3f GB, "
                      "%.3f GB of device memory are free", (long long) store_cap, (double) need * 1e-9, (double) free_b * 1e-9);
        free_b -= need;
        c = batch_cap(free_b, per, bound);
      }
    if (c * per > (int64_t) free_b)
      return fail(errbuf, errlen, SMG_ENOMEM, "a batch of %lld bases needs %.3f GB, %.3f GB of device memory are free",
                  (long long) c, (double) (c * per) * 1e-9, (double) free_b * 1e-9);
    cap = c;
    tails.assign((size_t) (nfiles > 0 ? nfiles : 1), std::vector<uint8_t>());
    DCHK(hipStreamCreate(&stream));
    DCHK(hipEventCreate(&ev0));
    DCHK(hipEventCreate(&ev1));
    RCHK(alloc(seq, (size_t) cap + 16));
    RCHK(alloc(ka, sizeof(u64) * (size_t) cap * W));
    RCHK(alloc(kb, sizeof(u64) * (size_t) cap * W));
    RCHK(alloc(flag, sizeof(uint32_t) * (size_t) cap));
    RCHK(alloc(pos, sizeof(uint32_t) * (size_t) cap));
    RCHK(alloc(start, sizeof(uint32_t) * ((size_t) cap + 1)));
    RCHK(alloc(ctr, 16));
    if (parted)
      { RCHK(alloc(scode, (size_t) store_cap / 4)); RCHK(alloc(sval, (size_t) store_cap / 8));
        pt.store_bytes = store_cap / 8 * 3;
      }
    return 0;
  }

  // room for `more` positions behind store_n (the size bound of the input does not count the separators and re-prefixed
  // tails that batches and interleaved files add, so the store may have to grow)
  int need_store(int64_t more)
  { if (store_n + more <= store_cap) return 0;
    int64_t nc = store_cap + store_cap / 2;
    if (nc < store_n + more) nc = store_n + more;
    nc = (nc + KC_TILE - 1) / KC_TILE * KC_TILE;
    Dev c2, v2;
    RCHK(alloc(c2, (size_t) nc / 4)); RCHK(alloc(v2, (size_t) nc / 8));
    DCHK(hipMemcpyAsync(c2.p, scode.p, (size_t) store_n / 4, hipMemcpyDeviceToDevice, stream));
    DCHK(hipMemcpyAsync(v2.p, sval.p, (size_t) store_n / 8, hipMemcpyDeviceToDevice, stream));
    DCHK(hipStreamSynchronize(stream));
    scode.take(c2); sval.take(v2);
    store_cap = nc; pt.store_bytes = nc / 8 * 3;
    return 0;
  }

  // the batch buffer -> 3 bits per position behind the store
  int pack()
  { const int64_t n = fill;
    fill = 0; last_file = -1;
    if (n < k) return 0;
    const int64_t npad = (n + 63) / 64 * 64;
    RCHK(need_store(npad));
    tic();
    hipLaunchKernelGGL(kc_pack, dim3(nblk(npad / 64)), dim3(KC_TPB), 0, stream, seq.as<uint8_t>(), n, npad, store_n,
                       scode.as<u64>(), sval.as<u64>());
    DCHK(hipGetLastError());
    RCHK(toc(&pt.ms_pack));
    store_n += npad;
    return 0;
  }

  // bytes of one file's stream, in order; pieces go into the batch buffer, full batches are counted
  int add(const uint8_t *p, int64_t n, int file)
  { std::vector<uint8_t> &tail = tails[(size_t) file];
    while (n > 0)
      { const bool joined = last_file == file && fill > 0;
        const int64_t lead = joined ? 0 : 1 + (int64_t) tail.size();
        if (cap - fill < lead + 1) { RCHK(flush()); continue; }
        if (!joined)
          { uint8_t head[SMG_MAX_KMER + 1];
            head[0] = SMG_COUNT_SEPARATOR;
            if (!tail.empty()) memcpy(head + 1, tail.data(), tail.size());
            DCHK(hipMemcpy(seq.as<uint8_t>() + fill, head, (size_t) lead, hipMemcpyHostToDevice));
            fill += lead;
          }
        const int64_t m = n < cap - fill ? n : cap - fill;
        DCHK(hipMemcpy(seq.as<uint8_t>() + fill, p, (size_t) m, hipMemcpyHostToDevice));
        fill += m;
        last_file = file;
        if (m >= k - 1) tail.assign(p + m - (k - 1), p + m);      // the last k-1 bytes of (tail + piece)
        else
          { tail.insert(tail.end(), p, p + m);
            if ((int64_t) tail.size() > k - 1) tail.erase(tail.begin(), tail.end() - (k - 1));
          }
        p += m; n -= m;
      }
    return 0;
  }

  // sorts n entries (W-word k-mers, optional uint32 values) that lie in (a, va); (b, vb) are buffers of the same size.
  // The result is in (*ko, *vo), one of the two.
  int sort_entries(u64 *a, u64 *b, uint32_t *va, uint32_t *vb, int64_t n, u64 **ko, uint32_t **vo)
  { if (W == 1)
      { rocprim::double_buffer<u64> dk2(a, b);
        rocprim::double_buffer<uint32_t> dv2(va, vb);
        // All 64 bits, not 64-2k .. 64: the pad bits are zero, so the order is the same, and a partial bit range is not
        // safe on rocPRIM's merge-sort path (sort_permutation, smg_keysort.hpp).
        const unsigned b0 = 0u;
        DCHK(with_scratch(tmp, [&](void *t, size_t &bytes)
          { return va ? rocprim::radix_sort_pairs(t, bytes, dk2, dv2, (size_t) n, b0, 64u, stream)
                      : rocprim::radix_sort_keys(t, bytes, dk2, (size_t) n, b0, 64u, stream); }));
        *ko = dk2.current();
        if (vo) *vo = va ? dv2.current() : nullptr;
        return 0;
      }
    // W > 1: the sorted order as a permutation (smg_keysort.hpp), then one gather
    Dev perm;
    DCHK(sort_permutation(a, W, n, stream, tmp, perm));
    with_words<4>(W, [&](auto w) { hipLaunchKernelGGL(kc_gather_entries<w()>, dim3(nblk(n)), dim3(KC_TPB), 0, stream, a, va, perm.as<uint32_t>(), n, b, vb); });
    DCHK(hipStreamSynchronize(stream));                        // (the permutation is freed on return)
    *ko = b;
    if (vo) *vo = va ? vb : nullptr;
    return 0;
  }

  // the batch buffer -> (k-mer, count) runs -> merged into the distinct list (a partitioned run packs it instead)
  int flush()
  { if (parted) return pack();
    const int64_t n = fill;
    fill = 0; last_file = -1;
    if (n < k) return 0;
    st.batches++;
    tic();
    DCHK(hipMemsetAsync(ctr.p, 0, 16, stream));
    const unsigned ntiles = (unsigned) ((n + KC_TILE - 1) / KC_TILE);
    with_words<4>(W, [&](auto w) { hipLaunchKernelGGL(kc_extract<w()>, dim3(ntiles), dim3(KC_TPB), 0, stream, seq.as<uint8_t>(), n, k, ka.as<u64>(),
        ctr.as<unsigned long long>()); });
    DCHK(hipGetLastError());
    unsigned long long nwin = 0;
    DCHK(hipMemcpyAsync(&nwin, ctr.p, 8, hipMemcpyDeviceToHost, stream));
    RCHK(toc(&st.ms_extract));
    if (nwin == 0) return 0;
    if ((int64_t) nwin > cap) return fail(errbuf, errlen, SMG_ENODEV, "internal error: %llu windows from %lld bytes", nwin, (long long) n);
    return count_keys((int64_t) nwin);
  }

  // nwin canonical k-mers in ka -> sorted -> (k-mer, count) runs -> merged into the distinct list
  int count_keys(int64_t nwin)
  { st.windows += nwin;
    u64 *sorted = nullptr;
    tic();
    RCHK(sort_entries(ka.as<u64>(), kb.as<u64>(), nullptr, nullptr, (int64_t) nwin, &sorted, nullptr));
    RCHK(toc(&st.ms_sort));
    u64 *uk = sorted == ka.as<u64>() ? kb.as<u64>() : ka.as<u64>();
    int64_t nruns = 0;
    tic();
    with_words<4>(W, [&](auto w) { hipLaunchKernelGGL(kc_flag_heads<w()>, dim3(nblk(nwin)), dim3(KC_TPB), 0, stream, sorted, (int64_t) nwin, flag.as<uint32_t>()); });
    DCHK(scan_flags(flag.as<uint32_t>(), pos.as<uint32_t>(), (int64_t) nwin, stream, tmp, &nruns));
    with_words<4>(W, [&](auto w) { hipLaunchKernelGGL(kc_runs<w()>, dim3(nblk(nwin)), dim3(KC_TPB), 0, stream, sorted, flag.as<uint32_t>(), pos.as<uint32_t>(),
        (int64_t) nwin, uk, start.as<uint32_t>()); });
    uint32_t *rc = flag.as<uint32_t>();                        // (the flags are spent: the run counts take their place)
    hipLaunchKernelGGL(kc_run_counts, dim3(nblk(nruns)), dim3(KC_TPB), 0, stream, start.as<uint32_t>(), nruns, rc);
    DCHK(hipGetLastError());
    RCHK(merge(uk, rc, nruns));
    RCHK(toc(&st.ms_reduce));
    return 0;
  }

  int merge(const u64 *uk, const uint32_t *rc, int64_t nr)
  { if (max_entries && nd + nr > max_entries)
      return fail(errbuf, errlen, SMG_ENOMEM, "the distinct k-mers of this data set do not fit the device: merging %lld entries, "
                  "one merge holds %lld (max_entries)", (long long) (nd + nr), (long long) max_entries);
    if (nd == 0)
      { Dev nk, nc;
        RCHK(alloc(nk, sizeof(u64) * (size_t) nr * W)); RCHK(alloc(nc, sizeof(uint32_t) * (size_t) nr));
        DCHK(hipMemcpyAsync(nk.p, uk, sizeof(u64) * (size_t) nr * W, hipMemcpyDeviceToDevice, stream));
        DCHK(hipMemcpyAsync(nc.p, rc, sizeof(uint32_t) * (size_t) nr, hipMemcpyDeviceToDevice, stream));
        DCHK(hipStreamSynchronize(stream));
        dk.take(nk); dc.take(nc); nd = nr;
        return 0;
      }
    const int64_t m = nd + nr;
    if (m >= 0xFFFFFFF0ll)
      return fail(errbuf, errlen, SMG_ENOMEM, "more than 2^32 - 16 entries in one merge (%lld): this many distinct k-mers need more than one "
                  "key range", (long long) m);
    const size_t want = (size_t) m * merge_price() + ((size_t) 64 << 20);
    size_t free_b = 0, total_b = 0;
    DCHK(hipMemGetInfo(&free_b, &total_b));
    if (want > free_b)
      return fail(errbuf, errlen, SMG_ENOMEM, "the distinct k-mers of this data set do not fit the device: merging %lld entries needs "
                  "%.3f GB, %.3f GB are free", (long long) m, (double) want * 1e-9, (double) free_b * 1e-9);
    Dev ck, cc, ak, ac, mf, mp, nk, nc;
    RCHK(alloc(ck, sizeof(u64) * (size_t) m * W)); RCHK(alloc(cc, sizeof(uint32_t) * (size_t) m));
    RCHK(alloc(ak, sizeof(u64) * (size_t) m * W)); RCHK(alloc(ac, sizeof(uint32_t) * (size_t) m));
    DCHK(hipMemcpyAsync(ck.p, dk.p, sizeof(u64) * (size_t) nd * W, hipMemcpyDeviceToDevice, stream));
    DCHK(hipMemcpyAsync(ck.as<u64>() + (size_t) nd * W, uk, sizeof(u64) * (size_t) nr * W, hipMemcpyDeviceToDevice, stream));
    DCHK(hipMemcpyAsync(cc.p, dc.p, sizeof(uint32_t) * (size_t) nd, hipMemcpyDeviceToDevice, stream));
    DCHK(hipMemcpyAsync(cc.as<uint32_t>() + nd, rc, sizeof(uint32_t) * (size_t) nr, hipMemcpyDeviceToDevice, stream));
    DCHK(hipStreamSynchronize(stream));
    dk.reset(); dc.reset(); nd = 0;
    u64 *sk = nullptr; uint32_t *sc = nullptr;
    RCHK(sort_entries(ck.as<u64>(), ak.as<u64>(), cc.as<uint32_t>(), ac.as<uint32_t>(), m, &sk, &sc));
    RCHK(alloc(mf, sizeof(uint32_t) * (size_t) m)); RCHK(alloc(mp, sizeof(uint32_t) * (size_t) m));
    with_words<4>(W, [&](auto w) { hipLaunchKernelGGL(kc_flag_heads<w()>, dim3(nblk(m)), dim3(KC_TPB), 0, stream, sk, m, mf.as<uint32_t>()); });
    int64_t nn = 0;
    DCHK(scan_flags(mf.as<uint32_t>(), mp.as<uint32_t>(), m, stream, tmp, &nn));
    RCHK(alloc(nk, sizeof(u64) * (size_t) nn * W)); RCHK(alloc(nc, sizeof(uint32_t) * (size_t) nn));
    with_words<4>(W, [&](auto w) { hipLaunchKernelGGL(kc_merge_write<w()>, dim3(nblk(m)), dim3(KC_TPB), 0, stream, sk, sc, mf.as<uint32_t>(), mp.as<uint32_t>(), m,
        nk.as<u64>(), nc.as<uint32_t>()); });
    DCHK(hipGetLastError());
    DCHK(hipStreamSynchronize(stream));
    dk.take(nk); dc.take(nc); nd = nn;
    return 0;
  }

  // histogram, clamp and trim of the distinct list, which is final; its kept entries go behind the host table
  int finish_range()
  { int64_t kept = 0;
    Dev ff, fp, ok, oc;
    tic();
    if (nd > 0)
      { RCHK(alloc(ff, sizeof(uint32_t) * (size_t) nd)); RCHK(alloc(fp, sizeof(uint32_t) * (size_t) nd));
        const unsigned g = nblk(nd) < 2048u ? nblk(nd) : 2048u;
        hipLaunchKernelGGL(kc_finish_flag, dim3(g), dim3(KC_TPB), 0, stream, dc.as<uint32_t>(), nd, (unsigned) t,
                           dh.as<unsigned long long>(), ff.as<uint32_t>());
        DCHK(scan_flags(ff.as<uint32_t>(), fp.as<uint32_t>(), nd, stream, tmp, &kept));
        RCHK(alloc(ok, sizeof(u64) * (size_t) kept * W)); RCHK(alloc(oc, sizeof(uint16_t) * (size_t) kept));
        with_words<4>(W, [&](auto w) { hipLaunchKernelGGL(kc_finish_compact<w()>, dim3(nblk(nd)), dim3(KC_TPB), 0, stream, dk.as<u64>(), dc.as<uint32_t>(),
            ff.as<uint32_t>(), fp.as<uint32_t>(), nd, ok.as<u64>(), oc.as<uint16_t>()); });
        DCHK(hipGetLastError());
      }
    RCHK(toc(&st.ms_finish));
    st.distinct += nd;
    st.kept += kept;
    if (dev_out)
      { RCHK(append_device(ok, oc, kept));
        dk.reset(); dc.reset(); nd = 0;
        return 0;
      }
    if (hn + kept > hcap || !hk)
      { int64_t nc = hcap + hcap / 2;
        if (nc < hn + kept) nc = hn + kept;
        if (nc < 1) nc = 1;
        uint64_t *k2 = (uint64_t *) realloc(hk, sizeof(uint64_t) * (size_t) nc * W);
        if (k2) hk = k2;
        uint16_t *c2 = (uint16_t *) realloc(hc, sizeof(uint16_t) * (size_t) nc);
        if (c2) hc = c2;
        if (!k2 || !c2) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory for %lld k-mers", (long long) nc);
        hcap = nc;
      }
    if (kept > 0)
      { DCHK(hipMemcpy(hk + (size_t) hn * W, ok.p, sizeof(uint64_t) * (size_t) kept * W, hipMemcpyDeviceToHost));
        DCHK(hipMemcpy(hc + hn, oc.p, sizeof(uint16_t) * (size_t) kept, hipMemcpyDeviceToHost));
      }
    hn += kept;
    dk.reset(); dc.reset(); nd = 0;
    return 0;
  }

  // the kept entries of a range (ok, oc: whole allocations, or empty) behind the device table.  The first range's buffers
  // become the table as they are; from then on it grows by half, like the store, with a device-to-device copy.
  int append_device(Dev &ok, Dev &oc, int64_t kept)
  { if (!tk.p && ok.p && oc.p) { tk.take(ok); tc.take(oc); tn = tcap = kept; return 0; }
    if (tn + kept > tcap || !tk.p)
      { int64_t nc = tcap + tcap / 2;
        if (nc < tn + kept) nc = tn + kept;
        if (nc < 1) nc = 1;
        const size_t want = (sizeof(u64) * W + sizeof(uint16_t)) * (size_t) nc + ((size_t) 64 << 20);
        size_t free_b = 0, total_b = 0;
        DCHK(hipMemGetInfo(&free_b, &total_b));
        if (want > free_b)
          return fail(errbuf, errlen, SMG_ENOMEM, "the counted table does not fit the device next to the input: room for %lld entries needs "
                      "%.3f GB, %.3f GB are free (count to a table on disk instead: the entries that return host arrays)", (long long) nc,
                      (double) want * 1e-9, (double) free_b * 1e-9);
        Dev k2, c2;
        RCHK(alloc(k2, sizeof(u64) * (size_t) nc * W)); RCHK(alloc(c2, sizeof(uint16_t) * (size_t) nc));
        if (tn > 0)
          { DCHK(hipMemcpyAsync(k2.p, tk.p, sizeof(u64) * (size_t) tn * W, hipMemcpyDeviceToDevice, stream));
            DCHK(hipMemcpyAsync(c2.p, tc.p, sizeof(uint16_t) * (size_t) tn, hipMemcpyDeviceToDevice, stream));
            DCHK(hipStreamSynchronize(stream));
          }
        tk.take(k2); tc.take(c2); tcap = nc;
      }
    if (kept > 0)
      { DCHK(hipMemcpyAsync(tk.as<u64>() + (size_t) tn * W, ok.p, sizeof(u64) * (size_t) kept * W, hipMemcpyDeviceToDevice, stream));
        DCHK(hipMemcpyAsync(tc.as<uint16_t>() + tn, oc.p, sizeof(uint16_t) * (size_t) kept, hipMemcpyDeviceToDevice, stream));
        DCHK(hipStreamSynchronize(stream));                        // (ok and oc are freed on return)
      }
    tn += kept;
    return 0;
  }

  // Entries one merge is guaranteed to hold, now that the store and the batch buffers are allocated: the smaller of the
  // uint32 limit of the scans and what is free, priced as merge() prices it (less a reserve for the sort's scratch).
  int merge_budget(int64_t *budget)
  { size_t free_b = 0, total_b = 0;
    DCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t reserve = (size_t) 320 << 20;
    int64_t b = free_b > reserve ? (int64_t) ((free_b - reserve) / merge_price()) : 0;
    if (b > 0xFFFFFFEFll) b = 0xFFFFFFEFll;
    if (max_entries && b > max_entries) b = max_entries;
    if (b < 1)
      return fail(errbuf, errlen, SMG_ENOMEM, "no device memory is left for a merge: %.3f GB are free next to the packed input (%.3f GB) "
                  "and the batch buffers", (double) free_b * 1e-9, (double) pt.store_bytes * 1e-9);
    *budget = b;
    return 0;
  }

  // Where smg_count_plan refuses a single bin: the windows of every bin above the budget by their next 12 bits (one
  // kc_subbins pass over the store each), and the flat plan over whole bins and sub-bins.  split: those bins; sub: their
  // 4096 sub-bin windows each; cuts: values of the leading 24 bits.
  int plan_split(const std::vector<uint64_t> &bins, int64_t budget, std::vector<int32_t> &split, std::vector<uint64_t> &sub,
                 std::vector<int32_t> &cuts, int32_t *nranges)
  { uint64_t total = 0;
    for (int b = 0; b < SMG_COUNT_BINS; b++)
      { total += bins[(size_t) b];
        if (bins[(size_t) b] > (uint64_t) budget) split.push_back(b);
      }
    sub.assign(split.size() * SMG_COUNT_BINS, 0);
    Dev ds;
    RCHK(alloc(ds, sizeof(uint64_t) * SMG_COUNT_BINS));
    const int64_t ntiles = (store_n + KC_TILE - 1) / KC_TILE;
    for (size_t s = 0; s < split.size(); s++)
      { DCHK(hipMemsetAsync(ds.p, 0, sizeof(uint64_t) * SMG_COUNT_BINS, stream));
        hipLaunchKernelGGL(kc_subbins, dim3((unsigned) (ntiles < 2048 ? ntiles : 2048)), dim3(KC_TPB), 0, stream, scode.as<u64>(), sval.as<u64>(),
                           store_n, k, (unsigned) split[s], ds.as<unsigned long long>());
        DCHK(hipGetLastError());
        DCHK(hipMemcpyAsync(sub.data() + s * SMG_COUNT_BINS, ds.p, sizeof(uint64_t) * SMG_COUNT_BINS, hipMemcpyDeviceToHost, stream));
        DCHK(hipStreamSynchronize(stream));
      }
    uint64_t room = 2 * (total / (uint64_t) budget) + 5;       // (two neighbouring ranges of a greedy plan hold more than the budget)
    if (room > (uint64_t) SMG_COUNT_FINE_BINS + 1) room = (uint64_t) SMG_COUNT_FINE_BINS + 1;
    cuts.assign((size_t) room, 0);
    return smg_count_plan_fine(bins.data(), split.data(), (int32_t) split.size(), sub.data(), budget, cuts.data(), (int64_t) room, nranges,
                               errbuf, errlen);
  }

  // the ranges of a partitioned run, in ascending order
  int run_ranges()
  { const double t0 = now_ms();
    Dev db;
    std::vector<uint64_t> bins(SMG_COUNT_BINS, 0);
    std::vector<int32_t> cuts(SMG_COUNT_BINS + 1, 0);
    int32_t nranges = 1;
    RCHK(alloc(db, sizeof(uint64_t) * SMG_COUNT_BINS));
    DCHK(hipMemsetAsync(db.p, 0, sizeof(uint64_t) * SMG_COUNT_BINS, stream));
    if (store_n > 0)
      { const int64_t ntiles = (store_n + KC_TILE - 1) / KC_TILE;
        hipLaunchKernelGGL(kc_bins, dim3((unsigned) (ntiles < 2048 ? ntiles : 2048)), dim3(KC_TPB), 0, stream, scode.as<u64>(), sval.as<u64>(),
                           store_n, k, db.as<unsigned long long>());
        DCHK(hipGetLastError());
      }
    DCHK(hipMemcpyAsync(bins.data(), db.p, sizeof(uint64_t) * SMG_COUNT_BINS, hipMemcpyDeviceToHost, stream));
    DCHK(hipStreamSynchronize(stream));
    int64_t budget = 0;
    RCHK(merge_budget(&budget));
    // Automatic mode: ranges of one sorted batch each, which never merge (an extra pass over the store costs less than the
    // merge it saves, profiles/count_partitioned.md); where a single bin is above a batch, the merge limit is the budget;
    // where a single bin is above that as well, it is split on its next 12 bits and the cuts are values of 24 bits.
    int rc = SMG_ENOMEM;
    if (req_parts == 0 && cap < budget) rc = smg_count_plan(bins.data(), cap, 0, cuts.data(), &nranges, errbuf, errlen);
    if (rc == SMG_ENOMEM) rc = smg_count_plan(bins.data(), budget, req_parts, cuts.data(), &nranges, errbuf, errlen);
    std::vector<int32_t> split;
    std::vector<uint64_t> sub;
    if (rc == SMG_ENOMEM) rc = plan_split(bins, budget, split, sub, cuts, &nranges);
    else
      for (int r = 0; r <= nranges && rc == 0; r++) cuts[(size_t) r] <<= SMG_COUNT_BIN_BITS;
    RCHK(rc);
    pt.used = nranges;
    pt.split = (int32_t) split.size();
    pt.ms_plan = now_ms() - t0;

    // windows below a cut: whole bins in front of it, and inside a split bin the sub-bins in front of it
    std::vector<int64_t> cum(SMG_COUNT_BINS + 1, 0);
    for (int b = 0; b < SMG_COUNT_BINS; b++) cum[(size_t) b + 1] = cum[(size_t) b] + (int64_t) bins[(size_t) b];
    auto below = [&](unsigned x) -> int64_t
      { const unsigned b = x >> SMG_COUNT_BIN_BITS, j = x & (SMG_COUNT_BINS - 1u);
        int64_t n = cum[b];
        if (j)
          { size_t s = 0;
            while (s + 1 < split.size() && (unsigned) split[s] != b) s++;
            for (unsigned i = 0; i < j; i++) n += (int64_t) sub[s * SMG_COUNT_BINS + i];
          }
        return n;
      };

    for (int r = 0; r < nranges; r++)
      { const unsigned lo = (unsigned) cuts[(size_t) r], hi = (unsigned) cuts[(size_t) r + 1];
        const bool fine = ((lo | hi) & (SMG_COUNT_BINS - 1u)) != 0;      // an end inside a split bin: the 24-bit filter
        int64_t left = below(hi) - below(lo);                  // windows of the range not yet in the key buffer
        if (left == 0) continue;
        int64_t p = 0, have = 0;                               // next store position, keys in the buffer
        DCHK(hipMemsetAsync(ctr.p, 0, 16, stream));
        while (left > 0 && p < store_n)
          { // a span of s positions holds at most s windows: all that is left of the store if the rest of the range fits
            const int64_t room = cap - have;
            const int64_t p1 = left <= room ? store_n : (p + room < store_n ? p + room : store_n);
            const unsigned ntiles = (unsigned) ((p1 - 1) / KC_TILE - p / KC_TILE + 1);
            tic();
            with_words<4>(W, [&](auto w)
              { if (fine) hipLaunchKernelGGL(kc_extract_fine<w()>, dim3(ntiles), dim3(KC_TPB), 0, stream, scode.as<u64>(), sval.as<u64>(), store_n,
                                             p, p1, k, lo, hi, ka.as<u64>(), (unsigned long long) cap, ctr.as<unsigned long long>());
                else hipLaunchKernelGGL(kc_extract_packed<w()>, dim3(ntiles), dim3(KC_TPB), 0, stream, scode.as<u64>(), sval.as<u64>(), store_n,
                                        p, p1, k, lo >> SMG_COUNT_BIN_BITS, hi >> SMG_COUNT_BIN_BITS, ka.as<u64>(), (unsigned long long) cap,
                                        ctr.as<unsigned long long>());
              });
            DCHK(hipGetLastError());
            unsigned long long now = 0;
            DCHK(hipMemcpyAsync(&now, ctr.p, 8, hipMemcpyDeviceToHost, stream));
            RCHK(toc(&st.ms_extract));
            if ((int64_t) now > cap || (int64_t) now - have > left)
              return fail(errbuf, errlen, SMG_ENODEV, "internal error: %llu keys of range %d in a buffer of %lld, %lld were left",
                          now, r, (long long) cap, (long long) left);
            left -= (int64_t) now - have;
            have = (int64_t) now;
            p = p1;
            if (left > 0 && cap - have < (cap / 8 > 1 ? cap / 8 : 1))       // full (or nearly): sort it
              { st.batches++;
                RCHK(count_keys(have));
                have = 0;
                DCHK(hipMemsetAsync(ctr.p, 0, 16, stream));
              }
          }
        if (left != 0) return fail(errbuf, errlen, SMG_ENODEV, "internal error: %lld windows of range %d were not found again", (long long) left, r);
        if (have > 0) { st.batches++; RCHK(count_keys(have)); }
        RCHK(finish_range());
      }
    return 0;
  }

  // the last batch, then histogram, clamp, trim; the table goes to malloc'ed host arrays, or (dev_out) stays in device memory
  int finish(uint64_t **keys, uint16_t **counts, int64_t *nels, int *key_words, uint64_t *hist, smg_count_parts *parts)
  { RCHK(flush());
    seq.reset();
    RCHK(alloc(dh, sizeof(uint64_t) * SMG_COUNT_HIST));
    DCHK(hipMemsetAsync(dh.p, 0, sizeof(uint64_t) * SMG_COUNT_HIST, stream));
    if (parted) RCHK(run_ranges());
    ka.reset(); kb.reset(); start.reset(); flag.reset(); pos.reset(); scode.reset(); sval.reset();
    if (!parted || !(dev_out ? tk.p : (void *) hk)) RCHK(finish_range());       // (also the empty table of a run without any window)
    if (hist) DCHK(hipMemcpy(hist, dh.p, sizeof(uint64_t) * SMG_COUNT_HIST, hipMemcpyDeviceToHost));
    if (dev_out)
      { DCHK(hipStreamSynchronize(stream));
        *keys = (uint64_t *) tk.release(); *counts = (uint16_t *) tc.release(); *nels = tn; *key_words = W;
      }
    else
      { *keys = hk; *counts = hc; *nels = hn; *key_words = W;
        hk = nullptr; hc = nullptr;
      }
    if (parts)
      { parts->used = pt.used; parts->store_bytes = pt.store_bytes; parts->ms_pack = pt.ms_pack; parts->ms_plan = pt.ms_plan;
        parts->split = pt.split;
      }
    return 0;
  }
};

// ---------------------------------------------------------------------------------------------------------------
//  host: reader threads and the pinned ring
// ---------------------------------------------------------------------------------------------------------------

#define RING_BLOCK ((size_t) 8 << 20)

struct Block { uint8_t *p; size_t len; int file; };

struct Ring
{ std::mutex m;
  std::condition_variable cv_ready, cv_free;
  std::deque<Block> ready;
  std::vector<uint8_t *> idle;
  int live = 0;                                                // readers still at work
  bool abort = false;
  int rc = 0;
  char err[512] = { 0 };
  int64_t bases = 0;
  double t_last = 0;
};

struct RingSink : Sink
{ Ring &r; int file; uint8_t *cur = nullptr; size_t len = 0;
  RingSink(Ring &ring, int f) : r(ring), file(f) {}
  bool push()
  { std::unique_lock<std::mutex> lk(r.m);
    if (r.abort) return false;
    r.ready.push_back(Block{ cur, len, file });
    cur = nullptr; len = 0;
    r.cv_ready.notify_one();
    return true;
  }
  bool put(const uint8_t *p, size_t n) override
  { while (n)
      { if (!cur)
          { std::unique_lock<std::mutex> lk(r.m);
            r.cv_free.wait(lk, [&] { return r.abort || !r.idle.empty(); });
            if (r.abort) return false;
            cur = r.idle.back(); r.idle.pop_back();
          }
        const size_t m = n < RING_BLOCK - len ? n : RING_BLOCK - len;
        memcpy(cur + len, p, m);
        len += m; p += m; n -= m;
        if (len == RING_BLOCK && !push()) return false;
      }
    return true;
  }
  void done()
  { if (cur && len) push();
    else if (cur) { std::unique_lock<std::mutex> lk(r.m); r.idle.push_back(cur); cur = nullptr; r.cv_free.notify_one(); }
  }
};

static void reader_main(Ring *r, const char *const *paths, int npaths, int first, int step)
{ for (int f = first; f < npaths; f += step)
    { char eb[512]; eb[0] = 0;
      int rc = 0;
      int64_t bases = 0;
      try
        { RingSink sink(*r, f);
          const int fd = open(paths[f], O_RDONLY);
          if (fd < 0) rc = fail(eb, sizeof(eb), SMG_EINVAL, "cannot open %s", paths[f]);
          else
            { rc = parse_fd(fd, paths[f], sink, &bases, eb, sizeof(eb));
              close(fd);
            }
          if (rc == 0) sink.done();
        }
      catch (...) { rc = fail(eb, sizeof(eb), SMG_ENOMEM, "out of host memory while reading %s", paths[f]); }
      std::unique_lock<std::mutex> lk(r->m);
      r->bases += bases;
      if (rc < 0 && !r->rc) { r->rc = rc; memcpy(r->err, eb, sizeof(eb)); r->abort = true; r->cv_free.notify_all(); }
      if (rc != 0 || r->abort) break;
    }
  std::unique_lock<std::mutex> lk(r->m);
  r->live--;
  r->t_last = now_ms();
  r->cv_ready.notify_all();
}

static int check_opts(const smg_count_opts *o, char *errbuf, size_t errlen)
{ if (!o) return fail(errbuf, errlen, SMG_EINVAL, "null options%s", "");
  if (o->kmer < SMG_COUNT_MIN_KMER || o->kmer > SMG_MAX_KMER)
    return fail(errbuf, errlen, SMG_EINVAL, "k = %d is out of range: the table has a 3-byte prefix index, so k must be %d .. %d",
                o->kmer, SMG_COUNT_MIN_KMER, SMG_MAX_KMER);
  if (o->minval < 1 || o->minval > SMG_COUNT_MAX_COUNT)
    return fail(errbuf, errlen, SMG_EINVAL, "count threshold %d is out of range 1 .. %d", o->minval, SMG_COUNT_MAX_COUNT);
  return 0;
}

static int count_files(const char *const *paths, int npaths, const smg_count_opts *opts, smg_count_parts *parts, bool dev_out, uint64_t **keys,
                       uint16_t **counts, int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen)
{ const double t0 = now_ms();
  RCHK(check_opts(opts, errbuf, errlen));
  if (!paths || npaths < 1 || !keys || !counts || !nels || !key_words) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  int64_t bound = 0;
  for (int f = 0; f < npaths; f++)                             // refuse what cannot be read before the device is touched
    { uint8_t magic[2] = { 0, 0 };
      const int fd = open(paths[f], O_RDONLY);
      if (fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", paths[f]);
      const ssize_t got = read(fd, magic, 2);
      const off_t size = lseek(fd, 0, SEEK_END);
      close(fd);
      if (got < 0 || size < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot read %s", paths[f]);
      if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b)
        return fail(errbuf, errlen, SMG_EINVAL, "%s is gzip compressed: compressed input is not supported, decompress it first", paths[f]);
      bound += (int64_t) size + opts->kmer + 1;
    }
  Counter c;
  c.dev_out = dev_out;
  RCHK(c.init(opts, parts, bound, npaths, errbuf, errlen));

  int nthr = opts->host_threads < 1 ? 1 : opts->host_threads > 16 ? 16 : opts->host_threads;
  if (nthr > npaths) nthr = npaths;
  Ring ring;
  std::vector<uint8_t *> pinned;
  struct Unpin { std::vector<uint8_t *> &v; ~Unpin() { for (uint8_t *p : v) (void) hipHostFree(p); } } unpin{ pinned };
  pinned.reserve((size_t) (2 * nthr + 2));
  for (int b = 0; b < 2 * nthr + 2; b++)
    { uint8_t *p = nullptr;
      if (hipHostMalloc((void **) &p, RING_BLOCK, hipHostMallocDefault) != hipSuccess)
        return fail(errbuf, errlen, SMG_ENOMEM, "cannot pin %zu bytes of host memory", RING_BLOCK);
      pinned.push_back(p); ring.idle.push_back(p);
    }
  std::vector<std::thread> thr;
  thr.reserve((size_t) nthr);
  int rc = 0;
  for (int j = 0; j < nthr && rc == 0; j++)
    { try
        { { std::unique_lock<std::mutex> lk(ring.m); ring.live++; }
          thr.emplace_back(reader_main, &ring, paths, npaths, j, nthr);
        }
      catch (...)
        { std::unique_lock<std::mutex> lk(ring.m);
          ring.live--; ring.abort = true; ring.cv_free.notify_all();
          rc = fail(errbuf, errlen, SMG_ENOMEM, "cannot start reader thread %d", j);
        }
    }
  for (;;)
    { Block b{ nullptr, 0, 0 };
      { std::unique_lock<std::mutex> lk(ring.m);
        ring.cv_ready.wait(lk, [&] { return !ring.ready.empty() || ring.live == 0; });
        if (ring.ready.empty()) break;
        b = ring.ready.front(); ring.ready.pop_front();
      }
      if (rc == 0) rc = c.add(b.p, (int64_t) b.len, b.file);
      std::unique_lock<std::mutex> lk(ring.m);
      ring.idle.push_back(b.p);
      if (rc) ring.abort = true;
      ring.cv_free.notify_all();
    }
  for (std::thread &th : thr) th.join();
  if (ring.rc) { snprintf(errbuf, errlen, "%s", ring.err); return ring.rc; }
  if (rc) return rc;
  c.st.bases = ring.bases;
  c.st.ms_read = ring.t_last - t0;
  RCHK(c.finish(keys, counts, nels, key_words, hist, parts));
  c.st.ms_wall = now_ms() - t0;
  if (stats) *stats = c.st;
  return 0;
}

static int count_bases(const uint8_t *seq, int64_t n, const smg_count_opts *opts, smg_count_parts *parts, bool dev_out, uint64_t **keys,
                       uint16_t **counts, int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen)
{ const double t0 = now_ms();
  RCHK(check_opts(opts, errbuf, errlen));
  if (n < 0 || (n > 0 && !seq) || !keys || !counts || !nels || !key_words) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  Counter c;
  c.dev_out = dev_out;
  RCHK(c.init(opts, parts, n, 1, errbuf, errlen));
  const int64_t piece = (int64_t) 256 << 20;
  for (int64_t o = 0; o < n; o += piece) RCHK(c.add(seq + o, n - o < piece ? n - o : piece, 0));
  c.st.bases = n;
  c.st.ms_read = now_ms() - t0;
  RCHK(c.finish(keys, counts, nels, key_words, hist, parts));
  c.st.ms_wall = now_ms() - t0;
  if (stats) *stats = c.st;
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

extern "C" int smg_count_files(const char *const *paths, int npaths, const smg_count_opts *opts, uint64_t **keys, uint16_t **counts,
                               int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen)
{ GUARD(count_files(paths, npaths, opts, nullptr, false, keys, counts, nels, key_words, hist, stats, errbuf, errlen)) }

extern "C" int smg_count_bases(const uint8_t *seq, int64_t n, const smg_count_opts *opts, uint64_t **keys, uint16_t **counts,
                               int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf, size_t errlen)
{ GUARD(count_bases(seq, n, opts, nullptr, false, keys, counts, nels, key_words, hist, stats, errbuf, errlen)) }

extern "C" int smg_count_files_parts(const char *const *paths, int npaths, const smg_count_opts *opts, smg_count_parts *parts, uint64_t **keys,
                                     uint16_t **counts, int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf,
                                     size_t errlen)
{ GUARD(count_files(paths, npaths, opts, parts, false, keys, counts, nels, key_words, hist, stats, errbuf, errlen)) }

extern "C" int smg_count_bases_parts(const uint8_t *seq, int64_t n, const smg_count_opts *opts, smg_count_parts *parts, uint64_t **keys,
                                     uint16_t **counts, int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf,
                                     size_t errlen)
{ GUARD(count_bases(seq, n, opts, parts, false, keys, counts, nels, key_words, hist, stats, errbuf, errlen)) }

extern "C" int smg_count_files_device(const char *const *paths, int npaths, const smg_count_opts *opts, smg_count_parts *parts, uint64_t **d_keys,
                                      uint16_t **d_counts, int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf,
                                      size_t errlen)
{ GUARD(count_files(paths, npaths, opts, parts, true, d_keys, d_counts, nels, key_words, hist, stats, errbuf, errlen)) }

extern "C" int smg_count_bases_device(const uint8_t *seq, int64_t n, const smg_count_opts *opts, smg_count_parts *parts, uint64_t **d_keys,
                                      uint16_t **d_counts, int64_t *nels, int *key_words, uint64_t *hist, smg_count_stats *stats, char *errbuf,
                                      size_t errlen)
{ GUARD(count_bases(seq, n, opts, parts, true, d_keys, d_counts, nels, key_words, hist, stats, errbuf, errlen)) }

extern "C" void smg_count_device_free(void *d) { if (d) (void) hipFree(d); }

// The cuts of a partitioned run (host only).  Greedy over the bins: a range takes bins while its windows stay within the
// budget, which gives the fewest contiguous ranges; the windows of a range bound its distinct k-mers and every merge of
// it, so a plan made this way cannot overflow.  A requested number of ranges gets cuts at the equal shares of the
// windows instead, moved where needed so that every range has a bin.
static int plan(const uint64_t *windows, int64_t budget, int32_t partitions, int32_t *cuts, int32_t *nranges, char *errbuf, size_t errlen)
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
            { char lead[KC_BIN_BASES + 1];
              for (int j = 0; j < KC_BIN_BASES; j++) lead[j] = "acgt"[(b >> (2 * (KC_BIN_BASES - 1 - j))) & 3];
              lead[KC_BIN_BASES] = 0;
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

extern "C" int smg_count_plan(const uint64_t *windows, int64_t budget, int32_t partitions, int32_t *cuts, int32_t *nranges, char *errbuf,
                              size_t errlen)
{ GUARD(plan(windows, budget, partitions, cuts, nranges, errbuf, errlen)) }

// The cuts where `plan` refuses a bin (host only): the same greedy rule over one ascending sequence of units, a bin that is
// not split or one of the 4096 sub-bins of a bin that is.  What is left to refuse is a single sub-bin above the budget.
static void lead_bases(char *out, unsigned v, int bases)
{ for (int j = 0; j < bases; j++) out[j] = "acgt"[(v >> (2 * (bases - 1 - j))) & 3];
  out[bases] = 0;
}

static int plan_fine(const uint64_t *windows, const int32_t *split, int32_t nsplit, const uint64_t *sub, int64_t budget, int32_t *cuts,
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
            { char lead[KC_BIN_BASES + 1], lead2[2 * KC_BIN_BASES + 1];
              lead_bases(lead, (unsigned) b, KC_BIN_BASES);
              lead_bases(lead2, ((unsigned) b << SMG_COUNT_BIN_BITS) | (unsigned) j, 2 * KC_BIN_BASES);
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

extern "C" int smg_count_plan_fine(const uint64_t *windows, const int32_t *split, int32_t nsplit, const uint64_t *sub, int64_t budget,
                                   int32_t *cuts, int64_t cuts_cap, int32_t *nranges, char *errbuf, size_t errlen)
{ GUARD(plan_fine(windows, split, nsplit, sub, budget, cuts, cuts_cap, nranges, errbuf, errlen)) }

static int parse_path(const char *path, uint8_t **seq, int64_t *n, char *errbuf, size_t errlen)
{ if (!path || !seq || !n) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  GrowSink sink;
  int rc;
  try { rc = parse_fd(fd, path, sink, nullptr, errbuf, errlen); }
  catch (...) { close(fd); throw; }
  close(fd);
  if (rc) return rc;
  if (!sink.p) sink.p = (uint8_t *) malloc(1);
  *seq = sink.p; *n = (int64_t) sink.len;
  sink.p = nullptr;
  return 0;
}

extern "C" int smg_count_parse(const char *path, uint8_t **seq, int64_t *n, char *errbuf, size_t errlen)
{ GUARD(parse_path(path, seq, n, errbuf, errlen)) }

extern "C" void smg_count_free(void *p) { free(p); }

extern "C" const char *smg_count_version(void) { return "smudgeplot_amd 0.5 (k-mer counter, gfx950)"; }
