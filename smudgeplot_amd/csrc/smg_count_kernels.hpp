// smg_count_kernels.hpp -- the device code of the k-mer counter (smg_count.hip holds the map of the whole counter).

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smg_count.h"
#include "smg_device.hpp"

#define KC_TPB   256
#define KC_TILE  4096                    // positions per workgroup: 16 bytes per thread
#define KC_HALO  128                     // >= SMG_MAX_KMER - 1, a multiple of 16
#define KC_CHUNKS ((KC_TILE + KC_HALO) / 16)
#define KC_HBINS 8192                    // counts below this go through per-workgroup LDS bins

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

// The 16 sequence bytes from seq[g] on; bytes at n and beyond read as 0, which is no base (past the end nothing is valid).
// One 16-byte load where all of them are there, byte by byte at the end of the buffer.
SMG_DEV uint4 kc_load16(const uint8_t *__restrict__ seq, int64_t g, int64_t n)
{ uint4 v = make_uint4(0, 0, 0, 0);
  if (g + 16 <= n) v = *reinterpret_cast<const uint4 *>(seq + g);
  else if (g < n)
    { unsigned d[4] = { 0, 0, 0, 0 };
      for (int b = 0; b < 16 && g + b < n; b++) d[b >> 2] |= (unsigned) seq[g + b] << (8 * (b & 3));
      v = make_uint4(d[0], d[1], d[2], d[3]);
    }
  return v;
}

template <int W> SMG_DEV bool kc_all_ones(const Key<W> &x)
{ bool e = true;
#pragma unroll
  for (int w = 0; w < W; w++) e &= (x.w[w] == ~0ull);
  return e;
}

// The leading BITS bits (12: the bin; 24, twelve bases: bin and sub-bin, kc_bin<24> >> 12 is kc_bin<12>) of the canonical
// k-mer of the window at position p of the LDS code stream: top(min(x, rc x)) = min(top x, top rc x), and top rc x is the
// complement of the window's last bases in reverse order, so two short reads of the stream give the bin and the k-mer
// itself is never built.  k >= 13, so both reads stay inside the window; at k = 13 the first and the last twelve bases
// overlap in all but one base.
template <int BITS> SMG_DEV unsigned kc_bin(const u64 *s_code, int p, int k)
{ const unsigned f = (unsigned) (kc_take64(s_code, 2 * p) >> (64 - BITS));
  const u64 l = kc_take64(s_code, 2 * (p + k - BITS / 2)) & (~0ull << (64 - BITS));
  const unsigned r = (unsigned) rev2_comp_word(l) & ((1u << BITS) - 1u);
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
// bits of its canonical k-mer (kc_bin<BITS>) lie in [lo, hi): the predicate is complete BEFORE the ballot, so a rejected
// window never builds, reverse-complements or compares its k-mer.  The canonical k-mers go out in position order behind
// ONE atomic per workgroup (64 ballot counts, scanned by the first wavefront): 8 W bytes out per accepted window.
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
        { const unsigned b = kc_bin<BITS>(s_code, p, k);       // (garbage where ok is false: ANDed away)
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
    { const uint4 v = kc_load16(seq, tile0 + 16 * (int64_t) c, n);
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
    { const uint4 v = kc_load16(seq, 64 * i + 16 * c, n);
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

// Windows per bin: LDS bins, flushed once per workgroup (grid-stride over tiles).  SUB = false: by the leading 12 bits of
// the canonical k-mer (`bin` is not read).  SUB = true: restricted to ONE bin, the windows whose leading 12 bits are `bin`
// by their next 12 bits; launched once per bin that is above one merge, which is rare.
template <bool SUB> __global__ void __launch_bounds__(KC_TPB)
kc_bins(const u64 *__restrict__ code, const u64 *__restrict__ val, int64_t npos, int k, unsigned bin, unsigned long long *__restrict__ bins)
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
          if (kc_window(s_val, p, k))
            { if constexpr (SUB)
                { const unsigned f = kc_bin<SMG_COUNT_FINE_BITS>(s_code, p, k);
                  if ((f >> SMG_COUNT_BIN_BITS) == bin) atomicAdd(&h[f & (SMG_COUNT_BINS - 1u)], 1u);
                }
              else atomicAdd(&h[kc_bin<SMG_COUNT_BIN_BITS>(s_code, p, k)], 1u);
            }
        }
    }
  __syncthreads();
  for (int b = t; b < SMG_COUNT_BINS; b += KC_TPB)
    if (h[b]) atomicAdd(&bins[b], (unsigned long long) h[b]);
}

// kc_extract with its front half replaced by loads of the two streams from the store: the windows that start in
// [p0, p1) and whose leading BITS bits lie in [lo, hi).  The grid starts at the tile that holds p0; 0.375 bytes in per
// position.  BITS = 12 for a range of whole bins, 24 for a range with an end inside a split bin.  A template argument and
// not a run-time switch: a range of whole 12-bit bins keeps the pass it had, which is bound by what it does per position
// (profiles/count_partitioned.md).
template <int W, int BITS> __global__ void __launch_bounds__(KC_TPB)
kc_extract_store(const u64 *__restrict__ code, const u64 *__restrict__ val, int64_t npos, int64_t p0, int64_t p1, int k,
                 unsigned lo, unsigned hi, u64 *__restrict__ out, unsigned long long limit, unsigned long long *__restrict__ nout)
{ __shared__ u64 s_code[KC_CHUNKS / 2 + 2];
  __shared__ u64 s_val[KC_CHUNKS / 4 + 2];
  __shared__ unsigned s_cnt[64];
  __shared__ unsigned long long s_base;
  const int64_t tile0 = (p0 / KC_TILE + blockIdx.x) * KC_TILE;
  kc_load_tile(code, val, npos, tile0, s_code, s_val);
  __syncthreads();
  kc_emit<W, BITS>(s_code, s_val, s_cnt, &s_base, tile0, p0, p1, k, lo, hi, out, limit, nout);
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
