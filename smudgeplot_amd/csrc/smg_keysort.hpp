// smg_keysort.hpp -- what the k-mer counter (smg_count.hip) and table conditioning (smg_condition.hpp) share: the device
// buffer of both and of the engine, rocPRIM's scratch around a call, the stable sort of W-word k-mers as a permutation, the scan that turns flags into
// positions, and the merge of two sorted lists of k-mers.  No state of its own; every function returns the HIP error and the caller gives it its own code and message.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/rocprim.hpp>

#include "smg_device.hpp"
#include "smg_mergepath.hpp"

#define KS_TPB 256
#define KS_TRY(call) do { const hipError_t _e = (call); if (_e != hipSuccess) return _e; } while (0)

#define KS_SLACK 256                                            // bytes past what rocPRIM asks for (with_scratch)

// A device allocation that frees itself and knows its size.  reserve() is grow-only: an allocation that is large enough
// stays, any other is freed and made anew with exactly the bytes asked for -- the contents are lost, and on failure the
// buffer is empty.  alloc() always allocates anew.
struct Dev
{ void *p = nullptr;
  size_t bytes = 0;
  Dev() = default;
  Dev(const Dev &) = delete;
  Dev &operator=(const Dev &) = delete;
  ~Dev() { reset(); }
  void reset() { if (p) (void) hipFree(p); p = nullptr; bytes = 0; }
  void swap(Dev &o) { void *q = p; p = o.p; o.p = q; const size_t b = bytes; bytes = o.bytes; o.bytes = b; }
  void take(Dev &o) { reset(); swap(o); }
  void *release() { void *q = p; p = nullptr; bytes = 0; return q; }     // the caller owns the allocation from here on
  hipError_t reserve(size_t need)
  { if (p && bytes >= need) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc(&p, need);
    if (e != hipSuccess) p = nullptr; else bytes = need;
    return e;
  }
  hipError_t alloc(size_t need) { reset(); return reserve(need ? need : 16); }
  template <class T> T *as() const { return (T *) p; }
};

template <class T> struct DevBuf : Dev                          // ... that reads as the T * it holds
{ operator T *() const { return (T *) p; }
  T *operator->() const { return (T *) p; }
};

// rocPRIM's two calls -- ask for the scratch size, run with that much -- around the caller's grow-only scratch
template <class F> static inline hipError_t with_scratch(Dev &tmp, F &&run)
{ size_t bytes = 0;
  KS_TRY(run((void *) nullptr, bytes));
  KS_TRY(tmp.reserve(bytes + KS_SLACK));
  return run(tmp.p, bytes);
}

__global__ void __launch_bounds__(KS_TPB) ks_iota(uint32_t *__restrict__ p, int64_t n)
{ const int64_t i = (int64_t) blockIdx.x * KS_TPB + threadIdx.x;
  if (i < n) p[i] = (uint32_t) i;
}

__global__ void __launch_bounds__(KS_TPB)
ks_gather_word(const u64 *__restrict__ keys, const uint32_t *__restrict__ perm, int W, int w, int64_t n, u64 *__restrict__ o)
{ const int64_t i = (int64_t) blockIdx.x * KS_TPB + threadIdx.x;
  if (i < n) o[i] = keys[(size_t) perm[i] * W + w];
}

// perm[i] = the entry of keys[n * W] that is the i-th in sorted order, equal k-mers in input order: stable sorts of
// (word, permutation), least significant word first.  Every sort covers bits 0 .. 64 with rocPRIM's default
// configuration: below its merge-sort limit (2^20 items) rocPRIM merge sorts, and on gfx950 / ROCm 7.2 that path went
// wrong with a partial bit range (garbage, or runs of 1024 keys left unmerged with a begin bit above 0), while the full
// range is exact on every path -- and costs a W-word k-mer nothing, since all 64 bits of a word count.  The four work
// buffers are freed on return, hence the wait for the stream.
static inline hipError_t sort_permutation(const u64 *keys, int W, int64_t n, hipStream_t stream, Dev &tmp, Dev &perm)
{ if (n < 1 || n >= 0xFFFFFFF0ll) return hipErrorInvalidValue;              // (uint32 permutation: the callers say so first)
  const unsigned nblk = (unsigned) ((n + KS_TPB - 1) / KS_TPB);
  Dev w1, w2, p1, p2;
  KS_TRY(w1.alloc(sizeof(u64) * (size_t) n)); KS_TRY(w2.alloc(sizeof(u64) * (size_t) n));
  KS_TRY(p1.alloc(sizeof(uint32_t) * (size_t) n)); KS_TRY(p2.alloc(sizeof(uint32_t) * (size_t) n));
  rocprim::double_buffer<uint32_t> pb(p1.as<uint32_t>(), p2.as<uint32_t>());
  hipLaunchKernelGGL(ks_iota, dim3(nblk), dim3(KS_TPB), 0, stream, pb.current(), n);
  for (int w = W - 1; w >= 0; w--)
    { rocprim::double_buffer<u64> word(w1.as<u64>(), w2.as<u64>());
      hipLaunchKernelGGL(ks_gather_word, dim3(nblk), dim3(KS_TPB), 0, stream, keys, pb.current(), W, w, n, word.current());
      KS_TRY(with_scratch(tmp, [&](void *t, size_t &bytes) { return rocprim::radix_sort_pairs(t, bytes, word, pb, (size_t) n, 0u, 64u, stream); }));
    }
  KS_TRY(hipGetLastError());
  KS_TRY(hipStreamSynchronize(stream));
  perm.take(pb.current() == p1.as<uint32_t>() ? p1 : p2);
  return hipSuccess;
}

// pos[] = exclusive scan of flag[0 .. n), n > 0; *total = the number of set flags (one wait for the stream)
static inline hipError_t scan_flags(uint32_t *flag, uint32_t *pos, int64_t n, hipStream_t stream, Dev &tmp, int64_t *total)
{ KS_TRY(with_scratch(tmp, [&](void *t, size_t &bytes)
    { return rocprim::exclusive_scan(t, bytes, flag, pos, 0u, (size_t) n, rocprim::plus<uint32_t>(), stream); }));
  uint32_t last[2] = { 0, 0 };
  KS_TRY(hipMemcpyAsync(&last[0], flag + n - 1, 4, hipMemcpyDeviceToHost, stream));
  KS_TRY(hipMemcpyAsync(&last[1], pos + n - 1, 4, hipMemcpyDeviceToHost, stream));
  KS_TRY(hipStreamSynchronize(stream));
  *total = (int64_t) last[0] + last[1];
  return hipSuccess;
}

// ---- merge path: two sorted lists of W-word k-mers with no k-mer in common -> one ----------------------------------------
// A is a table (k-mers a[na * W], counts acnt[na]).  B is given unsorted with its order beside it: its j-th k-mer in sorted
// order is b[bperm[j]], and it carries the count of A's entry bsrc[bperm[j]] (B holds reverse complements of entries of A:
// smg_engine_close_canonical) -- or, in the second form ks_merge_bcnt, the count bcnt[bperm[j]] given beside it.
// Output tile t is the outputs [t * T, (t + 1) * T): ks_merge_split finds with one diagonal
// search per tile (mp_split, smg_mergepath.hpp, on the k-mers in device memory) how many of the outputs in front of it come
// from A.  ks_merge stages the tile's two input spans -- T items together -- in LDS, A's span in front of B's, with their
// counts; every thread searches its own diagonal there, merges its T / 256 items into registers, and after a barrier the
// merged tile replaces the spans in LDS and leaves in coalesced stores.
// T per key width: 8 W + 2 bytes of LDS per item, 20 / 36 / 26 / 34 KiB per workgroup for W = 1 .. 4, so that four
// workgroups (16 wavefronts) fit the 160 KiB of a CU at every width, and 8 / 8 / 4 / 4 items per thread in registers.
// (KsMergeTile<W>, ks_merge_tile: smg_mergepath.hpp, where the host check reads them too)
// Where its time is expected to go: B is never written out in sorted order, so its span is staged by one random gather per
// item through bperm (8 W bytes out of a cache line each, and a second gather for the count), and every step of a tile's
// search in ks_merge_split is a dependent gather of the same kind (about log2 T .. log2 nb of them in a row per tile).
static_assert(KS_TPB == MP_TPB, "ks_merge runs with the threads smg_mergepath.hpp cuts its tiles for");

// split[t] = items of A among the first min(t * T, na + nb) outputs, t = 0 .. ntiles
template <int W> __global__ void __launch_bounds__(KS_TPB)
ks_merge_split(const u64 *__restrict__ a, int64_t na, const u64 *__restrict__ b, const uint32_t *__restrict__ bperm, int64_t nb,
               int64_t ntiles, uint32_t *__restrict__ split)
{ const int64_t t = (int64_t) blockIdx.x * KS_TPB + threadIdx.x;
  if (t > ntiles) return;
  int64_t diag = t * KsMergeTile<W>::value;
  if (diag > na + nb) diag = na + nb;
  split[t] = (uint32_t) mp_split(diag, na, nb, [&](int64_t j, int64_t i) { return mp_key_lt<W>(b + (size_t) bperm[j] * W, a + (size_t) i * W); });
}

// (the tile's work, for both forms of B's counts: cnt_of_b(p) is the count that goes with B's item p)
template <int W, class CntOfB> SMG_DEV void
ks_merge_tile_body(const u64 *__restrict__ a, const uint16_t *__restrict__ acnt, int64_t na, const u64 *__restrict__ b,
                   const uint32_t *__restrict__ bperm, int64_t nb, const uint32_t *__restrict__ split,
                   u64 *__restrict__ okeys, uint16_t *__restrict__ ocnt, CntOfB cnt_of_b)
{ constexpr int T = KsMergeTile<W>::value, IPT = T / KS_TPB;
  __shared__ __attribute__((aligned(16))) u64 s_key[T * W];
  __shared__ __attribute__((aligned(16))) uint16_t s_cnt[T];
  const int t = threadIdx.x;
  const int64_t d0 = (int64_t) blockIdx.x * T, d1 = d0 + T < na + nb ? d0 + T : na + nb;
  const int64_t a0 = split[blockIdx.x], a1 = split[blockIdx.x + 1], b0 = d0 - a0, b1 = d1 - a1;
  // mp_split keeps every split within both lists; on sorted lists the splits ascend as well.  Lists that are not sorted can
  // give spans of negative length: such a tile is left unwritten (the whole workgroup leaves), nothing is read out of bounds
  if (a1 < a0 || b1 < b0) return;
  const int ca = (int) (a1 - a0), cb = (int) (b1 - b0), ct = ca + cb;       // ct = d1 - d0 <= T

  for (int x = t; x < ca * W; x += KS_TPB) s_key[x] = a[(size_t) a0 * W + x];
  for (int x = t; x < ca; x += KS_TPB) s_cnt[x] = acnt[a0 + x];
  for (int x = t; x < cb; x += KS_TPB)
    { const uint32_t p = bperm[b0 + x];
      const Key<W> y = load_key<W>(b, p);
#pragma unroll
      for (int w = 0; w < W; w++) s_key[(ca + x) * W + w] = y.w[w];
      s_cnt[ca + x] = cnt_of_b(p);
    }
  __syncthreads();

  const u64 *sa = s_key, *sb = s_key + ca * W;
  const auto b_before_a = [&](int64_t j, int64_t i) { return mp_key_lt<W>(sb + j * W, sa + i * W); };
  const int diag = t * IPT < ct ? t * IPT : ct;
  const int mine = ct - diag < IPT ? ct - diag : IPT;
  const int64_t i0 = mp_split(diag, ca, cb, b_before_a);
  u64 rk[IPT][W];
  uint16_t rc[IPT];
  mp_merge_run<IPT>(i0, diag - i0, ca, cb, mine, b_before_a, [&](int c, bool from_a, int64_t x)
    { const int s = (int) (from_a ? x : ca + x);
#pragma unroll
      for (int w = 0; w < W; w++) rk[c][w] = s_key[s * W + w];
      rc[c] = s_cnt[s];
    });
  __syncthreads();
#pragma unroll
  for (int c = 0; c < IPT; c++)
    if (c < mine)
      {
#pragma unroll
        for (int w = 0; w < W; w++) s_key[(diag + c) * W + w] = rk[c][w];
        s_cnt[diag + c] = rc[c];
      }
  __syncthreads();

  for (int x = t; x < ct * W; x += KS_TPB) okeys[(size_t) d0 * W + x] = s_key[x];
  // (d0 is a multiple of T: the counts of a tile begin on a 4-byte boundary of a hipMalloc'ed array and leave two at a time)
  const uint32_t *c2 = reinterpret_cast<const uint32_t *>(s_cnt);
  uint32_t *o2 = reinterpret_cast<uint32_t *>(ocnt + d0);
  for (int x = t; x < ct / 2; x += KS_TPB) o2[x] = c2[x];
  if (t == 0 && (ct & 1)) ocnt[d0 + ct - 1] = s_cnt[ct - 1];
}

template <int W> __global__ void __launch_bounds__(KS_TPB)
ks_merge(const u64 *__restrict__ a, const uint16_t *__restrict__ acnt, int64_t na, const u64 *__restrict__ b,
         const uint32_t *__restrict__ bperm, const uint32_t *__restrict__ bsrc, int64_t nb, const uint32_t *__restrict__ split,
         u64 *__restrict__ okeys, uint16_t *__restrict__ ocnt)
{ ks_merge_tile_body<W>(a, acnt, na, b, bperm, nb, split, okeys, ocnt, [=](uint32_t p) { return acnt[bsrc[p]]; }); }

// the second form: B's counts are given per item of B (bcnt[p] beside b[p]) -- A is a SLICE of a table while B's sources lie
// anywhere in that table (smg_engine_close_canonical_range)
template <int W> __global__ void __launch_bounds__(KS_TPB)
ks_merge_bcnt(const u64 *__restrict__ a, const uint16_t *__restrict__ acnt, int64_t na, const u64 *__restrict__ b,
              const uint32_t *__restrict__ bperm, const uint16_t *__restrict__ bcnt, int64_t nb, const uint32_t *__restrict__ split,
              u64 *__restrict__ okeys, uint16_t *__restrict__ ocnt)
{ ks_merge_tile_body<W>(a, acnt, na, b, bperm, nb, split, okeys, ocnt, [=](uint32_t p) { return bcnt[p]; }); }

#undef KS_TRY
