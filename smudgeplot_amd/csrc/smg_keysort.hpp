// smg_keysort.hpp -- what the k-mer counter (smg_count.hip) and table conditioning (smg_hetmers.hip) share: a device
// buffer that frees itself, the stable sort of W-word k-mers as a permutation, and the scan that turns flags into
// positions.  No state of its own; every function returns the HIP error and the caller gives it its own code and message.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <rocprim/rocprim.hpp>

#include "smg_device.hpp"

#define KS_TPB 256
#define KS_TRY(call) do { const hipError_t _e = (call); if (_e != hipSuccess) return _e; } while (0)

struct Dev                                                     // a device allocation that frees itself
{ void *p = nullptr;
  ~Dev() { if (p) (void) hipFree(p); }
  void reset() { if (p) (void) hipFree(p); p = nullptr; }
  void take(Dev &o) { reset(); p = o.p; o.p = nullptr; }
  void *release() { void *q = p; p = nullptr; return q; }     // the caller owns the allocation from here on
  template <class T> T *as() const { return (T *) p; }
};

static inline hipError_t dev_alloc(Dev &d, size_t bytes)
{ d.reset();
  const hipError_t e = hipMalloc(&d.p, bytes ? bytes : 16);
  if (e != hipSuccess) d.p = nullptr;
  return e;
}

// the caller's grow-only rocPRIM scratch: at least `bytes` behind *tmp afterwards
static inline hipError_t ks_scratch(void **tmp, int64_t *cap, size_t bytes)
{ if (*tmp && (int64_t) bytes <= *cap) return hipSuccess;
  if (*tmp) (void) hipFree(*tmp);
  *tmp = nullptr; *cap = 0;
  const hipError_t e = hipMalloc(tmp, bytes + 256);
  if (e != hipSuccess) { *tmp = nullptr; return e; }
  *cap = (int64_t) bytes + 256;
  return hipSuccess;
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
static inline hipError_t sort_permutation(const u64 *keys, int W, int64_t n, hipStream_t stream, void **tmp, int64_t *tmp_cap, Dev &perm)
{ if (n < 1 || n >= 0xFFFFFFF0ll) return hipErrorInvalidValue;              // (uint32 permutation: the callers say so first)
  const unsigned nblk = (unsigned) ((n + KS_TPB - 1) / KS_TPB);
  Dev w1, w2, p1, p2;
  KS_TRY(dev_alloc(w1, sizeof(u64) * (size_t) n)); KS_TRY(dev_alloc(w2, sizeof(u64) * (size_t) n));
  KS_TRY(dev_alloc(p1, sizeof(uint32_t) * (size_t) n)); KS_TRY(dev_alloc(p2, sizeof(uint32_t) * (size_t) n));
  rocprim::double_buffer<uint32_t> pb(p1.as<uint32_t>(), p2.as<uint32_t>());
  hipLaunchKernelGGL(ks_iota, dim3(nblk), dim3(KS_TPB), 0, stream, pb.current(), n);
  for (int w = W - 1; w >= 0; w--)
    { rocprim::double_buffer<u64> word(w1.as<u64>(), w2.as<u64>());
      hipLaunchKernelGGL(ks_gather_word, dim3(nblk), dim3(KS_TPB), 0, stream, keys, pb.current(), W, w, n, word.current());
      size_t bytes = 0;
      KS_TRY(rocprim::radix_sort_pairs(nullptr, bytes, word, pb, (size_t) n, 0u, 64u, stream));
      KS_TRY(ks_scratch(tmp, tmp_cap, bytes));
      KS_TRY(rocprim::radix_sort_pairs(*tmp, bytes, word, pb, (size_t) n, 0u, 64u, stream));
    }
  KS_TRY(hipGetLastError());
  KS_TRY(hipStreamSynchronize(stream));
  perm.take(pb.current() == p1.as<uint32_t>() ? p1 : p2);
  return hipSuccess;
}

// pos[] = exclusive scan of flag[0 .. n), n > 0; *total = the number of set flags (one wait for the stream)
static inline hipError_t scan_flags(uint32_t *flag, uint32_t *pos, int64_t n, hipStream_t stream, void **tmp, int64_t *tmp_cap, int64_t *total)
{ size_t bytes = 0;
  KS_TRY(rocprim::exclusive_scan(nullptr, bytes, flag, pos, 0u, (size_t) n, rocprim::plus<uint32_t>(), stream));
  KS_TRY(ks_scratch(tmp, tmp_cap, bytes));
  KS_TRY(rocprim::exclusive_scan(*tmp, bytes, flag, pos, 0u, (size_t) n, rocprim::plus<uint32_t>(), stream));
  uint32_t last[2] = { 0, 0 };
  KS_TRY(hipMemcpyAsync(&last[0], flag + n - 1, 4, hipMemcpyDeviceToHost, stream));
  KS_TRY(hipMemcpyAsync(&last[1], pos + n - 1, 4, hipMemcpyDeviceToHost, stream));
  KS_TRY(hipStreamSynchronize(stream));
  *total = (int64_t) last[0] + last[1];
  return hipSuccess;
}

#undef KS_TRY
