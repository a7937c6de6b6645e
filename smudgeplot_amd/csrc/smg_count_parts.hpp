// smg_count_parts.hpp -- the parts of the k-mer counter's device driver, each owning its buffers and their growth: Run
// (what they share), Batch, Distinct, Store and the output Table (smg_count.hip holds the map of the whole counter and
// the Counter that runs them).

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <rocprim/rocprim.hpp>

#include <vector>

#include "smg_count.h"
#include "smg_device.hpp"
#include "smg_keysort.hpp"
#include "smg_count_kernels.hpp"
#include "smg_count_err.hpp"
#include "smg_count_plan.hpp"

static_assert(CP_TILE == KC_TILE, "the store is sized in tiles of the kernels that read it");

// the one check of a HIP call in the counter (x: the Run of the part that checks, or the Errors of a call outside a run)
#define DCHK(call) do { const hipError_t _e = (call); if (_e != hipSuccess) return x.hip_error(_e, #call); } while (0)
#define RCHK(call) do { const int _rc = (call); if (_rc) return _rc; } while (0)

// one launch of KC_TPB threads per workgroup on the run's stream; LAUNCH_W: of the instantiation for the run's word count
#define LAUNCH(kern, grid, ...) hipLaunchKernelGGL(kern, dim3(grid), dim3(KC_TPB), 0, x.stream, __VA_ARGS__)
#define LAUNCH_W(kern, grid, ...) with_words<4>(x.W, [&](auto w) { LAUNCH(kern<w()>, grid, __VA_ARGS__); })

static unsigned nblk(int64_t n) { return (unsigned) ((n + KC_TPB - 1) / KC_TPB); }
static unsigned ngrid(int64_t ntiles) { return (unsigned) (ntiles < 2048 ? ntiles : 2048); }      // grid-stride kernels

// where the errors of a call go, and the one code and message of a HIP error
struct Errors
{ char *errbuf = nullptr; size_t errlen = 0;
  int hip_error(hipError_t e, const char *call) const
  { return fail(errbuf, errlen, e == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV, "HIP error: %s (%s)", hipGetErrorString(e), call); }
};

// there is a device, and `device` names one
static int check_device(int device, char *errbuf, size_t errlen)
{ int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(errbuf, errlen, SMG_ENODEV, "no HIP device: the k-mer counter has no CPU fallback%s", "");
  if (device < 0 || device >= ndev) return fail(errbuf, errlen, SMG_EINVAL, "device %d of %d", device, ndev);
  return 0;
}

// pinned host memory that frees itself: what DevBuf (smg_keysort.hpp) is for device memory
template <class T> struct Pinned
{ T *p = nullptr;
  Pinned() = default;
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  Pinned(Pinned &&o) : p(o.p) { o.p = nullptr; }
  ~Pinned() { if (p) (void) hipHostFree(p); }
  hipError_t alloc(size_t bytes) { return hipHostMalloc((void **) &p, bytes, hipHostMallocDefault); }
  operator T *() const { return p; }
};

// What the parts of a run share: k, where errors go, the stream with its two timing events, rocPRIM's grow-only scratch,
// the statistics.
struct Run : Errors
{ int k = 0, W = 1, t = 1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  Dev tmp;
  smg_count_stats st;
  smg_count_parts pt;

  Run() { memset(&st, 0, sizeof(st)); memset(&pt, 0, sizeof(pt)); }
  ~Run()
  { if (ev0) (void) hipEventDestroy(ev0);
    if (ev1) (void) hipEventDestroy(ev1);
    if (stream) (void) hipStreamDestroy(stream);
  }

  int alloc(Dev &d, size_t bytes) const
  { const hipError_t e = d.alloc(bytes);
    if (e != hipSuccess)
      return fail(errbuf, errlen, e == hipErrorOutOfMemory ? SMG_ENOMEM : SMG_ENODEV,
                  "cannot allocate %.3f GB of device memory: %s", (double) bytes * 1e-9, hipGetErrorString(e));
    return 0;
  }

  int free_bytes(size_t *out) const
  { const Run &x = *this;
    size_t free_b = 0, total_b = 0;
    DCHK(hipMemGetInfo(&free_b, &total_b));
    *out = free_b;
    return 0;
  }

  void tic() { (void) hipEventRecord(ev0, stream); }
  int toc(double *acc)
  { const Run &x = *this;
    float ms = 0;
    DCHK(hipEventRecord(ev1, stream));
    DCHK(hipEventSynchronize(ev1));
    DCHK(hipEventElapsedTime(&ms, ev0, ev1));
    *acc += ms;
    return 0;
  }

  // The one way a pair of device buffers grows: allocate the new sizes, copy what is in use, swap.  (The sizes come from
  // grown_cap, smg_count_plan.hpp.)
  int regrow(Dev &a, size_t used_a, size_t bytes_a, Dev &b, size_t used_b, size_t bytes_b) const
  { const Run &x = *this;
    Dev a2, b2;
    RCHK(alloc(a2, bytes_a)); RCHK(alloc(b2, bytes_b));
    if (used_a) DCHK(hipMemcpyAsync(a2.p, a.p, used_a, hipMemcpyDeviceToDevice, stream));
    if (used_b) DCHK(hipMemcpyAsync(b2.p, b.p, used_b, hipMemcpyDeviceToDevice, stream));
    DCHK(hipStreamSynchronize(stream));
    a.take(a2); b.take(b2);
    return 0;
  }
};

// The batch: sequence bytes as they come from the files, and the key buffers their windows are sorted in.
struct Batch
{ Run &x;
  int64_t cap = 0;                                             // bytes of sequence a batch holds
  int64_t fill = 0;                                            // bytes in the batch buffer
  int last_file = -1;                                          // the file whose stream ends at `fill`
  std::vector<std::vector<uint8_t>> tails;                     // per file: the last k-1 bytes handed over
  DevBuf<uint8_t> seq;
  DevBuf<u64> ka, kb;                                          // the keys of a batch and the other half of their sort
  DevBuf<uint32_t> flag, pos, start;
  DevBuf<unsigned long long> ctr;                              // the number of keys in ka, counted by the extract kernels
  explicit Batch(Run &r) : x(r) {}

  int init(int64_t c, int nfiles)
  { const size_t W = (size_t) x.W;
    cap = c;
    tails.assign((size_t) (nfiles > 0 ? nfiles : 1), std::vector<uint8_t>());
    RCHK(x.alloc(seq, (size_t) cap + 16));
    RCHK(x.alloc(ka, sizeof(u64) * (size_t) cap * W));
    RCHK(x.alloc(kb, sizeof(u64) * (size_t) cap * W));
    RCHK(x.alloc(flag, sizeof(uint32_t) * (size_t) cap));
    RCHK(x.alloc(pos, sizeof(uint32_t) * (size_t) cap));
    RCHK(x.alloc(start, sizeof(uint32_t) * ((size_t) cap + 1)));
    return x.alloc(ctr, 16);
  }
  void drop_keys() { ka.reset(); kb.reset(); start.reset(); flag.reset(); pos.reset(); }

  // the bytes in the buffer, which counts as empty from here on
  int64_t take() { const int64_t n = fill; fill = 0; last_file = -1; return n; }

  // bytes of one file's stream, in order; pieces go into the batch buffer, flush() empties it when it is full
  template <class Flush> int add(const uint8_t *p, int64_t n, int file, Flush &&flush)
  { const int k = x.k;
    std::vector<uint8_t> &tail = tails[(size_t) file];
    while (n > 0)
      { const bool joined = last_file == file && fill > 0;
        const int64_t lead = joined ? 0 : 1 + (int64_t) tail.size();
        if (cap - fill < lead + 1) { RCHK(flush()); continue; }
        if (!joined)
          { uint8_t head[SMG_MAX_KMER + 1];
            head[0] = SMG_COUNT_SEPARATOR;
            if (!tail.empty()) memcpy(head + 1, tail.data(), tail.size());
            DCHK(hipMemcpy(seq + fill, head, (size_t) lead, hipMemcpyHostToDevice));
            fill += lead;
          }
        const int64_t m = n < cap - fill ? n : cap - fill;
        DCHK(hipMemcpy(seq + fill, p, (size_t) m, hipMemcpyHostToDevice));
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

  // the n bytes of the buffer -> the canonical k-mers of their windows in ka
  int extract(int64_t n, int64_t *nwin)
  { x.tic();
    DCHK(hipMemsetAsync(ctr.p, 0, 16, x.stream));
    const unsigned ntiles = (unsigned) ((n + KC_TILE - 1) / KC_TILE);
    LAUNCH_W(kc_extract, ntiles, seq, n, x.k, ka, ctr);
    DCHK(hipGetLastError());
    unsigned long long got = 0;
    DCHK(hipMemcpyAsync(&got, ctr.p, 8, hipMemcpyDeviceToHost, x.stream));
    RCHK(x.toc(&x.st.ms_extract));
    if ((int64_t) got > cap) return fail(x.errbuf, x.errlen, SMG_ENODEV, "internal error: %llu windows from %lld bytes", got, (long long) n);
    *nwin = (int64_t) got;
    return 0;
  }
};

// The running distinct list: (k-mer, uint32 count), sorted, duplicate free; a batch of keys is counted and merged into it.
struct Distinct
{ Run &x;
  int64_t max_entries = 0;                                     // test hook: refuse a merge of more (0: the device's own limit)
  DevBuf<u64> dk;
  DevBuf<uint32_t> dc;
  int64_t nd = 0;
  explicit Distinct(Run &r) : x(r) {}
  void clear() { dk.reset(); dc.reset(); nd = 0; }

  // sorts n entries (W-word k-mers, optional uint32 values) that lie in (a, va); (b, vb) are buffers of the same size.
  // The result is in (*ko, *vo), one of the two.
  int sort_entries(u64 *a, u64 *b, uint32_t *va, uint32_t *vb, int64_t n, u64 **ko, uint32_t **vo)
  { const int W = x.W;
    if (W == 1)
      { rocprim::double_buffer<u64> dk2(a, b);
        rocprim::double_buffer<uint32_t> dv2(va, vb);
        // All 64 bits, not 64-2k .. 64: the pad bits are zero, so the order is the same, and a partial bit range is not
        // safe on rocPRIM's merge-sort path (sort_permutation, smg_keysort.hpp).
        const unsigned b0 = 0u;
        DCHK(with_scratch(x.tmp, [&](void *t, size_t &bytes)
          { return va ? rocprim::radix_sort_pairs(t, bytes, dk2, dv2, (size_t) n, b0, 64u, x.stream)
                      : rocprim::radix_sort_keys(t, bytes, dk2, (size_t) n, b0, 64u, x.stream); }));
        *ko = dk2.current();
        if (vo) *vo = va ? dv2.current() : nullptr;
        return 0;
      }
    // W > 1: the sorted order as a permutation (smg_keysort.hpp), then one gather
    Dev perm;
    DCHK(sort_permutation(a, W, n, x.stream, x.tmp, perm));
    LAUNCH_W(kc_gather_entries, nblk(n), a, va, perm.as<uint32_t>(), n, b, vb);
    DCHK(hipStreamSynchronize(x.stream));                      // (the permutation is freed on return)
    *ko = b;
    if (vo) *vo = va ? vb : nullptr;
    return 0;
  }

  // nwin canonical k-mers in the batch's ka -> sorted -> (k-mer, count) runs -> merged into the list
  int count_keys(Batch &b, int64_t nwin)
  { x.st.windows += nwin;
    u64 *sorted = nullptr;
    x.tic();
    RCHK(sort_entries(b.ka, b.kb, nullptr, nullptr, nwin, &sorted, nullptr));
    RCHK(x.toc(&x.st.ms_sort));
    u64 *uk = sorted == b.ka ? b.kb : b.ka;
    int64_t nruns = 0;
    x.tic();
    LAUNCH_W(kc_flag_heads, nblk(nwin), sorted, nwin, b.flag);
    DCHK(scan_flags(b.flag, b.pos, nwin, x.stream, x.tmp, &nruns));
    LAUNCH_W(kc_runs, nblk(nwin), sorted, b.flag, b.pos, nwin, uk, b.start);
    uint32_t *rc = b.flag;                                     // (the flags are spent: the run counts take their place)
    LAUNCH(kc_run_counts, nblk(nruns), b.start, nruns, rc);
    DCHK(hipGetLastError());
    RCHK(merge(uk, rc, nruns));
    return x.toc(&x.st.ms_reduce);
  }

  int merge(const u64 *uk, const uint32_t *rc, int64_t nr)
  { const int W = x.W;
    hipStream_t stream = x.stream;
    if (max_entries && nd + nr > max_entries)
      return fail(x.errbuf, x.errlen, SMG_ENOMEM, "the distinct k-mers of this data set do not fit the device: merging %lld entries, "
                  "one merge holds %lld (max_entries)", (long long) (nd + nr), (long long) max_entries);
    if (nd == 0)
      { Dev nk, nc;
        RCHK(x.alloc(nk, sizeof(u64) * (size_t) nr * W)); RCHK(x.alloc(nc, sizeof(uint32_t) * (size_t) nr));
        DCHK(hipMemcpyAsync(nk.p, uk, sizeof(u64) * (size_t) nr * W, hipMemcpyDeviceToDevice, stream));
        DCHK(hipMemcpyAsync(nc.p, rc, sizeof(uint32_t) * (size_t) nr, hipMemcpyDeviceToDevice, stream));
        DCHK(hipStreamSynchronize(stream));
        dk.take(nk); dc.take(nc); nd = nr;
        return 0;
      }
    const int64_t m = nd + nr;
    if (m >= 0xFFFFFFF0ll)
      return fail(x.errbuf, x.errlen, SMG_ENOMEM, "more than 2^32 - 16 entries in one merge (%lld): this many distinct k-mers need more than one "
                  "key range", (long long) m);
    const size_t want = (size_t) m * merge_price(W) + CP_RESERVE;
    size_t free_b = 0;
    RCHK(x.free_bytes(&free_b));
    if (want > free_b)
      return fail(x.errbuf, x.errlen, SMG_ENOMEM, "the distinct k-mers of this data set do not fit the device: merging %lld entries needs "
                  "%.3f GB, %.3f GB are free", (long long) m, (double) want * 1e-9, (double) free_b * 1e-9);
    DevBuf<u64> ck; DevBuf<uint32_t> cc;                       // the concatenation,
    DevBuf<u64> ak; DevBuf<uint32_t> ac, mf, mp;               // the other half of its sort, head flags and positions,
    DevBuf<u64> nk; DevBuf<uint32_t> nc;                       // the merged list (declared, hence freed, in the order they always were)
    RCHK(x.alloc(ck, sizeof(u64) * (size_t) m * W)); RCHK(x.alloc(cc, sizeof(uint32_t) * (size_t) m));
    RCHK(x.alloc(ak, sizeof(u64) * (size_t) m * W)); RCHK(x.alloc(ac, sizeof(uint32_t) * (size_t) m));
    DCHK(hipMemcpyAsync(ck.p, dk.p, sizeof(u64) * (size_t) nd * W, hipMemcpyDeviceToDevice, stream));
    DCHK(hipMemcpyAsync(ck + (size_t) nd * W, uk, sizeof(u64) * (size_t) nr * W, hipMemcpyDeviceToDevice, stream));
    DCHK(hipMemcpyAsync(cc.p, dc.p, sizeof(uint32_t) * (size_t) nd, hipMemcpyDeviceToDevice, stream));
    DCHK(hipMemcpyAsync(cc + nd, rc, sizeof(uint32_t) * (size_t) nr, hipMemcpyDeviceToDevice, stream));
    DCHK(hipStreamSynchronize(stream));
    clear();
    u64 *sk = nullptr; uint32_t *sc = nullptr;
    RCHK(sort_entries(ck, ak, cc, ac, m, &sk, &sc));
    RCHK(x.alloc(mf, sizeof(uint32_t) * (size_t) m)); RCHK(x.alloc(mp, sizeof(uint32_t) * (size_t) m));
    LAUNCH_W(kc_flag_heads, nblk(m), sk, m, mf);
    int64_t nn = 0;
    DCHK(scan_flags(mf, mp, m, stream, x.tmp, &nn));
    RCHK(x.alloc(nk, sizeof(u64) * (size_t) nn * W)); RCHK(x.alloc(nc, sizeof(uint32_t) * (size_t) nn));
    LAUNCH_W(kc_merge_write, nblk(m), sk, sc, mf, mp, m, nk, nc);
    DCHK(hipGetLastError());
    DCHK(hipStreamSynchronize(stream));
    dk.take(nk); dc.take(nc); nd = nn;
    return 0;
  }
};

// The packed input of a partitioned run, resident on the device: n positions in use (a multiple of 64) of cap.
struct Store
{ Run &x;
  DevBuf<u64> code, val;
  int64_t cap = 0, n = 0;
  bool open_ended = false;
  explicit Store(Run &r) : x(r) {}
  void drop() { code.reset(); val.reset(); }

  int init(int64_t c)
  { cap = c; x.pt.store_bytes = cap / 8 * 3;
    RCHK(x.alloc(code, (size_t) cap / 4));
    return x.alloc(val, (size_t) cap / 8);
  }

  // room for `more` positions behind n (the size bound of the input does not count the separators and re-prefixed
  // tails that batches and interleaved files add, so the store may have to grow)
  // open_ended (a run that reads a stream, whose store began at a size nobody could derive from the input): a growth that
  // does not fit is refused here with its figures, the old store and the new one being there together while it is copied
  int need(int64_t more)
  { if (n + more <= cap) return 0;
    const int64_t nc = grown_cap(cap, n + more, KC_TILE);
    if (open_ended)
      { size_t free_b = 0;
        RCHK(x.free_bytes(&free_b));
        const size_t want = (size_t) nc / 8 * 3 + CP_RESERVE;
        if (want > free_b)
          return fail(x.errbuf, x.errlen, SMG_ENOMEM, "the packed input does not fit the device: %lld positions are packed, a store of %lld "
                      "positions next to them needs %.3f GB, %.3f GB of device memory are free", (long long) n, (long long) nc,
                      (double) want * 1e-9, (double) free_b * 1e-9);
      }
    RCHK(x.regrow(code, (size_t) n / 4, (size_t) nc / 4, val, (size_t) n / 8, (size_t) nc / 8));
    cap = nc; x.pt.store_bytes = nc / 8 * 3;
    return 0;
  }

  // the batch buffer -> 3 bits per position behind the store
  int pack(Batch &b)
  { const int64_t len = b.take();
    if (len < x.k) return 0;
    const int64_t npad = (len + 63) / 64 * 64;
    RCHK(need(npad));
    x.tic();
    LAUNCH(kc_pack, nblk(npad / 64), b.seq, len, npad, n, code, val);
    DCHK(hipGetLastError());
    RCHK(x.toc(&x.pt.ms_pack));
    n += npad;
    return 0;
  }

  // out[4096] = the windows of the store per bin of their leading 12 bits, or (SUB) those of `bin` by their next 12 bits
  template <bool SUB> int histogram(unsigned bin, uint64_t *out)
  { const size_t bytes = sizeof(uint64_t) * SMG_COUNT_BINS;
    DevBuf<unsigned long long> d;
    RCHK(x.alloc(d, bytes));
    DCHK(hipMemsetAsync(d.p, 0, bytes, x.stream));
    if (n > 0)
      { LAUNCH(kc_bins<SUB>, ngrid((n + KC_TILE - 1) / KC_TILE), code, val, n, x.k, bin, d);
        DCHK(hipGetLastError());
      }
    DCHK(hipMemcpyAsync(out, d.p, bytes, hipMemcpyDeviceToHost, x.stream));
    DCHK(hipStreamSynchronize(x.stream));
    return 0;
  }
};

// The output table: the kept entries of every range, appended in ascending order.  `any` says whether anything has been
// appended yet, an empty range included; n entries of cap are in use.
struct Table
{ Run &x;
  bool any = false;
  int64_t n = 0, cap = 0;
  explicit Table(Run &r) : x(r) {}
  virtual ~Table() {}
  // ok, oc: the k-mers and uint16 counts of a range, whole device allocations (or empty ones where kept = 0)
  virtual int append(Dev &ok, Dev &oc, int64_t kept) = 0;
  // the table goes to the caller, who frees it; never NULL, also where it is empty
  virtual int release(uint64_t **keys, uint16_t **counts, int64_t *nels) = 0;
};

struct HostTable : Table                                        // malloc'ed arrays
{ uint64_t *hk = nullptr; uint16_t *hc = nullptr;
  using Table::Table;
  ~HostTable() override { free(hk); free(hc); }
  int append(Dev &ok, Dev &oc, int64_t kept) override
  { const size_t W = (size_t) x.W;
    if (n + kept > cap || !any)
      { const int64_t nc = grown_cap(cap, n + kept, 1);
        uint64_t *k2 = (uint64_t *) realloc(hk, sizeof(uint64_t) * (size_t) nc * W);
        if (k2) hk = k2;
        uint16_t *c2 = (uint16_t *) realloc(hc, sizeof(uint16_t) * (size_t) nc);
        if (c2) hc = c2;
        if (!k2 || !c2) return fail(x.errbuf, x.errlen, SMG_ENOMEM, "out of host memory for %lld k-mers", (long long) nc);
        cap = nc;
      }
    any = true;
    if (kept > 0)
      { DCHK(hipMemcpy(hk + (size_t) n * W, ok.p, sizeof(uint64_t) * (size_t) kept * W, hipMemcpyDeviceToHost));
        DCHK(hipMemcpy(hc + n, oc.p, sizeof(uint16_t) * (size_t) kept, hipMemcpyDeviceToHost));
      }
    n += kept;
    return 0;
  }
  int release(uint64_t **keys, uint16_t **counts, int64_t *nels) override
  { *keys = hk; *counts = hc; *nels = n;
    hk = nullptr; hc = nullptr;
    return 0;
  }
};

// Two whole device allocations.  The first range's buffers become the table as they are; from then on it grows by half,
// like the store, with a device-to-device copy.
struct DeviceTable : Table
{ DevBuf<u64> tk;
  DevBuf<uint16_t> tc;
  using Table::Table;
  int append(Dev &ok, Dev &oc, int64_t kept) override
  { const size_t W = (size_t) x.W;
    if (!any && ok.p && oc.p) { tk.take(ok); tc.take(oc); n = cap = kept; any = true; return 0; }
    if (n + kept > cap || !any)
      { const int64_t nc = grown_cap(cap, n + kept, 1);
        const size_t want = (sizeof(u64) * W + sizeof(uint16_t)) * (size_t) nc + CP_RESERVE;
        size_t free_b = 0;
        RCHK(x.free_bytes(&free_b));
        if (want > free_b)
          return fail(x.errbuf, x.errlen, SMG_ENOMEM, "the counted table does not fit the device next to the input: room for %lld entries needs "
                      "%.3f GB, %.3f GB are free (count to a table on disk instead: the entries that return host arrays)", (long long) nc,
                      (double) want * 1e-9, (double) free_b * 1e-9);
        RCHK(x.regrow(tk, sizeof(u64) * (size_t) n * W, sizeof(u64) * (size_t) nc * W, tc, sizeof(uint16_t) * (size_t) n, sizeof(uint16_t) * (size_t) nc));
        cap = nc;
      }
    any = true;
    if (kept > 0)
      { DCHK(hipMemcpyAsync(tk + (size_t) n * W, ok.p, sizeof(u64) * (size_t) kept * W, hipMemcpyDeviceToDevice, x.stream));
        DCHK(hipMemcpyAsync(tc + n, oc.p, sizeof(uint16_t) * (size_t) kept, hipMemcpyDeviceToDevice, x.stream));
        DCHK(hipStreamSynchronize(x.stream));                  // (ok and oc are freed on return)
      }
    n += kept;
    return 0;
  }
  int release(uint64_t **keys, uint16_t **counts, int64_t *nels) override
  { DCHK(hipStreamSynchronize(x.stream));
    *keys = (uint64_t *) tk.release(); *counts = (uint16_t *) tc.release(); *nels = n;
    return 0;
  }
};
