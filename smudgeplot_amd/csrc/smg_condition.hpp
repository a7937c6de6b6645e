// smg_condition.hpp -- table conditioning of the hetmers engine on the device: trim and symmetrise a bound table, close a
// canonical one by merge, symmetrise a table that is cut into shards, and hand the table out.  Included by
// smg_hetmers.hip behind route_records (smg_phase.hpp); no state of its own.

#pragma once

// ---- table conditioning on device ----------------------------------------
// The reference shells out to FastK's Logex / Symmex (PloidyPlot.c:1381-1414), which are neither vendored
// nor pinned.  Restated semantics:
//   trim        : keep the entries with count >= ethresh                    (Logex 'A[e-]')
//   symmetrise  : add rc(x) with the count of x for every entry x, sort, keep one copy of a k-mer that
//                 occurs twice (a self-complementary k-mer, or -- only on input that is neither canonical
//                 nor symmetric -- a k-mer whose complement was already present: the original entry wins)
// The sort, the scans and the buffers are those of the k-mer counter (smg_keysort.hpp).

template <int W> __global__ void __launch_bounds__(TPB)
kc_append_rc(const u64 *__restrict__ keys, const uint16_t *__restrict__ cnt, int64_t n, int k,
             u64 *__restrict__ okeys, uint16_t *__restrict__ ocnt)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const Key<W> x = load_key<W>(keys, i);
  const Key<W> r = revcomp<W>(x, k);
#pragma unroll
  for (int w = 0; w < W; w++) { okeys[i * W + w] = x.w[w]; okeys[(n + i) * W + w] = r.w[w]; }
  ocnt[i] = cnt[i]; ocnt[n + i] = cnt[i];
}

// flag[i] = 1 when the i-th entry in sorted order survives (first of its k-mer)
template <int W> __global__ void __launch_bounds__(TPB)
kc_flag_first(const u64 *__restrict__ keys, const uint32_t *__restrict__ perm, int64_t n,
              uint32_t *__restrict__ flag)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  bool first = i == 0;
  if (i > 0) first = !key_eq<W>(load_key<W>(keys, perm[i]), load_key<W>(keys, perm[i - 1]));
  flag[i] = first;
}

__global__ void __launch_bounds__(TPB)
kc_flag_trim(const uint16_t *__restrict__ cnt, int64_t n, unsigned ethresh, uint32_t *__restrict__ flag)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i < n) flag[i] = cnt[i] >= ethresh;
}

// out[pos[i]] = in[perm ? perm[i] : i] for the flagged i
template <int W> __global__ void __launch_bounds__(TPB)
kc_compact(const u64 *__restrict__ keys, const uint16_t *__restrict__ cnt, const uint32_t *__restrict__ perm,
           const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t n,
           u64 *__restrict__ okeys, uint16_t *__restrict__ ocnt)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const int64_t src = perm ? (int64_t) perm[i] : i;
  const int64_t dst = pos[i];
#pragma unroll
  for (int w = 0; w < W; w++) okeys[dst * W + w] = keys[src * W + w];
  ocnt[dst] = cnt[src];
}

// like kc_compact, for a sorted permutation in which a k-mer occurs at most twice (once as an entry, once as a
// complement): the survivor is the first of the two, its count the ENTRY's
template <int W> __global__ void __launch_bounds__(TPB)
kc_compact_pref(const u64 *__restrict__ keys, const uint16_t *__restrict__ cnt, const uint8_t *__restrict__ copy,
                const uint32_t *__restrict__ perm, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                int64_t n, u64 *__restrict__ okeys, uint16_t *__restrict__ ocnt)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const int64_t src = perm[i];
  int64_t csrc = src;
  if (copy[src] && i + 1 < n && !flag[i + 1]) csrc = perm[i + 1];        // (the next one is the same k-mer: the entry)
  const int64_t dst = pos[i];
#pragma unroll
  for (int w = 0; w < W; w++) okeys[dst * W + w] = keys[src * W + w];
  ocnt[dst] = cnt[csrc];
}

// (k, c), n finished entries, leave their buffers and become the engine's own table.  The stream is idle: the old one is freed.
static void adopt_table(smg_engine *e, Dev &k, Dev &c, int64_t n)
{ e->own_keys.take(k); e->own_cnt.take(c);
  e->tab.keys = e->own_keys; e->tab.cnt = e->own_cnt;
  table_changed(e, n);
}

// sorted, duplicate-free table from 2-copies-at-most material: keys[n2 * W], counts, copy flags (NULL: the first of two
// equal k-mers in INPUT order wins, as the stable sort leaves it) -> the engine's own table.  Frees nothing of the caller's.
static int cond_sort_dedupe(smg_engine *e, const u64 *k2, const uint16_t *c2, const uint8_t *copy, int64_t n2,
                            int64_t *kept_out, char *errbuf, size_t errlen)
{ const int W = e->tab.W;
  if (n2 >= 0xFFFFFFF0ll) return fail(errbuf, errlen, SMG_EINVAL, "shard too large to symmetrise (2^32 entries per shard)%s");
  const unsigned nblk2 = (unsigned) ((n2 + TPB - 1) / TPB);
  Dev perm, flag, pos, ko, co;
  int64_t kept = 0;
  HIPCHK(sort_permutation(k2, W, n2, e->stream, e->sort_tmp, perm));
  HIPCHK(flag.alloc(sizeof(uint32_t) * (size_t) n2));
  HIPCHK(pos.alloc(sizeof(uint32_t) * (size_t) n2));
  with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_flag_first<w()>, dim3(nblk2), dim3(TPB), 0, e->stream, k2, perm.as<uint32_t>(), n2, flag.as<uint32_t>()); });
  HIPCHK(scan_flags(flag.as<uint32_t>(), pos.as<uint32_t>(), n2, e->stream, e->sort_tmp, &kept));
  HIPCHK(ko.alloc(sizeof(u64) * (size_t) (kept > 0 ? kept : 1) * W));
  HIPCHK(co.alloc(sizeof(uint16_t) * (size_t) (kept > 0 ? kept : 1) + 16));
  if (copy)
    {
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_compact_pref<w()>, dim3(nblk2), dim3(TPB), 0, e->stream, k2, c2, copy, perm.as<uint32_t>(),
          flag.as<uint32_t>(), pos.as<uint32_t>(), n2, ko.as<u64>(), co.as<uint16_t>()); });
    }
  else
    {
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_compact<w()>, dim3(nblk2), dim3(TPB), 0, e->stream, k2, c2, perm.as<uint32_t>(),
          flag.as<uint32_t>(), pos.as<uint32_t>(), n2, ko.as<u64>(), co.as<uint16_t>()); });
    }
  HIPCHK(hipStreamSynchronize(e->stream));
  adopt_table(e, ko, co, kept);
  *kept_out = kept;
  return SMG_OK;
}

extern "C" int smg_engine_condition(smg_engine *e, int ethresh, int do_trim, int do_symm,
                                    int64_t *new_nels, char *errbuf, size_t errlen)
{ if (!e) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");
  if (!e->tab.keys && e->tab.n > 0) return fail(errbuf, errlen, SMG_EINVAL, "no table bound%s");
  HIPCHK(hipSetDevice(e->device));
  const int W = e->tab.W;
  int rc;
  int64_t n = e->tab.n;
  hipEventRecord(e->ev[EV_DECODE_BEG], e->stream);                 // (the decode pair: conditioning is booked under ms_decode)

  if (do_trim && n > 0)
    { const unsigned nblk = (unsigned) ((n + TPB - 1) / TPB);
      Dev flag, pos, ko, co;
      HIPCHK(flag.alloc(sizeof(uint32_t) * (size_t) n));
      HIPCHK(pos.alloc(sizeof(uint32_t) * (size_t) n));
      hipLaunchKernelGGL(kc_flag_trim, dim3(nblk), dim3(TPB), 0, e->stream, e->tab.cnt, n, (unsigned) ethresh, flag.as<uint32_t>());
      int64_t kept = 0;
      HIPCHK(scan_flags(flag.as<uint32_t>(), pos.as<uint32_t>(), n, e->stream, e->sort_tmp, &kept));
      HIPCHK(ko.alloc(sizeof(u64) * (size_t) (kept > 0 ? kept : 1) * W));
      HIPCHK(co.alloc(sizeof(uint16_t) * (size_t) (kept > 0 ? kept : 1) + 16));
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_compact<w()>, dim3(nblk), dim3(TPB), 0, e->stream, e->tab.keys, e->tab.cnt,
          (const uint32_t *) NULL, flag.as<uint32_t>(), pos.as<uint32_t>(), n, ko.as<u64>(), co.as<uint16_t>()); });
      HIPCHK(hipStreamSynchronize(e->stream));
      adopt_table(e, ko, co, kept);
      n = kept;
    }

  if (do_symm && n > 0)
    { const int64_t n2 = 2 * n;
      if (n2 >= 0xFFFFFFF0ll) return fail(errbuf, errlen, SMG_EINVAL, "table too large to symmetrise in one shard%s");
      const unsigned nblk = (unsigned) ((n + TPB - 1) / TPB);
      Dev k2, c2;
      HIPCHK(k2.alloc(sizeof(u64) * (size_t) n2 * W));
      HIPCHK(c2.alloc(sizeof(uint16_t) * (size_t) n2));
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_append_rc<w()>, dim3(nblk), dim3(TPB), 0, e->stream, e->tab.keys, e->tab.cnt, n, e->tab.kmer,
          k2.as<u64>(), c2.as<uint16_t>()); });
      // (entries first, complements behind them: the stable sort keeps the entry in front of an equal complement)
      if ((rc = cond_sort_dedupe(e, k2.as<u64>(), c2.as<uint16_t>(), NULL, n2, &n, errbuf, errlen))) return rc;
    }
  hipEventRecord(e->ev[EV_DECODE_END], e->stream);
  HIPCHK(hipStreamSynchronize(e->stream));
  const float ms = ms_between(e, EV_DECODE_BEG, EV_DECODE_END);
  table_changed(e, n);                                 // (also where nothing was asked for, or of an empty table)
  e->rp.have = false; e->rp.active = false;
  e->st.ms_decode += ms;
  if (new_nels) *new_nels = n;
  return SMG_OK;
}

// ---- closure of a CANONICAL table by merge ------------------------------------------------------------------------------
// A table as the k-mer counter leaves it holds, of every k-mer and its reverse complement, the smaller one only (x <= rc x),
// sorted.  The complements R of its entries that are not their own complement are then disjoint from the table C (were
// rc x = y in C, y <= rc y = x and x <= rc x = y would make them equal), so the closure is C merged with sorted R: one sort
// of m <= n k-mers where smg_engine_condition sorts 2 n, nothing to de-duplicate, no count to choose.  Entry for entry the
// table smg_engine_condition(e, 0, 0, 1) leaves.

// rc[i] = the reverse complement of entry i, flag[i] = it is another k-mer; *bad is set where it is the SMALLER one
template <int W> __global__ void __launch_bounds__(TPB)
kc_rc_flag(const u64 *__restrict__ keys, int64_t n, int k, u64 *__restrict__ rc, uint32_t *__restrict__ flag, uint32_t *__restrict__ bad)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const Key<W> x = load_key<W>(keys, i);
  const Key<W> r = revcomp<W>(x, k);
#pragma unroll
  for (int w = 0; w < W; w++) rc[i * W + w] = r.w[w];
  flag[i] = !key_eq<W>(x, r);
  if (key_lt<W>(r, x)) *bad = 1u;
}

// the flagged complements, compacted, and the entry each came from
template <int W> __global__ void __launch_bounds__(TPB)
kc_rc_compact(const u64 *__restrict__ rc, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t n,
              u64 *__restrict__ okeys, uint32_t *__restrict__ osrc)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const int64_t dst = pos[i];
#pragma unroll
  for (int w = 0; w < W; w++) okeys[dst * W + w] = rc[i * W + w];
  osrc[dst] = (uint32_t) i;
}

extern "C" int smg_engine_merge_tile(int key_words)
{ return key_words >= 1 && key_words <= 4 ? ks_merge_tile(key_words) : 0; }

// *not_canonical tells that refusal (SMG_EINVAL like the others, the table untouched) from every other one
static int close_canonical(smg_engine *e, int64_t *new_nels, bool *not_canonical, char *errbuf, size_t errlen)
{ *not_canonical = false;
  if (!e) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");
  if (!e->tab.keys && e->tab.n > 0) return fail(errbuf, errlen, SMG_EINVAL, "no table bound%s");
  HIPCHK(hipSetDevice(e->device));
  const int W = e->tab.W;
  const int64_t n = e->tab.n;
  int64_t m = 0;
  hipEventRecord(e->ev[EV_DECODE_BEG], e->stream);                 // (booked under ms_decode, like smg_engine_condition)
  if (n > 0)
    { const unsigned nblk = (unsigned) ((n + TPB - 1) / TPB);
      Dev rc, flag, pos, bad, rk, rsrc, perm, split, ko, co;
      uint32_t h_bad = 0;
      HIPCHK(rc.alloc(sizeof(u64) * (size_t) n * W));
      HIPCHK(flag.alloc(sizeof(uint32_t) * (size_t) n));
      HIPCHK(pos.alloc(sizeof(uint32_t) * (size_t) n));
      HIPCHK(bad.alloc(16));
      HIPCHK(hipMemsetAsync(bad.p, 0, 16, e->stream));
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_rc_flag<w()>, dim3(nblk), dim3(TPB), 0, e->stream, e->tab.keys, n, e->tab.kmer, rc.as<u64>(),
          flag.as<uint32_t>(), bad.as<uint32_t>()); });
      HIPCHK(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(scan_flags(flag.as<uint32_t>(), pos.as<uint32_t>(), n, e->stream, e->sort_tmp, &m));    // (waits)
      if (h_bad)
        { *not_canonical = true;
          return fail(errbuf, errlen, SMG_EINVAL, "table is not canonical: an entry is larger than its reverse complement "
                      "(smg_engine_condition closes any sorted table)%s");
        }
      if (n + m >= 0xFFFFFFF0ll) return fail(errbuf, errlen, SMG_EINVAL, "table too large to symmetrise in one shard%s");
      HIPCHK(ko.alloc(sizeof(u64) * (size_t) (n + m) * W));
      HIPCHK(co.alloc(sizeof(uint16_t) * (size_t) (n + m) + 16));
      if (m == 0)                                      // every entry is its own complement: the closure is a copy
        { HIPCHK(hipMemcpyAsync(ko.p, e->tab.keys, sizeof(u64) * (size_t) n * W, hipMemcpyDeviceToDevice, e->stream));
          HIPCHK(hipMemcpyAsync(co.p, e->tab.cnt, sizeof(uint16_t) * (size_t) n, hipMemcpyDeviceToDevice, e->stream));
        }
      else
        { HIPCHK(rk.alloc(sizeof(u64) * (size_t) m * W));
          HIPCHK(rsrc.alloc(sizeof(uint32_t) * (size_t) m));
          with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_rc_compact<w()>, dim3(nblk), dim3(TPB), 0, e->stream, rc.as<u64>(), flag.as<uint32_t>(),
              pos.as<uint32_t>(), n, rk.as<u64>(), rsrc.as<uint32_t>()); });
          HIPCHK(hipStreamSynchronize(e->stream));
          rc.reset(); flag.reset(); pos.reset();
          HIPCHK(sort_permutation(rk.as<u64>(), W, m, e->stream, e->sort_tmp, perm));
          const int64_t ntiles = (n + m + ks_merge_tile(W) - 1) / ks_merge_tile(W);
          HIPCHK(split.alloc(sizeof(uint32_t) * (size_t) (ntiles + 1)));
          with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(ks_merge_split<w()>, dim3((unsigned) (ntiles / KS_TPB + 1)), dim3(KS_TPB), 0, e->stream, e->tab.keys, n,
              rk.as<u64>(), perm.as<uint32_t>(), m, ntiles, split.as<uint32_t>()); });
          with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(ks_merge<w()>, dim3((unsigned) ntiles), dim3(KS_TPB), 0, e->stream, e->tab.keys, e->tab.cnt, n, rk.as<u64>(),
              perm.as<uint32_t>(), rsrc.as<uint32_t>(), m, split.as<uint32_t>(), ko.as<u64>(), co.as<uint16_t>()); });
          HIPCHK(hipGetLastError());
        }
      HIPCHK(hipStreamSynchronize(e->stream));
      adopt_table(e, ko, co, n + m);
    }
  hipEventRecord(e->ev[EV_DECODE_END], e->stream);
  HIPCHK(hipStreamSynchronize(e->stream));
  const float ms = ms_between(e, EV_DECODE_BEG, EV_DECODE_END);
  table_changed(e, n + m);
  e->rp.have = false; e->rp.active = false;
  e->st.ms_decode += ms;
  if (new_nels) *new_nels = n + m;
  return SMG_OK;
}

extern "C" int smg_engine_close_canonical(smg_engine *e, int64_t *new_nels, char *errbuf, size_t errlen)
{ bool not_canonical;
  return close_canonical(e, new_nels, &not_canonical, errbuf, errlen);
}

extern "C" int smg_engine_table(smg_engine *e, int64_t *nels, const uint64_t **d_keys, const uint16_t **d_counts)
{ if (!e) return SMG_EINVAL;
  if (nels) *nels = e->tab.n;
  if (d_keys) *d_keys = (const uint64_t *) e->tab.keys;
  if (d_counts) *d_counts = e->tab.cnt;
  return SMG_OK;
}

// the same table copied to the host (tests and tools that want to look at a conditioned table): two copies and a wait
extern "C" int smg_engine_table_host(smg_engine *e, uint64_t *keys, uint16_t *counts, int64_t capacity, char *errbuf, size_t errlen)
{ NEED_ENGINE(e)
  if (capacity < e->tab.n || (e->tab.n > 0 && (!keys || !counts)))
    return fail(errbuf, errlen, SMG_EINVAL, "table_host: the buffers must hold every entry of the table%s");
  if (e->tab.n == 0) return SMG_OK;
  if (!e->tab.keys || !e->tab.cnt) return fail(errbuf, errlen, SMG_EINVAL, "no table bound%s");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipMemcpyAsync(keys, e->tab.keys, sizeof(u64) * (size_t) e->tab.n * e->tab.W, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(counts, e->tab.cnt, sizeof(uint16_t) * (size_t) e->tab.n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return SMG_OK;
}

// ---- symmetrising a table that is cut into prefix shards (several GPUs, or one device and more than 2^32 entries) -----
// The reference's Symmex has no size limit (PloidyPlot.c:1395-1414 hands it any table).  Here every shard
//   1. counts its own entries and their reverse complements per leading `bits` k-mer bits (smg_engine_symm_hist): the
//      sum over the shards is the shape of the CLOSED table, from which the caller takes balanced splitters -- a table
//      of canonical k-mers crowds the low end of the k-mer space (7/8 of the k-mers that start with an a are canonical,
//      1/8 of those that start with a t), its closure does not;
//   2. writes one record per entry and one per complement, grouped by the shard whose range holds the k-mer
//      (smg_engine_symm_route; records of W + 1 words: the k-mer, then count | is-a-complement << 16);
//   3. after the exchange sorts what it received and keeps one entry per k-mer (smg_engine_symm_finish; a k-mer that
//      arrives as an entry AND as a complement keeps the entry's count -- self-complementary k-mers, or input that was
//      neither canonical nor closed: the same rule as the single-shard code above).

#define SY_MAXBITS 12

template <int W> __global__ void __launch_bounds__(TPB)
kc_symm_hist(const u64 *__restrict__ keys, int64_t n, int k, int bits, u64 *__restrict__ hist /* [2 << bits]: own, complements */)
{ __shared__ unsigned h[2 << SY_MAXBITS];
  const int nb = 1 << bits;
  for (int b = threadIdx.x; b < 2 * nb; b += TPB) h[b] = 0;
  __syncthreads();
  for (int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t) gridDim.x * TPB)
    { const Key<W> x = load_key<W>(keys, i);
      const Key<W> r = revcomp<W>(x, k);
      atomicAdd(&h[(unsigned) (x.w[0] >> (64 - bits))], 1u);
      atomicAdd(&h[nb + (unsigned) (r.w[0] >> (64 - bits))], 1u);
    }
  __syncthreads();
  for (int b = threadIdx.x; b < 2 * nb; b += TPB)
    if (h[b]) atomicAdd(&hist[b], (u64) h[b]);
}

// record i = (entry i, count), record n + i = (its reverse complement, count | 1 << 16)
template <int W> __global__ void __launch_bounds__(TPB)
kc_symm_records(const u64 *__restrict__ keys, const uint16_t *__restrict__ cnt, int64_t n, int k, u64 *__restrict__ rec)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const Key<W> x = load_key<W>(keys, i);
  const Key<W> r = revcomp<W>(x, k);
  u64 *a = rec + (size_t) i * (W + 1), *b = rec + (size_t) (n + i) * (W + 1);
#pragma unroll
  for (int w = 0; w < W; w++) { a[w] = x.w[w]; b[w] = r.w[w]; }
  a[W] = (u64) cnt[i];
  b[W] = (u64) cnt[i] | (1ull << 16);
}

// records -> separate k-mer / count / is-a-complement arrays
template <int W> __global__ void __launch_bounds__(TPB)
kc_symm_unpack(const u64 *__restrict__ rec, int64_t n, u64 *__restrict__ keys, uint16_t *__restrict__ cnt, uint8_t *__restrict__ copy)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const u64 *q = rec + (size_t) i * (W + 1);
#pragma unroll
  for (int w = 0; w < W; w++) keys[i * W + w] = q[w];
  cnt[i] = (uint16_t) q[W];
  copy[i] = (uint8_t) ((q[W] >> 16) & 1u);
}

// bits of the leading k-mer prefix that the closed table is cut on: a boundary of <= 12 leading bits is a window-block
// boundary too (blocks share k / 2 bases)
static int symm_split_bits(int kmer)
{ const int b = 2 * (kmer / 2) < SY_MAXBITS ? 2 * (kmer / 2) : SY_MAXBITS;
  return b < 2 ? 2 : b;
}

// the histogram of any sorted table on the engine's device and stream: hist[0 .. nbin) entries, hist[nbin .. 2 nbin) complements
static int symm_hist_of(smg_engine *e, const u64 *keys, int64_t n, int kmer, int bits, int64_t *hist, char *errbuf, size_t errlen)
{ const size_t bytes = sizeof(u64) * ((size_t) 2 << bits);
  Dev d;
  HIPCHK(d.alloc(bytes));
  hipError_t he = hipMemsetAsync(d.p, 0, bytes, e->stream);
  if (he == hipSuccess && n > 0)
    { int64_t nb = (n + TPB - 1) / TPB;
      if (nb > 2048) nb = 2048;
      with_words<4>((kmer + 31) / 32, [&](auto w) { hipLaunchKernelGGL(kc_symm_hist<w()>, dim3((unsigned) nb), dim3(TPB), 0, e->stream, keys, n, kmer, bits, d.as<u64>()); });
      he = hipGetLastError();
    }
  if (he == hipSuccess) he = hipMemcpyAsync(hist, d.p, bytes, hipMemcpyDeviceToHost, e->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
  if (he != hipSuccess) return fail(errbuf, errlen, SMG_ENODEV, "symm_hist: %s", hipGetErrorString(he));
  return SMG_OK;
}

extern "C" int smg_engine_symm_hist(smg_engine *e, int bits, int64_t *hist, char *errbuf, size_t errlen)
{ if (!e || !hist) return fail(errbuf, errlen, SMG_EINVAL, "null argument%s");
  if (bits < 1 || bits > SY_MAXBITS || bits > 2 * e->tab.kmer) return fail(errbuf, errlen, SMG_EINVAL, "symm_hist: 1..12 leading bits, at most 2k%s");
  if (!e->tab.keys && e->tab.n > 0) return fail(errbuf, errlen, SMG_EINVAL, "no table bound%s");
  HIPCHK(hipSetDevice(e->device));
  return symm_hist_of(e, e->tab.keys, e->tab.n, e->tab.kmer, bits, hist, errbuf, errlen);
}

extern "C" int smg_engine_symm_route(smg_engine *e, const uint64_t *splitters, int nranks, uint64_t *d_send,
                                     int64_t capacity, int64_t *counts, char *errbuf, size_t errlen)
{ if (!e || !counts || nranks < 1 || nranks > 16) return fail(errbuf, errlen, SMG_EINVAL, "bad symm_route arguments (1..16 ranks)%s");
  if (!e->tab.keys && e->tab.n > 0) return fail(errbuf, errlen, SMG_EINVAL, "no table bound%s");
  const int64_t n2 = 2 * e->tab.n;
  if (capacity < n2 || (n2 > 0 && !d_send)) return fail(errbuf, errlen, SMG_EINVAL, "symm_route: the send buffer must hold two records per entry%s");
  for (int r = 0; r < nranks; r++) counts[r] = 0;
  if (n2 == 0) return SMG_OK;
  HIPCHK(hipSetDevice(e->device));
  const int rw = e->tab.W + 1;
  const int64_t nc = (n2 + F_CH - 1) / F_CH;
  if (nc >= 0x7FFFFFFFll) return fail(errbuf, errlen, SMG_EINVAL, "symm_route: shard too large%s");
  Dev rec, fill;
  int rc = SMG_OK;
  if (rec.alloc(sizeof(u64) * (size_t) n2 * rw) != hipSuccess || fill.alloc(sizeof(uint32_t) * (size_t) nc) != hipSuccess)
    return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory while symmetrising%s");
  const unsigned nblk = (unsigned) ((e->tab.n + TPB - 1) / TPB);
  with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_symm_records<w()>, dim3(nblk), dim3(TPB), 0, e->stream, e->tab.keys, e->tab.cnt, e->tab.n, e->tab.kmer, rec.as<u64>()); });
  hipLaunchKernelGGL(kc_fill_u32, dim3((unsigned) ((nc + TPB - 1) / TPB)), dim3(TPB), 0, e->stream, fill.as<uint32_t>(), nc, (uint32_t) F_CH,
                     (uint32_t) (n2 - (nc - 1) * F_CH));
  if (hipGetLastError() != hipSuccess) rc = fail(errbuf, errlen, SMG_ENODEV, "symm_route: launch failed%s");
  if (rc == SMG_OK) rc = route_records(e, rec.as<u64>(), fill.as<uint32_t>(), (unsigned) nc, rw, splitters, nranks, d_send, capacity, counts, NULL, errbuf, errlen);
  hipStreamSynchronize(e->stream);                     // (the records are freed on return)
  return rc;
}

extern "C" int smg_engine_symm_finish(smg_engine *e, const uint64_t *d_recv, int64_t nrecv, int64_t *new_nels,
                                      char *errbuf, size_t errlen)
{ if (!e || nrecv < 0 || (nrecv > 0 && !d_recv)) return fail(errbuf, errlen, SMG_EINVAL, "bad symm_finish arguments%s");
  if (e->tab.kmer < 1) return fail(errbuf, errlen, SMG_EINVAL, "no table bound%s");
  HIPCHK(hipSetDevice(e->device));
  int64_t kept = 0;
  if (nrecv == 0)
    { Dev ko, co;
      HIPCHK(ko.alloc(sizeof(u64) * e->tab.W)); HIPCHK(co.alloc(16));
      adopt_table(e, ko, co, 0);
    }
  else
    { if (nrecv >= 0xFFFFFFF0ll) return fail(errbuf, errlen, SMG_EINVAL, "shard too large to symmetrise (2^32 entries per shard)%s");
      Dev k2, c2, cp;
      if (k2.alloc(sizeof(u64) * (size_t) nrecv * e->tab.W) != hipSuccess || c2.alloc(sizeof(uint16_t) * (size_t) nrecv + 16) != hipSuccess
          || cp.alloc((size_t) nrecv + 16) != hipSuccess)
        return fail(errbuf, errlen, SMG_ENOMEM, "out of device memory while symmetrising%s");
      const unsigned nblk = (unsigned) ((nrecv + TPB - 1) / TPB);
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(kc_symm_unpack<w()>, dim3(nblk), dim3(TPB), 0, e->stream, (const u64 *) d_recv, nrecv, k2.as<u64>(),
          c2.as<uint16_t>(), cp.as<uint8_t>()); });
      const int rc = cond_sort_dedupe(e, k2.as<u64>(), c2.as<uint16_t>(), cp.as<uint8_t>(), nrecv, &kept, errbuf, errlen);
      if (rc) return rc;
    }
  if (new_nels) *new_nels = kept;
  return SMG_OK;
}

// ---- closure of a canonical table ONE KEY RANGE AT A TIME -----------------------------------------------------------------
// The part of the closed table T inside a key range [lo, hi) is the slice of C in the range merged with R_s, the sorted
// complements of those entries of ALL of C whose complement falls into the range.  The two are disjoint for the reason given
// above close_canonical, so there is nothing to de-duplicate.  What a range allocates is proportional to the range: the
// complements are selected in one pass over C that materialises nothing per entry of C (kc_rc_select), sorted
// (sort_permutation) and merged with the slice (ks_merge_split, ks_merge_bcnt).  closure_price (smg_shards.hpp) prices it.

template <int W> struct KeyRange { Key<W> lo, hi; int has_lo, has_hi; };      // [lo, hi); an end that is not there is open

template <int W> static KeyRange<W> key_range(const uint64_t *lo, const uint64_t *hi)
{ KeyRange<W> rg;
  rg.has_lo = lo != NULL; rg.has_hi = hi != NULL;
  for (int w = 0; w < W; w++) { rg.lo.w[w] = lo ? lo[w] : 0; rg.hi.w[w] = hi ? hi[w] : ~0ull; }
  return rg;
}

// One pass over C: the complement r of entry x is appended (with x's count) when it lies in the range and is another k-mer;
// ctl[1] is set where r < x (the table is not canonical).  A wave takes RS_ITEMS rows of 64 entries and reserves the slots of
// all its complements with one ballot per row and ONE atomic (every wave's goes to the same word: at one row per wave a
// closure of a quarter of a 1e8-entry table took 18.6 ms, at eight 5.9 ms, profiles/reads_to_smu.md); the order of the list
// is of no account, it is sorted next.  ctl[0] counts every
// selected complement, stored or not: nothing is written at or behind slot `cap`, and the host sees the overflow.
#define RS_ITEMS 8
template <int W> __global__ void __launch_bounds__(TPB)
kc_rc_select(const u64 *__restrict__ keys, const uint16_t *__restrict__ cnt, int64_t n, int k, KeyRange<W> rg, u64 cap,
             u64 *__restrict__ okeys, uint16_t *__restrict__ ocnt, u64 *__restrict__ ctl)
{ const int lane = threadIdx.x & 63;
  const int64_t first = ((((int64_t) blockIdx.x * TPB + threadIdx.x) >> 6) * RS_ITEMS) * 64 + lane;     // this lane's entry of row 0
  Key<W> r[RS_ITEMS];
  u64 mask[RS_ITEMS];
  unsigned total = 0;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < RS_ITEMS; j++)
    { const int64_t i = first + 64 * j;
      bool keep = false;
      if (i < n)
        { const Key<W> x = load_key<W>(keys, i);
          r[j] = revcomp<W>(x, k);
          keep = !key_eq<W>(x, r[j]) && !(rg.has_lo && key_lt<W>(r[j], rg.lo)) && (!rg.has_hi || key_lt<W>(r[j], rg.hi));
          bad |= key_lt<W>(r[j], x);
        }
      mask[j] = __ballot(keep);
      total += (unsigned) __popcll(mask[j]);
    }
  if (bad) ctl[1] = 1ull;
  if (!total) return;                                  // (the whole wave)
  u64 base = 0;
  if (lane == 0) base = atomicAdd(&ctl[0], (u64) total);
  base = __shfl(base, 0, 64);
#pragma unroll
  for (int j = 0; j < RS_ITEMS; j++)
    { const u64 slot = base + (u64) __popcll(mask[j] & ((1ull << lane) - 1ull));
      if (((mask[j] >> lane) & 1ull) && slot < cap)
        {
#pragma unroll
          for (int w = 0; w < W; w++) okeys[slot * W + w] = r[j].w[w];
          ocnt[slot] = cnt[first + 64 * j];
        }
      base += (u64) __popcll(mask[j]);
    }
}

// out[0], out[1] = the slice of C in the range: the first entry >= lo, the first entry >= hi (one bisection per cut)
template <int W> __global__ void __launch_bounds__(64)
kc_slice_bounds(const u64 *__restrict__ keys, int64_t n, KeyRange<W> rg, u64 *__restrict__ out)
{ if (threadIdx.x == 0) out[0] = rg.has_lo ? (u64) lower_bound_key<W>(keys, 0, n, rg.lo) : 0ull;
  if (threadIdx.x == 1) out[1] = rg.has_hi ? (u64) lower_bound_key<W>(keys, 0, n, rg.hi) : (u64) n;
}

// the bins [*b0, *b1) of the `bits`-bit histogram that the range touches
static void range_bins(const uint64_t *lo, const uint64_t *hi, int W, int bits, int *b0, int *b1)
{ *b0 = lo ? (int) (lo[0] >> (64 - bits)) : 0;
  *b1 = 1 << bits;
  if (hi)
    { bool on_boundary = (hi[0] << bits) == 0;
      for (int w = 1; w < W; w++) on_boundary = on_boundary && hi[w] == 0;
      *b1 = (int) (hi[0] >> (64 - bits)) + (on_boundary ? 0 : 1);
    }
}

static bool range_is_empty(const uint64_t *lo, const uint64_t *hi, int W)
{ if (!lo || !hi) return false;
  for (int w = 0; w < W; w++) if (lo[w] != hi[w]) return lo[w] > hi[w];
  return true;
}

// the selection pass and the slice bounds of one range on e's stream: at most `cap` complements into (rk, rcnt), which are
// allocated here for as many; *m = how many there are, *a0, *a1 = the slice of C.  cap = 0: only the canonical check is of use.
static int range_select(smg_engine *e, int kmer, int64_t n, const u64 *keys, const uint16_t *cnt, const uint64_t *lo, const uint64_t *hi,
                        int64_t cap, Dev &rk, Dev &rcnt, int64_t *m, bool *bad, int64_t *a0, int64_t *a1, char *errbuf, size_t errlen)
{ const int W = (kmer + 31) / 32;
  Dev ctl;
  u64 h[4] = { 0, 0, 0, 0 };
  HIPCHK(ctl.alloc(sizeof(u64) * 4));
  HIPCHK(rk.alloc(sizeof(u64) * (size_t) (cap > 0 ? cap : 1) * W));
  HIPCHK(rcnt.alloc(sizeof(uint16_t) * (size_t) (cap > 0 ? cap : 1) + 16));
  HIPCHK(hipMemsetAsync(ctl.p, 0, sizeof(u64) * 4, e->stream));
  if (n > 0)
    { const unsigned nblk = (unsigned) ((n + TPB * RS_ITEMS - 1) / (TPB * RS_ITEMS));
      with_words<4>(W, [&](auto w)
        { const KeyRange<w()> rg = key_range<w()>(lo, hi);
          hipLaunchKernelGGL(kc_rc_select<w()>, dim3(nblk), dim3(TPB), 0, e->stream, keys, cnt, n, kmer, rg, (u64) cap, rk.as<u64>(),
                             rcnt.as<uint16_t>(), ctl.as<u64>());
          hipLaunchKernelGGL(kc_slice_bounds<w()>, dim3(1), dim3(64), 0, e->stream, keys, n, rg, ctl.as<u64>() + 2);
        });
      HIPCHK(hipGetLastError());
    }
  HIPCHK(hipMemcpyAsync(h, ctl.p, sizeof(h), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *m = (int64_t) h[0]; *bad = h[1] != 0; *a0 = (int64_t) h[2]; *a1 = (int64_t) h[3];
  if (*a1 < *a0) *a1 = *a0;                            // (an empty range handed in with hi < lo)
  return SMG_OK;
}

#define RANGE_NELS_MAX (0xFFFFFFF0ll - 16)             // (SMG_ONE_SHARD_MAX, smg_shards.hpp)

// cap < 0: the room for the complements is taken from a histogram of C (one more pass); the shard driver, which has that
// histogram already, hands the capacity in.  *not_canonical tells that refusal from every other one.
static int close_canonical_range(smg_engine *e, int kmer, int64_t n, const u64 *keys, const uint16_t *cnt, const uint64_t *lo,
                                 const uint64_t *hi, int64_t cap, int64_t *new_nels, bool *not_canonical, char *errbuf, size_t errlen)
{ *not_canonical = false;
  if (!e) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");
  if (kmer < 1 || kmer > SMG_MAX_KMER) return fail(errbuf, errlen, SMG_EINVAL, "k-mer length out of range (1..128)%s");
  if (n < 0 || n >= RANGE_NELS_MAX) return fail(errbuf, errlen, SMG_EINVAL, "range closure: the table must have fewer than 2^32 - 32 entries%s");
  if (n > 0 && (!keys || !cnt)) return fail(errbuf, errlen, SMG_EINVAL, "null table pointer%s");
  if (((uintptr_t) keys & 15) || ((uintptr_t) cnt & 7))
    return fail(errbuf, errlen, SMG_EINVAL, "table pointers must be aligned (k-mers 16 bytes, counts 8 bytes)%s");
  HIPCHK(hipSetDevice(e->device));
  const int W = (kmer + 31) / 32;
  const bool empty = range_is_empty(lo, hi, W);
  int rc;
  hipEventRecord(e->ev[EV_DECODE_BEG], e->stream);                 // (booked under ms_decode, like close_canonical)
  if (empty) cap = 0;
  if (cap < 0 && n > 0)
    { const int bits = symm_split_bits(kmer), nbin = 1 << bits;
      std::vector<int64_t> hist((size_t) 2 * nbin, 0);
      int b0, b1;
      if ((rc = symm_hist_of(e, keys, n, kmer, bits, hist.data(), errbuf, errlen))) return rc;
      range_bins(lo, hi, W, bits, &b0, &b1);
      cap = 0;
      for (int b = b0; b < b1; b++) cap += hist[(size_t) nbin + b];
    }
  if (cap < 0) cap = 0;
  Dev rk, rcnt, perm, split, ko, co;
  int64_t m = 0, a0 = 0, a1 = 0;
  bool bad = false;
  if ((rc = range_select(e, kmer, n, keys, cnt, lo, hi, cap, rk, rcnt, &m, &bad, &a0, &a1, errbuf, errlen))) return rc;
  if (bad)
    { *not_canonical = true;
      return fail(errbuf, errlen, SMG_EINVAL, "table is not canonical: an entry is larger than its reverse complement "
                  "(smg_engine_condition closes any sorted table)%s");
    }
  if (m > cap)
    { if (errbuf && errlen) snprintf(errbuf, errlen, "range closure: %lld complements fall into the range, room was made for %lld",
                                     (long long) m, (long long) cap);
      return SMG_EINVAL;
    }
  const int64_t na = empty ? 0 : a1 - a0, ns = na + m;
  if (ns >= RANGE_NELS_MAX) return fail(errbuf, errlen, SMG_EINVAL, "range closure: the range holds 2^32 - 32 entries or more%s");
  const u64 *a = keys + (size_t) a0 * W;
  const uint16_t *ac = cnt + a0;
  HIPCHK(ko.alloc(sizeof(u64) * (size_t) (ns > 0 ? ns : 1) * W));
  HIPCHK(co.alloc(sizeof(uint16_t) * (size_t) (ns > 0 ? ns : 1) + 16));
  if (m == 0 && na > 0)                                // no complement falls into the range: the shard is a copy of the slice
    { HIPCHK(hipMemcpyAsync(ko.p, a, sizeof(u64) * (size_t) na * W, hipMemcpyDeviceToDevice, e->stream));
      HIPCHK(hipMemcpyAsync(co.p, ac, sizeof(uint16_t) * (size_t) na, hipMemcpyDeviceToDevice, e->stream));
    }
  else if (m > 0)
    { HIPCHK(sort_permutation(rk.as<u64>(), W, m, e->stream, e->sort_tmp, perm));
      const int64_t ntiles = (ns + ks_merge_tile(W) - 1) / ks_merge_tile(W);
      HIPCHK(split.alloc(sizeof(uint32_t) * (size_t) (ntiles + 1)));
      with_words<4>(W, [&](auto w)
        { hipLaunchKernelGGL(ks_merge_split<w()>, dim3((unsigned) (ntiles / KS_TPB + 1)), dim3(KS_TPB), 0, e->stream, a, na, rk.as<u64>(),
                             perm.as<uint32_t>(), m, ntiles, split.as<uint32_t>());
          hipLaunchKernelGGL(ks_merge_bcnt<w()>, dim3((unsigned) ntiles), dim3(KS_TPB), 0, e->stream, a, ac, na, rk.as<u64>(),
                             perm.as<uint32_t>(), rcnt.as<uint16_t>(), m, split.as<uint32_t>(), ko.as<u64>(), co.as<uint16_t>());
        });
      HIPCHK(hipGetLastError());
    }
  hipEventRecord(e->ev[EV_DECODE_END], e->stream);
  HIPCHK(hipStreamSynchronize(e->stream));
  const float ms = ms_between(e, EV_DECODE_BEG, EV_DECODE_END);
  if ((rc = set_table(e, kmer, ns, errbuf, errlen))) return rc;
  adopt_table(e, ko, co, ns);
  e->st.ms_decode = ms;
  if (new_nels) *new_nels = ns;
  return SMG_OK;
}

extern "C" int smg_engine_close_canonical_range(smg_engine *e, int kmer, int64_t nels, const uint64_t *d_keys, const uint16_t *d_counts,
                                                const uint64_t *lo, const uint64_t *hi, int64_t *new_nels, char *errbuf, size_t errlen)
{ bool not_canonical;
  return close_canonical_range(e, kmer, nels, (const u64 *) d_keys, d_counts, lo, hi, -1, new_nels, &not_canonical, errbuf, errlen);
}

// the same with the room for the complements handed in (the shard driver's door, and the tests' for a capacity that is too
// small: SMG_EINVAL, the engine's table as it was, nothing written behind the room)
extern "C" int smg_engine_close_canonical_range_cap(smg_engine *e, int kmer, int64_t nels, const uint64_t *d_keys, const uint16_t *d_counts,
                                                    const uint64_t *lo, const uint64_t *hi, int64_t capacity, int64_t *new_nels,
                                                    char *errbuf, size_t errlen)
{ bool not_canonical;
  if (capacity < 0) return fail(errbuf, errlen, SMG_EINVAL, "range closure: negative capacity%s");
  return close_canonical_range(e, kmer, nels, (const u64 *) d_keys, d_counts, lo, hi, capacity, new_nels, &not_canonical, errbuf, errlen);
}
