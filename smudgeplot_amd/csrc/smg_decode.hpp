// smg_decode.hpp -- the FastK record decoder of the hetmers engine: k_decode, its drivers (a whole table, or piece by piece
// behind the copies of smg_ingest.hpp), and the table's own prefix index as look-up directory.  Included by smg_hetmers.hip
// behind the engine struct; no state of its own.

#pragma once

// format F records -> interleaved left-aligned words + counts
// (restates Current_Entry, libfastk.c:1230-1269: prefix from the index, suffix from the record)
//
// One workgroup decodes DEC_TILE consecutive entries, four per thread:
//   * their record bytes (DEC_TILE * pbyte, contiguous) are staged in LDS with coalesced dword loads
//     (records are 3..34 bytes wide and unaligned: per-thread byte loads ran at ~4 G entries/s);
//   * a k-mer is put together 32 bits at a time: an unaligned little-endian dword of the staged bytes is one
//     v_alignbyte over two LDS dwords, its big-endian value one v_perm; the first dword takes the prefix bytes from
//     the index, the last one is masked behind the k-mer's last byte (the count bytes follow it in the record).
//     (Round 2 walked the 8 W bytes of an entry one at a time, runtime shifts and all: 36-77 ms per 1e9 entries,
//      6 % of the HBM roofline, the slowest kernel of the product path.)
//   * the prefix of an entry is the smallest p with index[p] > i.  Thread 0 bisects the index for the first and the
//     last entry of the tile, the (few) index values in between are staged in LDS; a thread bisects there for its
//     first entry and steps on for the other three; a tile that spans more than DEC_IX buckets (sparse table)
//     bisects the global index per entry.
#define DEC_TILE  1024
#define DEC_EPT   4
#define DEC_IX    512
#define DEC_MAXPB 34                      // pbyte <= ceil(128/4) + 2 - 1

SMG_DEV int dec_bisect(const int64_t *__restrict__ index, int lo, int hi, int64_t i)
{ while (lo < hi)                         // smallest p in [lo, hi] with index[p] > i  (index[hi] > i)
    { const int m = (lo + hi) >> 1;
      if (index[m] <= i) lo = m + 1; else hi = m;
    }
  return lo;
}

// the little-endian dword at byte offset o of the staged bytes
SMG_DEV unsigned dec_u32(const unsigned *sraw, int o)
{ return __builtin_amdgcn_alignbyte(sraw[(o >> 2) + 1], sraw[o >> 2], (unsigned) (o & 3)); }

static inline size_t dec_lds_bytes(int pbyte) { return sizeof(unsigned) * (size_t) ((DEC_TILE * pbyte + 3) / 4 + 4); }

template <int W> __global__ void __launch_bounds__(TPB)
k_decode(const uint8_t *__restrict__ rec, const int64_t *__restrict__ index, int ixlen,
         int ibyte, int kbyte, int64_t n, int64_t ibase, u64 *__restrict__ keys,
         uint16_t *__restrict__ cnt)
{ // rec / keys / cnt are indexed by the LOCAL entry number 0..n-1; the prefix index by ibase + local
  // (a piece of a table that is decoded as it arrives, or a shard of a table that was cut for several GPUs,
  //  starts at entry ibase of the whole table)
  extern __shared__ unsigned sraw[];         // dec_lds_bytes(pbyte): the staged record bytes of a tile (+ slack)
  __shared__ int64_t  six[DEC_IX];
  __shared__ int      s_lo, s_hi;
  const int t = threadIdx.x;
  const int hbyte = kbyte - ibyte, pbyte = hbyte + 2;
  const int64_t i0 = (int64_t) blockIdx.x * DEC_TILE;
  const int64_t i1 = i0 + DEC_TILE < n ? i0 + DEC_TILE : n;
  // record bytes of [i0, i1): aligned dword loads around the (unaligned) byte range
  const int64_t b0 = i0 * pbyte, b1 = i1 * pbyte;
  const uintptr_t base = (uintptr_t) rec + (uintptr_t) b0;
  const uintptr_t abase = base & ~(uintptr_t) 3;
  const int skew = (int) (base - abase);
  const int ndw = (int) ((b1 - b0 + skew + 3) >> 2);
  const uintptr_t rbeg = (uintptr_t) rec, rend = (uintptr_t) rec + (uintptr_t) (n * pbyte);
  for (int w = t; w < ndw + 2; w += TPB)      // (+2: dec_u32 reads one dword past the last byte it needs)
    { const uintptr_t a = abase + 4 * (uintptr_t) w;
      unsigned v = 0;
      if (a >= rbeg && a + 4 <= rend) v = *reinterpret_cast<const unsigned *>(a);
      else                                  // first / last dword of the table: never touch bytes outside it
        for (int q = 0; q < 4; q++)
          if (a + q >= rbeg && a + q < rend) v |= (unsigned) *reinterpret_cast<const uint8_t *>(a + q) << (8 * q);
      sraw[w] = v;
    }
  if (t == 0)
    { s_lo = dec_bisect(index, 0, ixlen - 1, ibase + i0);
      s_hi = dec_bisect(index, 0, ixlen - 1, ibase + i1 - 1);
    }
  __syncthreads();
  const int lo = s_lo, hi = s_hi;
  const bool staged = hi - lo < DEC_IX;
  if (staged)
    for (int p = lo + t; p <= hi; p += TPB) six[p - lo] = index[p];
  __syncthreads();

  const int64_t e0 = i0 + (int64_t) DEC_EPT * t;
  if (e0 >= i1) return;
  int pa = 0;                                // position of the first entry's prefix in the staged slice
  if (staged)
    { int a = 0, b = hi - lo;
      while (a < b)
        { const int m = (a + b) >> 1;
          if (six[m] <= ibase + e0) a = m + 1; else b = m;
        }
      pa = a;
    }
  const int psh = 32 - 8 * ibyte;            // the prefix sits on top of the first dword
  u64 kw[DEC_EPT][W]; unsigned cw[DEC_EPT];
#pragma unroll
  for (int r = 0; r < DEC_EPT; r++)
    { const int64_t i = e0 + r;
      if (i >= i1) { for (int w = 0; w < W; w++) kw[r][w] = 0; cw[r] = 0; continue; }
      int p;
      if (staged) { while (six[pa] <= ibase + i) pa++; p = lo + pa; }      // (index[hi] > i1 - 1: the walk ends)
      else p = dec_bisect(index, lo, hi, ibase + i);
      const int o = (int) (i - i0) * pbyte + skew;
      unsigned D[2 * W];
#pragma unroll
      for (int j = 0; j < 2 * W; j++)
        { unsigned v = 0;
          if (4 * j < kbyte)
            { if (j == 0)
                { const unsigned sv = __builtin_bswap32(dec_u32(sraw, o));
                  v = ((unsigned) p << psh) | (sv >> (8 * ibyte));
                }
              else v = __builtin_bswap32(dec_u32(sraw, o + 4 * j - ibyte));
              const int over = 4 * j + 4 - kbyte;                         // bytes of this dword behind the k-mer
              if (over > 0) v &= ~0u << (8 * over);
            }
          D[j] = v;
        }
#pragma unroll
      for (int w = 0; w < W; w++) kw[r][w] = ((u64) D[2 * w] << 32) | D[2 * w + 1];
      cw[r] = dec_u32(sraw, o + hbyte) & 0xFFFFu;
    }
  const bool full = e0 + DEC_EPT <= i1 && (((uintptr_t) (keys + e0 * W)) & 15) == 0 && (((uintptr_t) (cnt + e0)) & 7) == 0;
  if (full)
    { if constexpr (W == 1)
        { ulonglong2 a, b; a.x = kw[0][0]; a.y = kw[1][0]; b.x = kw[2][0]; b.y = kw[3][0];
          *reinterpret_cast<ulonglong2 *>(keys + e0) = a;
          *reinterpret_cast<ulonglong2 *>(keys + e0 + 2) = b;
        }
      else
        {
#pragma unroll
          for (int r = 0; r < DEC_EPT; r++)
#pragma unroll
            for (int w = 0; w < W; w += 2)
              { if (w + 1 < W)
                  { ulonglong2 a; a.x = kw[r][w]; a.y = kw[r][w + 1];
                    *reinterpret_cast<ulonglong2 *>(keys + (e0 + r) * W + w) = a;
                  }
                else keys[(e0 + r) * W + w] = kw[r][w];
              }
        }
      *reinterpret_cast<ushort4 *>(cnt + e0) = make_ushort4((unsigned short) cw[0], (unsigned short) cw[1],
                                                            (unsigned short) cw[2], (unsigned short) cw[3]);
    }
  else
    for (int r = 0; r < DEC_EPT; r++)
      if (e0 + r < i1)
        { for (int w = 0; w < W; w++) keys[(e0 + r) * W + w] = kw[r][w];
          cnt[e0 + r] = (uint16_t) cw[r];
        }
}

// the engine's own table for `nels` entries of a format-F table (allocated, not filled yet)
static int decode_begin(smg_engine *e, int kmer, int ibyte, int64_t nels, char *errbuf, size_t errlen)
{ if (!e) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");
  if (ibyte < 1 || ibyte > 3) return fail(errbuf, errlen, SMG_EINVAL, "ibyte must be 1, 2 or 3%s");
  HIPCHK(hipSetDevice(e->device));
  int rc = set_table(e, kmer, nels, errbuf, errlen);
  if (rc) return rc;
  const int kbyte = (kmer + 3) >> 2;
  if (kbyte <= ibyte) return fail(errbuf, errlen, SMG_EINVAL, "k-mer shorter than the index prefix%s");
  e->own_keys.reset(); e->own_cnt.reset();
  HIPCHK(e->own_keys.alloc(sizeof(u64) * (size_t) (nels > 0 ? nels : 1) * e->tab.W));
  HIPCHK(e->own_cnt.alloc(sizeof(uint16_t) * (size_t) (nels > 0 ? nels : 1) + 16));
  e->tab.keys = e->own_keys; e->tab.cnt = e->own_cnt;
  return SMG_OK;
}

// decode `nent` records at d_records into the entries [first, first + nent) of the engine's table; the first of them is
// entry ibase + first of the whole table (whose prefix index is d_prefix_index).  Queued on `stream`.
static int decode_piece(smg_engine *e, hipStream_t stream, int ibyte, const uint8_t *d_records, const int64_t *d_prefix_index,
                        int64_t ibase, int64_t first, int64_t nent)
{ if (nent <= 0) return 0;
  const int kbyte = (e->tab.kmer + 3) >> 2;
  const unsigned nblk = (unsigned) ((nent + DEC_TILE - 1) / DEC_TILE);
  with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(k_decode<w()>, dim3(nblk), dim3(TPB), dec_lds_bytes(kbyte + 2 - ibyte), stream, d_records,
      d_prefix_index, 1 << (8 * ibyte), ibyte, kbyte, nent, ibase + first, e->own_keys + first * e->tab.W, e->own_cnt + first); });
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

static int decode_at(smg_engine *e, int kmer, int ibyte, int64_t nels, int64_t ibase, const uint8_t *d_records,
                     const int64_t *d_prefix_index, char *errbuf, size_t errlen)
{ int rc = decode_begin(e, kmer, ibyte, nels, errbuf, errlen);
  if (rc) return rc;
  hipEventRecord(e->ev[EV_DECODE_BEG], e->stream);
  if (decode_piece(e, e->stream, ibyte, d_records, d_prefix_index, ibase, 0, nels))
    return fail(errbuf, errlen, SMG_ENODEV, "decode launch failed%s");
  hipEventRecord(e->ev[EV_DECODE_END], e->stream);
  HIPCHK(hipStreamSynchronize(e->stream));
  e->st.ms_decode = ms_between(e, EV_DECODE_BEG, EV_DECODE_END);
  return SMG_OK;
}

// ingest hook: decode a piece behind its copy (smg_ingest.hpp)
struct DecodeHook { smg_engine *e; const int64_t *d_index; int ibyte; int64_t ibase; };
static int decode_hook(void *ctx, hipStream_t stream, const uint8_t *d_piece, int64_t first, int64_t nent)
{ DecodeHook *h = (DecodeHook *) ctx;
  return decode_piece(h->e, stream, h->ibyte, d_piece, h->d_index, h->ibase, first, nent);
}

extern "C" int smg_engine_decode(smg_engine *e, int kmer, int ibyte, int64_t nels,
                                 const uint8_t *d_records, const int64_t *d_prefix_index,
                                 char *errbuf, size_t errlen)
{ return decode_at(e, kmer, ibyte, nels, 0, d_records, d_prefix_index, errbuf, errlen); }

// the same for a shard: d_records holds the entries first_entry .. first_entry + nels - 1 of the table the index belongs to
extern "C" int smg_engine_decode_at(smg_engine *e, int kmer, int ibyte, int64_t nels, int64_t first_entry,
                                    const uint8_t *d_records, const int64_t *d_prefix_index,
                                    char *errbuf, size_t errlen)
{ if (first_entry < 0) return fail(errbuf, errlen, SMG_EINVAL, "decode: first_entry must not be negative%s");
  return decode_at(e, kmer, ibyte, nels, first_entry, d_records, d_prefix_index, errbuf, errlen);
}

// ---- the table's own prefix index as look-up directory -------------------------------------------------------------
// A FastK table carries the number of entries up to every 3-byte prefix (libfastk.c:841, `index[p]` = entries whose first
// ibyte bytes are <= p).  With ibyte = 3 that IS a bucket directory over the leading 24 k-mer bits (bucket = hi32 >> 8;
// ~150 entries per bucket at 2.5e9 entries): ixdir[b] = first entry of bucket b relative to this shard, ixdir[2^24] = n.
// Pass 1 then writes no directory at all (round 3: a shift, a compare and a rare store per entry, and 130 MB cleared per
// run); the few million look-ups that survive the request filter bisect one or two steps longer.
#define IXDIR_BITS 24
__global__ void __launch_bounds__(TPB)
k_index_dir(const int64_t *__restrict__ index, int64_t ibase, int64_t n, uint32_t *__restrict__ out)
{ const int64_t b = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (b > (1ll << IXDIR_BITS)) return;
  int64_t v = (b ? index[b - 1] : 0) - ibase;
  if (b == (1ll << IXDIR_BITS)) v = n;
  out[b] = (uint32_t) (v < 0 ? 0 : v > n ? n : v);
}

extern "C" int smg_engine_set_prefix_index(smg_engine *e, const int64_t *d_prefix_index, int ibyte, int64_t first_entry,
                                           char *errbuf, size_t errlen)
{ if (!e) return fail(errbuf, errlen, SMG_EINVAL, "null engine%s");
  if (ibyte < 1 || ibyte > 3 || !d_prefix_index) return fail(errbuf, errlen, SMG_EINVAL, "prefix index: ibyte must be 1, 2 or 3%s");
  e->tab.have_ixdir = false;
  if (ibyte != 3 || e->tab.kmer < 12 || test_hook("SMG_NO_INDEX_DIR")) return SMG_OK;     // (a coarser index is of no use as a directory)
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(e->ixdir.reserve((int64_t) sizeof(uint32_t) * ((1ll << IXDIR_BITS) + 2)));
  hipLaunchKernelGGL(k_index_dir, dim3((unsigned) (((1ll << IXDIR_BITS) + 1 + TPB - 1) / TPB)), dim3(TPB), 0, e->stream,
                     d_prefix_index, first_entry, e->tab.n, e->ixdir);
  HIPCHK(hipGetLastError());
  e->tab.have_ixdir = true;
  return SMG_OK;
}
