// smg_gzip.hpp -- plain gzip (RFC 1952: what gzip, pigz and a sequencer write) in front of the k-mer counter, inflated in
// parallel on an MI355X (gfx950, wave64).  A gzip member is one DEFLATE stream: nothing in its framing says where a second
// wavefront could start, and a block may copy from the 32 KiB of text in front of it.  What makes it parallel:
//   the block finder   in the compressed bits [lo, hi) of a span, the first offset at which a non-final dynamic block can
//                      start: BFINAL 0, BTYPE 2, HLIT and HDIST <= 29, a complete code-length code (gz_filter: 64 offsets
//                      a step, one per lane), then both sets of code lengths decode and build, with a code for symbol 256
//                      (gz_block_start: the survivors, one after the other, with the tables of the wave)
//   the marker decoder the symbol loop of smg_inflate.hpp (inf_block) from such an offset with no text in front of it: it
//                      keeps the last 32 Ki symbols as 16-bit values, 0 .. 255 a byte, 0x8000 + j "byte j of the 32 KiB in
//                      front of my start", and otherwise only counts; it notes a checkpoint (bit offset, text offset, a copy
//                      of the ring) at the block boundaries where the text since the last one reached check_text bytes
//   the resolver       the markers of a saved ring through the window in front of the decode that wrote it -> 32 KiB of text
//   the exact decoder  inflate_member's loop through a WaveIo from a bit offset to a bit offset, its window preloaded, to
//                      text and to the CRC-32 register of the piece; the registers of a member are combined with x^(8n)
// and the chain that ties them (gz_build, host): the spans of a piece are decoded speculatively, then walked in order; a
// span whose candidate is where the decode in front of it ended is linked, anything else is repaired by a decode from
// that end with the window that is known by then, until it meets the candidate of a later span.  Only linked and repaired
// results enter the index, so the index is exact for every valid file; how much was linked changes the time alone.  The
// first pass stores no text: no buffer depends on the compression ratio.  The second pass (gz_feed) runs the exact
// decoder over the restart points of the index.
//
// One text for host and device, as smg_inflate.hpp whose rule heads this file too: for ANY bytes every read is checked
// against the end of the piece first and every loop consumes at least one bit.  A decode from a false candidate gives
// garbage and still stops, with a status or at the end of the compressed bytes.  `gzip_check` runs all of it on the host as
// one lane against zlib under the sanitizers; GzHostEngine is that twin, GzEngine what the device implements
// (smg_count_inflater.hpp).

#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <vector>

#include "smg_count.h"
#include "smg_count_err.hpp"
#include "smg_inflate.hpp"

#define GZ_NONE         (~0ull)
#define GZ_MARK         0x8000u                                // ring symbol: byte (s & 0x7fff) of the window in front of the start
#define GZ_POISON       0x4000u                                // ring symbol: a byte in front of the start of the member
#define GZ_SPAN         (256u << 10)                           // compressed bytes of a span
#define GZ_MIN_SPAN     (1u << 10)
#define GZ_MAX_SPAN     (1u << 20)
#define GZ_MAX_SPANS    256                                    // spans of a piece
#define GZ_MAX_PIECE    ((size_t) 64 << 20)                    // compressed bytes of a piece
#define GZ_CHECK_TEXT   (256u << 10)                           // text bytes between two checkpoints (at most 16 spans' worth of bytes)
#define GZ_QUOTA        8                                      // ring slots of a speculative decode: 7 checkpoints and its end
#define GZ_REPAIR_QUOTA 64                                     // ring slots of a repair
#define GZ_SLOTS        (GZ_MAX_SPANS * GZ_QUOTA + GZ_REPAIR_QUOTA)
#define GZ_MAX_EXACT    4096                                   // restart intervals of one launch of the exact decoder

// one decode of the first pass; bits count from the start of the piece
struct GzTask
{ uint64_t lo, hi;                                             // find: the first candidate in [lo, hi); else: start at lo (GZ_NONE: nothing to do)
  uint64_t stop;                                               // end at the first block boundary at or past this bit ..
  const uint8_t *win;                                          // known: the 32 KiB in front of lo (null where avail is 0)
  uint32_t find, match;                                        // .. match: that is the candidate of the span it lies in
  uint32_t known, avail;                                       // the window is known, its last `avail` bytes belong to the member
  uint32_t max_blocks;                                         // end after this many blocks (0: no such limit)
  uint32_t slot0, nslots;                                      // its ring slots: checkpoints, then its end
};

struct GzResult
{ uint64_t start, end, text;                                   // from this bit to this block boundary: so many bytes of text
  uint64_t bad, bad_at;                                        // status != 0: the block that failed began at `bad`, the failure was at `bad_at`
  uint32_t status, last;                                       // INF_*; it ended behind a final block
  uint32_t blocks, ncheck;                                     // blocks decoded without a failure; checkpoints written
};

struct GzCheck { uint64_t bit, text; };                        // a checkpoint: this boundary, after so many bytes of the decode

// a restart interval for the exact decoder; bits count from the start of the chunk
struct GzExact { uint64_t bit, end; const uint8_t *win; uint32_t out_off, len; };

INF_HD uint64_t gz_ballot(const HostWave &, bool p) { return p ? 1ull : 0ull; }
#if defined(__HIPCC__)
__device__ __forceinline__ uint64_t gz_ballot(const DevWave &, bool p) { return __ballot(p); }
#endif

// ---------------------------------------------------------------------------------------------------------------
//  the block finder
// ---------------------------------------------------------------------------------------------------------------

// at least 57 bits from `bit` on, zeros behind the end
INF_HD uint64_t gz_bits(const uint8_t *in, uint32_t clen, uint64_t bit)
{ const uint32_t p = (uint32_t) (bit >> 3);
  uint64_t v = 0;
  for (uint32_t j = 0; j < 8; j++)
    if (p + j < clen) v |= (uint64_t) in[p + j] << (8 * j);
  return v >> (bit & 7u);
}

// what a lane can say about an offset on its own: the 17 header bits and the Kraft sum of the code-length code
INF_HD bool gz_filter(const uint8_t *in, uint32_t clen, uint64_t bit)
{ const uint64_t nbits = 8ull * clen;
  if (bit + 17 > nbits) return false;
  uint64_t v = gz_bits(in, clen, bit);
  if ((v & 7u) != 4u) return false;                            // BFINAL 0, BTYPE 2
  if (((v >> 3) & 31u) > 29u || ((v >> 8) & 31u) > 29u) return false;
  const uint32_t hclen = (uint32_t) ((v >> 13) & 15u) + 4u;
  if (bit + 17 + 3 * hclen > nbits) return false;
  v = gz_bits(in, clen, bit + 17);
  uint32_t sum = 0;
  for (uint32_t i = 0; i < hclen; i++, v >>= 3)
    if (v & 7u) sum += 128u >> (v & 7u);
  return sum == 128u;
}

// input straight from memory, for the finder, whose offsets jump
template <class Wave> struct GzDirectIo
{ const uint8_t *in; uint32_t clen; Wave wv;
  INF_HD int lane() const { return wv.lane(); }
  INF_HD int lanes() const { return wv.lanes(); }
  INF_HD void sync() { wv.sync(); }
  INF_HD uint8_t in1(uint32_t i) const { return in[i]; }
  INF_HD uint32_t in4(uint32_t i) const { return (uint32_t) in[i] | (uint32_t) in[i + 1] << 8 | (uint32_t) in[i + 2] << 16 | (uint32_t) in[i + 3] << 24; }
};

// the full check of an offset that passed the filter: the header of a dynamic block, and both tables build
template <class Io> INF_HD bool gz_block_start(Io &io, const InfTables &t, uint64_t bit)
{ InfBits b{ 0, 0, (uint32_t) (bit >> 3) };
  uint32_t v;
  int nlit = 0, ndist = 0;
  inf_refill(io, b);
  if (!inf_take(b, (int) (bit & 7u) + 3, &v)) return false;
  if (inf_dynamic(io, b, t, &nlit, &ndist) != INF_OK) return false;
  if (inf_build(io, t.lens, nlit, t.lit, INF_LIT_BITS, t.sorted, t.cnt, t.work, 1) != INF_OK) return false;
  return inf_build(io, t.lens + nlit, ndist, t.dist, INF_DIST_BITS, t.sorted + INF_NLIT, t.cnt + 16, t.work, 2) == INF_OK;
}

// the first candidate in [lo, hi), or GZ_NONE: lanes() neighbouring offsets through the filter at once
template <class Io> INF_HD uint64_t gz_find(Io &io, const InfTables &t, uint64_t lo, uint64_t hi)
{ for (uint64_t base = lo; base < hi; base += (uint64_t) io.lanes())
    { const uint64_t bit = base + (uint64_t) io.lane();
      uint64_t m = gz_ballot(io.wv, bit < hi && gz_filter(io.in, io.clen, bit));
      while (m)
        { const uint64_t at = base + (uint64_t) __builtin_ctzll(m);
          m &= m - 1;
          if (gz_block_start(io, t, at)) return at;
        }
    }
  return GZ_NONE;
}

// ---------------------------------------------------------------------------------------------------------------
//  the marker decoder
// ---------------------------------------------------------------------------------------------------------------

// the accessor of inf_block that keeps the last 32 Ki symbols and no text: position p at sym[p % INF_WINDOW]; the payload
// staged through a ring as WaveIo stages it
template <class Wave> struct GzMarkIo
{ const uint8_t *in; uint32_t clen; uint64_t isize;
  uint16_t *sym; uint8_t *ring;
  uint32_t staged;
  Wave wv;

  INF_HD int lane() const { return wv.lane(); }
  INF_HD int lanes() const { return wv.lanes(); }
  INF_HD void sync() { wv.sync(); }
  INF_HD void stage(uint32_t ip)
  { const uint32_t room = INF_RING - (staged - ip), rest = clen - staged, m = room < rest ? room : rest;
    wv.sync();
    for (uint32_t j = (uint32_t) wv.lane(); j < m; j += (uint32_t) wv.lanes()) ring[(staged + j) & (INF_RING - 1)] = in[staged + j];
    staged += m;
    wv.sync();
  }
  INF_HD uint8_t in1(uint32_t i)
  { if (i >= staged) stage(i);
    return ring[i & (INF_RING - 1)];
  }
  INF_HD uint32_t in4(uint32_t i)
  { if (i + 4 > staged) stage(i);
    const uint32_t b0 = ring[i & (INF_RING - 1)], b1 = ring[(i + 1) & (INF_RING - 1)], b2 = ring[(i + 2) & (INF_RING - 1)],
                   b3 = ring[(i + 3) & (INF_RING - 1)];
    return b0 | b1 << 8 | b2 << 16 | b3 << 24;
  }
  INF_HD void lit(uint64_t pos, uint8_t c) { if (wv.lane() == 0) sym[pos & (INF_WINDOW - 1)] = c; }
  // (the order of reads and writes is that of WaveIo::match)
  INF_HD void match(uint64_t pos, uint32_t dist, uint32_t len)
  { wv.sync();
    const uint64_t from = pos - dist;
    for (uint32_t i = (uint32_t) wv.lane(); i < len; i += (uint32_t) wv.lanes())
      { const uint16_t c = sym[(from + (dist >= len ? i : i % dist)) & (INF_WINDOW - 1)];
        sym[(pos + i) & (INF_WINDOW - 1)] = c;
      }
  }
  INF_HD void stored(uint64_t pos, uint32_t i, uint32_t len)
  { wv.sync();
    for (uint32_t j = (uint32_t) wv.lane(); j < len; j += (uint32_t) wv.lanes()) sym[(pos + j) & (INF_WINDOW - 1)] = in[i + j];
    if (i + len > staged) staged = i + len;                    // (the ring holds nothing of what was passed over)
  }
};

template <class Wave> INF_HD void gz_copy_ring(const Wave &wv, const uint16_t *sym, uint16_t *to)
{ wv.sync();
  for (uint32_t j = (uint32_t) wv.lane(); j < INF_WINDOW / 2; j += (uint32_t) wv.lanes()) ((uint32_t *) to)[j] = ((const uint32_t *) sym)[j];
}

// Task k over the piece in[0 .. clen): result, checkpoints (check[0 .. ncheck)) and rings (rings[c * INF_WINDOW ..], the end
// behind the checkpoints; none after a failure).  spec[s].start: the candidate of span s, for a task that must match one.
// The text position starts at INF_WINDOW, so that no distance reaches below 0: what lies in front is in the ring, as
// markers, as the known bytes, or as poison where the member began less than 32 KiB ago.
template <class Wave>
INF_HD void gz_marker(Wave wv, const uint8_t *in, uint32_t clen, const GzTask &k, const GzResult *spec, uint32_t nspec, uint32_t span_bytes,
                      uint32_t check_text, const InfTables &t, uint16_t *sym, uint8_t *stage, uint16_t *rings, GzCheck *check, GzResult *res)
{ GzResult r{ GZ_NONE, 0, 0, 0, 0, INF_OK, 0, 0, 0 };
  uint64_t start = k.lo;
  if (k.find)
    { GzDirectIo<Wave> fio{ in, clen, wv };
      start = gz_find(fio, t, k.lo, k.hi);
    }
  if (start == GZ_NONE || (start >> 3) > clen)
    { if (wv.lane() == 0) *res = r;
      return;
    }
  wv.sync();
  for (uint32_t j = (uint32_t) wv.lane(); j < INF_WINDOW; j += (uint32_t) wv.lanes())
    sym[j] = (uint16_t) (!k.known ? GZ_MARK + j : j >= INF_WINDOW - k.avail ? k.win[j] : GZ_POISON);
  wv.sync();
  GzMarkIo<Wave> io{ in, clen, ~0ull, sym, stage, (uint32_t) (start >> 3), wv };
  InfBits b{ 0, 0, (uint32_t) (start >> 3) };
  uint64_t pos = INF_WINDOW, checked = 0;
  uint32_t v, last = 0;
  r.start = r.end = start;
  inf_refill(io, b);
  if (!inf_take(b, (int) (start & 7u), &v)) { r.status = INF_EXHAUSTED; r.bad = r.bad_at = start; }
  while (r.status == INF_OK)
    { const uint64_t blk = 8ull * b.ip - (uint64_t) b.cnt;
      const int s = inf_block(io, t, b, pos, &last);
      const uint64_t at = 8ull * b.ip - (uint64_t) b.cnt;
      if (s != INF_OK) { r.status = (uint32_t) s; r.bad = blk; r.bad_at = at; break; }
      r.end = at; r.text = pos - INF_WINDOW; r.blocks++;
      if (last) { r.last = 1; break; }
      if (k.max_blocks && r.blocks >= k.max_blocks) break;
      if (at >= k.stop)
        { if (!k.match) break;
          const uint64_t sp = (at >> 3) / span_bytes;
          if (sp < nspec && spec[sp].start == at) break;
        }
      if (r.text - checked >= check_text)
        { if (r.ncheck + 1 >= k.nslots) break;                   // the last slot is that of the end
          gz_copy_ring(wv, sym, rings + (size_t) r.ncheck * INF_WINDOW);
          if (wv.lane() == 0) check[r.ncheck] = GzCheck{ at, r.text };
          r.ncheck++; checked = r.text;
        }
    }
  if (r.status == INF_OK) gz_copy_ring(wv, sym, rings + (size_t) r.ncheck * INF_WINDOW);
  if (wv.lane() == 0) *res = r;
}

// ---------------------------------------------------------------------------------------------------------------
//  the resolver and the exact decoder
// ---------------------------------------------------------------------------------------------------------------

// The window behind `text` bytes of a decode from its ring: byte j of it is the symbol at ring[(text + j) % INF_WINDOW],
// a marker through `prev`, the window in front of that decode, of which the last prev_avail bytes belong to the member.
// true: a symbol of this lane reaches in front of the member
INF_HD bool gz_resolve(int lane, int lanes, const uint16_t *ring, uint64_t text, const uint8_t *prev, uint32_t prev_avail, uint8_t *dst)
{ const uint32_t avail = text >= INF_WINDOW - prev_avail ? INF_WINDOW : prev_avail + (uint32_t) text;     // of dst: the rest of it is no text
  bool bad = false;
  for (uint32_t j = (uint32_t) lane; j < INF_WINDOW; j += (uint32_t) lanes)
    { const uint32_t s = ring[(text + j) & (INF_WINDOW - 1)];
      uint8_t c = (uint8_t) s;
      if (j < INF_WINDOW - avail) c = 0;
      else if (s & GZ_MARK)
        { const uint32_t q = s & (GZ_MARK - 1u);
          if (q < INF_WINDOW - prev_avail) { bad = true; c = 0; }
          else c = prev[q];
        }
      else if (s & GZ_POISON) { bad = true; c = 0; }
      dst[j] = c;
    }
  return bad;
}

// Interval p of the chunk in[0 .. clen): exactly p.len bytes of text at text[p.out_off ..] and their CRC-32, from p.bit to
// the block boundary p.end.  win, ring: INF_WINDOW and INF_RING bytes of the wave.  The text position starts at INF_WINDOW
// with the window in front of it, so WaveIo's `out` is biased by as much; nothing below text[p.out_off] is touched, the
// flushes begin at INF_WINDOW.
template <class Wave>
INF_HD int gz_exact(Wave wv, const uint8_t *in, uint32_t clen, const GzExact &p, uint8_t *text, const InfTables &t, uint8_t *win, uint8_t *ring,
                    uint32_t *crc)
{ if ((p.bit >> 3) > clen) return INF_EXHAUSTED;
  wv.sync();
  for (uint32_t j = (uint32_t) wv.lane(); j < INF_WINDOW; j += (uint32_t) wv.lanes()) win[j] = p.win ? p.win[j] : (uint8_t) 0;
  wv.sync();
  const uintptr_t biased = (uintptr_t) text + p.out_off - INF_WINDOW;
  WaveIo<Wave> io{ in, clen, (uint8_t *) biased, INF_WINDOW + p.len, 0u, win, ring, (uint32_t) (p.bit >> 3), INF_WINDOW, 0xffffffffu, wv };
  InfBits b{ 0, 0, (uint32_t) (p.bit >> 3) };
  uint32_t pos = INF_WINDOW, v, last = 0;
  inf_refill(io, b);
  if (!inf_take(b, (int) (p.bit & 7u), &v)) return INF_EXHAUSTED;
  for (;;)
    { const uint64_t at = 8ull * b.ip - (uint64_t) b.cnt;
      if (at == p.end) break;
      if (at > p.end || last) return INF_LEFT_OVER;
      INF_TRY(inf_block(io, t, b, pos, &last));
    }
  if (pos != io.isize) return INF_TOO_SHORT;
  *crc = io.finish(pos);
  return INF_OK;
}

// the CRC-32 of A B from those of A and of B and the length of B
INF_HD uint32_t gz_crc_join(uint32_t a, uint32_t b, uint64_t nb)
{ uint32_t x = 0x80000000u;
  for (; nb; nb -= nb < 0x40000000u ? nb : 0x40000000u) x = crc_mul(x, crc_xpow8((uint32_t) (nb < 0x40000000u ? nb : 0x40000000u)));
  return crc_mul(a, x) ^ b;
}

// ---------------------------------------------------------------------------------------------------------------
//  the device: the kernels
// ---------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

// task b of the launch, one wave: the ring of symbols (64 KiB), the payload ring and the tables in LDS, two waves a CU
__global__ void __launch_bounds__(64) gz_marker_k(const uint8_t *__restrict__ piece, uint32_t clen, const GzTask *__restrict__ tasks, int n,
                                                  const GzResult *spec, uint32_t nspec, uint32_t span_bytes, uint32_t check_text,
                                                  uint16_t *__restrict__ rings, GzCheck *__restrict__ check, GzResult *res)
{ __shared__ __attribute__((aligned(16))) uint16_t sym[INF_WINDOW];
  __shared__ __attribute__((aligned(16))) uint8_t stage[INF_RING];
  __shared__ uint16_t lit[1 << INF_LIT_BITS], dist[1 << INF_DIST_BITS], sorted[INF_NLIT + INF_NDIST], cnt[32], work[32];
  __shared__ uint8_t lens[INF_NLIT + INF_NDIST];
  const int b = (int) blockIdx.x;
  if (b >= n) return;
  const GzTask k = tasks[b];
  if (k.nslots < 1 || (size_t) k.slot0 + k.nslots > GZ_SLOTS) return;
  gz_marker(DevWave{ (int) threadIdx.x }, piece, clen, k, spec, nspec, span_bytes, check_text, InfTables{ lit, dist, sorted, cnt, work, lens }, sym, stage,
            rings + (size_t) k.slot0 * INF_WINDOW, check + k.slot0, res + b);
}

// ring slot0 + c of a decode, c = blockIdx.x <= ncheck (the last: its end, behind end_text bytes) -> window dst + c * INF_WINDOW
__global__ void __launch_bounds__(256) gz_resolve_k(const uint16_t *__restrict__ rings, const GzCheck *__restrict__ check, uint32_t slot0, uint32_t ncheck,
                                                    uint64_t end_text, const uint8_t *prev, uint32_t prev_avail, uint8_t *dst, uint32_t *bad)
{ const uint32_t c = blockIdx.x;
  if (c > ncheck || slot0 + c >= GZ_SLOTS) return;
  const uint64_t text = c < ncheck ? check[slot0 + c].text : end_text;
  if (gz_resolve((int) threadIdx.x, 256, rings + (size_t) (slot0 + c) * INF_WINDOW, text, prev, prev_avail, dst + (size_t) c * INF_WINDOW)) atomicOr(bad, 1u);
}

// interval b of the launch, one wave, the LDS of inf_members
__global__ void __launch_bounds__(64) gz_exact_k(const uint8_t *__restrict__ chunk, uint32_t clen, const GzExact *__restrict__ iv, int n,
                                                 uint8_t *__restrict__ text, uint32_t text_n, uint32_t *__restrict__ crc, uint32_t *__restrict__ status)
{ __shared__ __attribute__((aligned(16))) uint8_t win[INF_WINDOW];
  __shared__ __attribute__((aligned(16))) uint8_t ring[INF_RING];
  __shared__ uint16_t lit[1 << INF_LIT_BITS], dist[1 << INF_DIST_BITS], sorted[INF_NLIT + INF_NDIST], cnt[32], work[32];
  __shared__ uint8_t lens[INF_NLIT + INF_NDIST];
  const int b = (int) blockIdx.x;
  if (b >= n) return;
  const GzExact p = iv[b];
  uint32_t c = 0;
  int s = INF_TOO_LONG;
  if ((uint64_t) p.out_off + p.len <= text_n)
    s = gz_exact(DevWave{ (int) threadIdx.x }, chunk, clen, p, text, InfTables{ lit, dist, sorted, cnt, work, lens }, win, ring, &c);
  if (threadIdx.x == 0) { status[b] = (uint32_t) s; crc[b] = c; }
}

#endif

// ---------------------------------------------------------------------------------------------------------------
//  the host: framing, the chain, the index, the second pass
// ---------------------------------------------------------------------------------------------------------------

// What runs the four steps: the device (DeviceGzEngine, smg_count_inflater.hpp) or one lane of the host (GzHostEngine).  The
// chain and the second pass are the same text over either.  Windows are numbered; those of one decode are neighbours.
struct GzEngine
{ uint32_t span = GZ_SPAN, check_text = GZ_CHECK_TEXT;
  double ms[3] = { 0, 0, 0 };                                  // finder + marker decoder, resolver, exact decoder: of all files so far
  char *errbuf = nullptr; size_t errlen = 0;                   // where a failing step leaves its message (set by gz_build and gz_feed)
  virtual uint8_t *piece_buf(size_t n) = 0;                    // room for the n compressed bytes of the next piece (or chunk)
  virtual int piece(size_t n) = 0;                             // they are there: the launches from now on read them
  // tasks [0, n): results and checkpoints (check[task * quota + c]); spec: the speculative launch of a piece, whose results
  // later tasks match against
  virtual int marker(const GzTask *tasks, int n, bool spec, GzResult *res, GzCheck *check) = 0;
  virtual int64_t windows(int n) = 0;                          // n new neighbouring windows: the number of the first, < 0: no memory
  virtual uint8_t *window(int64_t w) = 0;
  virtual int resolve(uint32_t slot0, uint32_t ncheck, uint64_t end_text, int64_t prev, uint32_t prev_avail, int64_t dst) = 0;
  virtual int resolved(bool *bad) = 0;                         // all of it is done: did a distance reach in front of a member?
  // the chunk of piece(n): text_n bytes of text (valid until the next call), the CRC-32 and status of every interval
  virtual int exact(const GzExact *iv, int n, size_t text_n, const uint8_t **text, uint32_t *crc, uint32_t *status) = 0;
  virtual void reset() = 0;                                    // the windows and what is left of an earlier file are forgotten
  virtual ~GzEngine() {}
  void set_span(uint32_t s)
  { span = s;
    check_text = 16 * s < GZ_CHECK_TEXT ? 16 * s : GZ_CHECK_TEXT;
  }
  size_t piece_cap() const
  { const size_t c = (size_t) span * GZ_MAX_SPANS;
    return c < GZ_MAX_PIECE ? c : GZ_MAX_PIECE;
  }
};

struct GzPoint { uint64_t bit, text; int64_t win; uint32_t member; };       // a restart point: file bit, text byte, its window (< 0: none)
struct GzMember { int64_t off; uint64_t end_bit, text0, text; uint32_t crc, isize; };
struct GzIndex
{ std::vector<GzPoint> pts;
  std::vector<GzMember> mem;
  int64_t text = 0, spans = 0, linked = 0, repaired = 0;
  double ms[3] = { 0, 0, 0 };                                  // what the engine spent on this file
  void clear() { pts.clear(); mem.clear(); text = spans = linked = repaired = 0; ms[0] = ms[1] = ms[2] = 0; }
};

// the span size of a call: its argument, else the test hook SMG_COUNT_GZIP_SPAN, else GZ_SPAN
static inline int gz_span(int64_t arg, uint32_t *span, char *errbuf, size_t errlen)
{ int64_t s = arg;
  if (s == 0) { const char *h = getenv("SMG_COUNT_GZIP_SPAN"); s = h ? atoll(h) : (int64_t) GZ_SPAN; }
  if (s < (int64_t) GZ_MIN_SPAN || s > (int64_t) GZ_MAX_SPAN)
    return fail(errbuf, errlen, SMG_EINVAL, "a gzip span of %lld bytes is out of range %u .. %u", (long long) s, GZ_MIN_SPAN, GZ_MAX_SPAN);
  *span = (uint32_t) s;
  return 0;
}

static inline int gz_bad_member(char *errbuf, size_t errlen, const char *path, int64_t off, const char *why)
{ return fail(errbuf, errlen, SMG_EFORMAT, "%s: gzip member at offset %lld: %s", path, (long long) off, why); }
static inline int gz_bad_block(char *errbuf, size_t errlen, const char *path, int64_t off, const char *why)
{ return fail(errbuf, errlen, SMG_EFORMAT, "%s: deflate block at offset %lld: %s", path, (long long) off, why); }

// The header of a member in p[0 .. avail): 0 and *hlen its bytes, 1 and *why, 2 more bytes are needed.  CM 8 only; the
// fields FEXTRA, FNAME, FCOMMENT and FHCRC (checked) are passed over.
static inline int gz_member_header(const uint8_t *p, size_t avail, size_t *hlen, const char **why)
{ if (avail >= 1 && p[0] != 31) { *why = "not a gzip header"; return 1; }
  if (avail >= 2 && p[1] != 139) { *why = "not a gzip header"; return 1; }
  if (avail >= 3 && p[2] != 8) { *why = "the compression method is not 8 (deflate)"; return 1; }
  if (avail >= 4 && (p[3] & 0xe0)) { *why = "reserved flag bits are set"; return 1; }
  if (avail < 10) return 2;
  const int flg = p[3];
  size_t q = 10;
  if (flg & 4)
    { if (q + 2 > avail) return 2;
      q += 2 + ((size_t) p[q] | (size_t) p[q + 1] << 8);
      if (q > avail) return 2;
    }
  for (int f = 8; f <= 16; f <<= 1)
    if (flg & f)
      for (;;)
        { if (q >= avail) return 2;
          if (p[q++] == 0) break;
        }
  if (flg & 2)
    { if (q + 2 > avail) return 2;
      uint32_t r = 0xffffffffu;
      for (size_t i = 0; i < q; i++) r = crc_byte(r, p[i]);
      r ^= 0xffffffffu;
      if ((r & 0xffffu) != ((uint32_t) p[q] | (uint32_t) p[q + 1] << 8)) { *why = "the CRC-16 of the header does not match"; return 1; }
      q += 2;
    }
  *hlen = q;
  return 0;
}

static inline int gz_pread(int fd, uint8_t *buf, size_t n, int64_t off, const char *path, char *errbuf, size_t errlen)
{ size_t got = 0;
  while (got < n)
    { const ssize_t r = pread(fd, buf + got, n - got, off + (int64_t) got);
      if (r < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
      if (r == 0) return fail(errbuf, errlen, SMG_EFORMAT, "%s changed while it was read", path);
      got += (size_t) r;
    }
  return 0;
}

// are the bytes of the file from `off` on all zero?
static inline int gz_zeros(int fd, int64_t off, int64_t fsize, const char *path, bool *zeros, char *errbuf, size_t errlen)
{ std::vector<uint8_t> buf((size_t) 1 << 16);
  *zeros = true;
  while (off < fsize && *zeros)
    { const size_t n = (size_t) (fsize - off < (int64_t) buf.size() ? fsize - off : (int64_t) buf.size());
      const int rc = gz_pread(fd, buf.data(), n, off, path, errbuf, errlen);
      if (rc) return rc;
      for (size_t i = 0; i < n; i++) if (buf[i]) *zeros = false;
      off += (int64_t) n;
    }
  return 0;
}

// The first pass over one gzip file: the index of its restart points and members, its text bytes exactly.
struct GzChain
{ GzEngine &e;
  GzIndex &ix;
  int fd; const char *path; int64_t fsize;
  char *errbuf; size_t errlen;
  enum { HEADER, BLOCKS, TRAILER } state = HEADER;
  int64_t at = 0;                                              // HEADER, TRAILER: the file byte they stand at
  uint64_t pos = 0;                                            // BLOCKS: the block boundary, a file bit
  int64_t cur_win = -1;                                        // the window in front of pos
  uint32_t avail = 0;
  uint64_t mtext = 0;                                          // text of the member so far
  std::vector<GzTask> tasks;
  std::vector<GzResult> spec;
  std::vector<GzCheck> spec_check, rep_check;

  GzChain(GzEngine &en, GzIndex &index, int f, const char *p, int64_t size, char *eb, size_t el)
    : e(en), ix(index), fd(f), path(p), fsize(size), errbuf(eb), errlen(el) {}

  // a linked or repaired result enters the index: its start and its checkpoints are restart points, its rings windows
  int accept(const GzResult &r, const GzCheck *check, uint32_t slot0, int64_t p0)
  { const int64_t w0 = e.windows((int) r.ncheck + 1);
    if (w0 < 0) return fail(errbuf, errlen, SMG_ENOMEM, "no memory for the windows of the restart points of %s", path);
    const uint32_t m = (uint32_t) ix.mem.size() - 1;
    ix.pts.push_back(GzPoint{ 8ull * (uint64_t) p0 + r.start, (uint64_t) ix.text, cur_win, m });
    for (uint32_t c = 0; c < r.ncheck; c++)
      ix.pts.push_back(GzPoint{ 8ull * (uint64_t) p0 + check[c].bit, (uint64_t) ix.text + check[c].text, w0 + c, m });
    const int rc = e.resolve(slot0, r.ncheck, r.text, cur_win, avail, w0);
    if (rc) return rc;
    cur_win = w0 + r.ncheck;
    avail = r.text >= INF_WINDOW - avail ? INF_WINDOW : avail + (uint32_t) r.text;
    ix.text += (int64_t) r.text; mtext += r.text;
    pos = 8ull * (uint64_t) p0 + r.end;
    return 0;
  }

  GzTask repair_task(uint64_t rel, uint64_t stop, uint32_t max_blocks) const
  { return GzTask{ rel, rel, stop, cur_win < 0 ? nullptr : e.window(cur_win), 0u, max_blocks ? 0u : 1u, 1u, avail, max_blocks,
                   (uint32_t) (GZ_MAX_SPANS * GZ_QUOTA), (uint32_t) GZ_REPAIR_QUOTA };
  }

  int run()
  { const size_t cap = e.piece_cap();
    rep_check.resize(GZ_REPAIR_QUOTA);
    for (;;)
      { if (state == HEADER && at >= fsize) break;
        const int64_t p0 = state == BLOCKS ? (int64_t) (pos >> 3) : at;
        const size_t n = (size_t) (fsize - p0 < (int64_t) cap ? fsize - p0 : (int64_t) cap);
        const bool final = p0 + (int64_t) n == fsize;
        uint8_t *buf = e.piece_buf(n);
        if (!buf) return fail(errbuf, errlen, SMG_ENOMEM, "no memory for a piece of %zu bytes of %s", n, path);
        int rc = gz_pread(fd, buf, n, p0, path, errbuf, errlen);
        if (rc) return rc;
        if ((rc = e.piece(n)) != 0) return rc;
        const uint32_t ns = (uint32_t) ((n + e.span - 1) / e.span);
        bool launched = false;
        for (;;)
          { if (state == TRAILER)
              { const size_t rel = (size_t) (at - p0);
                GzMember &m = ix.mem.back();
                if (rel + 8 > n)
                  { if (final) return gz_bad_member(errbuf, errlen, path, m.off, "the trailer is cut off by the end of the file");
                    break;
                  }
                const uint8_t *t = buf + rel;
                m.crc = (uint32_t) t[0] | (uint32_t) t[1] << 8 | (uint32_t) t[2] << 16 | (uint32_t) t[3] << 24;
                m.isize = (uint32_t) t[4] | (uint32_t) t[5] << 8 | (uint32_t) t[6] << 16 | (uint32_t) t[7] << 24;
                m.text = mtext;
                if (m.isize != (uint32_t) mtext) return gz_bad_member(errbuf, errlen, path, m.off, "the length of the text is not the ISIZE of the trailer");
                state = HEADER; at += 8;
                continue;
              }
            if (state == HEADER)
              { if (at >= fsize) break;
                const size_t rel = (size_t) (at - p0);
                if (rel >= n) break;
                if (buf[rel] == 0 && !ix.mem.empty())
                  { bool zeros = false;
                    if ((rc = gz_zeros(fd, at, fsize, path, &zeros, errbuf, errlen)) != 0) return rc;
                    if (!zeros) return gz_bad_member(errbuf, errlen, path, at, "trailing bytes that are neither zeros nor a gzip member");
                    at = fsize;
                    break;
                  }
                size_t hlen = 0;
                const char *why = "";
                const int h = gz_member_header(buf + rel, n - rel, &hlen, &why);
                if (h == 2)
                  { if (final) return gz_bad_member(errbuf, errlen, path, at, "the header is cut off by the end of the file");
                    if (rel == 0) return gz_bad_member(errbuf, errlen, path, at, "the header is longer than a piece");
                    break;
                  }
                if (h == 1)
                  return gz_bad_member(errbuf, errlen, path, at, ix.mem.empty() || buf[rel] == 31 ? why : "trailing bytes that are neither zeros nor a gzip member");
                ix.mem.push_back(GzMember{ at, 0, (uint64_t) ix.text, 0, 0, 0 });
                state = BLOCKS; pos = 8ull * (uint64_t) (at + (int64_t) hlen);
                cur_win = -1; avail = 0; mtext = 0;
                continue;
              }
            const uint64_t rel = pos - 8ull * (uint64_t) p0;
            if ((rel >> 3) >= n && !final) break;
            const uint32_t s = (uint32_t) ((rel >> 3) / e.span);
            const uint64_t end_s = 8ull * ((uint64_t) (s + 1) * e.span < n ? (uint64_t) (s + 1) * e.span : n);
            GzResult r;
            const GzCheck *check = rep_check.data();
            uint32_t slot0 = GZ_MAX_SPANS * GZ_QUOTA;
            bool link = false;
            if (!launched)                                     // the spans of the piece, all at once; the one pos lies in starts there
              { tasks.assign(ns > s ? ns : s + 1, GzTask{ GZ_NONE, GZ_NONE, 0, nullptr, 0, 0, 0, 0, 0, 0, GZ_QUOTA });
                for (uint32_t i = 0; i < (uint32_t) tasks.size(); i++)
                  { GzTask &k = tasks[i];
                    k.slot0 = i * GZ_QUOTA;
                    k.stop = k.hi = 8ull * ((uint64_t) (i + 1) * e.span < n ? (uint64_t) (i + 1) * e.span : n);
                    if (i > s) { k.lo = 8ull * (uint64_t) i * e.span; k.find = 1; }
                  }
                tasks[s].lo = rel; tasks[s].known = 1; tasks[s].avail = avail; tasks[s].win = cur_win < 0 ? nullptr : e.window(cur_win);
                spec.resize(tasks.size()); spec_check.resize(tasks.size() * GZ_QUOTA);
                if ((rc = e.marker(tasks.data(), (int) tasks.size(), true, spec.data(), spec_check.data())) != 0) return rc;
                launched = true;
                r = spec[s]; check = spec_check.data() + (size_t) s * GZ_QUOTA; slot0 = s * GZ_QUOTA; link = true;
              }
            else if (s < spec.size() && spec[s].start == rel)
              { r = spec[s]; check = spec_check.data() + (size_t) s * GZ_QUOTA; slot0 = s * GZ_QUOTA; link = true; }
            else
              { const GzTask k = repair_task(rel, end_s, 0);
                if ((rc = e.marker(&k, 1, false, &r, rep_check.data())) != 0) return rc;
              }
            if (r.status != INF_OK)
              { const bool ran_out = r.status == INF_EXHAUSTED || 8ull * n - r.bad_at < 16;
                if (final || !ran_out)
                  return gz_bad_block(errbuf, errlen, path, p0 + (int64_t) (r.bad >> 3), inflate_reason((int) r.status));
                if (r.blocks == 0) break;                      // the block goes on in the next piece
                const GzTask k = repair_task(rel, end_s, r.blocks);
                if ((rc = e.marker(&k, 1, false, &r, rep_check.data())) != 0) return rc;
                if (r.status != INF_OK || r.start != rel)
                  return fail(errbuf, errlen, SMG_ENODEV, "internal error: %u blocks of %s at offset %lld did not decode again", k.max_blocks, path,
                              (long long) (p0 + (int64_t) (rel >> 3)));
                check = rep_check.data(); slot0 = GZ_MAX_SPANS * GZ_QUOTA; link = false;
              }
            if (r.start != rel || r.end <= r.start || r.ncheck >= GZ_REPAIR_QUOTA)
              return fail(errbuf, errlen, SMG_ENODEV, "internal error: the decode of %s at offset %lld gave no block", path, (long long) (p0 + (int64_t) (rel >> 3)));
            if ((rc = accept(r, check, slot0, p0)) != 0) return rc;
            if (link) ix.linked++; else ix.repaired++;
            if (r.last)
              { ix.mem.back().end_bit = pos;
                state = TRAILER; at = (int64_t) ((pos + 7) >> 3);
              }
          }
        bool bad = false;
        if ((rc = e.resolved(&bad)) != 0) return rc;
        if (bad) return gz_bad_member(errbuf, errlen, path, ix.mem.empty() ? 0 : ix.mem.back().off, inflate_reason(INF_BAD_DISTANCE));
        const int64_t p1 = state == BLOCKS ? (int64_t) (pos >> 3) : at;
        ix.spans += (p1 - p0 + e.span - 1) / e.span;
        if (state == HEADER && at >= fsize) break;
        if (p1 <= p0)
          { if (final) return gz_bad_block(errbuf, errlen, path, p0, inflate_reason(INF_EXHAUSTED));
            return fail(errbuf, errlen, SMG_EINVAL, "%s: the deflate block at offset %lld is larger than a piece of %zu bytes: decompress the file first",
                        path, (long long) p0, cap);
          }
      }
    if (state != HEADER) return gz_bad_member(errbuf, errlen, path, ix.mem.empty() ? 0 : ix.mem.back().off, "the member is cut off by the end of the file");
    if (ix.mem.empty()) return gz_bad_member(errbuf, errlen, path, 0, "the header is cut off by the end of the file");
    return 0;
  }
};

// the interval that begins at point i ends at the next point of its member, or behind its final block
static inline uint64_t gz_end_bit(const GzIndex &ix, size_t i)
{ return i + 1 < ix.pts.size() && ix.pts[i + 1].member == ix.pts[i].member ? ix.pts[i + 1].bit : ix.mem[ix.pts[i].member].end_bit; }
static inline uint64_t gz_end_text(const GzIndex &ix, size_t i)
{ return i + 1 < ix.pts.size() ? ix.pts[i + 1].text : (uint64_t) ix.text; }

// The index of a gzip file (any gzip file, BGZF among them), its first pass.  text_cap, chunk_cap: what one call of the
// second pass holds; a restart interval above either is the one refusal, a single deflate block of that size.
static inline int gz_build(int fd, const char *path, GzEngine &e, GzIndex &ix, size_t text_cap, size_t chunk_cap, char *errbuf, size_t errlen)
{ struct stat sb;
  if (fstat(fd, &sb) != 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot read %s", path);
  ix.clear();
  e.errbuf = errbuf; e.errlen = errlen;
  bool left = false;
  int rc = e.resolved(&left);                                  // (what a file that failed half way left behind)
  if (rc) return rc;
  const double m0 = e.ms[0], m1 = e.ms[1];
  GzChain chain(e, ix, fd, path, (int64_t) sb.st_size, errbuf, errlen);
  rc = chain.run();
  ix.ms[0] = e.ms[0] - m0; ix.ms[1] = e.ms[1] - m1;
  if (rc) return rc;
  for (size_t i = 0; i < ix.pts.size(); i++)
    { const uint64_t nb = ((gz_end_bit(ix, i) + 7) >> 3) - (ix.pts[i].bit >> 3), nt = gz_end_text(ix, i) - ix.pts[i].text;
      if (nb > chunk_cap || nt > text_cap)
        return fail(errbuf, errlen, SMG_EINVAL, "%s: the deflate block at offset %lld takes %llu bytes and inflates to %llu, above the %zu and %zu of one call: "
                    "decompress the file first", path, (long long) (ix.pts[i].bit >> 3), (unsigned long long) nb, (unsigned long long) nt, chunk_cap, text_cap);
    }
  return 0;
}

// The second pass: the text of the file, as many restart intervals a call as fit text_cap bytes of text and chunk_cap of
// the file, to consume(text, n) -> 0 or what ends the run; every member's CRC-32 against its trailer.
template <class Consume>
static inline int gz_feed(int fd, const char *path, GzEngine &e, GzIndex &ix, size_t text_cap, size_t chunk_cap, Consume &&consume,
                          char *errbuf, size_t errlen)
{ e.errbuf = errbuf; e.errlen = errlen;
  const double m2 = e.ms[2];
  std::vector<GzExact> iv;
  std::vector<uint32_t> crc, status;
  uint32_t run = 0;                                            // the CRC-32 of the member so far
  size_t i = 0;
  while (i < ix.pts.size())
    { const int64_t c0 = (int64_t) (ix.pts[i].bit >> 3);
      const uint64_t t0 = ix.pts[i].text;
      size_t j = i, cn = 0, tn = 0;
      iv.clear();
      while (j < ix.pts.size() && iv.size() < GZ_MAX_EXACT)
        { const uint64_t cb = ((gz_end_bit(ix, j) + 7) >> 3) - (uint64_t) c0, tb = gz_end_text(ix, j) - t0;
          if (cb > chunk_cap || tb > text_cap) break;
          iv.push_back(GzExact{ ix.pts[j].bit - 8ull * (uint64_t) c0, gz_end_bit(ix, j) - 8ull * (uint64_t) c0,
                                ix.pts[j].win < 0 ? nullptr : e.window(ix.pts[j].win), (uint32_t) (ix.pts[j].text - t0), (uint32_t) (tb - (ix.pts[j].text - t0)) });
          cn = (size_t) cb; tn = (size_t) tb;
          j++;
        }
      if (j == i) return fail(errbuf, errlen, SMG_ENODEV, "internal error: a restart interval of %s does not fit one call", path);
      uint8_t *buf = e.piece_buf(cn);
      if (!buf) return fail(errbuf, errlen, SMG_ENOMEM, "no memory for %zu bytes of %s", cn, path);
      int rc = gz_pread(fd, buf, cn, c0, path, errbuf, errlen);
      if (rc) return rc;
      if ((rc = e.piece(cn)) != 0) return rc;
      crc.assign(iv.size(), 0); status.assign(iv.size(), 0);
      const uint8_t *text = nullptr;
      if ((rc = e.exact(iv.data(), (int) iv.size(), tn, &text, crc.data(), status.data())) != 0) return rc;
      ix.ms[2] = e.ms[2] - m2;
      for (size_t q = i; q < j; q++)
        { const GzMember &m = ix.mem[ix.pts[q].member];
          if (status[q - i] != INF_OK)
            return gz_bad_block(errbuf, errlen, path, (int64_t) (ix.pts[q].bit >> 3), inflate_reason((int) status[q - i]));
          run = q == 0 || ix.pts[q - 1].member != ix.pts[q].member ? crc[q - i] : gz_crc_join(run, crc[q - i], iv[q - i].len);
          if ((q + 1 == ix.pts.size() || ix.pts[q + 1].member != ix.pts[q].member) && run != m.crc)
            return gz_bad_member(errbuf, errlen, path, m.off, inflate_reason(INF_BAD_CRC));
        }
      if ((rc = consume(text, tn)) != 0) return rc;
      i = j;
    }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
//  the host twin: the four steps as one lane, every buffer malloc'ed at its exact size
// ---------------------------------------------------------------------------------------------------------------

struct GzHostEngine : GzEngine
{ uint8_t *buf = nullptr; size_t buf_n = 0;
  uint16_t *rings = nullptr, *sym = nullptr;
  uint8_t *stage = nullptr, *win = nullptr, *text = nullptr;
  std::vector<GzResult> spec;
  std::vector<GzCheck> slot_check = std::vector<GzCheck>(GZ_SLOTS);
  std::vector<uint8_t *> wins;
  bool bad = false;

  GzHostEngine() = default;
  GzHostEngine(const GzHostEngine &) = delete;
  GzHostEngine &operator=(const GzHostEngine &) = delete;
  ~GzHostEngine() override
  { reset();
    free(buf); free(rings); free(sym); free(stage); free(win); free(text);
  }
  uint8_t *piece_buf(size_t n) override
  { free(buf);
    buf = (uint8_t *) malloc(n ? n : 1); buf_n = n;
    return buf;
  }
  int piece(size_t n) override { return n == buf_n ? 0 : SMG_EINVAL; }
  int marker(const GzTask *tasks, int n, bool is_spec, GzResult *res, GzCheck *check) override
  { if (!rings) rings = (uint16_t *) malloc(sizeof(uint16_t) * INF_WINDOW * (size_t) GZ_SLOTS);
    if (!sym) sym = (uint16_t *) malloc(sizeof(uint16_t) * INF_WINDOW);
    if (!stage) stage = (uint8_t *) malloc(INF_RING);
    if (!rings || !sym || !stage) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s", "");
    HostTables t;
    for (int i = 0; i < n; i++)
      { const GzTask &k = tasks[i];
        if (k.nslots < 1 || (size_t) k.slot0 + k.nslots > GZ_SLOTS) return SMG_EINVAL;
        gz_marker(HostWave(), buf, (uint32_t) buf_n, k, spec.data(), (uint32_t) spec.size(), span, check_text, t.view(), sym, stage,
                  rings + (size_t) k.slot0 * INF_WINDOW, slot_check.data() + k.slot0, res + i);
        for (uint32_t c = 0; c < res[i].ncheck; c++) check[(size_t) i * (is_spec ? GZ_QUOTA : GZ_REPAIR_QUOTA) + c] = slot_check[k.slot0 + c];
      }
    if (is_spec) spec.assign(res, res + n);
    return 0;
  }
  int64_t windows(int n) override
  { const int64_t w0 = (int64_t) wins.size();
    for (int i = 0; i < n; i++)
      { uint8_t *w = (uint8_t *) malloc(INF_WINDOW);
        if (!w) return -1;
        wins.push_back(w);
      }
    return w0;
  }
  uint8_t *window(int64_t w) override { return wins[(size_t) w]; }
  int resolve(uint32_t slot0, uint32_t ncheck, uint64_t end_text, int64_t prev, uint32_t prev_avail, int64_t dst) override
  { for (uint32_t c = 0; c <= ncheck; c++)
      if (gz_resolve(0, 1, rings + (size_t) (slot0 + c) * INF_WINDOW, c < ncheck ? slot_check[slot0 + c].text : end_text, prev < 0 ? nullptr : wins[(size_t) prev],
                     prev_avail, wins[(size_t) dst + c]))
        bad = true;
    return 0;
  }
  int resolved(bool *b) override { *b = bad; bad = false; return 0; }
  int exact(const GzExact *iv, int n, size_t text_n, const uint8_t **out, uint32_t *crc, uint32_t *status) override
  { free(text);
    text = (uint8_t *) malloc(text_n ? text_n : 1);
    if (!win) win = (uint8_t *) malloc(INF_WINDOW);
    if (!stage) stage = (uint8_t *) malloc(INF_RING);
    if (!text || !win || !stage) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s", "");
    HostTables t;
    for (int i = 0; i < n; i++)
      { crc[i] = 0;
        status[i] = (uint64_t) iv[i].out_off + iv[i].len <= text_n
                      ? (uint32_t) gz_exact(HostWave(), buf, (uint32_t) buf_n, iv[i], text, t.view(), win, stage, crc + i) : (uint32_t) INF_TOO_LONG;
      }
    *out = text;
    return 0;
  }
  void reset() override
  { for (uint8_t *w : wins) free(w);
    wins.clear();
    bad = false;
  }
};

// the text of a gzip file by the twin: both passes, text_cap and chunk_cap as a call of the device's second pass holds them
static inline int gz_text_host(int fd, const char *path, uint32_t span, size_t text_cap, size_t chunk_cap, GzHostEngine &e, GzIndex &ix,
                               std::vector<uint8_t> &text, char *errbuf, size_t errlen)
{ e.set_span(span);
  e.reset();
  int rc = gz_build(fd, path, e, ix, text_cap, chunk_cap, errbuf, errlen);
  if (rc) return rc;
  text.clear();
  text.reserve((size_t) ix.text);
  rc = gz_feed(fd, path, e, ix, text_cap, chunk_cap, [&](const uint8_t *t, size_t n) { text.insert(text.end(), t, t + n); return 0; }, errbuf, errlen);
  e.reset();
  return rc;
}
