// smg_inflate.hpp -- DEFLATE for the members of a BGZF file (RFC 1951 / 1952), one member per wavefront of an MI355X
// (gfx950, wave64); smg_count_reader.hpp finds the members, smg_count.hip holds the map of the whole counter.
//
// A member is at most 64 KiB of compressed bytes and at most 64 KiB of text, and knows its own CRC-32 and length.  The
// decoder trusts none of it: for ANY bytes it reads only payload bytes [0, clen), writes only text bytes [0, isize),
// and every loop consumes at least one bit or produces at least one byte, both checked against their limit first.
//
// One text for host and device (as smg_mergepath.hpp with mergepath_check.cpp): the bit reader, the table builder, the
// symbol loop and every status decision are INF_HD functions over an accessor Io,
//     lane(), lanes()                 which lane of how many runs this text (host: 0 of 1)
//     in1(i), in4(i)                  payload byte i / bytes i .. i + 3 little endian; the caller has checked i (+ 4) <= clen
//     lit(pos, c)                     text byte pos = c; the caller has checked pos < isize
//     match(pos, dist, len)           text[pos + i] = text[pos - dist + i], i = 0 .. len - 1 in this order; checked: dist <= pos,
//                                     dist <= 32768, pos + len <= isize
//     stored(pos, i, len)             text[pos ..] = payload[i .. i + len); checked: i + len <= clen, pos + len <= isize
//     sync()                          what lanes wrote to the tables is visible to all of them
//     finish(pos)                     the CRC-32 of text [0, pos)
// and `inflate_check` runs them on the host against zlib under the sanitizers, over valid and over mutated members.
//
// On the device ALL 64 lanes of the wave walk the symbols in lockstep with the same state (a wave executes one
// instruction stream whether one lane is active or all are, and this way nothing has to be broadcast), lane 0 stores
// the literals, and the lanes share what is wide: staging the payload into an LDS ring, filling the decode tables,
// copying a match, flushing the text to global memory and its CRC (WaveIo below).  The serial walk never waits for global memory: the
// payload ring (2 KiB), both decode tables and the last 32 KiB of text are in LDS, 38 KiB a wave, four waves per CU.
//
// Decode tables: one level plus overflow.  A table of 2^10 (literal/length) or 2^9 (distance) entries, (symbol << 4) |
// code length, is indexed by the next bits; a code longer than that finds an entry of length 0 and is decoded bit by bit
// from the counts per length and the symbols in code order (at most one symbol in 2^9 does, by its probability).  The base
// values and extra bits of lengths and distances are computed, not looked up.

#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define INF_HD __host__ __device__ __forceinline__
#else
#define INF_HD inline
#endif

enum
{ INF_OK = 0, INF_EXHAUSTED, INF_BAD_TYPE, INF_BAD_STORED, INF_BAD_CODES, INF_BAD_SYMBOL, INF_BAD_DISTANCE, INF_TOO_LONG, INF_TOO_SHORT,
  INF_LEFT_OVER, INF_BAD_CRC, INF_NSTATUS
};

static inline const char *inflate_reason(int status)
{ static const char *const why[INF_NSTATUS] =
    { "ok", "the compressed data end inside a symbol", "DEFLATE block type 3", "the length of a stored block does not match its complement",
      "an over-subscribed or incomplete set of code lengths", "an invalid literal/length or distance symbol",
      "a distance reaches before the start of the member", "more text than ISIZE says", "less text than ISIZE says",
      "bytes are left over behind the final DEFLATE block", "the CRC-32 of the text is not the one in the trailer" };
  return status >= 0 && status < INF_NSTATUS ? why[status] : "unknown status";
}

#define INF_WINDOW    32768
#define INF_LIT_BITS  10
#define INF_DIST_BITS 9
#define INF_NLIT      288
#define INF_NDIST     32

// where the tables of one member live (LDS on the device)
struct InfTables
{ uint16_t *lit;                                               // 1 << INF_LIT_BITS
  uint16_t *dist;                                              // 1 << INF_DIST_BITS; its first 128 entries serve the code-length code
  uint16_t *sorted;                                            // INF_NLIT + INF_NDIST: the symbols in code order
  uint16_t *cnt;                                               // 2 x 16: codes per length
  uint16_t *work;                                              // 2 x 16: next code and next place per length, while one table is built
  uint8_t *lens;                                               // INF_NLIT + INF_NDIST code lengths
};

struct InfBits { uint64_t buf; int cnt; uint32_t ip; };        // cnt real bits in buf (the bits above them are zero), ip: next payload byte

// at least 32 bits in the buffer, or all that is left of the payload
template <class Io> INF_HD void inf_refill(Io &io, InfBits &b)
{ if (b.cnt >= 32) return;
  if (b.ip + 4 <= io.clen) { b.buf |= (uint64_t) io.in4(b.ip) << b.cnt; b.ip += 4; b.cnt += 32; }
  else
    while (b.ip < io.clen && b.cnt <= 56) { b.buf |= (uint64_t) io.in1(b.ip) << b.cnt; b.ip++; b.cnt += 8; }
}

// the next n <= 16 bits; false: the payload does not hold them
INF_HD bool inf_take(InfBits &b, int n, uint32_t *v)
{ if (n > b.cnt) return false;
  *v = (uint32_t) b.buf & ((1u << n) - 1u);
  b.buf >>= n; b.cnt -= n;
  return true;
}

INF_HD uint32_t inf_reverse(uint32_t code, int len)            // the low `len` <= 15 bits in reverse order
{ uint32_t r = ((code & 0x5555u) << 1) | ((code >> 1) & 0x5555u);
  r = ((r & 0x3333u) << 2) | ((r >> 2) & 0x3333u);
  r = ((r & 0x0f0fu) << 4) | ((r >> 4) & 0x0f0fu);
  r = ((r & 0x00ffu) << 8) | ((r >> 8) & 0x00ffu);
  return r >> (16 - len);
}

// The decode table of the code lengths lens[0 .. n): kind 0 the code-length code, 1 literal/length, 2 distance.  What is
// accepted is what zlib accepts: no over-subscribed set; an incomplete one only where it is a single code of length 1
// (literal/length, distance), or no code at all (distance).  The unused patterns of those decode to INF_BAD_SYMBOL.
template <class Io>
INF_HD int inf_build(Io &io, const uint8_t *lens, int n, uint16_t *tab, int tbits, uint16_t *sorted, uint16_t *cnt, uint16_t *work, int kind)
{ uint16_t *next = work, *place = work + 16;
  for (int l = 0; l < 16; l++) cnt[l] = 0;
  for (int s = 0; s < n; s++) cnt[lens[s]]++;
  cnt[0] = 0;
  int max = 0, left = 1;
  for (int l = 1; l < 16; l++)
    { const int c = cnt[l];
      if (c) max = l;
      left = (left << 1) - c;
      if (left < 0) return INF_BAD_CODES;
    }
  if (max == 0 && kind != 2) return INF_BAD_CODES;
  if (left > 0 && max != 0 && (kind == 0 || max != 1)) return INF_BAD_CODES;
  if (left > 0 || max > tbits)                                 // patterns of no code or of the start of a long one: entries of length 0
    { for (int j = io.lane(); j < (1 << tbits); j += io.lanes()) tab[j] = 0;
      io.sync();
    }
  int code = 0, at = 0;
  for (int l = 1; l < 16; l++)
    { code = (code + cnt[l - 1]) << 1;
      next[l] = (uint16_t) code; place[l] = (uint16_t) at;
      at += cnt[l];
    }
  for (int s = 0; s < n; s++)
    { const int l = lens[s];
      if (l == 0) continue;
      const uint32_t c = next[l];
      next[l] = (uint16_t) (c + 1);
      sorted[place[l]] = (uint16_t) s;                        // (place[l] < n: the lengths are not over-subscribed)
      place[l]++;
      if (l <= tbits)
        for (uint32_t j = inf_reverse(c, l) + ((uint32_t) io.lane() << l); j < (1u << tbits); j += (uint32_t) io.lanes() << l)
          tab[j] = (uint16_t) ((s << 4) | l);
    }
  io.sync();
  return INF_OK;
}

// a code of the set (cnt, sorted) from the 15 bits `bits`, bit by bit: -1 where no code matches
INF_HD int inf_slow(uint32_t bits, const uint16_t *cnt, const uint16_t *sorted, int *len)
{ int code = 0, first = 0, index = 0;
  for (int l = 1; l < 16; l++)
    { code |= (int) (bits & 1u); bits >>= 1;
      const int c = cnt[l];
      if (code - c < first) { *len = l; return sorted[index + (code - first)]; }
      index += c; first = (first + c) << 1; code <<= 1;
    }
  return -1;
}

INF_HD int inf_symbol(InfBits &b, const uint16_t *tab, int tbits, const uint16_t *cnt, const uint16_t *sorted, int *sym)
{ const uint32_t peek = (uint32_t) b.buf & 0x7fffu;
  const uint32_t e = tab[peek & ((1u << tbits) - 1u)];
  int len = (int) (e & 15u), s = (int) (e >> 4);
  if (len == 0)
    { s = inf_slow(peek, cnt, sorted, &len);
      if (s < 0) return INF_BAD_SYMBOL;
    }
  if (len > b.cnt) return INF_EXHAUSTED;
  b.buf >>= len; b.cnt -= len;
  *sym = s;
  return INF_OK;
}

#define INF_TRY(call) do { const int _s = (call); if (_s != INF_OK) return _s; } while (0)
#define INF_BITS(n, v) do { if (!inf_take(b, (n), &(v))) return INF_EXHAUSTED; } while (0)

// the header of a dynamic block: both sets of code lengths, one sequence in t.lens
template <class Io> INF_HD int inf_dynamic(Io &io, InfBits &b, const InfTables &t, int *nlit, int *ndist)
{ // the order of the code-length code lengths, 5 bits each: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
  const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                            11ull << 50 | 4ull << 55;
  const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  uint32_t hlit, hdist, hclen, v;
  inf_refill(io, b);
  INF_BITS(5, hlit); INF_BITS(5, hdist); INF_BITS(4, hclen);
  hlit += 257; hdist += 1; hclen += 4;
  if (hlit > 286 || hdist > 30) return INF_BAD_CODES;
  for (int i = 0; i < 19; i++) t.lens[i] = 0;
  for (uint32_t i = 0; i < hclen; i++)
    { inf_refill(io, b);
      INF_BITS(3, v);
      t.lens[(i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31u] = (uint8_t) v;
    }
  INF_TRY(inf_build(io, t.lens, 19, t.dist, 7, t.sorted + INF_NLIT, t.cnt + 16, t.work, 0));
  const uint32_t n = hlit + hdist;
  uint32_t i = 0;
  while (i < n)
    { int sym = 0;
      inf_refill(io, b);
      INF_TRY(inf_symbol(b, t.dist, 7, t.cnt + 16, t.sorted + INF_NLIT, &sym));
      if (sym < 16) { t.lens[i++] = (uint8_t) sym; continue; }
      uint32_t rep;
      uint8_t val = 0;
      if (sym == 16)
        { if (i == 0) return INF_BAD_CODES;
          val = t.lens[i - 1];
          INF_BITS(2, rep); rep += 3;
        }
      else if (sym == 17) { INF_BITS(3, rep); rep += 3; }
      else { INF_BITS(7, rep); rep += 11; }
      if (i + rep > n) return INF_BAD_CODES;
      while (rep--) t.lens[i++] = val;
    }
  if (t.lens[256] == 0) return INF_BAD_CODES;                  // no end-of-block code
  *nlit = (int) hlit; *ndist = (int) hdist;
  return INF_OK;
}

// One block from its header on: text from `pos` on (Pos: the type of io.isize, 32 bits for a member, 64 for a stream of any
// length, smg_gzip.hpp), *last = its BFINAL.  Reads payload bytes below io.clen and writes text below io.isize only.
template <class Io, class Pos> INF_HD int inf_block(Io &io, const InfTables &t, InfBits &b, Pos &pos, uint32_t *last)
{ uint32_t v;
    { inf_refill(io, b);
      INF_BITS(3, v);
      *last = v & 1u;
      const uint32_t type = v >> 1;
      if (type == 3) return INF_BAD_TYPE;
      if (type == 0)
        { v = (uint32_t) b.cnt & 7u;                           // to the next byte boundary
          b.buf >>= v; b.cnt -= (int) v;
          inf_refill(io, b);
          if (b.cnt < 32) return INF_EXHAUSTED;
          uint32_t len = (uint32_t) b.buf & 0xffffu;
          const uint32_t nlen = (uint32_t) (b.buf >> 16) & 0xffffu;
          b.buf >>= 32; b.cnt -= 32;
          if (len != (nlen ^ 0xffffu)) return INF_BAD_STORED;
          if (len > io.isize - pos) return INF_TOO_LONG;
          while (len > 0 && b.cnt > 0)                         // the whole bytes the bit buffer holds are the first of the block
            { io.lit(pos, (uint8_t) b.buf);
              b.buf >>= 8; b.cnt -= 8;
              pos++; len--;
            }
          if (len > io.clen - b.ip) return INF_EXHAUSTED;
          if (len) { io.stored(pos, b.ip, len); pos += len; b.ip += len; }
          return INF_OK;
        }
      int nlit = INF_NLIT, ndist = INF_NDIST;
      if (type == 1)
        { for (int s = io.lane(); s < INF_NLIT + INF_NDIST; s += io.lanes())
            t.lens[s] = (uint8_t) (s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < INF_NLIT ? 8 : 5);
          io.sync();
        }
      else INF_TRY(inf_dynamic(io, b, t, &nlit, &ndist));
      INF_TRY(inf_build(io, t.lens, nlit, t.lit, INF_LIT_BITS, t.sorted, t.cnt, t.work, 1));
      INF_TRY(inf_build(io, t.lens + nlit, ndist, t.dist, INF_DIST_BITS, t.sorted + INF_NLIT, t.cnt + 16, t.work, 2));
      for (;;)
        { int sym = 0;
          inf_refill(io, b);
          INF_TRY(inf_symbol(b, t.lit, INF_LIT_BITS, t.cnt, t.sorted, &sym));
          if (sym < 256)
            { if (pos >= io.isize) return INF_TOO_LONG;
              io.lit(pos, (uint8_t) sym);
              pos++;
              continue;
            }
          if (sym == 256) break;
          if (sym > 285) return INF_BAD_SYMBOL;
          uint32_t len, dist;
          { const int i = sym - 257, x = i < 8 || i == 28 ? 0 : (i >> 2) - 1;     // 3 .. 10 | 11 13 15 17 | 19 23 27 31 | .. | 258
            INF_BITS(x, v);
            len = (i < 8 ? 3u + (uint32_t) i : i == 28 ? 258u : 3u + ((4u + ((uint32_t) i & 3u)) << x)) + v;
          }
          inf_refill(io, b);
          INF_TRY(inf_symbol(b, t.dist, INF_DIST_BITS, t.cnt + 16, t.sorted + INF_NLIT, &sym));
          if (sym > 29) return INF_BAD_SYMBOL;
          { const int x = sym < 4 ? 0 : (sym >> 1) - 1;        // 1 2 3 4 | 5 7 | 9 13 | 17 25 | .. | 16385 24577
            INF_BITS(x, v);
            dist = (sym < 4 ? 1u + (uint32_t) sym : 1u + ((2u + ((uint32_t) sym & 1u)) << x)) + v;
          }
          if (dist > pos) return INF_BAD_DISTANCE;
          if (len > io.isize - pos) return INF_TOO_LONG;
          io.match(pos, dist, len);
          pos += len;
        }
    }
  return INF_OK;
}

// One member: io.clen payload bytes -> exactly io.isize bytes of text with the CRC-32 io.crc, or the first reason why not.
template <class Io> INF_HD int inflate_member(Io &io, const InfTables &t)
{ InfBits b{ 0, 0, 0 };
  uint32_t pos = 0, last;
  do INF_TRY(inf_block(io, t, b, pos, &last));
  while (!last);
  if (pos != io.isize) return INF_TOO_SHORT;
  if (io.clen - b.ip + (uint32_t) (b.cnt >> 3) != 0) return INF_LEFT_OVER;
  if (io.finish(pos) != io.crc) return INF_BAD_CRC;
  return INF_OK;
}

// ---------------------------------------------------------------------------------------------------------------
//  CRC-32 (reflected, polynomial 0xedb88320) in 64 slices.  The register after the bytes M from the state c is
//  c x^(8|M|) + M(x) x^32 mod P, so the register over A B is that over A times x^(8|B|) plus that over B from state 0,
//  and bytes that are missing in FRONT of a slice that starts from 0 change nothing.  Lane l takes the S bytes that end
//  (63 - l) S before the end of the range; the lane in which the range begins starts from the running register, the
//  others from 0; six rounds combine neighbouring groups of 1, 2, .. 32 lanes.
// ---------------------------------------------------------------------------------------------------------------

INF_HD uint32_t crc_mul(uint32_t a, uint32_t b)                // a(x) b(x) mod P, bit 31 is x^0
{ uint32_t p = 0;
  for (int i = 0; i < 32; i++)
    { p ^= b & (0u - ((a >> 31) & 1u));
      a <<= 1;
      b = (b >> 1) ^ (0xedb88320u & (0u - (b & 1u)));
    }
  return p;
}

INF_HD uint32_t crc_xpow8(uint32_t n)                          // x^(8 n) mod P
{ uint32_t r = 0x80000000u, q = 0x00800000u;
  for (; n; n >>= 1)
    { if (n & 1u) r = crc_mul(r, q);
      q = crc_mul(q, q);
    }
  return r;
}

INF_HD uint32_t crc_byte(uint32_t r, uint8_t c)
{ r ^= c;
  for (int i = 0; i < 8; i++) r = (r >> 1) ^ (0xedb88320u & (0u - (r & 1u)));
  return r;
}

// bytes per lane for a range of n >= 1 bytes: 4 x an odd number, so that the 32 lanes of a half wave read 32 LDS banks
INF_HD uint32_t crc_slice_bytes(uint32_t n) { const uint32_t s = (n + 63u) / 64u; return ((s + 3u) / 8u) * 8u + 4u; }

// the register of lane `lane` over its slice of text [a, b), S = crc_slice_bytes(b - a), `run` = the register over [0, a)
template <class Read> INF_HD uint32_t crc_lane(int lane, uint32_t a, uint32_t b, uint32_t S, uint32_t run, Read read)
{ const int64_t s = (int64_t) b - (int64_t) (64 - lane) * S, e = s + S;
  uint32_t r = s <= (int64_t) a && (int64_t) a < e ? run : 0u;
  for (int64_t p = s > (int64_t) a ? s : (int64_t) a; p < e; p++) r = crc_byte(r, read((uint32_t) p));
  return r;
}

// one round of the combination: `mine` and `other` are the registers of two neighbouring groups of lanes, x = x^(8 bytes
// of a group); low: mine is the group in front
INF_HD uint32_t crc_join(uint32_t mine, uint32_t other, uint32_t x, bool low)
{ return low ? crc_mul(mine, x) ^ other : crc_mul(other, x) ^ mine; }

// ---------------------------------------------------------------------------------------------------------------
//  the accessor of the host: plain arrays (inflate_check gives it arrays of exactly clen and isize bytes)
// ---------------------------------------------------------------------------------------------------------------

struct HostIo
{ const uint8_t *in; uint32_t clen; uint8_t *out; uint32_t isize, crc;
  int lane() const { return 0; }
  int lanes() const { return 1; }
  uint8_t in1(uint32_t i) const { return in[i]; }
  uint32_t in4(uint32_t i) const { return (uint32_t) in[i] | (uint32_t) in[i + 1] << 8 | (uint32_t) in[i + 2] << 16 | (uint32_t) in[i + 3] << 24; }
  void lit(uint32_t pos, uint8_t c) { out[pos] = c; }
  void match(uint32_t pos, uint32_t dist, uint32_t len) { for (uint32_t i = 0; i < len; i++) out[pos + i] = out[pos + i - dist]; }
  void stored(uint32_t pos, uint32_t i, uint32_t len) { for (uint32_t j = 0; j < len; j++) out[pos + j] = in[i + j]; }
  void sync() {}
  uint32_t finish(uint32_t pos) const
  { uint32_t r = 0xffffffffu;
    for (uint32_t p = 0; p < pos; p++) r = crc_byte(r, out[p]);
    return r ^ 0xffffffffu;
  }
};

struct HostTables
{ uint16_t lit[1 << INF_LIT_BITS], dist[1 << INF_DIST_BITS], sorted[INF_NLIT + INF_NDIST], cnt[32], work[32];
  uint8_t lens[INF_NLIT + INF_NDIST];
  InfTables view() { return InfTables{ lit, dist, sorted, cnt, work, lens }; }
};

// the host twin of the kernel: one member, status as the kernel's
static inline int inflate_member_host(const uint8_t *in, uint32_t clen, uint8_t *out, uint32_t isize, uint32_t crc)
{ HostIo io{ in, clen, out, isize, crc };
  HostTables t;
  return inflate_member(io, t.view());
}

// ---------------------------------------------------------------------------------------------------------------
//  the accessor of a wave: the payload staged through a ring, the last 32 KiB of text in a window, flushed as it fills,
//  both in LDS.  Wave says what a wave is -- lane(), lanes(), sync(), crc(a, b, run, window) -- so that inflate_check runs
//  this very index arithmetic on the host, as one lane, with ring, window, payload and text malloc'ed at their exact sizes.
// ---------------------------------------------------------------------------------------------------------------

#define INF_RING 2048                                          // payload bytes staged in LDS

template <class Wave> struct WaveIo
{ const uint8_t *in; uint32_t clen; uint8_t *out; uint32_t isize, crc;
  uint8_t *win, *ring;                                         // text byte p at win[p % INF_WINDOW], payload byte i at ring[i % INF_RING]
  uint32_t staged, flushed, run;                               // payload bytes staged; text bytes flushed; the CRC register over them
  Wave wv;

  INF_HD int lane() const { return wv.lane(); }
  INF_HD int lanes() const { return wv.lanes(); }
  INF_HD void sync() { wv.sync(); }

  // payload [staged, staged + m) into the ring, over bytes below `ip` (all consumed): m <= clen - staged by construction
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

  // text [flushed, pos) to global memory, and into the CRC; pos <= isize by construction
  INF_HD void flush(uint32_t pos)
  { if (pos == flushed) return;
    wv.sync();
    for (uint32_t p = flushed + (uint32_t) wv.lane(); p < pos; p += (uint32_t) wv.lanes()) out[p] = win[p & (INF_WINDOW - 1)];
    run = wv.crc(flushed, pos, run, win);
    flushed = pos;
  }
  // before text [pos, pos + n) is written: what it overwrites in the window has been flushed
  INF_HD void room(uint32_t pos, uint32_t n) { if (pos + n - flushed > INF_WINDOW) flush(pos); }

  INF_HD void lit(uint32_t pos, uint8_t c)
  { room(pos, 1);
    if (wv.lane() == 0) win[pos & (INF_WINDOW - 1)] = c;
  }
  // lanes() bytes a step: every lane reads its source before any lane of the step writes, and a source byte is never one
  // that a LATER step writes first (dist >= len: the source lies in front; dist < len: it is taken modulo dist from the
  // bytes in front of pos), so the steps in ascending order give the byte-by-byte copy
  INF_HD void match(uint32_t pos, uint32_t dist, uint32_t len)
  { room(pos, len);
    wv.sync();
    const uint32_t from = pos - dist;
    for (uint32_t i = (uint32_t) wv.lane(); i < len; i += (uint32_t) wv.lanes())
      { const uint8_t c = win[(from + (dist >= len ? i : i % dist)) & (INF_WINDOW - 1)];
        win[(pos + i) & (INF_WINDOW - 1)] = c;
      }
  }
  INF_HD void stored(uint32_t pos, uint32_t i, uint32_t len)
  { while (len)
      { room(pos, 1);
        const uint32_t free_w = INF_WINDOW - (pos - flushed), m = len < free_w ? len : free_w;
        for (uint32_t j = (uint32_t) wv.lane(); j < m; j += (uint32_t) wv.lanes()) win[(pos + j) & (INF_WINDOW - 1)] = in[i + j];
        pos += m; i += m; len -= m;
      }
    if (i > staged) staged = i;                                // (the ring holds nothing of what was passed over)
  }
  INF_HD uint32_t finish(uint32_t pos) { flush(pos); return run ^ 0xffffffffu; }
};

// one lane that stands for the wave: the 64 slices of the CRC one after the other
struct HostWave
{ int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() const {}
  uint32_t crc(uint32_t a, uint32_t b, uint32_t run, const uint8_t *win) const
  { const uint32_t S = crc_slice_bytes(b - a);
    uint32_t r[64], x = crc_xpow8(S);
    for (int l = 0; l < 64; l++) r[l] = crc_lane(l, a, b, S, run, [win](uint32_t p) { return win[p & (INF_WINDOW - 1)]; });
    for (int o = 1; o < 64; o <<= 1)
      { uint32_t nr[64];
        for (int l = 0; l < 64; l++) nr[l] = crc_join(r[l], r[l ^ o], x, (l & o) == 0);
        for (int l = 0; l < 64; l++) r[l] = nr[l];
        x = crc_mul(x, x);
      }
    return r[0];
  }
};

// the kernel's accessor on the host: ring and win are the caller's, of INF_RING and INF_WINDOW bytes
static inline int inflate_member_wave_host(const uint8_t *in, uint32_t clen, uint8_t *out, uint32_t isize, uint32_t crc, uint8_t *win, uint8_t *ring)
{ WaveIo<HostWave> io{ in, clen, out, isize, crc, win, ring, 0u, 0u, 0xffffffffu, HostWave() };
  HostTables t;
  return inflate_member(io, t.view());
}

// ---------------------------------------------------------------------------------------------------------------
//  the device: what a wave is, and the kernel
// ---------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

struct InfBlock { uint32_t in_off, clen, out_off, isize, crc; };         // (the layout of BgzfBlock, smg_count_reader.hpp)

struct DevWave
{ int ln;
  __device__ __forceinline__ int lane() const { return ln; }
  __device__ __forceinline__ int lanes() const { return 64; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }     // (a workgroup is one wave)
  __device__ __forceinline__ uint32_t crc(uint32_t a, uint32_t b, uint32_t run, const uint8_t *win) const
  { const uint32_t S = crc_slice_bytes(b - a);
    uint32_t r = crc_lane(ln, a, b, S, run, [win](uint32_t p) { return win[p & (INF_WINDOW - 1)]; });
    uint32_t x = crc_xpow8(S);
#pragma unroll 1
    for (int o = 1; o < 64; o <<= 1)
      { r = crc_join(r, (uint32_t) __shfl_xor((int) r, o, 64), x, (ln & o) == 0);
        x = crc_mul(x, x);
      }
    return r;
  }
};

// member b of the launch: blk[b] names its payload in `chunk` and its text in `text`; status[b] = why it is not ok
__global__ void __launch_bounds__(64) inf_members(const uint8_t *__restrict__ chunk, const InfBlock *__restrict__ blk, int n,
                                                  uint8_t *__restrict__ text, uint32_t *__restrict__ status)
{ __shared__ __attribute__((aligned(16))) uint8_t win[INF_WINDOW];
  __shared__ __attribute__((aligned(16))) uint8_t ring[INF_RING];
  __shared__ uint16_t lit[1 << INF_LIT_BITS], dist[1 << INF_DIST_BITS], sorted[INF_NLIT + INF_NDIST], cnt[32], work[32];
  __shared__ uint8_t lens[INF_NLIT + INF_NDIST];
  const int b = (int) blockIdx.x;
  if (b >= n) return;
  const InfBlock m = blk[b];
  WaveIo<DevWave> io{ chunk + m.in_off, m.clen, text + m.out_off, m.isize, m.crc, win, ring, 0u, 0u, 0xffffffffu, DevWave{ (int) threadIdx.x } };
  const int s = inflate_member(io, InfTables{ lit, dist, sorted, cnt, work, lens });
  if (threadIdx.x == 0) status[b] = (uint32_t) s;
}

#endif
