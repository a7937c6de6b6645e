// smg_bam.hpp -- unaligned BAM (what PacBio HiFi reads are delivered in) in front of the k-mer counter: the inflated text
// of a BAM file -> the stripped byte stream the counter takes (smg_count.hip holds the map of the whole counter).
//
// The stripped stream of a BAM file: behind the header (magic, l_text, text, n_ref, per reference l_name, name, l_ref) come
// the alignment records, each block_size (int32) and that many bytes.  In file order every record whose FLAG has neither
// 0x100 (secondary) nor 0x800 (supplementary) set contributes its l_seq bases, each 4-bit code mapped through
// "=ACMGRSVTWYHKDBN" (the letters samtools fasta prints), high nibble first, and one SMG_COUNT_SEPARATOR stands between two
// contributing records.  A skipped record contributes nothing, a record of l_seq = 0 an empty record: the stream is what
// smg_count_parse gives for a FASTA file of the same reads.  Names, CIGAR, qualities, tags and the strand are ignored.
//
//   BamFramer    host only: a state machine over the text in arbitrary pieces, which touches the fixed fields of a record
//                only.  Per piece: a descriptor for every contributing record whose seq field lies wholly in the piece, and
//                the bytes of the one record whose seq field a piece boundary cut, unpacked on the host (bam_unpack_host)
//   bam_lane     the tile logic of the kernel, host and device: an output tile of SMG_COUNT_BAM_TILE bytes belongs to one
//                workgroup, which finds the records under it by binary search in the output offsets; a lane makes 16 output
//                bytes and stores them at once.  `make bam_check` runs it on the host under the sanitizers (bam_check.cpp)
//   bam_unpack   the kernel (gfx950): the packed sequences where the inflate kernel left them -> the stripped bytes

#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "smg_count.h"
#include "smg_count_err.hpp"

#if defined(__HIPCC__)
#define BAM_HD __host__ __device__ __forceinline__
#else
#define BAM_HD inline
#endif

#if defined(__clang__)
#define BAM_UNROLL _Pragma("unroll")
#else
#define BAM_UNROLL
#endif

#define BAM_TILE  SMG_COUNT_BAM_TILE                           // output bytes of one workgroup
#define BAM_LANES 256                                          // its lanes: 16 output bytes each
static_assert(BAM_TILE == BAM_LANES * 16, "a lane makes 16 bytes of its tile");

// One contributing record whose seq field lies in the piece: its packed bases at text[seq_off .. seq_off + (l_seq + 1) / 2),
// its bases at out[out_off .. out_off + l_seq).  The separator in front of it is out[out_off - 1]; only the first record of a
// file has none (out_off = 0), so the records of a piece cover its output without a gap:
//   out_off[0] is 0 or 1, and out_off[i + 1] = out_off[i] + l_seq[i] + 1.
struct BamDesc { uint32_t seq_off, l_seq, out_off; };

// the letter of a 4-bit code, "=ACMGRSVTWYHKDBN"[c], from two registers
BAM_HD uint8_t bam_letter(uint32_t c)
{ const uint64_t a = (uint64_t) '=' | (uint64_t) 'A' << 8 | (uint64_t) 'C' << 16 | (uint64_t) 'M' << 24 | (uint64_t) 'G' << 32 |
                     (uint64_t) 'R' << 40 | (uint64_t) 'S' << 48 | (uint64_t) 'V' << 56;
  const uint64_t b = (uint64_t) 'T' | (uint64_t) 'W' << 8 | (uint64_t) 'Y' << 16 | (uint64_t) 'H' << 24 | (uint64_t) 'K' << 32 |
                     (uint64_t) 'D' << 40 | (uint64_t) 'B' << 48 | (uint64_t) 'N' << 56;
  return (uint8_t) ((c & 8u ? b : a) >> (8u * (c & 7u)));
}

// the two letters of a byte whose LOW nibble comes first in the stream (bam_lane swaps the nibbles of the packed bytes, so
// that an odd start is a shift by four bits): entry x of the table a workgroup keeps in LDS
BAM_HD uint16_t bam_pair(uint32_t x) { return (uint16_t) (bam_letter(x & 15u) | (uint32_t) bam_letter(x >> 4) << 8); }

// the host routine: all bases of one record (it serves the record a piece boundary cut, and smg_count_bam_text)
static inline void bam_unpack_host(const uint8_t *seq, int64_t l_seq, uint8_t *out)
{ for (int64_t j = 0; j < l_seq; j++) out[j] = bam_letter(j & 1 ? seq[j >> 1] & 15u : (uint32_t) seq[j >> 1] >> 4); }

// ---------------------------------------------------------------------------------------------------------------
//  framing (host only)
// ---------------------------------------------------------------------------------------------------------------

#define BAM_MAX_PIECE ((size_t) 1 << 30)                       // text bytes of one piece: offsets are uint32

struct BamFramer
{ enum State { H_MAGIC, H_TEXT, H_NREF, H_LNAME, H_NAME, H_LREF, R_SIZE, R_FIXED, R_PRE, R_SEQ0, R_SEQ, R_POST };
  enum Mode { COLLECT, SKIP, CARRY };
  // what a piece gave (valid until the next feed)
  std::vector<BamDesc> desc;
  size_t out_len = 0;                                          // bytes the descriptors stand for, separators included
  std::vector<uint8_t> head;                                   // stripped bytes that go in front of them
  // the whole file so far
  int64_t records = 0, bases = 0;                              // contributing records, their bases
  bool all_host = false;                                       // every record goes the way of a cut one (smg_count_bam_text)
  double ms_feed = 0;                                          // host clock of the feeds, kept by the caller

  State st = H_MAGIC;
  Mode mode = COLLECT;
  int64_t want = 8, pos = 0, rec_at = 0;                       // bytes the state still takes; text offset; that of the record
  uint8_t fix[32];
  int have = 0;
  int32_t refs_left = 0, block_size = 0, l_seq = 0;
  int64_t rest = 0;                                            // bytes of the record behind its seq field
  bool kept = false, first = true;
  std::vector<uint8_t> carry;

  static int32_t i32(const uint8_t *p) { return (int32_t) ((uint32_t) p[0] | (uint32_t) p[1] << 8 | (uint32_t) p[2] << 16 | (uint32_t) p[3] << 24); }

  int bad_header(const char *path, char *errbuf, size_t errlen, const char *why) const
  { return fail(errbuf, errlen, SMG_EFORMAT, "%s: BAM header: %s", path, why); }
  int bad_record(const char *path, char *errbuf, size_t errlen, const char *why) const
  { return fail(errbuf, errlen, SMG_EFORMAT, "%s: BAM record at text offset %lld: %s", path, (long long) rec_at, why); }

  void take(State s, Mode m, int64_t n) { st = s; mode = m; want = n; have = 0; }
  void next_ref() { if (refs_left > 0) { refs_left--; take(H_LNAME, COLLECT, 4); } else take(R_SIZE, COLLECT, 4); }

  // a contributing record is complete in `carry`: its bytes behind head
  void emit_carried()
  { const size_t at = head.size(), sep = first ? 0 : 1;
    head.resize(at + sep + (size_t) l_seq);
    if (sep) head[at] = SMG_COUNT_SEPARATOR;
    bam_unpack_host(carry.data(), l_seq, head.data() + at + sep);
    first = false; records++; bases += l_seq;
    carry.clear();
  }

  // block_size, then the 32 bytes of the fixed fields f: l_seq, kept, *pre = bytes of name and CIGAR, rest; 0, or the refusal
  int size_field(const uint8_t *f, const char *path, char *errbuf, size_t errlen)
  { block_size = i32(f);
    if (block_size < 32) return bad_record(path, errbuf, errlen, "block_size is smaller than the 32 bytes of the fixed fields");
    return 0;
  }
  int fixed_fields(const uint8_t *f, int64_t *pre, const char *path, char *errbuf, size_t errlen)
  { const int64_t l_read_name = f[8], n_cigar = (int64_t) f[12] | (int64_t) f[13] << 8;
    const uint32_t flag = (uint32_t) f[14] | (uint32_t) f[15] << 8;
    l_seq = i32(f + 16);
    if (l_seq < 0) return bad_record(path, errbuf, errlen, "l_seq is negative");
    const int64_t packed = ((int64_t) l_seq + 1) / 2;
    *pre = l_read_name + 4 * n_cigar;
    if ((int64_t) block_size < 32 + *pre + packed + l_seq)
      return bad_record(path, errbuf, errlen, "block_size is smaller than its name, CIGAR, sequence and qualities");
    kept = (flag & 0x900u) == 0;
    rest = (int64_t) block_size - 32 - *pre - packed;
    return 0;
  }

  // a contributing record whose seq field is text[i .. i + (l_seq + 1) / 2) of this piece: its descriptor
  void describe(size_t i)
  { const size_t sep = first ? 0 : 1;
    desc.push_back(BamDesc{ (uint32_t) i, (uint32_t) l_seq, (uint32_t) (out_len + sep) });
    out_len += sep + (size_t) l_seq;
    first = false; records++; bases += l_seq;
  }

  // the state has all its bytes: the next one.  i = offset in the piece of n bytes.  0, or the refusal.
  int advance(size_t i, size_t n, const char *path, char *errbuf, size_t errlen)
  { switch (st)
      { case H_MAGIC:
          if (memcmp(fix, "BAM\1", 4) != 0) return bad_header(path, errbuf, errlen, "the text does not begin with the magic BAM\\1");
          if (i32(fix + 4) < 0) return bad_header(path, errbuf, errlen, "l_text is negative");
          take(H_TEXT, SKIP, i32(fix + 4));
          break;
        case H_TEXT: take(H_NREF, COLLECT, 4); break;
        case H_NREF:
          if (i32(fix) < 0) return bad_header(path, errbuf, errlen, "n_ref is negative");
          refs_left = i32(fix);
          next_ref();
          break;
        case H_LNAME:
          if (i32(fix) < 0) return bad_header(path, errbuf, errlen, "l_name is negative");
          take(H_NAME, SKIP, i32(fix));
          break;
        case H_NAME: take(H_LREF, COLLECT, 4); break;
        case H_LREF: next_ref(); break;
        case R_SIZE:
          { const int rc = size_field(fix, path, errbuf, errlen);
            if (rc) return rc;
            take(R_FIXED, COLLECT, 32);
            break;
          }
        case R_FIXED:
          { int64_t pre = 0;
            const int rc = fixed_fields(fix, &pre, path, errbuf, errlen);
            if (rc) return rc;
            take(R_PRE, SKIP, pre);
            break;
          }
        case R_PRE: take(R_SEQ0, SKIP, 0); break;
        case R_SEQ0:                                            // the seq field begins at offset i of this piece
          { const int64_t packed = ((int64_t) l_seq + 1) / 2;
            if (!kept) take(R_SEQ, SKIP, packed);
            else if (!all_host && (int64_t) (n - i) >= packed) { describe(i); take(R_SEQ, SKIP, packed); }
            else { carry.clear(); take(R_SEQ, CARRY, packed); }      // (it grows with the bytes that come, not with what l_seq says)
            break;
          }
        case R_SEQ:
          if (mode == CARRY) emit_carried();
          take(R_POST, SKIP, rest);
          break;
        case R_POST: take(R_SIZE, COLLECT, 4); break;
      }
    return 0;
  }

  // one piece of the text: 0 and desc, out_len, head; or the refusal (SMG_EFORMAT, with message)
  int feed(const uint8_t *p, size_t n, const char *path, char *errbuf, size_t errlen)
  { desc.clear(); out_len = 0; head.clear();
    if (n > BAM_MAX_PIECE) return fail(errbuf, errlen, SMG_EINVAL, "internal error: a piece of %zu bytes of BAM text", n);
    size_t i = 0;
    for (;;)
      { // A record begins here and the piece holds it up to the end of its seq field, as nearly every record of a large piece
        // does: the same checks on the bytes where they lie, the same descriptor, and on to the end of the record.
        if (st == R_SIZE && have == 0 && n - i >= 36 && !all_host)
          { int64_t pre = 0;
            rec_at = pos;
            int rc = size_field(p + i, path, errbuf, errlen);
            if (rc == 0) rc = fixed_fields(p + i + 4, &pre, path, errbuf, errlen);
            if (rc) return rc;
            const int64_t upto = 36 + pre + ((int64_t) l_seq + 1) / 2, all = 4 + (int64_t) block_size, left = (int64_t) (n - i);
            if (left >= upto)
              { if (kept) describe(i + 36 + (size_t) pre);
                const int64_t m = left < all ? left : all;
                i += (size_t) m; pos += m;
                if (m < all) take(R_POST, SKIP, all - m); else rec_at = pos;
                continue;
              }
          }
        if (want == 0)
          { // a seq field that begins where the piece ends belongs to the next piece as a whole: wait for it
            if (st == R_SEQ0 && i == n && l_seq > 0 && kept && !all_host) break;
            const int rc = advance(i, n, path, errbuf, errlen);
            if (rc) return rc;
            if (st == R_SIZE) rec_at = pos;
            continue;
          }
        if (i == n) break;
        const size_t m = (int64_t) (n - i) < want ? n - i : (size_t) want;
        if (mode == COLLECT) { memcpy(fix + have, p + i, m); have += (int) m; }
        else if (mode == CARRY) carry.insert(carry.end(), p + i, p + i + m);
        i += m; pos += (int64_t) m; want -= (int64_t) m;
      }
    return 0;
  }

  // the text is at its end: 0, or the refusal of a file that ends inside the header or inside a record
  int finish(const char *path, char *errbuf, size_t errlen)
  { if (st == R_SIZE && have == 0) return 0;
    if (st < R_SIZE) return bad_header(path, errbuf, errlen, "the file ends inside the header");
    return bad_record(path, errbuf, errlen, "the file ends inside the record");
  }
};

// ---------------------------------------------------------------------------------------------------------------
//  the tile logic: host and device
// ---------------------------------------------------------------------------------------------------------------

// the last record of d[lo .. hi] that begins (with its separator) at or in front of output byte p; d[lo] does
BAM_HD uint32_t bam_find(const BamDesc *d, uint32_t lo, uint32_t hi, uint32_t p)
{ while (lo < hi)
    { const uint32_t mid = lo + (hi - lo + 1) / 2;
      if (d[mid].out_off <= p + 1) lo = mid; else hi = mid - 1;
    }
  return lo;
}

struct alignas(16) BamQuad { uint64_t a, b; };

// Lane `lane` of the workgroup of tile `tile`: output bytes [p0, p0 + 16) of the piece, p0 = base + tile * BAM_TILE + 16 lane,
// as far as they lie below base + len, to out[p0 - base ..].  text[0 .. text_n): the text of the piece, text and out 16-byte
// aligned; d[0 .. nd), nd >= 1: its descriptors; base: a multiple of BAM_TILE; tab[x] = bam_pair(x).
// Nothing outside out[0 .. len) is written and nothing outside text[0 .. text_n) is read, whatever the descriptors say.
BAM_HD void bam_lane(const uint8_t *text, uint32_t text_n, const BamDesc *d, uint32_t nd, uint8_t *out, uint32_t base, uint32_t len,
                     uint32_t tile, uint32_t lane, const uint16_t *tab)
{ const uint32_t end = base + len, t0 = base + tile * BAM_TILE, p0 = t0 + lane * 16u;
  if (p0 >= end) return;
  const uint32_t t1 = (end - t0 < BAM_TILE ? end : t0 + BAM_TILE) - 1u;
  const uint32_t lo = bam_find(d, 0u, nd - 1u, t0), hi = bam_find(d, lo, nd - 1u, t1);      // the records under the tile: the same in every lane
  uint32_t i = bam_find(d, lo, hi, p0);
  BamDesc r = d[i];
  const uint32_t np = end - p0 < 16u ? end - p0 : 16u;
  uint64_t w0 = 0, w1 = 0;
  bool done = false;
  if (np == 16u && p0 >= r.out_off && p0 - r.out_off + 16u <= r.l_seq)
    { // sixteen bases of one record: eight or nine packed bytes from two aligned loads
      const uint32_t j0 = p0 - r.out_off, s = r.seq_off + (j0 >> 1), a = s & ~7u, sh = 8u * (s & 7u);
      if (a + 16u <= text_n)
        { uint64_t x0, x1;
          memcpy(&x0, (const uint8_t *) __builtin_assume_aligned(text + a, 8), 8);
          memcpy(&x1, (const uint8_t *) __builtin_assume_aligned(text + a + 8, 8), 8);
          uint64_t src = sh ? x0 >> sh | x1 << (64u - sh) : x0;
          const uint64_t ninth = x1 >> sh & 0xffu;              // text[s + 8]
          const uint64_t m = 0x0f0f0f0f0f0f0f0full;
          src = (src & m) << 4 | (src >> 4 & m);                // nibble 2k of the number is now the high nibble of byte k
          if (j0 & 1u) src = src >> 4 | (ninth >> 4) << 60;
BAM_UNROLL
          for (int k = 0; k < 4; k++)
            { w0 |= (uint64_t) tab[src >> (8 * k) & 0xffu] << (16 * k);
              w1 |= (uint64_t) tab[src >> (8 * k + 32) & 0xffu] << (16 * k);
            }
          done = true;
        }
    }
  if (!done)
    {
BAM_UNROLL
      for (uint32_t q = 0; q < 16u; q++)
        if (q < np)
          { const uint32_t p = p0 + q;
            while (i + 1u < nd && d[i + 1u].out_off <= p + 1u) { i++; r = d[i]; }
            uint8_t c = SMG_COUNT_SEPARATOR;
            if (p >= r.out_off)
              { const uint32_t j = p - r.out_off, at = r.seq_off + (j >> 1);
                const uint32_t b = j < r.l_seq && at < text_n ? text[at] : 0xffu;
                c = (uint8_t) (tab[j & 1u ? b & 15u : b >> 4] & 0xffu);
              }
            if (q < 8u) w0 |= (uint64_t) c << (8u * q); else w1 |= (uint64_t) c << (8u * (q - 8u));
          }
    }
  uint8_t *o = out + (p0 - base);
  if (np == 16u) *reinterpret_cast<BamQuad *>(__builtin_assume_aligned(o, 16)) = BamQuad{ w0, w1 };
  else
    for (uint32_t q = 0; q < np; q++) o[q] = (uint8_t) ((q < 8u ? w0 >> (8u * q) : w1 >> (8u * (q - 8u))) & 0xffu);
}

// Are these the descriptors of a piece of text_n bytes with out_len bytes of output?  What bam_lane relies on, checked
// where the descriptors are handed to the device.
static inline bool bam_desc_ok(const BamDesc *d, size_t nd, size_t text_n, size_t out_len)
{ if (nd == 0) return out_len == 0;
  if (d[0].out_off > 1) return false;
  for (size_t i = 0; i < nd; i++)
    { if ((size_t) d[i].seq_off + ((size_t) d[i].l_seq + 1) / 2 > text_n) return false;
      const size_t next = (size_t) d[i].out_off + d[i].l_seq;
      if (i + 1 < nd ? next + 1 != d[i + 1].out_off : next != out_len) return false;
    }
  return true;
}

#if defined(__HIPCC__)
// One workgroup per tile of the output [base, base + len) of a piece; out is the buffer of that span.
__global__ void __launch_bounds__(BAM_LANES) bam_unpack(const uint8_t *__restrict__ text, uint32_t text_n, const BamDesc *__restrict__ d, uint32_t nd,
                                                       uint8_t *__restrict__ out, uint32_t base, uint32_t len)
{ __shared__ uint16_t tab[256];
  tab[threadIdx.x] = bam_pair(threadIdx.x);
  __syncthreads();
  bam_lane(text, text_n, d, nd, out, base, len, blockIdx.x, threadIdx.x, tab);
}
#endif
