// smg_dump.hpp -- k-mer dumps (what kmc_dump, `jellyfish dump -c` and `meryl print` write: one line per k-mer,
// <k-mer><sep><count>\n) in front of the k-mer counter (smg_count.hip holds the map of the whole counter).
//
// The line decoder is ONE text for the kernel (kd_lines, smg_count_dump.hpp) and for the host twin (DumpHost below,
// smg_count_dump_parse, dump_check.cpp), over an accessor that says how a byte, a window of bases and 64 bits of the 2-bit
// code stream are read and how a k-mer is reverse-complemented: where a line starts, its canonical key, its count and every
// reason for which it is refused.  The grammar is strict:
//     k bases ACGTacgt, exactly one ' ' or '\t', 1 .. 20 decimal digits, an optional '\r', '\n'
// so the longest legal line is SMG_COUNT_DUMP_LINE = 128 + 1 + 20 + 2 bytes and the decoder never looks further than that
// from the first byte of a line.  The value saturates at 2^32 - 1; 0 is refused (hist[0] is 0 by contract).
//
// The host side in front of the batch is here too: the cutter that turns the text of a file, fed in arbitrary pieces, into
// chunks of whole lines (one memrchr a piece, nothing per line), which therefore concatenate freely in the batch buffer.
// No HIP in this file: `make dump_check` compiles it for the host under the address and undefined-behaviour sanitizers.

#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "smg_count.h"
#include "smg_count_err.hpp"

#if defined(__HIPCC__)
#define DUMP_HD __host__ __device__ __forceinline__
#else
#define DUMP_HD inline
#endif

enum { DUMP_OK = 0, DUMP_BASES = 1, DUMP_NOCOUNT = 2, DUMP_ZERO = 3, DUMP_NOEND = 4 };

// does a line start at position p?  first: p is the first byte of the text (of a batch, of a chunk of the cutter: both
// begin with a line)
template <class A> DUMP_HD bool dump_starts(const A &a, int64_t p, bool first) { return first || a.byte(p - 1) == '\n'; }

// The line that starts at p: DUMP_OK with its canonical key (W left-aligned words), its count and its length in bytes, line
// end included, or the reason it is refused for.  Reads a.byte(p + k .. p + k + 22) at most.
template <int W, class A> DUMP_HD int dump_line(const A &a, int64_t p, int k, uint64_t *key, uint32_t *count, int *len)
{ if (!a.bases(p, k)) return DUMP_BASES;
  const unsigned sep = a.byte(p + k);
  if (sep != ' ' && sep != '\t') return DUMP_BASES;
  const int64_t q = p + k + 1;
  uint64_t v = 0;
  int nd = 0;
  for (; nd < 20; nd++)
    { const unsigned c = a.byte(q + nd);
      if (c < '0' || c > '9') break;
      v = v * 10 + (c - '0');
      if (v > 0xFFFFFFFFull) v = 0xFFFFFFFFull;                // (saturated: it stays there)
    }
  if (nd == 0) return DUMP_NOCOUNT;
  int e = nd;
  if (a.byte(q + e) == '\r') e++;
  if (a.byte(q + e) != '\n') return DUMP_NOEND;
  if (v == 0) return DUMP_ZERO;
  uint64_t x[W], r[W];
  for (int w = 0; w < W; w++) x[w] = a.take64(2 * p + 64 * w);
  x[W - 1] &= ~0ull << (64 - (2 * k - 64 * (W - 1)));          // the bits of the last word that belong to the k-mer
  a.template revcomp<W>(x, k, r);
  bool lt = false;
  for (int w = 0; w < W; w++)
    if (r[w] != x[w]) { lt = r[w] < x[w]; break; }
  for (int w = 0; w < W; w++) key[w] = lt ? r[w] : x[w];
  *count = (uint32_t) v;
  *len = k + 1 + e + 1;
  return DUMP_OK;
}

static inline const char *dump_reason(int r, int k, char *buf, size_t n)
{ switch (r)
    { case DUMP_BASES:   snprintf(buf, n, "is not %d bases and a separator (is k right?)", k); return buf;
      case DUMP_NOCOUNT: return "has no count";
      case DUMP_ZERO:    return "count is 0";
      case DUMP_NOEND:   return "count is not followed by a line end";
    }
  return "internal error";
}

static inline int dump_bad_line(char *errbuf, size_t errlen, const char *path, int64_t off, int reason, int k)
{ char why[96];
  return fail(errbuf, errlen, SMG_EFORMAT, "%s: dump line at offset %lld: %s", path, (long long) off, dump_reason(reason, k, why, sizeof(why)));
}

// ---- the host's accessor: plain bytes ---------------------------------------------------------------------------------

struct DumpText
{ const uint8_t *t; int64_t n;                                 // bytes at n and beyond read as 0, which is nothing legal
  static int code(unsigned b)                                  // a c g t -> 0 1 2 3, anything else -1
  { switch (b | 0x20u) { case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': return 3; }
    return -1;
  }
  unsigned byte(int64_t p) const { return p >= 0 && p < n ? t[p] : 0u; }
  bool bases(int64_t p, int k) const
  { if (p + k > n) return false;
    for (int j = 0; j < k; j++) if (code(t[p + j]) < 0) return false;
    return true;
  }
  uint64_t take64(int64_t bit) const                           // 32 positions of the code stream; what is no base codes as 0
  { uint64_t v = 0;
    for (int j = 0; j < 32; j++)
      { const int c = code(byte(bit / 2 + j));
        v = (v << 2) | (uint64_t) (c < 0 ? 0 : c);
      }
    return v;
  }
  template <int W> void revcomp(const uint64_t *x, int k, uint64_t *r) const
  { for (int w = 0; w < W; w++) r[w] = 0;
    for (int j = 0; j < k; j++)                                // base j of the complement is 3 - base k-1-j
      { const int s = k - 1 - j;
        const uint64_t b = 3u - ((x[s >> 5] >> (62 - 2 * (s & 31))) & 3u);
        r[j >> 5] |= b << (62 - 2 * (j & 31));
      }
  }
};

// dump_line for a word count known at run time
template <class A> static inline int dump_line_w(int W, const A &a, int64_t p, int k, uint64_t *key, uint32_t *count, int *len)
{ switch (W)
    { case 1: return dump_line<1>(a, p, k, key, count, len);
      case 2: return dump_line<2>(a, p, k, key, count, len);
      case 3: return dump_line<3>(a, p, k, key, count, len);
    }
  return dump_line<4>(a, p, k, key, count, len);
}

// ---- the cutter ---------------------------------------------------------------------------------------------------------
// The text of one file, in pieces of any size, to a sink in chunks of whole lines: every put() ends behind a '\n'.  The sink
// says how much it takes before it must begin a new block (room()) and begins one on request (cut(), after which room() is
// that of an empty block), so that no block of a ring ends inside a line either.  A last line without '\n' gets one.
// A line is never looked at here, with one exception: a line that cannot be legal and is in the way -- the rest of a piece
// longer than SMG_COUNT_DUMP_LINE without a line end, or a line that no empty block holds.  Its first SMG_COUNT_DUMP_LINE + 1
// bytes go on with a '\n' behind them, which the decoder refuses for the reason and at the offset it would refuse the
// whole line for; nothing of the file follows it (the offsets behind it would be wrong, and the run fails at that line or
// in front of it).
template <class S> struct DumpCutter
{ S &out;
  std::vector<uint8_t> carry;                                  // the line the last piece ended in, no '\n' in it
  bool started = false, dead = false;
  explicit DumpCutter(S &s) : out(s) {}

  bool poison(const uint8_t *p)                                // (SMG_COUNT_DUMP_LINE + 1 bytes are there)
  { uint8_t line[SMG_COUNT_DUMP_LINE + 2];
    memcpy(line, p, SMG_COUNT_DUMP_LINE + 1);
    line[SMG_COUNT_DUMP_LINE + 1] = '\n';
    dead = true;
    if (out.room() < sizeof(line) && !out.cut()) return false;
    return out.put(line, sizeof(line));
  }

  bool emit(const uint8_t *p, size_t m)                        // whole lines
  { while (m && !dead)
      { const size_t room = out.room();
        if (m <= room) return out.put(p, m);
        const uint8_t *q = room ? (const uint8_t *) memrchr(p, '\n', room) : nullptr;
        if (q)
          { const size_t l = (size_t) (q - p) + 1;
            if (!out.put(p, l) || !out.cut()) return false;
            p += l; m -= l;
            continue;
          }
        if (!out.cut()) return false;
        if (out.room() > room) continue;                       // (the block was not empty)
        return poison(p);                                      // no block holds this line (room >= SMG_COUNT_DUMP_LINE + 2: the ring's blocks)
      }
    return true;
  }

  // 0, 1: the consumer gave up, SMG_EINVAL with a message: the text does not begin like a dump
  int feed(const uint8_t *p, size_t n, const char *path, char *errbuf, size_t errlen)
  { if (n == 0 || dead) return 0;
    if (!started)
      { started = true;
        if (DumpText::code(p[0]) < 0)
          return fail(errbuf, errlen, SMG_EINVAL, "%s is not a k-mer dump (its text begins with the byte 0x%02x, a dump line with a base): "
                      "a call with the dump option reads dumps only", path, p[0]);
      }
    if (!carry.empty())
      { const uint8_t *nl = (const uint8_t *) memchr(p, '\n', n);
        const size_t m = nl ? (size_t) (nl - p) + 1 : n;
        carry.insert(carry.end(), p, p + m);
        p += m; n -= m;
        if (nl)
          { if (!emit(carry.data(), carry.size())) return 1;
            carry.clear();
          }
      }
    if (n)
      { const uint8_t *last = (const uint8_t *) memrchr(p, '\n', n);
        const size_t head = last ? (size_t) (last - p) + 1 : 0;
        if (head && !emit(p, head)) return 1;
        carry.assign(p + head, p + n);
      }
    if (!dead && carry.size() > SMG_COUNT_DUMP_LINE && !poison(carry.data())) return 1;
    return 0;
  }

  int finish()
  { if (dead || carry.empty()) return 0;
    carry.push_back('\n');
    const bool ok = emit(carry.data(), carry.size());
    carry.clear();
    return ok ? 0 : 1;
  }
};

// ---- the host twin: the records of a dump, line by line ------------------------------------------------------------------
// A sink for the cutter.  Every chunk is decoded line after line by dump_line over DumpText; the first bad line ends it
// (rc, reason, offset).  A test twin of kd_lines, not a fallback.
struct DumpHost
{ int k, W;
  std::vector<uint64_t> keys;                                  // W words a record
  std::vector<uint32_t> counts;
  int64_t base = 0;                                            // text bytes in front of the next chunk
  int bad = 0;                                                 // the reason of the first bad line,
  int64_t bad_off = 0;                                         // and where it starts
  explicit DumpHost(int kmer) : k(kmer), W((kmer + 31) / 32) {}

  size_t room() const { return (size_t) -1; }
  bool cut() { return true; }
  bool put(const uint8_t *p, size_t n)
  { const DumpText a{ p, (int64_t) n };
    int64_t pos = 0;
    while (pos < (int64_t) n)
      { uint64_t key[4];
        uint32_t c = 0;
        int len = 0;
        const int r = dump_line_w(W, a, pos, k, key, &c, &len);
        if (r != DUMP_OK) { bad = r; bad_off = base + pos; return false; }
        keys.insert(keys.end(), key, key + W);
        counts.push_back(c);
        pos += len;
      }
    base += (int64_t) n;
    return true;
  }
};
