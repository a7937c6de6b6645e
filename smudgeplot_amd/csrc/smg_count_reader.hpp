// smg_count_reader.hpp -- the host side in front of the k-mer counter: FASTA / FASTQ files -> stripped sequence bytes, and
// the reader threads that deliver them block by block (smg_count.hip holds the map of the whole counter).  Host only, no
// HIP: `make reader_check` runs it under the address, undefined-behaviour and thread sanitizers (reader_check.cpp).
//
// A file may be block-gzipped (BGZF, what bgzip and htslib write): a gzip file of independent members of at most 64 KiB,
// each with its length in its header (the BC subfield) and its CRC-32 and text length in its trailer.  This file finds
// the members; their text comes from an Inflater, which the counter implements on the device (smg_inflate.hpp) and a
// reader without one refuses.  Any other gzip file is refused as it always was, unless the call opted in (smg_count_opts.gzip)
// and the survey left the index of the file with the thread's Inflater (smg_gzip.hpp), which then gives its text too.
//
// BGZF text that begins with the four bytes BAM\1 is a BAM file (smg_bam.hpp): its reader thread frames the records of
// every piece of text (BamFramer) and hands their descriptors back to the Inflater, whose second step unpacks the 4-bit
// sequences where the text lies; the one record a piece boundary cuts is unpacked here.  The survey does not look inside:
// the bound of a BAM file is the sum of its ISIZE fields like that of any BGZF file, at least 1.5 times its bases (a base
// takes half a byte and its quality one), so a large BAM may be counted by key range where one pass would have done; the
// result is the same whichever way it is counted.
//
// An input may be a stream instead of a regular file (Source, Taken): it is opened once, by the survey, which takes from it the
// bytes that tell what it is and hands it to its reader thread, and from then on it is read forward only; bgzf_feed carries the
// member that the end of its chunk cuts to the front of the next.  A regular file is read as it always was.
//
// What a reader learns about a file on the way (its route, records, bases, the times spent on it) is a FileRead, a plain
// value that parse_file hands back and read_files collects per file; nothing of it goes through the Inflater.

#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "smg_count.h"
#include "smg_count_err.hpp"
#include "smg_bam.hpp"
#include "smg_dump.hpp"

static inline double now_ms()
{ return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Sink
{ virtual bool put(const uint8_t *p, size_t n) = 0;          // false: the consumer gave up
  // for the cutter of a dump (smg_dump.hpp), whose blocks end with a line: the bytes that still go into the block being
  // filled, and "begin a new block" (false: the consumer gave up); a sink without blocks takes anything
  virtual size_t room() const { return (size_t) -1; }
  virtual bool cut() { return true; }
  virtual ~Sink() {}
};

// a file opened for reading, closed when it goes out of scope (fd < 0: it could not be opened); the path "-" is standard
// input, a descriptor of its own (dup), so that closing it leaves descriptor 0 alone
static inline bool is_stdin(const char *path) { return path[0] == '-' && path[1] == 0; }
struct Fd
{ const int fd;
  explicit Fd(const char *path) : fd(is_stdin(path) ? dup(0) : open(path, O_RDONLY)) {}
  Fd(const Fd &) = delete;
  Fd &operator=(const Fd &) = delete;
  ~Fd() { if (fd >= 0) close(fd); }
};

// Where the bytes of one input come from.  A regular file is read as it always was: file_kind, bgzf_walk and bgzf_feed
// pread it, the parser and the dump route read it from its start.  A stream (whatever fstat does not call a regular file:
// a FIFO, a socket, a character device such as /dev/stdin or /dev/fd/N) is read once and forward only: what was taken
// from it to tell what it is (take) is handed on first (get), then what read gives.
struct Source
{ int fd = -1;
  bool stream = false, ended = false;                          // ended: read has returned 0
  std::vector<uint8_t> head;                                   // taken and not yet handed on: head[at ..)
  size_t at = 0;
  Source() = default;
  Source(int f, bool s) : fd(f), stream(s) {}

  // (stream only) at least `want` bytes taken, or all there is: blocks until then.  Their number, or -1 for a read error.
  ssize_t take(size_t want)
  { size_t have = head.size() - at;
    if (have < want && !ended)
      { head.erase(head.begin(), head.begin() + (long) at); at = 0;
        head.resize(want);
        while (have < want)
          { const ssize_t r = read(fd, head.data() + have, want - have);
            if (r < 0) { head.resize(have); return -1; }
            if (r == 0) { ended = true; break; }
            have += (size_t) r;
          }
        head.resize(have);
      }
    return (ssize_t) have;
  }
  const uint8_t *taken() const { return head.data() + at; }

  // the next bytes, as read(2) returns them: short counts are the rule on a stream, 0 is the end
  ssize_t get(uint8_t *p, size_t n)
  { if (at < head.size())
      { const size_t m = n < head.size() - at ? n : head.size() - at;
        memcpy(p, head.data() + at, m);
        at += m;
        return (ssize_t) m;
      }
    const ssize_t r = read(fd, p, n);
    if (r == 0) ended = true;
    return r;
  }
};

// Fd's companion: an input opened once, with the Source over it.  Opening a FIFO a second time, or opening and closing
// it, ends its writer, so the survey of a call hands every stream it opened to the reader thread that gets the file.
struct Taken
{ Fd file;
  Source src;
  explicit Taken(const char *path) : file(path)
  { struct stat sb;
    src.fd = file.fd;
    // (standard input is a stream whatever it is: redirected from a file it shares its offset with descriptor 0, which a
    //  seek of the survey would move for the reader too; read forward from where it stands, a file is a stream like any)
    src.stream = file.fd >= 0 && (is_stdin(path) || (fstat(file.fd, &sb) == 0 && !S_ISREG(sb.st_mode)));
  }
};

// for the calls that read a file twice or seek in it: is `path` a stream?  By stat, which opens nothing.
static inline bool names_stream(const char *path)
{ struct stat sb;
  return is_stdin(path) || (stat(path, &sb) == 0 && !S_ISREG(sb.st_mode));
}
static inline int refuse_stream(const char *path, char *errbuf, size_t errlen)
{ return names_stream(path) ? fail(errbuf, errlen, SMG_EINVAL, "%s is a stream: this call reads a file", path) : 0; }

// Line-wise state machine over the bytes of one file, fed in arbitrary pieces.  A '\r' is dropped only in front of a
// '\n' or at the end of the file; anywhere else it is a byte like any other (and ends a stretch).
struct Parser
{ Sink &out;
  int fmt = 0, phase = 0, kind = 0;                           // fmt 1 FASTA, 2 FASTQ; kind 0 skip, 1 sequence, 2 blank
  bool bol = true, first = true, pending_cr = false, started = false;
  int64_t bases = 0, records = 0;
  explicit Parser(Sink &s) : out(s) {}

  bool emit(const uint8_t *p, size_t n) { bases += (int64_t) n; return n == 0 || out.put(p, n); }
  bool record() { const uint8_t sep = SMG_COUNT_SEPARATOR; const bool ok = first || out.put(&sep, 1); first = false; records++; return ok; }

  // 0 ok, 1 the consumer gave up, SMG_EINVAL with a message
  int feed(const uint8_t *p, size_t n, const char *path, char *errbuf, size_t errlen)
  { size_t i = 0;
    if (n == 0) return 0;
    if (!started)
      { started = true;
        if (p[0] == 0x1f && (n < 2 || p[1] == 0x8b))
          return fail(errbuf, errlen, SMG_EINVAL, "%s is gzip compressed: compressed input is not supported, decompress it first", path);
        if (p[0] == '>') fmt = 1;
        else if (p[0] == '@') fmt = 2;
        else return fail(errbuf, errlen, SMG_EINVAL, "%s is neither FASTA nor FASTQ (first byte 0x%02x)", path, p[0]);
      }
    if (pending_cr)
      { const uint8_t cr = '\r';
        pending_cr = false;
        if (p[0] != '\n' && !emit(&cr, 1)) return 1;
      }
    while (i < n)
      { if (bol)
          { const uint8_t c = p[i];
            bol = false;
            if (fmt == 1)
              { kind = c != '>';
                if (c == '>' && !record()) return 1;
              }
            else if (phase == 0)
              { kind = (c == '\n' || c == '\r') ? 2 : 0;     // (blank lines between records are passed over)
                if (kind == 0 && !record()) return 1;
              }
            else kind = phase == 1;
          }
        const uint8_t *nl = (const uint8_t *) memchr(p + i, '\n', n - i);
        const size_t end = nl ? (size_t) (nl - p) : n;
        if (kind == 1)
          { size_t e = end;
            if (e > i && p[e - 1] == '\r') { e--; if (!nl) pending_cr = true; }
            if (!emit(p + i, e - i)) return 1;
          }
        if (nl)
          { bol = true;
            if (fmt == 2 && kind != 2) phase = (phase + 1) & 3;
            i = end + 1;
          }
        else i = n;
      }
    return 0;
  }
};


// ---------------------------------------------------------------------------------------------------------------
//  BGZF: finding the members
// ---------------------------------------------------------------------------------------------------------------

#define BGZF_MAX_ISIZE  65536                                  // text bytes of one member
#define BGZF_MAX_BLOCKS 65536                                  // members of one call of an Inflater
#define BGZF_TEXT       ((size_t) 4 * SMG_COUNT_BGZF_CHUNK)    // text bytes of one call of an Inflater

// one member for the inflater: its DEFLATE payload at chunk[in_off .. in_off + clen), its text at text[out_off .. + isize)
struct BgzfBlock { uint32_t in_off, clen, out_off, isize, crc; };

// the cumulative times of an inflater in ms: its two kernels, and the copies of the unpacked bytes to the host
struct InflaterTimes
{ double inflate = 0, unpack = 0, d2h = 0;
  InflaterTimes operator-(const InflaterTimes &o) const { return InflaterTimes{ inflate - o.inflate, unpack - o.unpack, d2h - o.d2h }; }
};

// "These whole blocks of this buffer" -> "their text, or the first bad block and why".  The reader fills chunk (pinned
// where the inflater is the device's) and blk[0 .. n) and calls inflate: 0 and *text (valid until the next call), or
// > 0: the status (smg_inflate.hpp) of the first block that is not ok, *bad its index, or < 0: an error code, with message.
struct Inflater
{ uint8_t *chunk = nullptr;                                    // SMG_COUNT_BGZF_CHUNK bytes
  BgzfBlock *blk = nullptr;                                    // BGZF_MAX_BLOCKS
  virtual int inflate(int n, const uint8_t **text, int *bad, char *errbuf, size_t errlen) = 0;
  virtual const char *reason(int status) const = 0;
  // The second step, for BAM: d[0 .. nd) describe packed sequences in the text of the last inflate call (bam_desc_ok holds
  // for them and out_len); their out_len stripped bytes go to the sink in order.  0, 1: the consumer gave up, < 0: an error
  // code, with message.  An inflater without this step refuses.
  virtual int unpack(const BamDesc *, size_t, size_t, Sink &, char *errbuf, size_t errlen)
  { return fail(errbuf, errlen, SMG_EINVAL, "internal error: this inflater cannot unpack BAM sequences%s", ""); }
  virtual InflaterTimes times() const { return InflaterTimes(); }      // of all calls so far
  // Plain gzip: does this inflater hold the index of the file (the survey of a call that opted in built it)?  Then its text,
  // piece after piece, to put(text, n) -> 0 or what ends the run; 0, or that, or an error code with message.
  virtual bool has_gzip(const char *) const { return false; }
  virtual int gzip_text(int, const char *path, const std::function<int(const uint8_t *, size_t)> &, char *errbuf, size_t errlen)
  { return fail(errbuf, errlen, SMG_EINVAL, "internal error: this inflater holds no gzip index of %s", path); }
  virtual ~Inflater() {}
};

// What reading one file to its end gave: the route it took, its records (of a BAM file: the contributing ones) and their
// bases, the host time of the BAM framer, and what the inflater spent on it.  (Of a dump the host knows neither lines nor
// bases: its lines are first looked at on the device.)
enum { ROUTE_NONE = 0, ROUTE_TEXT = 1, ROUTE_BAM = 2, ROUTE_DUMP = 3 };      // not read to its end; FASTA / FASTQ; BAM; k-mer dump
struct FileRead
{ int route = ROUTE_NONE;
  int64_t records = 0, bases = 0;
  double ms_frame = 0;
  InflaterTimes dev;
};

// The header of a member in p[0 .. avail): 0 BGZF (*blen bytes in all, *hlen of them header), 1 not BGZF, 2 more bytes
// are needed to tell.  BGZF is ID1 31, ID2 139, CM 8, FLG 4 and a BC subfield of length 2 somewhere in the extra field.
static inline int bgzf_header(const uint8_t *p, size_t avail, int64_t *blen, int *hlen)
{ static const uint8_t magic[4] = { 31, 139, 8, 4 };
  if (memcmp(p, magic, avail < 4 ? avail : 4) != 0) return 1;
  if (avail < 12) return 2;
  const size_t xlen = (size_t) p[10] | (size_t) p[11] << 8;
  if (xlen < 6) return 1;
  for (size_t q = 12; q + 4 <= 12 + xlen; )
    { if (q + 4 > avail) return 2;
      const size_t slen = (size_t) p[q + 2] | (size_t) p[q + 3] << 8;
      if (q + 4 + slen > 12 + xlen) return 1;
      if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2)
        { if (q + 6 > avail) return 2;
          *blen = ((int64_t) p[q + 4] | (int64_t) p[q + 5] << 8) + 1;
          *hlen = (int) (12 + xlen);
          return 0;
        }
      q += 4 + slen;
    }
  return 1;
}

static inline int bgzf_bad(char *errbuf, size_t errlen, const char *path, int64_t off, const char *why)
{ return fail(errbuf, errlen, SMG_EFORMAT, "%s: BGZF block at offset %lld: %s", path, (long long) off, why); }

// what every member is checked for before anything is inflated; p[0 .. avail) are the bytes of the file from `off` on
// (of a stream fsize is where it ended, or BGZF_NO_END while it has not: only its end cuts a header or a member off)
#define BGZF_NO_END ((int64_t) 1 << 62)
static inline int bgzf_member(const uint8_t *p, size_t avail, const char *path, int64_t off, int64_t fsize, int64_t *blen, int *hlen,
                              char *errbuf, size_t errlen, bool stream = false)
{ const int rc = bgzf_header(p, avail, blen, hlen);
  if (rc == 1) return bgzf_bad(errbuf, errlen, path, off, "not a BGZF member (gzip with the BC subfield)");
  if (rc == 2) return (int64_t) avail < fsize - off ? 2 : bgzf_bad(errbuf, errlen, path, off, stream ? "the header is cut off by the end of the stream"
                                                                                                         : "the header is cut off by the end of the file");
  if (*blen < *hlen + 8) return bgzf_bad(errbuf, errlen, path, off, "BSIZE is smaller than the header and the trailer");
  if (off + *blen > fsize) return bgzf_bad(errbuf, errlen, path, off, stream ? "the member is cut off by the end of the stream"
                                                                             : "BSIZE reaches past the end of the file");
  return 0;
}

// What a file is by its first bytes: FILE_PLAIN (no gzip magic: the parser says what it is), FILE_BGZF (by the header of its
// first member; a header cut by the end of the file counts, the walk says where), or SMG_EINVAL with message: the file
// cannot be read, or it is gzip and not BGZF -- FILE_GZIP instead where the caller reads that (gzip_ok: the call opted in).
// The one place that decides this, for the survey, the scan and the readers.
//
// A stream is told by the bytes taken from it, which stay with its Source: the 18 of a BGZF header with the BC subfield
// in front, or all there is of a shorter one; more only where bgzf_header asks for more.  Plain gzip on a stream is refused
// either way: the index of its restart points (smg_gzip.hpp) reads the file twice.
enum { FILE_PLAIN = 0, FILE_BGZF = 1, FILE_GZIP = 2 };
static inline int file_kind(Source &src, const char *path, char *errbuf, size_t errlen, bool gzip_ok = false)
{ std::vector<uint8_t> h(src.stream ? 0 : 32);
  size_t want = src.stream ? 18 : 32;
  for (;;)
    { const ssize_t got = src.stream ? src.take(want) : pread(src.fd, h.data(), h.size(), 0);
      if (got < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot read %s", path);
      const uint8_t *p = src.stream ? src.taken() : h.data();
      int64_t blen = 0; int hlen = 0;
      const int rc = got == 0 ? 1 : bgzf_header(p, (size_t) got, &blen, &hlen);
      if (rc == 2 && (size_t) got == want && want < 12 + 65536) { want = 12 + 65536; h.resize(src.stream ? 0 : want); continue; }
      if (rc == 0 || (rc == 2 && got >= 4)) return FILE_BGZF;
      if (got >= 2 && p[0] == 0x1f && p[1] == 0x8b)
        { if (!gzip_ok) return fail(errbuf, errlen, SMG_EINVAL, "%s is gzip compressed: compressed input is not supported, decompress it first", path);
          if (src.stream)
            return fail(errbuf, errlen, SMG_EINVAL, "%s is a stream of plain gzip: its restart index reads the file twice; give the file itself, "
                        "or decompress it in the pipe", path);
          return FILE_GZIP;
        }
      return FILE_PLAIN;
    }
}

// From header to header: members and the sum of their ISIZE fields, one small read a member (the trailer of one and the
// header of the next are neighbours).  The inflater enforces that a member gives exactly ISIZE bytes, so the sum bounds
// the text of a lying file too.
static inline int bgzf_walk(int fd, const char *path, int64_t *blocks, int64_t *text, char *errbuf, size_t errlen)
{ struct stat sb;
  if (fstat(fd, &sb) != 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot read %s", path);
  const int64_t fsize = (int64_t) sb.st_size;
  std::vector<uint8_t> h(8 + 12 + 65536 + 8);
  int64_t off = 0, nb = 0, nt = 0;
  size_t have = 0;                                             // bytes of h from `off` on
  while (off < fsize)
    { int64_t blen = 0; int hlen = 0;
      int rc = have ? bgzf_member(h.data(), have, path, off, fsize, &blen, &hlen, errbuf, errlen) : 2;
      if (rc == 2)
        { const ssize_t got = pread(fd, h.data(), have ? 12 + 65536 : 18, off);
          if (got < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
          have = (size_t) got;
          rc = bgzf_member(h.data(), have, path, off, fsize, &blen, &hlen, errbuf, errlen);
          if (rc == 2)
            { const ssize_t more = pread(fd, h.data(), 12 + 65536, off);
              if (more < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
              have = (size_t) more;
              rc = bgzf_member(h.data(), have, path, off, fsize, &blen, &hlen, errbuf, errlen);
              if (rc == 2) return bgzf_bad(errbuf, errlen, path, off, "the header is cut off by the end of the file");
            }
        }
      if (rc) return rc;
      const ssize_t got = pread(fd, h.data(), 8 + 18, off + blen - 8);           // this trailer, the next header
      if (got < 8) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
      const uint32_t isize = (uint32_t) h[4] | (uint32_t) h[5] << 8 | (uint32_t) h[6] << 16 | (uint32_t) h[7] << 24;
      if (isize > BGZF_MAX_ISIZE) return bgzf_bad(errbuf, errlen, path, off, "ISIZE is above 65536");
      nb++; nt += isize;
      off += blen;
      have = (size_t) got - 8;
      memmove(h.data(), h.data() + 8, have);
    }
  *blocks = nb; *text = nt;
  return 0;
}

// The text of a BGZF file, chunk after chunk: whole members into infl.chunk, as many as fit it, their text to
// consume(text, n) -> 0 or what ends the run.
// One turn of that: the whole members among the `got` bytes of infl.chunk, which lie at `off` in a file or stream that ends
// at fsize, inflated and consumed.  *used = the bytes of those members; what lies behind them goes on in the next turn.
template <class Consume>
static inline int bgzf_turn(const char *path, Inflater &infl, int64_t got, int64_t off, int64_t fsize, bool stream, std::vector<int64_t> &at,
                            int64_t *used, Consume &&consume, char *errbuf, size_t errlen)
{ int n = 0;
  int64_t p = 0;
  size_t nt = 0;
  while (p < got && n < BGZF_MAX_BLOCKS)
    { int64_t blen = 0; int hlen = 0;
      const int rc = bgzf_member(infl.chunk + p, (size_t) (got - p), path, off + p, fsize, &blen, &hlen, errbuf, errlen, stream);
      if (rc < 0) return rc;
      if (rc == 2 || p + blen > got) break;                     // the member goes on in the next chunk
      const uint8_t *t = infl.chunk + p + blen - 8;
      const uint32_t crc = (uint32_t) t[0] | (uint32_t) t[1] << 8 | (uint32_t) t[2] << 16 | (uint32_t) t[3] << 24;
      const uint32_t isize = (uint32_t) t[4] | (uint32_t) t[5] << 8 | (uint32_t) t[6] << 16 | (uint32_t) t[7] << 24;
      if (isize > BGZF_MAX_ISIZE) return bgzf_bad(errbuf, errlen, path, off + p, "ISIZE is above 65536");
      if (nt + isize > BGZF_TEXT) break;
      infl.blk[n] = BgzfBlock{ (uint32_t) (p + hlen), (uint32_t) (blen - hlen - 8), (uint32_t) nt, isize, crc };
      at[(size_t) n] = off + p;
      n++; nt += isize; p += blen;
    }
  if (n == 0) return bgzf_bad(errbuf, errlen, path, off, stream ? "the member is cut off by the end of the stream"
                                                                : "the member is cut off by the end of the file");
  const uint8_t *text = nullptr;
  int bad = 0;
  const int rc = infl.inflate(n, &text, &bad, errbuf, errlen);
  if (rc < 0) return rc;
  if (rc > 0) return bgzf_bad(errbuf, errlen, path, at[(size_t) bad], infl.reason(rc));
  *used = p;
  return consume(text, nt);
}

// A stream: the chunk is filled by read until it is full or the stream ends (short reads are the rule), and the tail that
// the last whole member leaves is moved to its front for the next turn.  Offsets count from the first byte of the stream.
template <class Consume>
static inline int bgzf_feed_stream(Source &src, const char *path, Inflater &infl, Consume &&consume, char *errbuf, size_t errlen)
{ std::vector<int64_t> at((size_t) BGZF_MAX_BLOCKS);
  int64_t off = 0, have = 0;                                   // chunk[0 .. have) are the bytes of the stream from `off` on
  bool end = false;
  for (;;)
    { while (!end && have < (int64_t) SMG_COUNT_BGZF_CHUNK)
        { const ssize_t r = src.get(infl.chunk + have, (size_t) ((int64_t) SMG_COUNT_BGZF_CHUNK - have));
          if (r < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
          if (r == 0) end = true;
          have += r;
        }
      if (have == 0) return 0;
      int64_t used = 0;
      const int rc = bgzf_turn(path, infl, have, off, end ? off + have : BGZF_NO_END, true, at, &used, consume, errbuf, errlen);
      if (rc) return rc;
      memmove(infl.chunk, infl.chunk + used, (size_t) (have - used));
      have -= used; off += used;
    }
}

template <class Consume>
static inline int bgzf_feed(Source &src, const char *path, Inflater &infl, Consume &&consume, char *errbuf, size_t errlen)
{ if (src.stream) return bgzf_feed_stream(src, path, infl, consume, errbuf, errlen);
  const int fd = src.fd;
  struct stat sb;
  if (fstat(fd, &sb) != 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot read %s", path);
  const int64_t fsize = (int64_t) sb.st_size;
  std::vector<int64_t> at((size_t) BGZF_MAX_BLOCKS);
  int64_t off = 0;
  while (off < fsize)
    { const int64_t want = fsize - off < (int64_t) SMG_COUNT_BGZF_CHUNK ? fsize - off : (int64_t) SMG_COUNT_BGZF_CHUNK;
      int64_t got = 0;
      while (got < want)
        { const ssize_t r = pread(fd, infl.chunk + got, (size_t) (want - got), off + got);
          if (r < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
          if (r == 0) break;
          got += r;
        }
      int64_t used = 0;
      const int rc = bgzf_turn(path, infl, got, off, got < want ? off + got : fsize, false, at, &used, consume, errbuf, errlen);
      if (rc) return rc;
      off += used;
    }
  return 0;
}

// what a FASTA / FASTQ file (dev: what its inflater spent on it) and a BAM file gave, once read to their end
static inline FileRead text_read(const Parser &ps, const InflaterTimes &dev)
{ FileRead r;
  r.route = ROUTE_TEXT; r.records = ps.records; r.bases = ps.bases; r.dev = dev;
  return r;
}
static inline FileRead bam_read(const BamFramer &bam, const InflaterTimes &dev)
{ FileRead r;
  r.route = ROUTE_BAM; r.records = bam.records; r.bases = bam.bases; r.ms_frame = bam.ms_feed; r.dev = dev;
  return r;
}

static inline int parse_fd(Source &src, const char *path, Sink &sink, FileRead *fr, char *errbuf, size_t errlen)
{ std::vector<uint8_t> buf((size_t) 4 << 20);
  Parser ps(sink);
  for (;;)
    { const ssize_t got = src.get(buf.data(), buf.size());
      if (got < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
      if (got == 0) break;
      const int rc = ps.feed(buf.data(), (size_t) got, path, errbuf, errlen);
      if (rc) return rc;
    }
  *fr = text_read(ps, InflaterTimes());
  return 0;
}

static inline bool is_bam_text(const uint8_t *t, size_t n) { return n >= 4 && memcmp(t, "BAM\1", 4) == 0; }

// one piece of the text of a BAM file to the sink: the record the last boundary cut, then what the inflater unpacks
static inline int bam_piece(BamFramer &fr, const uint8_t *t, size_t n, const char *path, Inflater &infl, Sink &sink, char *errbuf, size_t errlen)
{ const double t0 = now_ms();
  const int rc = fr.feed(t, n, path, errbuf, errlen);
  fr.ms_feed += now_ms() - t0;
  if (rc) return rc;
  if (!fr.head.empty() && !sink.put(fr.head.data(), fr.head.size())) return 1;
  return fr.out_len ? infl.unpack(fr.desc.data(), fr.desc.size(), fr.out_len, sink, errbuf, errlen) : 0;
}

// One k-mer dump to the sink in chunks of whole lines (DumpCutter, smg_dump.hpp), its text routed by the header of the file
// as that of reads is: plain, BGZF, or plain gzip where the inflater holds its index.
static inline int parse_dump_file(Source &src, int kind, const char *path, Sink &sink, Inflater *infl, FileRead *fr, char *errbuf, size_t errlen)
{ DumpCutter<Sink> cut(sink);
  const InflaterTimes before = infl ? infl->times() : InflaterTimes();
  int rc = 0;
  if (kind == FILE_PLAIN)
    { std::vector<uint8_t> buf((size_t) 4 << 20);
      for (;;)
        { const ssize_t got = src.get(buf.data(), buf.size());
          if (got < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
          if (got == 0) break;
          if ((rc = cut.feed(buf.data(), (size_t) got, path, errbuf, errlen)) != 0) return rc;
        }
    }
  else if (kind == FILE_GZIP)
    rc = infl->gzip_text(src.fd, path, [&](const uint8_t *t, size_t n) { return cut.feed(t, n, path, errbuf, errlen); }, errbuf, errlen);
  else if (!infl)
    return fail(errbuf, errlen, SMG_EINVAL, "%s is BGZF compressed: this call has no device to inflate it on, "
                "use one of the counting calls or smg_count_dump_records", path);
  else rc = bgzf_feed(src, path, *infl, [&](const uint8_t *t, size_t n) { return cut.feed(t, n, path, errbuf, errlen); }, errbuf, errlen);
  if (rc == 0) rc = cut.finish();
  if (rc) return rc;
  fr->route = ROUTE_DUMP;
  if (infl) fr->dev = infl->times() - before;
  return 0;
}

// one file or stream to the sink, routed by its own header: BGZF through the inflater (and its text by its first bytes: BAM through
// the framer, anything else through the parser), anything else as it is.  *fr: what it gave, where it was read to its end.
// dump: the call reads k-mer dumps, whose text goes to the cutter instead
static inline int parse_file(Source &src, const char *path, Sink &sink, Inflater *infl, FileRead *fr, char *errbuf, size_t errlen, bool dump = false)
{ const int kind = file_kind(src, path, errbuf, errlen, infl && infl->has_gzip(path));
  if (kind < 0) return kind;
  if (dump) return parse_dump_file(src, kind, path, sink, infl, fr, errbuf, errlen);
  if (kind == FILE_PLAIN) return parse_fd(src, path, sink, fr, errbuf, errlen);
  if (kind == FILE_GZIP)
    { Parser ps(sink);
      const InflaterTimes before = infl->times();
      const int rc = infl->gzip_text(src.fd, path, [&](const uint8_t *t, size_t n) { return ps.feed(t, n, path, errbuf, errlen); }, errbuf, errlen);
      if (rc) return rc;
      *fr = text_read(ps, infl->times() - before);
      return 0;
    }
  if (!infl)
    return fail(errbuf, errlen, SMG_EINVAL, "%s is BGZF compressed: this call has no device to inflate it on, "
                "use smg_count_bgzf_inflate or one of the counting calls", path);
  Parser ps(sink);
  BamFramer bam;
  const InflaterTimes before = infl->times();
  int route = ROUTE_NONE;                                      // by the first text there is
  int rc = bgzf_feed(src, path, *infl, [&](const uint8_t *t, size_t n)
    { if (route == ROUTE_NONE && n) route = is_bam_text(t, n) ? ROUTE_BAM : ROUTE_TEXT;
      return route == ROUTE_BAM ? bam_piece(bam, t, n, path, *infl, sink, errbuf, errlen) : ps.feed(t, n, path, errbuf, errlen);
    }, errbuf, errlen);
  if (rc == 0 && route == ROUTE_BAM) rc = bam.finish(path, errbuf, errlen);
  if (rc) return rc;
  const InflaterTimes dev = infl->times() - before;
  *fr = route == ROUTE_BAM ? bam_read(bam, dev) : text_read(ps, dev);
  return 0;
}

struct GrowSink : Sink
{ uint8_t *p = nullptr; size_t len = 0, cap = 0;
  void reserve(size_t n)
  { if (n <= cap) return;
    uint8_t *q = (uint8_t *) realloc(p, n);
    if (!q) throw std::bad_alloc();
    p = q; cap = n;
  }
  bool put(const uint8_t *s, size_t n) override
  { if (len + n > cap)
      { size_t nc = cap ? cap * 2 : (size_t) 1 << 16;
        while (nc < len + n) nc *= 2;
        reserve(nc);
      }
    memcpy(p + len, s, n); len += n;
    return true;
  }
  // the grown stream goes to the caller as a malloc'ed array (one byte where it is empty)
  int hand_over(uint8_t **out, int64_t *n, char *errbuf, size_t errlen)
  { if (!p) p = (uint8_t *) malloc(1);
    if (!p) return fail(errbuf, errlen, SMG_ENOMEM, "out of host memory%s", "");
    *out = p; *n = (int64_t) len;
    p = nullptr; len = cap = 0;
    return 0;
  }
  ~GrowSink() override { free(p); }
};

// the stripped stream of one file or stream as a malloc'ed array
static inline int parse_path(const char *path, uint8_t **seq, int64_t *n, char *errbuf, size_t errlen)
{ if (!path || !seq || !n) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  Taken f(path);
  if (f.file.fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  GrowSink sink;
  FileRead read;
  const int rc = parse_file(f.src, path, sink, nullptr, &read, errbuf, errlen);
  return rc ? rc : sink.hand_over(seq, n, errbuf, errlen);
}

// Refuse what cannot be read before anything is set up for it.  *bound = the most sequence the files can hold: their
// sizes (of a BGZF file: the text its members announce), and k + 1 bytes per file for the separator and the tail a batch
// boundary puts in front of a piece.  bgzf (may be null): per file, is it BGZF (1)?  gzip_ok: the call reads plain gzip; such
// a file is FILE_GZIP in bgzf and adds only its k + 1 bytes: its text is known once its index is built.
// taken (a call that reads streams): per path, the stream as the survey opened it, once, with the bytes it took to tell what
// it is, for the reader thread that gets the file; null for a regular file, which its reader opens itself.  A stream has no
// size: it adds its k + 1 bytes, and the bound is that of the regular files of the call.  Standard input ("-") can be named
// once.  Without `taken` a stream is refused.
static inline int survey_files(const char *const *paths, int npaths, int k, int64_t *bound, char *errbuf, size_t errlen,
                               std::vector<char> *bgzf = nullptr, bool gzip_ok = false, std::vector<std::unique_ptr<Taken>> *taken = nullptr)
{ *bound = 0;
  if (bgzf) bgzf->assign((size_t) npaths, 0);
  if (taken) { taken->clear(); taken->resize((size_t) npaths); }
  for (int f = 0, seen = 0; f < npaths; f++)
    if (is_stdin(paths[f]) && seen++)
      return fail(errbuf, errlen, SMG_EINVAL, "%s (standard input) is named twice: it can be read once", paths[f]);
  for (int f = 0; f < npaths; f++)
    { std::unique_ptr<Taken> in(new Taken(paths[f]));
      const Fd &fd = in->file;
      if (fd.fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", paths[f]);
      if (in->src.stream)
        { if (!taken) return fail(errbuf, errlen, SMG_EINVAL, "%s is a stream: this call reads a file", paths[f]);
          const int kind = file_kind(in->src, paths[f], errbuf, errlen, gzip_ok);
          if (kind < 0) return kind;
          if (bgzf) (*bgzf)[(size_t) f] = (char) kind;
          (*taken)[(size_t) f] = std::move(in);
          *bound += k + 1;
          continue;
        }
      int64_t size = (int64_t) lseek(fd.fd, 0, SEEK_END), blocks = 0;
      if (size < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot read %s", paths[f]);
      int rc = file_kind(in->src, paths[f], errbuf, errlen, gzip_ok);
      if (rc == FILE_BGZF)
        { rc = bgzf_walk(fd.fd, paths[f], &blocks, &size, errbuf, errlen);
          if (bgzf) (*bgzf)[(size_t) f] = FILE_BGZF;
        }
      else if (rc == FILE_GZIP)
        { rc = 0; size = 0;
          if (bgzf) (*bgzf)[(size_t) f] = FILE_GZIP;
        }
      if (rc) return rc;
      *bound += size + k + 1;
    }
  return 0;
}

// members and text bytes of a BGZF file; what is not BGZF is refused with the words of the counting calls
static inline int bgzf_scan(const char *path, int64_t *blocks, int64_t *text_bytes, char *errbuf, size_t errlen)
{ if (!path || !blocks || !text_bytes) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  const int is = refuse_stream(path, errbuf, errlen);
  if (is) return is;
  const Fd f(path);
  if (f.fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  Source src(f.fd, false);
  const int kind = file_kind(src, path, errbuf, errlen);
  if (kind < 0) return kind;
  if (kind == FILE_PLAIN) return fail(errbuf, errlen, SMG_EINVAL, "%s is not BGZF: it does not begin with a gzip header", path);
  return bgzf_walk(f.fd, path, blocks, text_bytes, errbuf, errlen);
}

// ---------------------------------------------------------------------------------------------------------------
//  reader threads and the ring of blocks between them and the one consumer
// ---------------------------------------------------------------------------------------------------------------

struct Block { uint8_t *p; size_t len; int file; };

struct Ring
{ std::mutex m;
  std::condition_variable cv_ready, cv_free;
  std::deque<Block> ready;
  std::vector<uint8_t *> idle;
  size_t block = 0;                                            // bytes every block holds (set before the readers start)
  int live = 0;                                                // readers still at work
  bool abort = false;
  int rc = 0;
  char err[512] = { 0 };
  int64_t bases = 0;
  double t_last = 0;
  std::vector<FileRead> files;                                 // per file: what reading it to its end gave
};

struct RingSink : Sink
{ Ring &r; int file; uint8_t *cur = nullptr; size_t len = 0;
  RingSink(Ring &ring, int f) : r(ring), file(f) {}
  bool push()
  { std::unique_lock<std::mutex> lk(r.m);
    if (r.abort) return false;
    r.ready.push_back(Block{ cur, len, file });
    cur = nullptr; len = 0;
    r.cv_ready.notify_one();
    return true;
  }
  bool put(const uint8_t *p, size_t n) override
  { while (n)
      { if (!cur)
          { std::unique_lock<std::mutex> lk(r.m);
            r.cv_free.wait(lk, [&] { return r.abort || !r.idle.empty(); });
            if (r.abort) return false;
            cur = r.idle.back(); r.idle.pop_back();
          }
        const size_t m = n < r.block - len ? n : r.block - len;
        memcpy(cur + len, p, m);
        len += m; p += m; n -= m;
        if (len == r.block && !push()) return false;
      }
    return true;
  }
  size_t room() const override { return r.block - len; }
  bool cut() override { return !(cur && len) || push(); }
  void done()
  { if (cur && len) push();
    else if (cur) { std::unique_lock<std::mutex> lk(r.m); r.idle.push_back(cur); cur = nullptr; r.cv_free.notify_one(); }
  }
};

// (taken: null, or per path what the survey opened; a path without one is opened here, a stream among them too)
static inline void reader_main(Ring *r, const char *const *paths, int npaths, int first, int step, Inflater *infl, bool dump,
                               const std::unique_ptr<Taken> *taken)
{ for (int f = first; f < npaths; f += step)
    { char eb[512]; eb[0] = 0;
      int rc = 0;
      FileRead read;
      try
        { RingSink sink(*r, f);
          std::unique_ptr<Taken> mine;
          if (!taken || !taken[f]) mine.reset(new Taken(paths[f]));
          Taken &in = mine ? *mine : *taken[f];
          rc = in.file.fd < 0 ? fail(eb, sizeof(eb), SMG_EINVAL, "cannot open %s", paths[f])
                              : parse_file(in.src, paths[f], sink, infl, &read, eb, sizeof(eb), dump);
          if (rc == 0) sink.done();
        }
      catch (...) { rc = fail(eb, sizeof(eb), SMG_ENOMEM, "out of host memory while reading %s", paths[f]); }
      std::unique_lock<std::mutex> lk(r->m);
      r->bases += read.bases;
      r->files[(size_t) f] = read;
      if (rc < 0 && !r->rc) { r->rc = rc; memcpy(r->err, eb, sizeof(eb)); r->abort = true; r->cv_free.notify_all(); }
      if (rc != 0 || r->abort) break;
    }
  std::unique_lock<std::mutex> lk(r->m);
  r->live--;
  r->t_last = now_ms();
  r->cv_ready.notify_all();
}

// reader threads for `want` asked for: one file each, at most 16
static inline int reader_threads(int want, int npaths)
{ const int n = want < 1 ? 1 : want > 16 ? 16 : want;
  return n < npaths ? n : npaths;
}

// The files, stripped, to one consumer: thread j of nthr reads files j, j + nthr, .. into the blocks (nblocks >= 1 of
// `block` bytes each, the caller's: 2 nthr + 2 keep every reader and the consumer busy), and this thread hands every
// filled block to consume(bytes, length, file) -> 0 or an error code, the blocks of one file in the order of the file.
// After the first error, a reader's or the consumer's, nothing more is consumed; the blocks in flight are drained and
// every thread is joined before this returns.  A reader's error (code and message) goes in front of the consumer's, whose
// message is its own business.  *bases = sequence bytes read, *t_last = now_ms() when the last reader was done.
// *files = per file what reading it gave (route ROUTE_NONE: it was not read to its end), after an error as well.
// infl (may be null: BGZF files are refused): the inflater of thread j, or null where none of its files is BGZF.
// dump: the files are k-mer dumps; every block then holds whole lines of one file.
// taken (may be null): per path, the stream the survey opened and took bytes from (survey_files), or null.
template <class Consume>
static inline int read_files(const char *const *paths, int npaths, int nthr, uint8_t *const *blocks, int nblocks, size_t block, Consume &&consume,
                             int64_t *bases, double *t_last, std::vector<FileRead> *files, char *errbuf, size_t errlen,
                             Inflater *const *infl = nullptr, bool dump = false, const std::unique_ptr<Taken> *taken = nullptr)
{ Ring ring;
  ring.block = block;
  ring.files.assign((size_t) npaths, FileRead());
  ring.idle.assign(blocks, blocks + nblocks);
  std::vector<std::thread> thr;
  thr.reserve((size_t) nthr);
  int rc = 0;
  for (int j = 0; j < nthr && rc == 0; j++)
    { try
        { { std::unique_lock<std::mutex> lk(ring.m); ring.live++; }
          thr.emplace_back(reader_main, &ring, paths, npaths, j, nthr, infl ? infl[j] : nullptr, dump, taken);
        }
      catch (...)
        { std::unique_lock<std::mutex> lk(ring.m);
          ring.live--; ring.abort = true; ring.cv_free.notify_all();
          rc = fail(errbuf, errlen, SMG_ENOMEM, "cannot start reader thread %d", j);
        }
    }
  for (;;)
    { Block b{ nullptr, 0, 0 };
      { std::unique_lock<std::mutex> lk(ring.m);
        ring.cv_ready.wait(lk, [&] { return !ring.ready.empty() || ring.live == 0; });
        if (ring.ready.empty()) break;
        b = ring.ready.front(); ring.ready.pop_front();
      }
      if (rc == 0) rc = consume(b.p, (int64_t) b.len, b.file);
      std::unique_lock<std::mutex> lk(ring.m);
      ring.idle.push_back(b.p);
      if (rc) ring.abort = true;
      ring.cv_free.notify_all();
    }
  for (std::thread &th : thr) th.join();
  files->swap(ring.files);
  if (ring.rc) return fail(errbuf, errlen, ring.rc, "%s", ring.err);
  if (rc) return rc;
  *bases = ring.bases;
  *t_last = ring.t_last;
  return 0;
}
