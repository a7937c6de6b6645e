// smg_count_reader.hpp -- the host side in front of the k-mer counter: FASTA / FASTQ files -> stripped sequence bytes, and
// the reader threads that deliver them block by block (smg_count.hip holds the map of the whole counter).  Host only, no
// HIP: `make reader_check` runs it under the address, undefined-behaviour and thread sanitizers (reader_check.cpp).

#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "smg_count.h"
#include "smg_count_err.hpp"

static inline double now_ms()
{ return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Sink
{ virtual bool put(const uint8_t *p, size_t n) = 0;          // false: the consumer gave up
  virtual ~Sink() {}
};

// Line-wise state machine over the bytes of one file, fed in arbitrary pieces.  A '\r' is dropped only in front of a
// '\n' or at the end of the file; anywhere else it is a byte like any other (and ends a stretch).
struct Parser
{ Sink &out;
  int fmt = 0, phase = 0, kind = 0;                           // fmt 1 FASTA, 2 FASTQ; kind 0 skip, 1 sequence, 2 blank
  bool bol = true, first = true, pending_cr = false, started = false;
  int64_t bases = 0;
  explicit Parser(Sink &s) : out(s) {}

  bool emit(const uint8_t *p, size_t n) { bases += (int64_t) n; return n == 0 || out.put(p, n); }
  bool record() { const uint8_t sep = SMG_COUNT_SEPARATOR; const bool ok = first || out.put(&sep, 1); first = false; return ok; }

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

static inline int parse_fd(int fd, const char *path, Sink &sink, int64_t *bases, char *errbuf, size_t errlen)
{ std::vector<uint8_t> buf((size_t) 4 << 20);
  Parser ps(sink);
  for (;;)
    { const ssize_t got = read(fd, buf.data(), buf.size());
      if (got < 0) return fail(errbuf, errlen, SMG_EINVAL, "read error on %s", path);
      if (got == 0) break;
      const int rc = ps.feed(buf.data(), (size_t) got, path, errbuf, errlen);
      if (rc) return rc;
    }
  if (bases) *bases = ps.bases;
  return 0;
}

struct GrowSink : Sink
{ uint8_t *p = nullptr; size_t len = 0, cap = 0;
  bool put(const uint8_t *s, size_t n) override
  { if (len + n > cap)
      { size_t nc = cap ? cap * 2 : (size_t) 1 << 16;
        while (nc < len + n) nc *= 2;
        uint8_t *q = (uint8_t *) realloc(p, nc);
        if (!q) throw std::bad_alloc();
        p = q; cap = nc;
      }
    memcpy(p + len, s, n); len += n;
    return true;
  }
  ~GrowSink() override { free(p); }
};

// the stripped stream of one file as a malloc'ed array (one byte where it is empty)
static inline int parse_path(const char *path, uint8_t **seq, int64_t *n, char *errbuf, size_t errlen)
{ if (!path || !seq || !n) return fail(errbuf, errlen, SMG_EINVAL, "bad arguments%s", "");
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", path);
  GrowSink sink;
  int rc;
  try { rc = parse_fd(fd, path, sink, nullptr, errbuf, errlen); }
  catch (...) { close(fd); throw; }
  close(fd);
  if (rc) return rc;
  if (!sink.p) sink.p = (uint8_t *) malloc(1);
  *seq = sink.p; *n = (int64_t) sink.len;
  sink.p = nullptr;
  return 0;
}

// Refuse what cannot be read before anything is set up for it.  *bound = the most sequence the files can hold: their
// sizes, and k + 1 bytes per file for the separator and the tail a batch boundary puts in front of a piece.
static inline int survey_files(const char *const *paths, int npaths, int k, int64_t *bound, char *errbuf, size_t errlen)
{ *bound = 0;
  for (int f = 0; f < npaths; f++)
    { uint8_t magic[2] = { 0, 0 };
      const int fd = open(paths[f], O_RDONLY);
      if (fd < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot open %s", paths[f]);
      const ssize_t got = read(fd, magic, 2);
      const off_t size = lseek(fd, 0, SEEK_END);
      close(fd);
      if (got < 0 || size < 0) return fail(errbuf, errlen, SMG_EINVAL, "cannot read %s", paths[f]);
      if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b)
        return fail(errbuf, errlen, SMG_EINVAL, "%s is gzip compressed: compressed input is not supported, decompress it first", paths[f]);
      *bound += (int64_t) size + k + 1;
    }
  return 0;
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
  void done()
  { if (cur && len) push();
    else if (cur) { std::unique_lock<std::mutex> lk(r.m); r.idle.push_back(cur); cur = nullptr; r.cv_free.notify_one(); }
  }
};

static inline void reader_main(Ring *r, const char *const *paths, int npaths, int first, int step)
{ for (int f = first; f < npaths; f += step)
    { char eb[512]; eb[0] = 0;
      int rc = 0;
      int64_t bases = 0;
      try
        { RingSink sink(*r, f);
          const int fd = open(paths[f], O_RDONLY);
          if (fd < 0) rc = fail(eb, sizeof(eb), SMG_EINVAL, "cannot open %s", paths[f]);
          else
            { rc = parse_fd(fd, paths[f], sink, &bases, eb, sizeof(eb));
              close(fd);
            }
          if (rc == 0) sink.done();
        }
      catch (...) { rc = fail(eb, sizeof(eb), SMG_ENOMEM, "out of host memory while reading %s", paths[f]); }
      std::unique_lock<std::mutex> lk(r->m);
      r->bases += bases;
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
template <class Consume>
static inline int read_files(const char *const *paths, int npaths, int nthr, uint8_t *const *blocks, int nblocks, size_t block, Consume &&consume,
                             int64_t *bases, double *t_last, char *errbuf, size_t errlen)
{ Ring ring;
  ring.block = block;
  ring.idle.assign(blocks, blocks + nblocks);
  std::vector<std::thread> thr;
  thr.reserve((size_t) nthr);
  int rc = 0;
  for (int j = 0; j < nthr && rc == 0; j++)
    { try
        { { std::unique_lock<std::mutex> lk(ring.m); ring.live++; }
          thr.emplace_back(reader_main, &ring, paths, npaths, j, nthr);
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
  if (ring.rc) return fail(errbuf, errlen, ring.rc, "%s", ring.err);
  if (rc) return rc;
  *bases = ring.bases;
  *t_last = ring.t_last;
  return 0;
}
