// dump_check.cpp -- the k-mer dump route (smg_dump.hpp: the line decoder that kd_lines compiles, the cutter in front of the
// batch, the host twin) on the host under the address and undefined-behaviour sanitizers (`make dump_check`).
//   pieces     seeded dumps (k = 13 .. 128, both separators, CRLF, lower case, 1 .. 20 digits, a last line without its line
//              end) handed to the cutter in pieces of every size from 1 to SMG_COUNT_DUMP_LINE + 2: the records are those of the
//              one-piece run and of a decoder written here from the grammar; the same through a sink of small blocks (the ring of
//              the reader threads): every block ends with a line and the blocks add up to the text
//   mutants    a few ten thousand mutated dumps (bytes overwritten, inserted, removed; lines cut, doubled, made overlong): each
//              is read or refused with one of the four reasons at the offset of a line start -- the first line that the
//              decoder written here refuses --, the same at every piece size tried
// Every text is malloc'ed at its exact size, so a read outside is reported.  Host only; no device code.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "smg_dump.hpp"

typedef std::vector<uint8_t> Bytes;

static int bad = 0;
static void expect(bool ok, const char *what, const std::string &detail)
{ if (!ok && bad < 50) printf("FAILED  %s (%s)\n", what, detail.c_str());
  if (!ok) bad++;
}

struct Result
{ int rc = 0;                                                  // 0 read, SMG_EINVAL no dump, SMG_EFORMAT a bad line
  int reason = 0;
  int64_t off = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> counts;
  bool operator==(const Result &o) const { return rc == o.rc && reason == o.reason && off == o.off && keys == o.keys && counts == o.counts; }
};

// ---- a decoder of its own, from the grammar: byte by byte, nothing shared with smg_dump.hpp ---------------------------------
static int base_of(uint8_t c)
{ switch (c)
    { case 'A': case 'a': return 0;
      case 'C': case 'c': return 1;
      case 'G': case 'g': return 2;
      case 'T': case 't': return 3;
    }
  return -1;
}

static Result reference(const Bytes &t, int k)
{ Result r;
  const int W = (k + 31) / 32;
  if (!t.empty() && base_of(t[0]) < 0) { r.rc = SMG_EINVAL; return r; }
  size_t p = 0;
  while (p < t.size())
    { size_t e = p;
      while (e < t.size() && t[e] != '\n') e++;                // the line is t[p .. e), with or without a '\n' at e
      std::string line(t.begin() + (long) p, t.begin() + (long) e);
      if (!line.empty() && line.back() == '\r') line.pop_back();
      int reason = 0;
      unsigned __int128 v = 0;
      bool basesok = (int) line.size() > k;
      for (int j = 0; basesok && j < k; j++) basesok = base_of((uint8_t) line[(size_t) j]) >= 0;
      if (!basesok || (line[(size_t) k] != ' ' && line[(size_t) k] != '\t')) reason = DUMP_BASES;
      else
        { size_t d = (size_t) k + 1, nd = 0;
          while (d + nd < line.size() && line[d + nd] >= '0' && line[d + nd] <= '9' && nd < 20) { v = v * 10 + (unsigned) (line[d + nd] - '0'); nd++; }
          // (a '\r' inside the line that is not its last byte ends the digits like any other byte)
          if (nd == 0) reason = DUMP_NOCOUNT;
          else if (d + nd != line.size()) reason = DUMP_NOEND;
          else if (v == 0) reason = DUMP_ZERO;
        }
      if (reason) { r.rc = SMG_EFORMAT; r.reason = reason; r.off = (int64_t) p; r.keys.clear(); r.counts.clear(); return r; }
      std::vector<int> fw((size_t) k), rc((size_t) k);
      for (int j = 0; j < k; j++) fw[(size_t) j] = base_of((uint8_t) line[(size_t) j]);
      for (int j = 0; j < k; j++) rc[(size_t) j] = 3 - fw[(size_t) (k - 1 - j)];
      const std::vector<int> &c = rc < fw ? rc : fw;
      std::vector<uint64_t> key((size_t) W, 0);
      for (int j = 0; j < k; j++) key[(size_t) (j >> 5)] |= (uint64_t) c[(size_t) j] << (62 - 2 * (j & 31));
      r.keys.insert(r.keys.end(), key.begin(), key.end());
      r.counts.push_back(v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) v);
      p = e + 1;
    }
  return r;
}

// ---- the twin: the cutter in pieces of `piece` bytes into DumpHost, or through blocks of `block` bytes first ----------------
struct BlockSink                                               // what RingSink is to the cutter: blocks of a fixed size
{ DumpHost &host;
  size_t block;
  Bytes cur;
  int64_t total = 0;
  bool lines_ok = true;
  BlockSink(DumpHost &h, size_t b) : host(h), block(b) {}
  size_t room() const { return block - cur.size(); }
  bool cut()
  { if (cur.empty()) return true;
    if (cur.back() != '\n') lines_ok = false;
    uint8_t *exact = (uint8_t *) malloc(cur.size());           // (exact size: the decoder must not read past a block)
    memcpy(exact, cur.data(), cur.size());
    const bool ok = host.put(exact, cur.size());
    free(exact);
    total += (int64_t) cur.size();
    cur.clear();
    return ok;
  }
  bool put(const uint8_t *p, size_t n)
  { while (n)
      { const size_t m = n < room() ? n : room();
        cur.insert(cur.end(), p, p + m);
        p += m; n -= m;
        if (cur.size() == block && !cut()) return false;
      }
    return true;
  }
};

template <class S> static int feed_all(DumpCutter<S> &cut, const Bytes &t, size_t piece)
{ char err[256];
  for (size_t o = 0; o < t.size(); o += piece)
    { const size_t m = t.size() - o < piece ? t.size() - o : piece;
      uint8_t *exact = (uint8_t *) malloc(m);
      memcpy(exact, t.data() + o, m);
      const int rc = cut.feed(exact, m, "<text>", err, sizeof(err));
      free(exact);
      if (rc) return rc;
    }
  return cut.finish();
}

static Result finish(const DumpHost &h, int rc)
{ Result r;
  if (rc < 0) { r.rc = rc; return r; }
  if (h.bad) { r.rc = SMG_EFORMAT; r.reason = h.bad; r.off = h.bad_off; return r; }
  r.keys = h.keys; r.counts = h.counts;
  return r;
}

static Result twin(const Bytes &t, int k, size_t piece)
{ DumpHost h(k);
  DumpCutter<DumpHost> cut(h);
  return finish(h, feed_all(cut, t, piece ? piece : (t.size() ? t.size() : 1)));
}

static Result twin_blocks(const Bytes &t, int k, size_t piece, size_t block, bool *lines_ok)
{ DumpHost h(k);
  BlockSink sink(h, block);
  DumpCutter<BlockSink> cut(sink);
  int rc = feed_all(cut, t, piece);
  if (rc == 0 && !sink.cut()) rc = 1;
  *lines_ok = sink.lines_ok;
  return finish(h, rc);
}

static Bytes make_dump(std::mt19937_64 &rng, int k, int lines, bool last_end)
{ Bytes t;
  for (int i = 0; i < lines; i++)
    { std::string l;
      const bool lower = rng() % 4 == 0;
      for (int j = 0; j < k; j++) l += (lower ? "acgt" : "ACGT")[rng() % 4];
      l += rng() % 2 ? ' ' : '\t';
      const int nd = 1 + (int) (rng() % 20);
      for (int j = 0; j < nd; j++) l += (char) ('0' + (j == nd - 1 ? 1 + rng() % 9 : rng() % 10));
      if (i + 1 < lines || last_end) l += rng() % 3 == 0 ? "\r\n" : "\n";
      t.insert(t.end(), l.begin(), l.end());
    }
  return t;
}

static std::string show(const Result &r)
{ return "rc " + std::to_string(r.rc) + " reason " + std::to_string(r.reason) + " offset " + std::to_string(r.off) + " records " + std::to_string(r.counts.size()); }

int main()
{ std::mt19937_64 rng(20240607);
  const int ks[] = { 13, 31, 32, 33, 64, 65, 96, 97, 128 };

  int64_t runs = 0;
  for (int k : ks)
    for (int last = 0; last < 2; last++)
      { const Bytes t = make_dump(rng, k, 60, last != 0);
        const Result want = reference(t, k), one = twin(t, k, 0);
        expect(want.rc == 0 && want.counts.size() == 60, "the reference reads a valid dump", show(want));
        expect(one == want, "one piece equals the reference", "k " + std::to_string(k) + ": " + show(one) + " / " + show(want));
        for (size_t piece = 1; piece <= SMG_COUNT_DUMP_LINE + 2; piece++)
          { expect(twin(t, k, piece) == one, "every piece size equals one piece", "k " + std::to_string(k) + " piece " + std::to_string(piece));
            bool lines_ok = false;
            const size_t block = SMG_COUNT_DUMP_LINE + 2 + (piece * 7) % 300;
            expect(twin_blocks(t, k, piece, block, &lines_ok) == one && lines_ok, "blocks of whole lines equal one piece",
                   "k " + std::to_string(k) + " piece " + std::to_string(piece) + " block " + std::to_string(block));
            runs += 2;
          }
      }
  printf("valid dumps: %lld runs of the twin over %zu values of k, pieces of 1 .. %d bytes, blocks of %d .. %d\n", (long long) runs,
         sizeof(ks) / sizeof(ks[0]), SMG_COUNT_DUMP_LINE + 2, SMG_COUNT_DUMP_LINE + 2, SMG_COUNT_DUMP_LINE + 2 + 299);

  int64_t mutants = 0, read = 0, refused[5] = { 0, 0, 0, 0, 0 }, nodump = 0;
  for (int it = 0; it < 40000; it++)
    { const int k = ks[rng() % 9];
      Bytes t = make_dump(rng, k, 1 + (int) (rng() % 12), rng() % 4 != 0);
      const int nmut = 1 + (int) (rng() % 3);
      for (int m = 0; m < nmut && !t.empty(); m++)
        { const size_t at = rng() % t.size();
          static const char pool[] = "ACGTacgtNn \t\r\n0123456789-+.,>@";
          switch (rng() % 6)
            { case 0: t[at] = (uint8_t) pool[rng() % (sizeof(pool) - 1)]; break;
              case 1: t.insert(t.begin() + (long) at, (uint8_t) pool[rng() % (sizeof(pool) - 1)]); break;
              case 2: t.erase(t.begin() + (long) at); break;
              case 3: t.resize(at); break;
              case 4: t.insert(t.begin() + (long) at, 1 + rng() % 400, (uint8_t) "A7 \r"[rng() % 4]); break;      // overlong lines
              case 5: t[at] = (uint8_t) (rng() & 0xFF); break;
            }
        }
      const Result want = reference(t, k);
      const size_t pieces[4] = { 0, 1, 1 + (size_t) (rng() % (SMG_COUNT_DUMP_LINE + 2)), 1 + (size_t) (rng() % 700) };
      for (size_t piece : pieces)
        { const Result got = twin(t, k, piece);
          const bool known = got.rc == 0 || got.rc == SMG_EINVAL || (got.rc == SMG_EFORMAT && got.reason >= DUMP_BASES && got.reason <= DUMP_NOEND);
          expect(known, "a mutant is read or refused with one of the four reasons", show(got));
          expect(got == want, "a mutant is read or refused as the reference reads or refuses it",
                 "k " + std::to_string(k) + " piece " + std::to_string(piece) + ": " + show(got) + " / " + show(want));
          bool lines_ok = false;
          const Result blk = twin_blocks(t, k, piece ? piece : 64, SMG_COUNT_DUMP_LINE + 2 + (size_t) (rng() % 200), &lines_ok);
          expect(blk == want && lines_ok, "through blocks as well", "k " + std::to_string(k) + ": " + show(blk) + " / " + show(want));
        }
      mutants++;
      if (want.rc == 0) read++; else if (want.rc == SMG_EINVAL) nodump++; else refused[want.reason]++;
    }
  printf("mutated dumps: %lld, each at 4 piece sizes and through blocks: %lld read, %lld no dump (first byte), refused: %lld bases/separator, "
         "%lld no count, %lld count 0, %lld no line end\n", (long long) mutants, (long long) read, (long long) nodump, (long long) refused[DUMP_BASES],
         (long long) refused[DUMP_NOCOUNT], (long long) refused[DUMP_ZERO], (long long) refused[DUMP_NOEND]);
  if (bad) { printf("dump_check: %d FAILED\n", bad); return 1; }
  printf("dump_check: all passed\n");
  return 0;
}
