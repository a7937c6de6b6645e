// gzip_check.cpp -- the plain-gzip route (smg_gzip.hpp: finder, marker decoder, chain, resolver, exact decoder -- the text
// the kernels compile) on the host as one lane against zlib, under the address and undefined-behaviour sanitizers
// (`make gzip_check`).  Every buffer of the twin is malloc'ed at its exact size, so a read or a write outside is reported.
//   valid files     zlib at levels 0/1/6/9, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, memLevel 1, a sync flush inside, several
//                   members (an empty one among them), optional header fields, trailing zeros, gzip inside stored gzip; at
//                   spans of 1 KiB, 4 KiB, 64 KiB and 1 MiB: the text of zlib's own inflate
//   mutated files   seeded bit flips, truncations, overwritten and inserted bytes for as long as the time allows (the
//                   number is printed): the call returns, the sanitizers stay silent, and the file is accepted exactly
//                   where zlib accepts it -- with equal bytes
// Host only; no device code.

#include <zlib.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "smg_gzip.hpp"

typedef std::vector<uint8_t> Bytes;

static int bad = 0;
static void expect(bool ok, const char *what, const std::string &detail)
{ if (!ok && bad < 50) printf("FAILED  %s (%s)\n", what, detail.c_str());
  if (!ok) bad++;
}

static Bytes make_text(std::mt19937_64 &rng, size_t n)
{ Bytes t;
  int r = 0;
  while (t.size() < n)
    { std::string rec = "@read" + std::to_string(r++) + "\n";
      const size_t len = 30 + rng() % 120;
      for (size_t j = 0; j < len; j++) rec += "ACGTN"[rng() % 100 < 99 ? rng() % 4 : 4];
      rec += "\n+\n";
      for (size_t j = 0; j < len; j++) rec += (char) ('!' + (rng() % 8 == 0 ? rng() % 40 : 40));
      rec += "\n";
      t.insert(t.end(), rec.begin(), rec.end());
      if (t.size() > n / 2 && t.size() < n / 2 + 400) t.insert(t.end(), n / 8, (uint8_t) 'A');      // a run of one base
    }
  return t;
}

static Bytes gz(const Bytes &text, int level, int strategy, int mem, bool flush, int fields)
{ z_stream z;
  memset(&z, 0, sizeof(z));
  if (deflateInit2(&z, level, Z_DEFLATED, 31, mem, strategy) != Z_OK) { printf("FAILED  deflateInit2\n"); exit(1); }
  gz_header h;
  static uint8_t extra[5] = { 'X', 'Y', 1, 0, 7 };
  if (fields)
    { memset(&h, 0, sizeof(h));
      h.extra = extra; h.extra_len = 5; h.name = (Bytef *) "reads.fq"; h.comment = (Bytef *) "a comment"; h.hcrc = 1;
      deflateSetHeader(&z, &h);
    }
  Bytes out(deflateBound(&z, (uLong) text.size()) + 256);
  static uint8_t none;
  z.next_out = out.data(); z.avail_out = (uInt) out.size();
  const size_t half = flush ? text.size() / 2 : 0;
  z.next_in = text.empty() ? &none : (Bytef *) text.data(); z.avail_in = (uInt) half;
  if (flush && deflate(&z, Z_SYNC_FLUSH) != Z_OK) { printf("FAILED  deflate(Z_SYNC_FLUSH)\n"); exit(1); }
  z.avail_in = (uInt) (text.size() - half);
  if (deflate(&z, Z_FINISH) != Z_STREAM_END) { printf("FAILED  deflate(Z_FINISH)\n"); exit(1); }
  out.resize(z.total_out);
  deflateEnd(&z);
  return out;
}

struct Ref { bool ok; Bytes text; };

// zlib's verdict: members one after the other, then nothing or zeros
static Ref reference(const Bytes &file)
{ Ref r{ false, Bytes() };
  z_stream z;
  memset(&z, 0, sizeof(z));
  if (inflateInit2(&z, 31) != Z_OK) { printf("FAILED  inflateInit2\n"); exit(1); }
  static uint8_t none;
  Bytes buf((size_t) 1 << 16);
  z.next_in = file.empty() ? &none : (Bytef *) file.data(); z.avail_in = (uInt) file.size();
  for (;;)
    { z.next_out = buf.data(); z.avail_out = (uInt) buf.size();
      const int rc = inflate(&z, Z_NO_FLUSH);
      r.text.insert(r.text.end(), buf.data(), buf.data() + (buf.size() - z.avail_out));
      if (rc == Z_STREAM_END)
        { bool zeros = true;
          for (uInt i = 0; i < z.avail_in; i++) if (z.next_in[i]) zeros = false;
          if (zeros) { r.ok = true; break; }
          inflateReset(&z);
          continue;
        }
      if (rc != Z_OK || (z.avail_in == 0 && z.avail_out != 0)) break;
    }
  inflateEnd(&z);
  if (!r.ok) r.text.clear();
  return r;
}

static GzHostEngine *engine;

static bool ours(const Bytes &file, uint32_t span, Bytes &text, GzIndex &ix, std::string &msg)
{ FILE *f = tmpfile();
  if (!f) { printf("FAILED  tmpfile\n"); exit(1); }
  if (!file.empty() && fwrite(file.data(), 1, file.size(), f) != file.size()) { printf("FAILED  fwrite\n"); exit(1); }
  fflush(f);
  char err[512]; err[0] = 0;
  const int rc = gz_text_host(fileno(f), "<file>", span, (size_t) 1 << 20, (size_t) 1 << 19, *engine, ix, text, err, sizeof(err));
  fclose(f);
  msg = err;
  return rc == 0;
}

int main()
{ std::mt19937_64 rng(20240611);
  engine = new GzHostEngine();
  const Bytes text = make_text(rng, 300000), small = make_text(rng, 40000);
  struct File { Bytes bytes; std::string what; };
  std::vector<File> files;
  const uint32_t spans[4] = { 1u << 10, 4u << 10, 64u << 10, 1u << 20 };
  for (const Bytes *t : { &text, &small })
    { const std::string sz = " of " + std::to_string(t->size());
      for (int level : { 1, 6, 9, 0 }) files.push_back(File{ gz(*t, level, Z_DEFAULT_STRATEGY, 8, false, 0), "level " + std::to_string(level) + sz });
      files.push_back(File{ gz(*t, 6, Z_FIXED, 8, false, 0), "Z_FIXED" + sz });
      files.push_back(File{ gz(*t, 6, Z_HUFFMAN_ONLY, 8, false, 0), "Z_HUFFMAN_ONLY" + sz });
      files.push_back(File{ gz(*t, 6, Z_RLE, 8, false, 0), "Z_RLE" + sz });
      files.push_back(File{ gz(*t, 6, Z_DEFAULT_STRATEGY, 1, false, 0), "memLevel 1" + sz });
      files.push_back(File{ gz(*t, 6, Z_DEFAULT_STRATEGY, 8, true, 0), "sync flush" + sz });
      files.push_back(File{ gz(*t, 6, Z_DEFAULT_STRATEGY, 8, false, 1), "header fields" + sz });
      { Bytes two = gz(*t, 6, Z_DEFAULT_STRATEGY, 8, false, 0);
        const Bytes b = gz(Bytes(t->begin(), t->begin() + (long) t->size() / 3), 9, Z_DEFAULT_STRATEGY, 8, false, 1), none = gz(Bytes(), 6, Z_DEFAULT_STRATEGY, 8, false, 0);
        two.insert(two.end(), none.begin(), none.end());
        two.insert(two.end(), b.begin(), b.end());
        files.push_back(File{ two, "three members" + sz });
        two.insert(two.end(), 100, 0);
        files.push_back(File{ two, "trailing zeros" + sz });
      }
      files.push_back(File{ gz(gz(*t, 6, Z_DEFAULT_STRATEGY, 8, false, 0), 0, Z_DEFAULT_STRATEGY, 8, false, 0), "gzip in stored gzip" + sz });
    }
  { Bytes many;
    for (int i = 0; i < 50; i++)
      { const Bytes m = gz(i == 17 ? Bytes() : Bytes(text.begin() + i * 5000, text.begin() + (i + 1) * 5000 + i), 1 + i % 9, Z_DEFAULT_STRATEGY, 8, false, i % 7 == 0);
        many.insert(many.end(), m.begin(), m.end());
      }
    files.push_back(File{ many, "fifty members" });
  }
  int nvalid = 0;
  for (const File &f : files)
    { const Ref ref = reference(f.bytes);
      expect(ref.ok, "zlib reads the valid file", f.what);
      for (uint32_t span : spans)
        { Bytes got; GzIndex ix; std::string msg;
          const bool ok = ours(f.bytes, span, got, ix, msg);
          expect(ok, "a valid file is read", f.what + ", span " + std::to_string(span) + ": " + msg);
          if (ok) expect(got == ref.text, "the text is zlib's", f.what + ", span " + std::to_string(span));
          if (ok && span == 4096)
            printf("  %-34s %8zu bytes  span 4096: %lld spans, %lld linked, %lld repaired, %zu restart points\n", f.what.c_str(), f.bytes.size(),
                   (long long) ix.spans, (long long) ix.linked, (long long) ix.repaired, ix.pts.size());
          nvalid++;
        }
    }
  printf("%d runs over %zu valid files\n", nvalid, files.size());

  const char *budget = getenv("GZIP_CHECK_SECONDS");
  const double seconds = budget ? atof(budget) : 50.0;
  const auto t0 = std::chrono::steady_clock::now();
  long nmut = 0, naccepted = 0;
  while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < seconds)
    { const File &f = files[files.size() / 2 + rng() % (files.size() - files.size() / 2)];       // (the small ones and the fifty members)
      Bytes m = f.bytes;
      const int kind = (int) (rng() % 6);
      if (kind == 0) m[rng() % m.size()] ^= (uint8_t) (1u << (rng() % 8));
      else if (kind == 1) m.resize(rng() % m.size());
      else if (kind == 2) m[rng() % m.size()] = (uint8_t) rng();
      else if (kind == 3) m.insert(m.begin() + (long) (rng() % m.size()), (uint8_t) rng());
      else if (kind == 4) { const size_t at = rng() % 64 < 32 ? rng() % 24 : m.size() - 1 - rng() % 12; m[at % m.size()] = (uint8_t) rng(); }
      else for (int j = 0; j < 3; j++) m[rng() % m.size()] ^= (uint8_t) (1u << (rng() % 8));
      const Ref ref = reference(m);
      Bytes got; GzIndex ix; std::string msg;
      const uint32_t span = spans[rng() % 3];
      const bool ok = ours(m, span, got, ix, msg);
      const std::string what = f.what + ", mutation " + std::to_string(nmut) + " of kind " + std::to_string(kind) + ", span " + std::to_string(span) + ": " + msg;
      expect(ok == ref.ok, ref.ok ? "what zlib accepts is accepted" : "what zlib refuses is refused", what);
      if (ok && ref.ok) expect(got == ref.text, "the text of a mutated file is zlib's", what);
      if (!ok) expect(!msg.empty(), "a refusal has a message", what);
      nmut++; naccepted += ok;
    }
  printf("%ld mutated files in %.0f s, %ld of them accepted\n", nmut, seconds, naccepted);
  delete engine;
  if (bad) { printf("%d FAILED\n", bad); return 1; }
  printf("gzip_check: all ok\n");
  return 0;
}
