// reader_check.cpp -- the reader threads of the k-mer counter and their ring of blocks (smg_count_reader.hpp: read_files)
// on the host, as the counter runs them but with malloc'ed blocks: the blocks of every file, put together in the order
// they were delivered, against Parser run over the whole file in one piece; and the three ways a run is given up.
// Built once with -fsanitize=address,undefined and once with -fsanitize=thread, run under a time limit: a hang is a
// failure (`make reader_check`).  Host only; no device code.

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "smg_count_reader.hpp"

typedef std::vector<uint8_t> Bytes;

static int bad = 0;
static void expect(bool ok, const char *what, const std::string &detail)
{ if (!ok) { printf("FAILED  %s (%s)\n", what, detail.c_str()); bad++; }
}

static std::string bases(std::mt19937_64 &rng, size_t n)
{ std::string s(n, 'A');
  for (char &c : s) c = "ACGTacgtN"[rng() % 9];
  return s;
}

// FASTA or FASTQ text: records of 0 .. maxlen bases (an empty record now and then), FASTA sequence over several lines,
// '\n' or "\r\n" line ends, with or without a final newline
static std::string make_text(std::mt19937_64 &rng, bool fastq, int records, size_t maxlen, bool crlf, bool final_newline)
{ const std::string nl = crlf ? "\r\n" : "\n";
  std::string t;
  for (int r = 0; r < records; r++)
    { const std::string s = rng() % 5 == 0 ? std::string() : bases(rng, rng() % (maxlen + 1));
      t += (fastq ? "@r" : ">r") + std::to_string(r) + " some text" + nl;
      if (fastq) t += s + nl + "+" + nl + std::string(s.size(), 'I') + nl;
      else
        for (size_t o = 0; o < s.size() || o == 0; o += 70)
          { t += s.substr(o, 70) + nl;
            if (s.empty()) break;
          }
      if (fastq && rng() % 7 == 0) t += nl;                    // a blank line between two records
    }
  if (!final_newline && t.size() >= nl.size()) t.resize(t.size() - nl.size());
  return t;
}

struct VecSink : Sink
{ Bytes v;
  bool put(const uint8_t *p, size_t n) override { v.insert(v.end(), p, p + n); return true; }
};

static Bytes parse_whole(const std::string &text)
{ VecSink s;
  Parser ps(s);
  char eb[256];
  if (ps.feed((const uint8_t *) text.data(), text.size(), "text", eb, sizeof(eb)) != 0) { printf("FAILED  the parser refuses a test file: %s\n", eb); exit(1); }
  return s.v;
}

static std::string write_file(const std::string &dir, int i, const std::string &text)
{ const std::string path = dir + "/f" + std::to_string(i);
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(text.data(), 1, text.size(), f) != text.size()) { printf("FAILED  cannot write %s\n", path.c_str()); exit(1); }
  fclose(f);
  return path;
}

struct Blocks                                                  // malloc'ed, each of exactly `size` bytes: an overrun is reported
{ std::vector<uint8_t *> p;
  Blocks(int n, size_t size) { for (int i = 0; i < n; i++) { p.push_back((uint8_t *) malloc(size)); if (!p.back()) exit(1); } }
  ~Blocks() { for (uint8_t *q : p) free(q); }
};

// what read_files returned, and what its consumer saw
struct Got { int rc; std::string err; std::vector<Bytes> per_file; int64_t bases; int blocks; };

// fail_at > 0: the consumer returns `code` for its fail_at-th block (and must not be called again)
static Got run(const std::vector<std::string> &paths, int threads, int nblocks, size_t block, int fail_at = 0, int code = 0)
{ std::vector<const char *> cp;
  for (const std::string &p : paths) cp.push_back(p.c_str());
  Blocks blocks(nblocks, block);
  Got g{ 0, "", std::vector<Bytes>(paths.size()), -1, 0 };
  double t_last = 0;
  char eb[512]; eb[0] = 0;
  bool after_failure = false;
  g.rc = read_files(cp.data(), (int) cp.size(), reader_threads(threads, (int) cp.size()), blocks.p.data(), nblocks, block,
                    [&](const uint8_t *p, int64_t n, int file)
                      { if (g.blocks >= fail_at && fail_at > 0) after_failure = true;
                        g.blocks++;
                        if (n < 1 || (size_t) n > block) { printf("FAILED  a block of %lld bytes\n", (long long) n); bad++; }
                        g.per_file[(size_t) file].insert(g.per_file[(size_t) file].end(), p, p + n);
                        return g.blocks == fail_at ? code : 0;
                      }, &g.bases, &t_last, eb, sizeof(eb));
  g.err = eb;
  expect(!after_failure, "no block is consumed after the consumer failed", std::to_string(g.blocks));
  return g;
}

int main()
{ std::mt19937_64 rng(20261020);
  char tmpl[] = "/tmp/reader_check_XXXXXX";
  const char *d = mkdtemp(tmpl);
  if (!d) { printf("FAILED  no temporary directory\n"); return 1; }
  const std::string dir = d;

  // five files: FASTA and FASTQ, LF and CRLF, with and without a final newline, one of them long enough for many blocks
  // (and for several 4 MiB reads of the file, so that a "\r\n" can be cut between two of them), one without any base
  std::vector<std::string> texts = { make_text(rng, false, 40, 300, false, true), make_text(rng, true, 60, 200, true, false),
                                     make_text(rng, false, 30000, 1200, true, false), make_text(rng, true, 500, 150, false, true),
                                     ">empty\n\n>also empty\r\n" };
  std::vector<std::string> paths;
  std::vector<Bytes> want;
  int64_t total[6] = { 0, 0, 0, 0, 0, 0 };                     // sequence bytes of the first n files (separators not counted)
  for (size_t i = 0; i < texts.size(); i++)
    { paths.push_back(write_file(dir, (int) i, texts[i]));
      want.push_back(parse_whole(texts[i]));
      int64_t n = 0;
      for (uint8_t c : want[i]) n += c != SMG_COUNT_SEPARATOR;
      total[i + 1] = total[i] + n;
    }
  expect(want[2].size() > ((size_t) 8 << 20) && texts[2].size() > ((size_t) 12 << 20), "the long file spans blocks and reads", std::to_string(want[2].size()));

  const size_t sizes[3] = { 64, 4096, (size_t) 8 << 20 };
  int runs = 0;
  for (int nfiles = 1; nfiles <= 5; nfiles++)
    for (int threads = 1; threads <= 4; threads++)
      for (size_t block : sizes)
        { if (block == 64 && nfiles >= 3 && !(nfiles == 3 && threads == 2)) continue;        // (the long file in 64-byte blocks: once)
          const std::vector<std::string> some(paths.begin(), paths.begin() + nfiles);
          const int nthr = reader_threads(threads, nfiles);
          const Got g = run(some, threads, block == 4096 ? 1 + (int) (rng() % 3) : 2 * nthr + 2, block);
          const std::string what = std::to_string(nfiles) + " files, " + std::to_string(threads) + " threads, blocks of " + std::to_string(block);
          expect(g.rc == 0, "a run succeeds", what + ": " + g.err);
          for (int f = 0; f < nfiles; f++) expect(g.per_file[(size_t) f] == want[(size_t) f], "the blocks of a file are its stripped stream", what + ", file " + std::to_string(f));
          expect(g.bases == total[nfiles], "the bases are counted", what);
          runs++;
        }

  // given up by the consumer: its code comes back, every thread is joined (the sanitizers and the time limit say so)
  for (int threads = 1; threads <= 4; threads++)
    for (int fail_at : { 1, 2, 7, 500 })
      { const Got g = run(paths, threads, 2 * threads + 2, 4096, fail_at, -77 - fail_at);
        expect(g.rc == -77 - fail_at && g.blocks == fail_at, "the consumer's code ends the run", std::to_string(g.rc) + " after " + std::to_string(g.blocks));
        runs++;
      }

  // an unreadable file among readable ones
  for (int threads = 1; threads <= 4; threads++)
    for (size_t at : { (size_t) 0, (size_t) 2, paths.size() })
      { std::vector<std::string> some = paths;
        some.insert(some.begin() + (long) at, dir + "/there_is_no_such_file");
        const Got g = run(some, threads, 2 * threads + 2, 4096);
        expect(g.rc == SMG_EINVAL && g.err == "cannot open " + dir + "/there_is_no_such_file", "a file that cannot be opened", g.err);
        runs++;
      }

  // gzip is refused by its header, wherever the file stands
  const std::string gz = write_file(dir, 9, std::string("\x1f\x8b\x08\x00", 4) + "anything");
  for (int threads = 1; threads <= 4; threads += 3)
    for (size_t at : { (size_t) 0, paths.size() })
      { std::vector<std::string> some = paths;
        some.insert(some.begin() + (long) at, gz);
        const Got g = run(some, threads, 2 * threads + 2, 4096);
        expect(g.rc == SMG_EINVAL && g.err == gz + " is gzip compressed: compressed input is not supported, decompress it first", "gzip is refused", g.err);
        int64_t bound = 0;
        char eb[512]; eb[0] = 0;
        std::vector<const char *> cp;
        for (const std::string &p : some) cp.push_back(p.c_str());
        expect(survey_files(cp.data(), (int) cp.size(), 21, &bound, eb, sizeof(eb)) == SMG_EINVAL && g.err == eb, "gzip is refused before anything is read", eb);
        runs++;
      }
  { int64_t bound = 0;
    char eb[512]; eb[0] = 0;
    std::vector<const char *> cp;
    int64_t bytes = 0;
    for (size_t i = 0; i < paths.size(); i++) { cp.push_back(paths[i].c_str()); bytes += (int64_t) texts[i].size() + 21 + 1; }
    expect(survey_files(cp.data(), (int) cp.size(), 21, &bound, eb, sizeof(eb)) == 0 && bound == bytes, "the bound is the sizes and k + 1 a file", std::to_string(bound));
  }

  for (const std::string &p : paths) remove(p.c_str());
  remove(gz.c_str());
  rmdir(dir.c_str());
  printf("%s (%d runs)\n", bad ? "reader_check: FAILED" : "reader_check: every run delivered the parser's stream or its error", runs);
  return bad ? 1 : 0;
}
