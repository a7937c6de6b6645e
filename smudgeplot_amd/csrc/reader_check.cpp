// reader_check.cpp -- the reader threads of the k-mer counter and their ring of blocks (smg_count_reader.hpp: read_files)
// on the host, as the counter runs them but with malloc'ed blocks: the blocks of every file, put together in the order
// they were delivered, against Parser run over the whole file in one piece; and the three ways a run is given up.
// Built once with -fsanitize=address,undefined and once with -fsanitize=thread, run under a time limit: a hang is a
// failure (`make reader_check`).  Host only; no device code.
//
// The same for the seam to the device stage of compressed input: BGZF and BAM files crafted here (stored-block members) go
// through bgzf_feed, the routing of parse_file and bam_piece with a HostInflater in the place of the device's, whose
// inflate is the host twin of the kernel (inflate_member_host) and whose unpack is the host routine (bam_unpack_host), its
// buffers malloc'ed at their exact sizes.
//
// And for streams: the same inputs (plain FASTA and FASTQ, BGZF, BAM, k-mer dumps) through a pipe(2) that a writer thread
// fills in pieces of 1, 7, 4096 and 65 537 bytes, handed over by the survey or opened by the reader thread, each against the
// same bytes read from a file; and streams that end inside a member, a header, a BAM record, and after no byte at all.

#include <signal.h>

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "smg_count_reader.hpp"
#include "smg_inflate.hpp"

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

// ---------------------------------------------------------------------------------------------------------------
//  BGZF and BAM files made here, and the Inflater of the host
// ---------------------------------------------------------------------------------------------------------------

static uint32_t crc32_of(const uint8_t *p, size_t n)
{ static uint32_t tab[256];
  if (!tab[1]) for (uint32_t c = 0; c < 256; c++) tab[c] = crc_byte(0, (uint8_t) c);
  uint32_t r = 0xffffffffu;
  for (size_t i = 0; i < n; i++) r = tab[(r ^ p[i]) & 0xffu] ^ (r >> 8);
  return r ^ 0xffffffffu;
}

static void le(std::string &s, uint32_t v, int bytes) { for (int i = 0; i < bytes; i++) s += (char) (v >> (8 * i) & 0xffu); }

// one member: the 18-byte header with the BC subfield, the text as one stored block, CRC-32 and ISIZE
static std::string bgzf_member(const std::string &text, uint32_t crc_xor = 0)
{ const uint32_t n = (uint32_t) text.size();
  std::string m("\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", 16);
  le(m, 18 + 5 + n + 8 - 1, 2);
  m += '\x01'; le(m, n, 2); le(m, ~n & 0xffffu, 2);
  m += text;
  le(m, crc32_of((const uint8_t *) text.data(), n) ^ crc_xor, 4); le(m, n, 4);
  return m;
}

// the text in members of `isize` bytes (0: of 1 .. 5000 bytes, by rng), then the empty member bgzip ends a file with;
// bad_member >= 0: that member gets a wrong CRC-32, *bad_at = its offset in the file
static std::string bgzf_file(const std::string &text, size_t isize, std::mt19937_64 &rng, int bad_member = -1, size_t *bad_at = nullptr)
{ std::string f;
  int m = 0;
  for (size_t o = 0; o < text.size(); m++)
    { const size_t n = std::min(text.size() - o, isize ? isize : 1 + (size_t) (rng() % 5000));
      if (m == bad_member && bad_at) *bad_at = f.size();
      f += bgzf_member(text.substr(o, n), m == bad_member ? 0x5a5a5a5au : 0u);
      o += n;
    }
  return f + std::string("\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0", 28);
}

struct BamRec { std::string name, seq; uint32_t flag; };       // seq: letters of "=ACMGRSVTWYHKDBN"

static std::string bam_letters(std::mt19937_64 &rng, size_t n)
{ std::string s(n, '=');
  for (char &c : s) c = "=ACMGRSVTWYHKDBN"[rng() % 16];
  return s;
}

// block_size < 0: what the fields give
static std::string bam_record(const BamRec &r, int32_t block_size = -1)
{ std::string b;
  le(b, 0xffffffffu, 4); le(b, 0xffffffffu, 4);
  le(b, (uint32_t) r.name.size() + 1, 1); le(b, 0, 1); le(b, 4680, 2); le(b, 0, 2); le(b, r.flag, 2);
  le(b, (uint32_t) r.seq.size(), 4); le(b, 0xffffffffu, 4); le(b, 0xffffffffu, 4); le(b, 0, 4);
  b += r.name; b += '\0';
  for (size_t j = 0; j < r.seq.size(); j += 2)
    { const uint32_t hi = (uint32_t) (strchr("=ACMGRSVTWYHKDBN", r.seq[j]) - "=ACMGRSVTWYHKDBN");
      const uint32_t lo = j + 1 < r.seq.size() ? (uint32_t) (strchr("=ACMGRSVTWYHKDBN", r.seq[j + 1]) - "=ACMGRSVTWYHKDBN") : 0u;
      b += (char) (hi << 4 | lo);
    }
  b += std::string(r.seq.size(), '\xff');
  std::string out;
  le(out, block_size < 0 ? (uint32_t) b.size() : (uint32_t) block_size, 4);
  return out + b;
}

static std::string bam_header()
{ std::string h("BAM\1", 4);
  const std::string text = "@HD\tVN:1.6\tSO:unknown\n";
  le(h, (uint32_t) text.size(), 4); h += text; le(h, 1, 4);
  le(h, 5, 4); h += std::string("chr1\0", 5); le(h, 1000, 4);
  return h;
}

// the one-pass reference of a BAM file: the bases of its primary records, one separator between two of them
static Bytes bam_stripped(const std::vector<BamRec> &recs, int64_t *records, int64_t *nbases)
{ Bytes v;
  *records = 0; *nbases = 0;
  for (const BamRec &r : recs)
    if ((r.flag & 0x900u) == 0)
      { if ((*records)++) v.push_back(SMG_COUNT_SEPARATOR);
        v.insert(v.end(), r.seq.begin(), r.seq.end());
        *nbases += (int64_t) r.seq.size();
      }
  return v;
}

// The Inflater on the host.  chunk and blk have the sizes the reader may fill, the text that of the call and the
// unpacked bytes that of the descriptors: a byte too many, read or written, is reported.
struct HostInflater : Inflater
{ uint8_t *text = nullptr;
  size_t text_n = 0;
  int calls = 0, unpacks = 0;
  HostInflater()
  { chunk = (uint8_t *) malloc(SMG_COUNT_BGZF_CHUNK);
    blk = (BgzfBlock *) malloc(sizeof(BgzfBlock) * BGZF_MAX_BLOCKS);
    if (!chunk || !blk) exit(1);
  }
  HostInflater(const HostInflater &) = delete;
  ~HostInflater() override { free(chunk); free(blk); free(text); }
  const char *reason(int status) const override { return inflate_reason(status); }
  int inflate(int n, const uint8_t **out, int *bad_block, char *, size_t) override
  { size_t end = 0;
    for (int i = 0; i < n; i++) end = std::max(end, (size_t) blk[i].out_off + blk[i].isize);
    free(text);
    text = (uint8_t *) malloc(end ? end : 1);
    if (!text) exit(1);
    text_n = 0; calls++;
    for (int i = 0; i < n; i++)
      { const int st = inflate_member_host(chunk + blk[i].in_off, blk[i].clen, text + blk[i].out_off, blk[i].isize, blk[i].crc);
        if (st != INF_OK) { *bad_block = i; return st; }
      }
    *out = text; text_n = end;
    return 0;
  }
  int unpack(const BamDesc *d, size_t nd, size_t out_len, Sink &sink, char *errbuf, size_t errlen) override
  { if (!bam_desc_ok(d, nd, text_n, out_len)) return fail(errbuf, errlen, SMG_EINVAL, "internal error: %zu descriptors do not describe the text", nd);
    uint8_t *out = (uint8_t *) malloc(out_len ? out_len : 1);
    if (!out) exit(1);
    for (size_t i = 0; i < nd; i++)
      { if (d[i].out_off) out[d[i].out_off - 1] = SMG_COUNT_SEPARATOR;
        bam_unpack_host(text + d[i].seq_off, d[i].l_seq, out + d[i].out_off);
      }
    unpacks++;
    const bool ok = sink.put(out, out_len);
    free(out);
    return ok ? 0 : 1;
  }
};

// what read_files returned, and what its consumer saw
struct Got { int rc; std::string err; std::vector<Bytes> per_file; int64_t bases; int blocks; std::vector<FileRead> files; int calls, unpacks; };

// fail_at > 0: the consumer returns `code` for its fail_at-th block (and must not be called again); inflaters: every reader
// thread has a HostInflater (without one a BGZF file is refused)
// inputs: every reader thread has a HostInflater (without one a BGZF file is refused); dump: the files are k-mer dumps; taken:
// what a survey opened of the paths (survey_files), or null
static Got run(const std::vector<std::string> &paths, int threads, int nblocks, size_t block, int fail_at = 0, int code = 0, bool inflaters = false,
               bool dump = false, const std::unique_ptr<Taken> *taken = nullptr)
{ std::vector<const char *> cp;
  for (const std::string &p : paths) cp.push_back(p.c_str());
  Blocks blocks(nblocks, block);
  Got g{ 0, "", std::vector<Bytes>(paths.size()), -1, 0, {}, 0, 0 };
  double t_last = 0;
  char eb[512]; eb[0] = 0;
  bool after_failure = false;
  const int nthr = reader_threads(threads, (int) cp.size());
  std::vector<HostInflater> own((size_t) (inflaters ? nthr : 0));
  std::vector<Inflater *> infl;
  for (HostInflater &h : own) infl.push_back(&h);
  g.rc = read_files(cp.data(), (int) cp.size(), nthr, blocks.p.data(), nblocks, block,
                    [&](const uint8_t *p, int64_t n, int file)
                      { if (g.blocks >= fail_at && fail_at > 0) after_failure = true;
                        g.blocks++;
                        if (n < 1 || (size_t) n > block) { printf("FAILED  a block of %lld bytes\n", (long long) n); bad++; }
                        g.per_file[(size_t) file].insert(g.per_file[(size_t) file].end(), p, p + n);
                        return g.blocks == fail_at ? code : 0;
                      }, &g.bases, &t_last, &g.files, eb, sizeof(eb), inflaters ? infl.data() : nullptr, dump, taken);
  g.err = eb;
  for (const HostInflater &h : own) { g.calls += h.calls; g.unpacks += h.unpacks; }
  expect(g.files.size() == paths.size(), "one record per file", std::to_string(g.files.size()));
  expect(!after_failure, "no block is consumed after the consumer failed", std::to_string(g.blocks));
  return g;
}

// A stream made here: a pipe(2) whose write end a thread fills with a copy of the bytes in pieces of `piece` bytes; the
// reader is given the read end under its name /dev/fd/N.  done(): the read end is closed (a writer whose reader gave up
// then sees EPIPE, SIGPIPE being ignored) and the thread joined -> it wrote everything.
struct Piped
{ int fd[2] = { -1, -1 };
  std::string path;
  std::thread writer;
  bool all = false;
  const std::string data;
  Piped(const std::string &bytes, size_t piece) : data(bytes)
  { if (pipe(fd) != 0) { printf("FAILED  no pipe\n"); exit(1); }
    path = "/dev/fd/" + std::to_string(fd[0]);
    const int w = fd[1];
    writer = std::thread([this, w, piece]
      { size_t at = 0;
        while (at < data.size())
          { const ssize_t r = write(w, data.data() + at, std::min(piece, data.size() - at));
            if (r <= 0) break;
            at += (size_t) r;
          }
        all = at == data.size();
        close(w);
      });
  }
  Piped(const Piped &) = delete;
  bool done() { close(fd[0]); writer.join(); return all; }
};

// the file's message with the stream's path in the place of the file's
static std::string renamed(const std::string &msg, const std::string &from, const std::string &to)
{ const size_t at = msg.find(from);
  return at == std::string::npos ? msg : msg.substr(0, at) + to + msg.substr(at + from.size());
}

// `bytes` as a stream in pieces of `piece`, read by one thread as the counter reads it -- surveyed (the survey opens it, takes
// the bytes that tell what it is and hands it on) or opened by the reader thread itself -- against what the same bytes gave
// as a file (`want`, read from `file`): the same stripped stream and record, or the same error under the stream's path
static void stream_case(const std::string &what, const std::string &bytes, size_t piece, const Got &want, const std::string &file, bool inflaters,
                        bool dump, bool surveyed)
{ Piped p(bytes, piece);
  const std::string name = what + " in pieces of " + std::to_string(piece) + (surveyed ? ", surveyed" : ", opened by its reader");
  std::vector<std::unique_ptr<Taken>> taken;
  if (surveyed)
    { const char *cp = p.path.c_str(), *fp = file.c_str();
      std::vector<char> kind, file_kinds;
      int64_t bound = 0, file_bound = 0;
      char eb[512]; eb[0] = 0;
      const int rc = survey_files(&cp, 1, 21, &bound, eb, sizeof(eb), &kind, false, &taken);
      expect(rc == 0 && taken.size() == 1 && taken[0] && taken[0]->src.stream && bound == 22, "the survey opens a stream and keeps it", name + ": " + eb);
      if (want.rc == 0)
        expect(survey_files(&fp, 1, 21, &file_bound, eb, sizeof(eb), &file_kinds) == 0 && kind == file_kinds, "a stream is told as its file is", name);
    }
  const Got g = run({ p.path }, 1, 4, (size_t) 1 << 20, 0, 0, inflaters, dump, surveyed ? taken.data() : nullptr);
  taken.clear();
  const bool all = p.done();
  expect(g.rc == want.rc && g.err == renamed(want.err, file, p.path), "a stream ends as its file does", name + ": " + g.err + " / " + want.err);
  if (want.rc == 0)
    { expect(all, "the writer of a stream wrote everything", name);
      expect(g.per_file[0] == want.per_file[0], "the blocks of a stream are the stripped stream of its file", name);
      const FileRead &a = g.files[0], &b = want.files[0];
      expect(a.route == b.route && a.records == b.records && a.bases == b.bases && g.bases == want.bases, "the record of a stream is that of its file", name);
    }
  else expect(g.files[0].route == ROUTE_NONE, "a stream that was refused has no record", name);
}

int main()
{ std::mt19937_64 rng(20261020);
  signal(SIGPIPE, SIG_IGN);
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
          for (int f = 0; f < nfiles; f++)
            expect(g.files[(size_t) f].route == ROUTE_TEXT && g.files[(size_t) f].bases == total[f + 1] - total[f], "the record of a plain file", what);
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

  // ---- BGZF and BAM through the Inflater seam ----
  int zruns = 0;
  const std::string no_device = " is BGZF compressed: this call has no device to inflate it on, use smg_count_bgzf_inflate or one of the counting calls";
  auto nbases = [](const Bytes &v) { int64_t n = 0; for (uint8_t c : v) n += c != SMG_COUNT_SEPARATOR; return n; };
  auto check_file = [&](const Got &g, size_t f, const Bytes &stream, int route, int64_t records, int64_t nb, const std::string &what)
    { expect(g.per_file[f] == stream, "the blocks of a compressed file are its stripped stream", what);
      const FileRead &r = g.files[f];
      expect(r.route == route && r.records == records && r.bases == nb, "the record of a compressed file",
             what + ": route " + std::to_string(r.route) + ", " + std::to_string(r.records) + " records, " + std::to_string(r.bases) + " bases");
    };

  // a BGZF FASTQ in members of 1 .. 5000 bytes
  const std::string fq_text = make_text(rng, true, 300, 400, false, true);
  const Bytes fq_want = parse_whole(fq_text);
  int64_t fq_records = 1;
  for (uint8_t c : fq_want) fq_records += c == SMG_COUNT_SEPARATOR;
  const std::string fqz_bytes = bgzf_file(fq_text, 0, rng);
  const std::string fqz = write_file(dir, 20, fqz_bytes);

  // a BAM: a few primary records, a secondary and a supplementary one that are skipped, an empty one; members of 37 bytes
  const std::vector<BamRec> small = { { "r0", bam_letters(rng, 150), 4 }, { "r1", bam_letters(rng, 31), 0x100 }, { "r2", "", 4 },
                                      { "r3", bam_letters(rng, 4097), 16 }, { "r4", bam_letters(rng, 77), 0x800 | 16 }, { "r5", bam_letters(rng, 1), 0 } };
  std::string small_text = bam_header();
  for (const BamRec &r : small) small_text += bam_record(r);
  int64_t small_records = 0, small_bases = 0;
  const Bytes small_want = bam_stripped(small, &small_records, &small_bases);
  const std::string bam_bytes = bgzf_file(small_text, 37, rng);
  const std::string bam = write_file(dir, 21, bam_bytes);
  expect(small_records == 4 && small_bases == 150 + 4097 + 1, "the small BAM is what it was made to be", std::to_string(small_records));

  // a BAM whose members exceed one chunk of the reader: members of 60000 bytes (60031 in the file, which do not divide the
  // chunk: one is cut by its end), and a record of 20000 bases placed so that the text of the first call ends inside its
  // seq field
  const size_t member = 60000, first_call = (size_t) SMG_COUNT_BGZF_CHUNK / (member + 31) * member;       // text bytes of the first inflate call
  std::vector<BamRec> large;
  std::string large_text = bam_header();
  bool placed = false;
  while (large_text.size() < first_call + 2 * member)
    { const bool now = !placed && large_text.size() + 5000 > first_call;
      large.push_back(BamRec{ "m" + std::to_string(large.size()), bam_letters(rng, now ? 20000 : rng() % 600), rng() % 23 == 0 ? 0x900u : 4u });
      if (now)
        { const size_t seq_at = large_text.size() + 36 + large.back().name.size() + 1;
          large.back().flag = 4;
          placed = seq_at < first_call && first_call < seq_at + 10000;
          expect(placed, "the chunk seam lies in a seq field", std::to_string(seq_at));
        }
      large_text += bam_record(large.back());
    }
  int64_t large_records = 0, large_bases = 0;
  const Bytes large_want = bam_stripped(large, &large_records, &large_bases);
  const std::string large_file = bgzf_file(large_text, member, rng);
  const std::string big = write_file(dir, 22, large_file);
  expect(placed && large_file.size() > (size_t) SMG_COUNT_BGZF_CHUNK && (size_t) SMG_COUNT_BGZF_CHUNK % (member + 31) != 0,
         "the large BAM exceeds one chunk and a member is cut by its end", std::to_string(large_file.size()));

  // each alone, one reader
  for (size_t block : { (size_t) 4096, (size_t) 8 << 20 })
    { Got g = run({ fqz }, 1, 4, block, 0, 0, true);
      expect(g.rc == 0 && g.calls == 1 && g.unpacks == 0, "a BGZF FASTQ is read", g.err);
      check_file(g, 0, fq_want, ROUTE_TEXT, fq_records, nbases(fq_want), "BGZF FASTQ");
      g = run({ bam }, 1, 4, block, 0, 0, true);
      expect(g.rc == 0 && g.calls == 1 && g.unpacks == 1, "a BAM is read", g.err);
      check_file(g, 0, small_want, ROUTE_BAM, small_records, small_bases, "small BAM");
      expect(g.bases == small_bases, "the bases of a BAM are counted", std::to_string(g.bases));
      zruns += 2;
    }
  { const Got g = run({ big }, 1, 4, (size_t) 8 << 20, 0, 0, true);
    expect(g.rc == 0 && g.calls == 2 && g.unpacks == 2, "a BAM of two chunks is read in two calls", g.err + " " + std::to_string(g.calls));
    check_file(g, 0, large_want, ROUTE_BAM, large_records, large_bases, "large BAM");
    zruns++;
  }

  // in a mixed list with plain files, one inflater per reader thread
  for (int threads : { 1, 3 })
    { const std::vector<std::string> some = { paths[0], fqz, paths[1], bam, big, paths[3], fqz };
      const Got g = run(some, threads, 2 * threads + 2, (size_t) 1 << 20, 0, 0, true);
      const std::string what = "mixed list, " + std::to_string(threads) + " threads";
      expect(g.rc == 0, "a mixed list is read", what + ": " + g.err);
      for (size_t f : { (size_t) 0, (size_t) 2, (size_t) 5 })
        { const size_t i = f == 0 ? 0 : f == 2 ? 1 : 3;
          expect(g.per_file[f] == want[i] && g.files[f].route == ROUTE_TEXT && g.files[f].bases == total[i + 1] - total[i], "a plain file of a mixed list", what);
        }
      check_file(g, 1, fq_want, ROUTE_TEXT, fq_records, nbases(fq_want), what);
      check_file(g, 6, fq_want, ROUTE_TEXT, fq_records, nbases(fq_want), what);
      check_file(g, 3, small_want, ROUTE_BAM, small_records, small_bases, what);
      check_file(g, 4, large_want, ROUTE_BAM, large_records, large_bases, what);
      std::vector<const char *> cp;
      for (const std::string &p : some) cp.push_back(p.c_str());
      std::vector<char> is_bgzf;
      int64_t bound = 0, text_bytes = (int64_t) (2 * fq_text.size() + small_text.size() + large_text.size() + texts[0].size() + texts[1].size() + texts[3].size());
      char eb[512]; eb[0] = 0;
      expect(survey_files(cp.data(), (int) cp.size(), 21, &bound, eb, sizeof(eb), &is_bgzf) == 0 && bound == text_bytes + 7 * 22 &&
             is_bgzf == std::vector<char>({ 0, 1, 0, 1, 1, 0, 1 }), "the survey bounds a BGZF file by its text", eb);
      zruns++;
    }

  // without an inflater a BGZF file is refused, and so is a reader thread that has none
  for (int threads : { 1, 3 })
    { const Got g = run({ paths[0], paths[1], bam }, threads, 2 * threads + 2, 4096);
      expect(g.rc == SMG_EINVAL && g.err == bam + no_device, "a BGZF file without an inflater is refused", g.err);
      expect(g.files[2].route == ROUTE_NONE, "a refused file has no record", std::to_string(g.files[2].route));
      zruns++;
    }

  // a bad member and a bad record end the run with their message; every thread is joined
  { size_t bad_at = 0;
    const std::string bad_crc = write_file(dir, 23, bgzf_file(small_text, 37, rng, 5, &bad_at));
    std::string short_text = bam_header() + bam_record(small[0]);
    const size_t rec_at = short_text.size();
    short_text += bam_record(small[3], 10) ;
    const std::string bad_rec = write_file(dir, 24, bgzf_file(short_text, 37, rng));
    for (int threads : { 1, 3 })
      { Got g = run({ paths[0], bam, bad_crc, paths[1], fqz }, threads, 2 * threads + 2, 4096, 0, 0, true);
        expect(g.rc == SMG_EFORMAT && g.err == bad_crc + ": BGZF block at offset " + std::to_string(bad_at) + ": " + inflate_reason(INF_BAD_CRC),
               "a bad member ends the run", g.err);
        expect(g.files[2].route == ROUTE_NONE, "a file with a bad member has no record", "");
        g = run({ paths[0], bam, bad_rec, paths[1], fqz }, threads, 2 * threads + 2, 4096, 0, 0, true);
        expect(g.rc == SMG_EFORMAT && g.err == bad_rec + ": BAM record at text offset " + std::to_string(rec_at) +
               ": block_size is smaller than the 32 bytes of the fixed fields", "a bad record ends the run", g.err);
        expect(g.files[2].route == ROUTE_NONE, "a file with a bad record has no record", "");
        if (threads == 1) check_file(g, 1, small_want, ROUTE_BAM, small_records, small_bases, "the BAM read before the bad one");
        zruns += 2;
      }
    remove(bad_crc.c_str()); remove(bad_rec.c_str());
  }
  // the scan, as the survey classifies
  { int64_t nb = 0, nt = 0;
    char eb[512]; eb[0] = 0;
    expect(bgzf_scan(big.c_str(), &nb, &nt, eb, sizeof(eb)) == 0 && nt == (int64_t) large_text.size() && nb == (int64_t) ((large_text.size() + member - 1) / member) + 1,
           "the scan of a BGZF file", eb);
    expect(bgzf_scan(paths[0].c_str(), &nb, &nt, eb, sizeof(eb)) == SMG_EINVAL && eb == paths[0] + " is not BGZF: it does not begin with a gzip header", "the scan of a plain file", eb);
    expect(bgzf_scan(gz.c_str(), &nb, &nt, eb, sizeof(eb)) == SMG_EINVAL && eb == gz + " is gzip compressed: compressed input is not supported, decompress it first", "the scan of a gzip file", eb);
  }
  // ---- streams: the same bytes through a pipe, written in pieces, against the file ----
  int sruns = 0;
  { std::string dump_text;
    for (int i = 0; i < 3000; i++)
      { std::string s(31, 'A');
        for (char &c : s) c = "ACGTacgt"[rng() % 8];
        dump_text += s + (i % 2 ? "\t" : " ") + std::to_string(1 + rng() % 100000) + (i % 3 ? "\n" : "\r\n");
      }
    dump_text.resize(dump_text.size() - 1);                    // (no line end at the end of the text)
    const std::string dump_file = write_file(dir, 30, dump_text);
    const std::string dumpz_bytes = bgzf_file(dump_text, 0, rng);
    const std::string dumpz = write_file(dir, 31, dumpz_bytes);
    struct Case { const char *what; const std::string *bytes; std::string file; bool inflaters, dump, large; };
    const std::vector<Case> cases = { { "FASTA", &texts[0], paths[0], false, false, false },
                                      { "FASTQ, CR-LF, no final newline", &texts[1], paths[1], false, false, false },
                                      { "long FASTA, CR-LF, no final newline", &texts[2], paths[2], false, false, true },
                                      { "FASTQ", &texts[3], paths[3], false, false, false },
                                      { "records without bases", &texts[4], paths[4], false, false, false },
                                      { "BGZF FASTQ", &fqz_bytes, fqz, true, false, false },
                                      { "BAM", &bam_bytes, bam, true, false, false },
                                      { "BAM of two chunks", &large_file, big, true, false, true },
                                      { "dump", &dump_text, dump_file, false, true, false },
                                      { "BGZF dump", &dumpz_bytes, dumpz, true, true, false } };
    for (const Case &c : cases)
      { const Got want = run({ c.file }, 1, 4, (size_t) 1 << 20, 0, 0, c.inflaters, c.dump);
        expect(want.rc == 0, "the file of a stream case is read", std::string(c.what) + ": " + want.err);
        for (size_t piece : { (size_t) 1, (size_t) 7, (size_t) 4096, (size_t) 65537 })
          { if (c.large && piece < 4096) continue;            // (some ten million writes: the small inputs cover these pieces)
            stream_case(c.what, *c.bytes, piece, want, c.file, c.inflaters, c.dump, true);
            sruns++;
            if (piece == 7 || piece == 65537) { stream_case(c.what, *c.bytes, piece, want, c.file, c.inflaters, c.dump, false); sruns++; }
          }
      }
    expect(large_file.size() > (size_t) SMG_COUNT_BGZF_CHUNK + 65537, "a member of the large stream is carried to the front of the chunk", "");

    // two streams and a file on two reader threads, the streams handed over by the survey
    { Piped a(fqz_bytes, 4096), b(texts[1], 7);
      const std::vector<std::string> some = { a.path, paths[0], b.path };
      std::vector<const char *> cp;
      for (const std::string &p : some) cp.push_back(p.c_str());
      std::vector<std::unique_ptr<Taken>> taken;
      std::vector<char> kind;
      int64_t bound = 0;
      char eb[512]; eb[0] = 0;
      expect(survey_files(cp.data(), 3, 21, &bound, eb, sizeof(eb), &kind, false, &taken) == 0 && taken[0] && !taken[1] && taken[2] &&
             kind == std::vector<char>({ 1, 0, 0 }) && bound == (int64_t) texts[0].size() + 3 * 22, "the survey of streams and a file: the bound is the file's", eb);
      const Got g = run(some, 2, 6, (size_t) 1 << 20, 0, 0, true, false, taken.data());
      taken.clear();
      expect(a.done() && b.done(), "the writers of two streams wrote everything", "");
      expect(g.rc == 0 && g.per_file[0] == fq_want && g.per_file[1] == want[0] && g.per_file[2] == want[1], "two streams and a file on two threads", g.err);
      sruns++;
    }

    // a stream that ends inside a member, inside a header, inside a BAM record, after no byte at all; gzip on a stream
    { const std::string even = bgzf_file(fq_text, 1000, rng);   // (members of 18 + 5 + 1000 + 8 bytes)
      for (size_t into : { (size_t) 500, (size_t) 10 })
        { const std::string cut = even.substr(0, 3 * 1031 + into);
          for (bool surveyed : { true, false })
            { Got want{ SMG_EFORMAT, std::string("F: BGZF block at offset 3093: ") + (into == 500 ? "the member is cut off by the end of the stream"
                                                                                                    : "the header is cut off by the end of the stream"),
                        {}, 0, 0, {}, 0, 0 };
              stream_case("a BGZF stream cut in a member", cut, 7, want, "F", true, false, surveyed);
              sruns++;
            }
        }
      std::string cut_text = bam_header() + bam_record(small[0]);
      cut_text += bam_record(small[3]).substr(0, 1000);
      const std::string cut_bam = bgzf_file(cut_text, 37, rng), empty;
      const std::string cut_file = write_file(dir, 32, cut_bam), empty_file = write_file(dir, 33, empty);
      const Got cut_want = run({ cut_file }, 1, 4, 4096, 0, 0, true), empty_want = run({ empty_file }, 1, 4, 4096, 0, 0, true);
      expect(cut_want.rc == SMG_EFORMAT && cut_want.err.find(": BAM record at text offset ") != std::string::npos, "a BAM file that ends in a record", cut_want.err);
      expect(empty_want.rc == 0 && empty_want.per_file[0].empty(), "an empty file", empty_want.err);
      const Got gz_want = run({ gz }, 1, 4, 4096);
      for (bool surveyed : { true, false })
        { stream_case("a BAM stream cut in a record", cut_bam, 4096, cut_want, cut_file, true, false, surveyed);
          stream_case("a stream of no bytes", empty, 7, empty_want, empty_file, true, false, surveyed);
          sruns += 2;
        }
      stream_case("a gzip stream", std::string("\x1f\x8b\x08\x00", 4) + "anything", 1, gz_want, gz, false, false, false);
      sruns++;
      for (bool gzip_ok : { false, true })
        { Piped p(texts[0], 4096);                              // (never read: the survey refuses the stream in front of it)
          Piped z(fqz_bytes.substr(0, 2) + "\x08\x00 anything", 1);
          const char *cp[2] = { z.path.c_str(), p.path.c_str() };
          std::vector<std::unique_ptr<Taken>> taken;
          int64_t bound = 0;
          char eb[512]; eb[0] = 0;
          const int rc = survey_files(cp, 2, 21, &bound, eb, sizeof(eb), nullptr, gzip_ok, &taken);
          expect(rc == SMG_EINVAL && eb == z.path + (gzip_ok ? " is a stream of plain gzip: its restart index reads the file twice; give the file itself, or decompress it in the pipe"
                                                              : " is gzip compressed: compressed input is not supported, decompress it first"), "gzip on a stream is refused by the survey", eb);
          taken.clear();
          z.done(); p.done();
          sruns++;
        }
      // standard input can be named once, and a survey that hands nothing on refuses a stream
      { const char *twice[3] = { "-", paths[0].c_str(), "-" };
        int64_t bound = 0;
        char eb[512]; eb[0] = 0;
        std::vector<std::unique_ptr<Taken>> taken;
        expect(survey_files(twice, 3, 21, &bound, eb, sizeof(eb), nullptr, false, &taken) == SMG_EINVAL && std::string(eb) == "- (standard input) is named twice: it can be read once",
               "standard input is named twice", eb);
        Piped p(texts[0], 4096);
        const char *cp = p.path.c_str();
        expect(survey_files(&cp, 1, 21, &bound, eb, sizeof(eb)) == SMG_EINVAL && eb == p.path + " is a stream: this call reads a file", "a survey without a hand-over", eb);
        expect(bgzf_scan(cp, &bound, &bound, eb, sizeof(eb)) == SMG_EINVAL && eb == p.path + " is a stream: this call reads a file", "the scan of a stream", eb);
        p.done();
      }
      remove(cut_file.c_str()); remove(empty_file.c_str());
    }
    remove(dump_file.c_str()); remove(dumpz.c_str());
  }

  remove(fqz.c_str()); remove(bam.c_str()); remove(big.c_str());

  for (const std::string &p : paths) remove(p.c_str());
  remove(gz.c_str());
  rmdir(dir.c_str());
  printf("%s (%d runs, %d of them over BGZF and BAM files, %d over streams)\n",
         bad ? "reader_check: FAILED" : "reader_check: every run delivered the parser's stream or its error", runs + zruns + sruns, zruns, sruns);
  return bad ? 1 : 0;
}
