// bam_check.cpp -- the BAM route of the k-mer counter (smg_bam.hpp) on the host, under the address and undefined-behaviour
// sanitizers (`make bam_check`).  Every piece of text, every descriptor array and every output buffer is malloc'ed at exactly
// its size, so that a read or a write outside them is reported.
//   the framer      seeded BAM texts (headers with and without references, records of 0 .. 70 bases and a few long ones, skipped
//                   records, CIGAR and tags) fed in pieces of 1 .. 70 bytes and a handful of large sizes, every record unpacked
//                   by the host routine: the stream of a direct one-pass reference in this file
//   the tile logic  the same texts and one made for the tiles (lengths around SMG_COUNT_BAM_TILE, 5 000 empty records, one long
//                   read) through the framer as the counting calls run it, the descriptors of every piece through bam_lane --
//                   the text the kernel compiles -- tile by tile and lane by lane, in spans as the driver launches them
//   mutants         random bytes in the fixed fields and a cut at every offset of a small text: each is refused with a message
//                   exactly where the reference refuses, or gives the reference's stream; every reason is met
// Host only; no device code.  This is where malformed input is explored, before any of it is shown to a GPU.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "smg_bam.hpp"

typedef std::vector<uint8_t> Bytes;

static int bad = 0;
static void expect(bool ok, const char *what, const std::string &detail)
{ if (!ok && bad < 50) printf("FAILED  %s (%s)\n", what, detail.c_str());
  if (!ok) bad++;
}

static void put32(Bytes &t, int32_t v) { for (int i = 0; i < 4; i++) t.push_back((uint8_t) ((uint32_t) v >> (8 * i))); }

static void put_header(Bytes &t, std::mt19937_64 &rng, int l_text, int n_ref)
{ t.insert(t.end(), { 'B', 'A', 'M', 1 });
  put32(t, l_text);
  for (int i = 0; i < l_text; i++) t.push_back((uint8_t) ('a' + rng() % 26));
  put32(t, n_ref);
  for (int r = 0; r < n_ref; r++)
    { const int l_name = 1 + (int) (rng() % 12);
      put32(t, l_name);
      for (int i = 0; i < l_name; i++) t.push_back(i + 1 < l_name ? (uint8_t) ('A' + rng() % 26) : 0);
      put32(t, (int32_t) (rng() % 100000));
    }
}

static void put_record(Bytes &t, std::mt19937_64 &rng, int l_seq, unsigned flag, int l_name, int n_cigar, int l_tags)
{ const int packed = (l_seq + 1) / 2;
  put32(t, 32 + l_name + 4 * n_cigar + packed + l_seq + l_tags);
  put32(t, -1); put32(t, -1);
  t.push_back((uint8_t) l_name); t.push_back(0); t.push_back(0x48); t.push_back(0x12);
  t.push_back((uint8_t) n_cigar); t.push_back((uint8_t) (n_cigar >> 8));
  t.push_back((uint8_t) flag); t.push_back((uint8_t) (flag >> 8));
  put32(t, l_seq); put32(t, -1); put32(t, -1); put32(t, 0);
  for (int i = 0; i < l_name; i++) t.push_back(i + 1 < l_name ? (uint8_t) ('a' + rng() % 26) : 0);
  for (int i = 0; i < 4 * n_cigar; i++) t.push_back((uint8_t) rng());
  for (int i = 0; i < packed; i++) t.push_back((uint8_t) (i + 1 == packed && l_seq % 2 ? rng() & 0xf0 : rng()));
  for (int i = 0; i < l_seq + l_tags; i++) t.push_back((uint8_t) rng());
}

static unsigned some_flag(std::mt19937_64 &rng)
{ static const unsigned f[8] = { 4, 4, 4, 0, 16, 0x100, 0x800, 0x904 };
  return f[rng() % 8];
}

// the direct reference: one pass over the whole text.  "" and the stream, or the reason of the refusal
static std::string reference(const Bytes &t, Bytes &out)
{ static const char *letters = "=ACMGRSVTWYHKDBN";
  const int64_t n = (int64_t) t.size();
  int64_t p = 0;
  auto i32 = [&](int64_t at) { return (int32_t) ((uint32_t) t[at] | (uint32_t) t[at + 1] << 8 | (uint32_t) t[at + 2] << 16 | (uint32_t) t[at + 3] << 24); };
  out.clear();
  const std::string cut = "the file ends inside the header";
  if (n < 8) return cut;
  if (memcmp(t.data(), "BAM\1", 4) != 0) return "magic";
  if (i32(4) < 0) return "l_text is negative";
  p = 8 + (int64_t) i32(4);
  if (p + 4 > n) return cut;
  const int32_t n_ref = i32(p);
  if (n_ref < 0) return "n_ref is negative";
  p += 4;
  for (int32_t r = 0; r < n_ref; r++)
    { if (p + 4 > n) return cut;
      if (i32(p) < 0) return "l_name is negative";
      p += 4 + (int64_t) i32(p);
      if (p + 4 > n) return cut;
      p += 4;
    }
  bool first = true;
  while (p < n)
    { const std::string at = " @" + std::to_string(p);
      if (p + 4 > n) return "the file ends inside the record" + at;
      const int64_t bs = i32(p);
      if (bs < 32) return "block_size is smaller than the 32 bytes of the fixed fields" + at;
      if (p + 36 > n) return "the file ends inside the record" + at;
      const int64_t l_name = t[p + 12], n_cigar = t[p + 16] | t[p + 17] << 8, l_seq = i32(p + 20);
      const unsigned flag = t[p + 18] | t[p + 19] << 8;
      if (l_seq < 0) return "l_seq is negative" + at;
      if (bs < 32 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq) return "block_size is smaller than its name, CIGAR, sequence and qualities" + at;
      if (p + 4 + bs > n) return "the file ends inside the record" + at;
      if ((flag & 0x900) == 0)
        { const uint8_t *s = t.data() + p + 36 + l_name + 4 * n_cigar;
          if (!first) out.push_back('\n');
          first = false;
          for (int64_t j = 0; j < l_seq; j++) out.push_back((uint8_t) letters[j % 2 ? s[j / 2] & 15 : s[j / 2] >> 4]);
        }
      p += 4 + bs;
    }
  return "";
}

// what the framer says, as the reference says it: the reason, and " @offset" for a record
static std::string said(const char *msg)
{ const std::string m(msg);
  const size_t h = m.find("BAM header: ");
  if (h != std::string::npos) return m.find("magic") != std::string::npos ? "magic" : m.substr(h + 12);
  const size_t r = m.find("BAM record at text offset ");
  if (r == std::string::npos) return "?" + m;
  const size_t colon = m.find(": ", r);
  return m.substr(colon + 2) + " @" + m.substr(r + 26, colon - r - 26);
}

static uint16_t pair_tab[256];
static long lanes_run = 0, pieces_run = 0, straddlers = 0;

// The output of the descriptors of one piece, by bam_lane over every tile and lane, in spans of `span` bytes (a multiple of
// the tile) as the driver launches them; text and output are exact-size copies
static void run_tiles(const uint8_t *piece, size_t n, const std::vector<BamDesc> &desc, size_t out_len, size_t span, Bytes &stream)
{ expect(bam_desc_ok(desc.data(), desc.size(), n, out_len), "the descriptors of a piece describe it", std::to_string(desc.size()));
  if (out_len == 0) return;
  uint8_t *text = (uint8_t *) malloc(n ? n : 1);
  BamDesc *d = (BamDesc *) malloc(sizeof(BamDesc) * desc.size());
  if (!text || !d) exit(1);
  if (n) memcpy(text, piece, n);
  memcpy(d, desc.data(), sizeof(BamDesc) * desc.size());
  for (size_t base = 0; base < out_len; base += span)
    { const size_t len = out_len - base < span ? out_len - base : span;
      uint8_t *out = (uint8_t *) malloc(len);
      if (!out) exit(1);
      memset(out, 0xee, len);
      const uint32_t tiles = (uint32_t) ((len + BAM_TILE - 1) / BAM_TILE);
      for (uint32_t tile = 0; tile < tiles; tile++)
        for (uint32_t lane = 0; lane < BAM_LANES; lane++)
          { bam_lane(text, (uint32_t) n, d, (uint32_t) desc.size(), out, (uint32_t) base, (uint32_t) len, tile, lane, pair_tab); lanes_run++; }
      stream.insert(stream.end(), out, out + len);
      free(out);
    }
  free(text); free(d);
}

// the text through the framer in pieces of `piece` bytes; host: every record by the host routine, else the tile logic
static std::string ours(const Bytes &t, size_t piece, bool host, size_t span, Bytes &stream, int64_t *records = nullptr)
{ BamFramer fr;
  fr.all_host = host;
  char eb[256]; eb[0] = 0;
  stream.clear();
  for (size_t o = 0; o < t.size(); o += piece)
    { const size_t n = t.size() - o < piece ? t.size() - o : piece;
      uint8_t *p = (uint8_t *) malloc(n);                      // (exact size: the framer must not look past its piece)
      if (!p) exit(1);
      memcpy(p, t.data() + o, n);
      const int rc = fr.feed(p, n, "t", eb, sizeof(eb));
      if (rc == 0)
        { stream.insert(stream.end(), fr.head.begin(), fr.head.end());
          if (!fr.head.empty() && !host) straddlers++;
          expect(!host || fr.desc.empty(), "the host mode hands no record to the device", std::to_string(o));
          run_tiles(p, n, fr.desc, fr.out_len, span, stream);
          pieces_run++;
        }
      free(p);
      if (rc) { expect(rc == SMG_EFORMAT && eb[0], "a refusal is SMG_EFORMAT with a message", eb); return said(eb); }
    }
  if (fr.finish("t", eb, sizeof(eb))) return said(eb);
  if (records) *records = fr.records;
  return "";
}

static void same(const Bytes &t, size_t piece, bool host, size_t span, const char *what)
{ Bytes want, got;
  const std::string w = reference(t, want), g = ours(t, piece, host, span, got);
  const std::string where = std::string(what) + ", pieces of " + std::to_string(piece) + (host ? ", host" : ", tiles");
  expect(w == g, "the framer refuses exactly where the reference does", where + ": '" + g + "' / '" + w + "'");
  if (w.empty() && g.empty())
    { size_t at = 0;
      while (at < want.size() && at < got.size() && want[at] == got[at]) at++;
      expect(want == got, "the stream is the reference's", where + ": first difference at " + std::to_string(at) + " of " + std::to_string(want.size()) + " / " + std::to_string(got.size()));
    }
}

int main()
{ std::mt19937_64 rng(20261020);
  for (int x = 0; x < 256; x++) pair_tab[x] = bam_pair((uint32_t) x);

  // seeded texts: every length 0 .. 70 and a few long records, names of every length mod 16
  std::vector<Bytes> texts;
  for (int v = 0; v < 4; v++)
    { Bytes t;
      put_header(t, rng, v == 0 ? 0 : (int) (rng() % 200), v == 1 ? 0 : v == 2 ? 1 : 40);
      for (int r = 0; r < 150; r++)
        { const int l_seq = r < 71 ? (v % 2 ? 70 - r : r) : rng() % 9 == 0 ? (int) (rng() % 3000) : (int) (rng() % 71);
          put_record(t, rng, l_seq, r == 0 && v == 3 ? 0x100u : some_flag(rng), 1 + (int) ((r + v) % 16), (int) (rng() % 4), (int) (rng() % 20));
        }
      texts.push_back(t);
    }
  const size_t large[] = { 97, 256, 1000, 4095, 4096, 4097, 20011, 65536, 1u << 20 };
  for (const Bytes &t : texts)
    { for (size_t piece = 1; piece <= 70; piece++) { same(t, piece, true, BAM_TILE, "seeded"); same(t, piece, false, BAM_TILE, "seeded"); }
      for (size_t piece : large) { same(t, piece, true, 2 * BAM_TILE, "seeded"); same(t, piece, false, 2 * BAM_TILE, "seeded"); }
    }
  printf("seeded texts: %zu of %zu .. %zu bytes, pieces of 1 .. 70 and %zu large sizes, host routine and tile logic\n", texts.size(), texts[0].size(),
         texts.back().size(), sizeof(large) / sizeof(large[0]));

  // a text for the tiles
  { Bytes t;
    put_header(t, rng, 30, 2);
    const int around[] = { BAM_TILE - 1, BAM_TILE, BAM_TILE + 1, 3 * BAM_TILE + 5, BAM_TILE - 2, BAM_TILE + 2, 3 * BAM_TILE + 6, 2 * BAM_TILE - 1 };
    int r = 0;
    for (int l : around) put_record(t, rng, l, 4, 1 + r++ % 16, 0, 3);
    for (int i = 0; i < 5000; i++) put_record(t, rng, 0, i % 500 == 7 ? 0x800u : 4u, 2, 0, 0);
    put_record(t, rng, 1, 4, 5, 0, 0);
    put_record(t, rng, 300001, 4, 6, 1, 9);
    put_record(t, rng, 1, 4, 7, 0, 0);
    for (int l = 0; l <= 70; l++) put_record(t, rng, l, 4, 1 + l % 16, 0, 0);
    for (size_t piece : { t.size(), t.size() / 2, (size_t) 100003, (size_t) 65536, (size_t) 9973 })
      for (size_t span : { (size_t) BAM_TILE, (size_t) 8 * BAM_TILE, (size_t) 1 << 22 })
        same(t, piece, false, span, "tiles");
    same(t, 4099, true, BAM_TILE, "tiles");
    printf("tile text: %zu bytes; %ld lanes of bam_lane over %ld pieces so far, %ld records cut by a piece boundary\n", t.size(), lanes_run, pieces_run, straddlers);
  }

  // mutants of a small text
  { Bytes t;
    put_header(t, rng, 12, 2);
    std::vector<size_t> fixed;                                  // offsets of the bytes the walk reads
    for (size_t o = 0; o < 8; o++) fixed.push_back(o);
    for (size_t o = 20; o < t.size(); o++) fixed.push_back(o);  // n_ref and the references (names included: harmless)
    const int lens[] = { 0, 1, 5, 20, 33, 64, 7, 2 };
    for (int i = 0; i < 8; i++)
      { const size_t at = t.size();
        put_record(t, rng, lens[i], i == 3 ? 0x100u : 4u, 3 + i, i % 3, i);
        for (size_t o = at; o < at + 36; o++) fixed.push_back(o);
      }
    std::map<std::string, long> reasons;
    long mutants = 0, read = 0;
    auto run = [&](const Bytes &m, size_t piece)
      { Bytes want, got;
        const std::string w = reference(m, want), g = ours(m, piece, rng() % 4 == 0, BAM_TILE, got);
        expect(w == g, "a mutant is refused exactly where the reference refuses it", "'" + g + "' / '" + w + "'");
        if (w.empty()) { read++; expect(want == got, "the stream of a mutant that is read", std::to_string(mutants)); }
        else reasons[w.substr(0, w.find(" @"))]++;
        mutants++;
      };
    for (size_t cut = 0; cut <= t.size(); cut++)
      for (size_t piece : { (size_t) 1, (size_t) 13, t.size() + 1 })
        run(Bytes(t.begin(), t.begin() + (long) cut), piece);
    for (int i = 0; i < 60000; i++)
      { Bytes m = t;
        const int edits = 1 + (int) (rng() % 2);
        for (int e = 0; e < edits; e++)
          { const size_t o = fixed[rng() % fixed.size()];
            switch (rng() % 4)
              { case 0: m[o] = (uint8_t) rng(); break;
                case 1: m[o] ^= (uint8_t) (1u << (rng() % 8)); break;
                case 2: m[o] = 0xff; break;
                default: m[o] = (uint8_t) (rng() % 3 ? m[o] + 1 : m[o] - 1); break;
              }
          }
        run(m, rng() % 3 ? 1 + rng() % 80 : m.size());
      }
    printf("mutants: %ld, %ld of them read; refused because", mutants, read);
    for (const auto &r : reasons) printf("\n  %7ld  %s", r.second, r.first.c_str());
    printf("\n");
    const char *every[] = { "magic", "l_text is negative", "n_ref is negative", "l_name is negative", "l_seq is negative",
                            "block_size is smaller than the 32 bytes of the fixed fields", "block_size is smaller than its name, CIGAR, sequence and qualities",
                            "the file ends inside the header", "the file ends inside the record" };
    for (const char *why : every) expect(reasons.count(why) > 0, "every reason is met among the mutants", why);
  }
  printf("%s\n", bad ? "bam_check: FAILED" : "bam_check: the framer, the host routine and the tile logic agree with the reference on every text");
  return bad ? 1 : 0;
}
