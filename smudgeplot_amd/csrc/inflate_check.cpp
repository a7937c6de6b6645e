// inflate_check.cpp -- the DEFLATE decoder of the BGZF route (smg_inflate.hpp: inflate_member, the text the kernel
// compiles) on the host against zlib, under the address and undefined-behaviour sanitizers (`make inflate_check`).
// Payload and text are malloc'ed at exactly clen and isize bytes, so that a read or a write outside them is reported.
//   valid members    zlib at levels 0/1/6/9 and strategies default, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, with and without a
//                    Z_FULL_FLUSH inside: status ok and the text of zlib's own inflate
//   mutated members  seeded bit flips, truncations, overwritten bytes, changed ISIZE / CRC fields: the call returns, the
//                    sanitizers stay silent, and the member is accepted exactly where zlib's raw inflate ends at the end
//                    of the payload with ISIZE bytes of that CRC -- with equal bytes
//   both accessors   every member goes through the plain arrays AND through the accessor the kernel uses (WaveIo: the
//                    payload ring, the 32 KiB window with its flushes, the sliced CRC), run as one lane: same status, same text
//   the CRC slices   crc_lane / crc_join as the 64 lanes of a wave run them, against zlib's crc32
// Host only; no device code.  This is where malformed input is explored, before any of it is shown to a GPU.

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "smg_inflate.hpp"

typedef std::vector<uint8_t> Bytes;

static int bad = 0;
static void expect(bool ok, const char *what, const std::string &detail)
{ if (!ok && bad < 50) printf("FAILED  %s (%s)\n", what, detail.c_str());
  if (!ok) bad++;
}

static Bytes make_text(std::mt19937_64 &rng, int kind, size_t n)
{ Bytes t(n);
  if (kind == 0)                                               // FASTQ
    { size_t i = 0;
      int r = 0;
      while (i < n)
        { std::string rec = "@read" + std::to_string(r++) + "\n";
          const size_t len = 30 + rng() % 120;
          for (size_t j = 0; j < len; j++) rec += "ACGTN"[rng() % 100 < 99 ? rng() % 4 : 4];
          rec += "\n+\n";
          for (size_t j = 0; j < len; j++) rec += (char) ('!' + (rng() % 8 == 0 ? rng() % 40 : 40));
          rec += "\n";
          for (size_t j = 0; j < rec.size() && i < n; j++) t[i++] = (uint8_t) rec[j];
        }
    }
  else if (kind == 1) for (uint8_t &c : t) c = (uint8_t) rng();                         // incompressible
  else if (kind == 2) for (size_t i = 0; i < n; i++) t[i] = (uint8_t) "ab"[(i / 7) & 1]; // long matches, short distances
  else if (kind == 3) for (uint8_t &c : t) c = 'A';                                     // distance 1
  else                                                                                  // skewed bytes: long codes
    for (uint8_t &c : t) { int b = 0; while (b < 255 && rng() % 100 < 70) b++; c = (uint8_t) b; }
  return t;
}

static Bytes deflate_raw(const Bytes &text, int level, int strategy, bool full_flush)
{ z_stream z;
  memset(&z, 0, sizeof(z));
  if (deflateInit2(&z, level, Z_DEFLATED, -15, 9, strategy) != Z_OK) { printf("FAILED  deflateInit2\n"); exit(1); }
  Bytes out(deflateBound(&z, (uLong) text.size()) + 64);
  static uint8_t none;
  z.next_out = out.data(); z.avail_out = (uInt) out.size();
  const size_t half = full_flush ? text.size() / 2 : 0;
  z.next_in = text.empty() ? &none : (Bytef *) text.data(); z.avail_in = (uInt) half;
  if (full_flush && deflate(&z, Z_FULL_FLUSH) != Z_OK) { printf("FAILED  deflate(Z_FULL_FLUSH)\n"); exit(1); }
  z.avail_in = (uInt) (text.size() - half);
  if (deflate(&z, Z_FINISH) != Z_STREAM_END) { printf("FAILED  deflate(Z_FINISH)\n"); exit(1); }
  out.resize(z.total_out);
  deflateEnd(&z);
  return out;
}

struct Ref { bool ok; Bytes text; };

// zlib's verdict on a member: raw inflate to the end of the stream, which is the end of the payload, ISIZE bytes, that CRC
static Ref reference(const Bytes &payload, uint32_t isize, uint32_t crc)
{ z_stream z;
  memset(&z, 0, sizeof(z));
  if (inflateInit2(&z, -15) != Z_OK) { printf("FAILED  inflateInit2\n"); exit(1); }
  Ref r{ false, Bytes((size_t) isize + 1) };
  static uint8_t none;
  z.next_in = payload.empty() ? &none : (Bytef *) payload.data(); z.avail_in = (uInt) payload.size();
  z.next_out = r.text.data(); z.avail_out = (uInt) r.text.size();
  const int rc = inflate(&z, Z_FINISH);
  r.ok = rc == Z_STREAM_END && z.avail_in == 0 && z.total_out == isize && crc32(0L, r.text.data(), (uInt) isize) == crc;
  r.text.resize(r.ok ? isize : 0);
  inflateEnd(&z);
  return r;
}

struct Got { int status; Bytes text; };

static Got ours(const Bytes &payload, uint32_t isize, uint32_t crc)
{ uint8_t *in = (uint8_t *) malloc(payload.size() ? payload.size() : 1);
  uint8_t *out = (uint8_t *) malloc(isize ? isize : 1);
  if (!in || !out) exit(1);
  if (!payload.empty()) memcpy(in, payload.data(), payload.size());
  if (payload.empty()) { free(in); in = (uint8_t *) malloc(1); }
  memset(out, 0xee, isize ? isize : 1);
  Got g;
  g.status = inflate_member_host(in, (uint32_t) payload.size(), out, isize, crc);
  if (g.status == INF_OK) g.text.assign(out, out + isize);
  // the same through the accessor of the kernel (ring, window, flushes, sliced CRC): the same status, the same text
  uint8_t *out2 = (uint8_t *) malloc(isize ? isize : 1), *win = (uint8_t *) malloc(INF_WINDOW), *ring = (uint8_t *) malloc(INF_RING);
  if (!out2 || !win || !ring) exit(1);
  memset(out2, 0xee, isize ? isize : 1); memset(win, 0xdd, INF_WINDOW); memset(ring, 0xcc, INF_RING);
  const int s2 = inflate_member_wave_host(in, (uint32_t) payload.size(), out2, isize, crc, win, ring);
  expect(s2 == g.status, "the accessor of the kernel gives the status of the plain one", std::string(inflate_reason(g.status)) + " / " + inflate_reason(s2));
  if (s2 == INF_OK && g.status == INF_OK) expect(memcmp(out, out2, isize) == 0, "the accessor of the kernel gives the text of the plain one", std::to_string(isize));
  free(out2); free(win); free(ring);
  free(in); free(out);
  return g;
}

struct Member { Bytes payload; uint32_t isize, crc; std::string what; };

static void check_crc_slices(std::mt19937_64 &rng)
{ Bytes text = make_text(rng, 1, 70000);
  int cases = 0;
  for (int t = 0; t < 300; t++)
    { // a member's text in up to three flushes, as the window makes them
      uint32_t a = 0, run = 0xffffffffu;
      const uint32_t total = t < 40 ? (uint32_t) t : (uint32_t) (rng() % 65537);
      while (a < total)
        { uint32_t n = t % 3 == 0 ? total - a : 1 + (uint32_t) (rng() % 32768);
          if (n > total - a) n = total - a;
          if (n > 32768) n = 32768;
          const uint32_t b = a + n, S = crc_slice_bytes(n);
          expect((uint64_t) S * 64 >= n && S % 8 == 4, "a slice is 4 x odd bytes and 64 of them cover the range", std::to_string(n));
          uint32_t r[64];
          for (int l = 0; l < 64; l++) r[l] = crc_lane(l, a, b, S, run, [&](uint32_t p) { return text[p]; });
          uint32_t x = crc_xpow8(S);
          for (int o = 1; o < 64; o <<= 1)
            { uint32_t nr[64];
              for (int l = 0; l < 64; l++) nr[l] = crc_join(r[l], r[l ^ o], x, (l & o) == 0);
              memcpy(r, nr, sizeof(r));
              x = crc_mul(x, x);
            }
          for (int l = 1; l < 64; l++) expect(r[l] == r[0], "every lane ends with the same register", std::to_string(l));
          run = r[0];
          a = b;
          expect((run ^ 0xffffffffu) == crc32(0L, text.data(), a), "the sliced CRC is zlib's", std::to_string(a) + " of " + std::to_string(total));
          cases++;
        }
    }
  printf("crc slices: %d ranges\n", cases);
}

int main()
{ std::mt19937_64 rng(20261020);
  check_crc_slices(rng);

  // valid members
  std::vector<Member> members;
  const int levels[4] = { 0, 1, 6, 9 };
  const int strategies[4] = { Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE };
  const size_t sizes[] = { 0, 1, 2, 3, 257, 258, 259, 1000, 5000, 32767, 32768, 32769, 65280, 65535, 65536 };
  for (int kind = 0; kind < 5; kind++)
    for (size_t n : sizes)
      for (int level : levels)
        for (int strategy : strategies)
          for (int flush = 0; flush < 2; flush++)
            { if (n > 5000 && kind != 0 && (level == 9 || flush)) continue;          // (the large ones: fewer combinations)
              const Bytes text = make_text(rng, kind, n);
              Member m{ deflate_raw(text, level, strategy, flush != 0), (uint32_t) n, (uint32_t) crc32(0L, text.data(), (uInt) n),
                        "kind " + std::to_string(kind) + ", " + std::to_string(n) + " bytes, level " + std::to_string(level) + ", strategy " +
                        std::to_string(strategy) + (flush ? ", full flush" : "") };
              if (m.payload.size() > 65536 - 26) continue;                             // (does not fit a BGZF block)
              const Ref ref = reference(m.payload, m.isize, m.crc);
              const Got got = ours(m.payload, m.isize, m.crc);
              expect(ref.ok && ref.text == text, "zlib inflates what it deflated", m.what);
              expect(got.status == INF_OK, "a valid member is ok", m.what + ": " + inflate_reason(got.status));
              expect(got.text == text, "the text of a valid member", m.what);
              if (n <= 5000 || kind == 0) members.push_back(m);
            }
  printf("valid members: %zu kept for mutation\n", members.size());

  // mutated members
  long mutants = 0, accepted = 0, by_status[INF_NSTATUS] = { 0 };
  const long want = 120000;
  while (mutants < want)
    { const Member &src = members[rng() % members.size()];
      if (src.payload.size() > 6000 && rng() % 16) continue;                          // (mostly the small ones: they are quick)
      Member m = src;
      const int edits = 1 + (int) (rng() % 3);
      for (int e = 0; e < edits; e++)
        switch (rng() % 8)
          { case 0: case 1: if (!m.payload.empty()) m.payload[rng() % m.payload.size()] ^= (uint8_t) (1u << (rng() % 8)); break;
            case 2: if (!m.payload.empty()) m.payload[rng() % m.payload.size()] = (uint8_t) rng(); break;
            case 3: m.payload.resize(m.payload.empty() ? 0 : rng() % m.payload.size()); break;
            case 4: if (m.payload.size() < 65000) m.payload.push_back((uint8_t) rng()); break;
            case 5: m.isize = rng() % 2 ? m.isize + 1 : m.isize ? m.isize - 1 : 7; break;
            case 6: m.isize = (uint32_t) (rng() % 65537); break;
            default: m.crc ^= 1u << (rng() % 32); break;
          }
      if (m.isize > 65536) m.isize = 65536;
      const Ref ref = reference(m.payload, m.isize, m.crc);
      const Got got = ours(m.payload, m.isize, m.crc);
      mutants++;
      if (got.status >= 0 && got.status < INF_NSTATUS) by_status[got.status]++;
      expect(got.status >= 0 && got.status < INF_NSTATUS, "the status is one of the list", std::to_string(got.status));
      expect((got.status == INF_OK) == ref.ok, "a mutant is accepted exactly where zlib accepts it",
             src.what + ": ours " + inflate_reason(got.status) + ", zlib " + (ref.ok ? "ok" : "not ok"));
      if (got.status == INF_OK && ref.ok) { accepted++; expect(got.text == ref.text, "the text of an accepted mutant", src.what); }
    }
  printf("mutated members: %ld, %ld of them accepted by both; by status:", mutants, accepted);
  for (int s = 0; s < INF_NSTATUS; s++) printf(" %d:%ld", s, by_status[s]);
  printf("\n");
  for (int s = 1; s < INF_NSTATUS; s++) expect(by_status[s] > 0, "every reason is met among the mutants", inflate_reason(s));
  printf("%s\n", bad ? "inflate_check: FAILED" : "inflate_check: the decoder agrees with zlib on every member");
  return bad ? 1 : 0;
}
