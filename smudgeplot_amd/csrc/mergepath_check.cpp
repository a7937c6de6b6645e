// mergepath_check.cpp -- the merge of ks_merge<W> (smg_keysort.hpp) on the host, tile by tile and thread by thread as the
// kernel does it, from the same text (smg_mergepath.hpp: mp_split, mp_merge_run, the tile sizes), against std::merge.
// Built with -fsanitize=address,undefined (`make mergepath_check`): every "LDS" array is a heap block of exactly the
// kernel's size, so an index that the kernel would take out of its tile is reported here.  Host only; no device code.

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "smg_mergepath.hpp"

typedef unsigned long long u64;

template <int W> struct Lists
{ std::vector<u64> a, b;                  // A sorted; B unsorted, bperm its sorted order, bsrc the entry of A a B item came from
  std::vector<uint16_t> acnt;
  std::vector<uint32_t> bperm, bsrc;
  int64_t na = 0, nb = 0;
};

// what the two kernels do, one "workgroup" and one "thread" after the other
template <int W> static void merge_as_the_kernel(const Lists<W> &L, std::vector<u64> &okeys, std::vector<uint16_t> &ocnt)
{ constexpr int T = KsMergeTile<W>::value, IPT = T / MP_TPB;
  const int64_t na = L.na, nb = L.nb, total = na + nb, ntiles = (total + T - 1) / T;
  const u64 *a = L.a.data(), *b = L.b.data();
  okeys.assign((size_t) total * W, 0); ocnt.assign((size_t) total, 0);
  std::vector<uint32_t> split((size_t) ntiles + 1);
  for (int64_t t = 0; t <= ntiles; t++)                                      // ks_merge_split
    { int64_t diag = t * T;
      if (diag > total) diag = total;
      split[(size_t) t] = (uint32_t) mp_split(diag, na, nb, [&](int64_t j, int64_t i)
        { return mp_key_lt<W>(b + (size_t) L.bperm[(size_t) j] * W, a + (size_t) i * W); });
    }
  for (int64_t tile = 0; tile < ntiles; tile++)                              // ks_merge
    { std::unique_ptr<u64[]> s_key(new u64[(size_t) T * W]);
      std::unique_ptr<uint16_t[]> s_cnt(new uint16_t[T]);
      const int64_t d0 = tile * T, d1 = d0 + T < total ? d0 + T : total;
      const int64_t a0 = split[(size_t) tile], a1 = split[(size_t) tile + 1], b0 = d0 - a0, b1 = d1 - a1;
      if (a1 < a0 || b1 < b0) { fprintf(stderr, "tile %lld: spans of negative length\n", (long long) tile); exit(1); }
      const int ca = (int) (a1 - a0), cb = (int) (b1 - b0), ct = ca + cb;
      for (int x = 0; x < ca * W; x++) s_key[x] = a[(size_t) a0 * W + x];
      for (int x = 0; x < ca; x++) s_cnt[x] = L.acnt[(size_t) (a0 + x)];
      for (int x = 0; x < cb; x++)
        { const uint32_t p = L.bperm[(size_t) (b0 + x)];
          for (int w = 0; w < W; w++) s_key[(ca + x) * W + w] = b[(size_t) p * W + w];
          s_cnt[ca + x] = L.acnt[L.bsrc[p]];
        }
      const u64 *sa = s_key.get(), *sb = s_key.get() + ca * W;
      const auto b_before_a = [&](int64_t j, int64_t i) { return mp_key_lt<W>(sb + j * W, sa + i * W); };
      std::vector<std::array<u64, IPT * W>> rk(MP_TPB);
      std::vector<std::array<uint16_t, IPT>> rc(MP_TPB);
      for (int t = 0; t < MP_TPB; t++)
        { const int diag = t * IPT < ct ? t * IPT : ct;
          const int mine = ct - diag < IPT ? ct - diag : IPT;
          const int64_t i0 = mp_split(diag, ca, cb, b_before_a);
          mp_merge_run<IPT>(i0, diag - i0, ca, cb, mine, b_before_a, [&](int c, bool from_a, int64_t x)
            { const int s = (int) (from_a ? x : ca + x);
              for (int w = 0; w < W; w++) rk[t][c * W + w] = s_key[s * W + w];
              rc[t][c] = s_cnt[s];
            });
        }
      for (int t = 0; t < MP_TPB; t++)                                       // (behind the barrier)
        { const int diag = t * IPT < ct ? t * IPT : ct;
          const int mine = ct - diag < IPT ? ct - diag : IPT;
          for (int c = 0; c < mine; c++)
            { for (int w = 0; w < W; w++) s_key[(diag + c) * W + w] = rk[t][c * W + w];
              s_cnt[diag + c] = rc[t][c];
            }
        }
      for (int x = 0; x < ct * W; x++) okeys[(size_t) d0 * W + x] = s_key[x];
      for (int x = 0; x < ct; x++) ocnt[(size_t) (d0 + x)] = s_cnt[x];
    }
}

template <int W> struct Item { std::array<u64, W> k; uint16_t c; };

template <int W> static int check(const char *what, const Lists<W> &L)
{ std::vector<u64> okeys; std::vector<uint16_t> ocnt;
  merge_as_the_kernel<W>(L, okeys, ocnt);
  std::vector<Item<W>> A((size_t) L.na), B((size_t) L.nb), M((size_t) (L.na + L.nb));
  for (int64_t i = 0; i < L.na; i++)
    { for (int w = 0; w < W; w++) A[(size_t) i].k[w] = L.a[(size_t) i * W + w];
      A[(size_t) i].c = L.acnt[(size_t) i];
    }
  for (int64_t j = 0; j < L.nb; j++)
    { const uint32_t p = L.bperm[(size_t) j];
      for (int w = 0; w < W; w++) B[(size_t) j].k[w] = L.b[(size_t) p * W + w];
      B[(size_t) j].c = L.acnt[L.bsrc[p]];
    }
  std::merge(A.begin(), A.end(), B.begin(), B.end(), M.begin(), [](const Item<W> &x, const Item<W> &y) { return x.k < y.k; });
  int64_t bad = 0;
  for (size_t q = 0; q < M.size(); q++)
    { bool same = ocnt[q] == M[q].c;
      for (int w = 0; w < W; w++) same &= okeys[q * W + w] == M[q].k[w];
      bad += !same;
    }
  printf("W=%d %-28s na=%-6lld nb=%-6lld %s\n", W, what, (long long) L.na, (long long) L.nb, bad ? "DIFFERS" : "ok");
  return bad != 0;
}

// na + nb distinct keys, `from_a(q)` says which list the q-th smallest goes to; few values in the leading words, so that
// the last word decides between neighbours
template <int W, class Pick> static Lists<W> make(std::mt19937_64 &rng, int64_t total, Pick from_a)
{ std::vector<std::array<u64, W>> keys((size_t) total);
  for (auto &k : keys)
    { for (int w = 0; w + 1 < W; w++) k[w] = rng() % 3;
      k[W - 1] = rng();
    }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  Lists<W> L;
  std::vector<std::array<u64, W>> bs;
  for (size_t q = 0; q < keys.size(); q++)
    if (from_a((int64_t) q, (int64_t) keys.size()))
      { for (int w = 0; w < W; w++) L.a.push_back(keys[q][w]);
        L.acnt.push_back((uint16_t) (rng() % 32767 + 1));
      }
    else bs.push_back(keys[q]);
  L.na = (int64_t) L.acnt.size(); L.nb = (int64_t) bs.size();
  if (L.na == 0 && L.nb > 0) { L.acnt.push_back(7); }             // (a count for B's items to point at)
  // B goes in shuffled, with the permutation that sorts it
  std::vector<uint32_t> place((size_t) L.nb);
  for (size_t j = 0; j < place.size(); j++) place[j] = (uint32_t) j;
  std::shuffle(place.begin(), place.end(), rng);
  L.b.assign((size_t) L.nb * W, 0); L.bperm.assign((size_t) L.nb, 0); L.bsrc.assign((size_t) L.nb, 0);
  for (size_t j = 0; j < bs.size(); j++)
    { for (int w = 0; w < W; w++) L.b[(size_t) place[j] * W + w] = bs[j][w];
      L.bperm[j] = place[j];
      L.bsrc[place[j]] = (uint32_t) (rng() % L.acnt.size());
    }
  return L;
}

template <int W> static int run_width(std::mt19937_64 &rng)
{ constexpr int T = KsMergeTile<W>::value;
  int bad = 0;
  const auto mixed = [&](int64_t, int64_t) { return (rng() & 1) != 0; };
  for (int64_t total : { (int64_t) T - 1, (int64_t) T, (int64_t) T + 1, (int64_t) 3 * T + 5 })
    { char what[64];
      snprintf(what, sizeof(what), "interleaved, %lld outputs", (long long) total);
      bad += check<W>(what, make<W>(rng, total, mixed));
    }
  bad += check<W>("A whole, then B whole", make<W>(rng, 4 * T + 3, [](int64_t q, int64_t n) { return q < n / 2; }));
  bad += check<W>("B whole, then A whole", make<W>(rng, 4 * T + 3, [](int64_t q, int64_t n) { return q >= n / 2 + 1; }));
  bad += check<W>("runs of 300 from one list", make<W>(rng, 5 * T, [](int64_t q, int64_t) { return (q / 300) % 2 == 0; }));
  bad += check<W>("A alone (m = 0)", make<W>(rng, 2 * T + 9, [](int64_t, int64_t) { return true; }));
  bad += check<W>("B alone", make<W>(rng, 2 * T + 9, [](int64_t, int64_t) { return false; }));
  bad += check<W>("one entry and its complement", make<W>(rng, 2, [](int64_t q, int64_t) { return q == 0; }));
  bad += check<W>("one entry (n = 1, m = 0)", make<W>(rng, 1, [](int64_t, int64_t) { return true; }));
  bad += check<W>("nothing (n = 0)", make<W>(rng, 0, mixed));
  bad += check<W>("one item of B in 3 tiles of A", make<W>(rng, 3 * T, [](int64_t q, int64_t n) { return q != n / 3; }));
  return bad;
}

int main()
{ std::mt19937_64 rng(20251018);
  const int bad = run_width<1>(rng) + run_width<2>(rng) + run_width<3>(rng) + run_width<4>(rng);
  printf("%s\n", bad ? "mergepath_check: FAILED" : "mergepath_check: all cases equal std::merge");
  return bad ? 1 : 0;
}
