// smg_counted.hpp -- the counted path (k > 85: degrees counted with the reference's uint8 wrap) and the general path (a
// table that is not closed under reverse complement: every position, nothing assumed) of the hetmers engine: their
// kernels and their drivers, one-shot, in the steps of the phase API, and over the shards of one device.  Exact, not
// fast.  Included by smg_hetmers.hip behind dir_geometry and plot_sum; no state of its own.

#pragma once

// bucket directory + strict-order validation
template <int W> __global__ void __launch_bounds__(TPB)
k_directory(Tab t, uint32_t *__restrict__ bstart, Ctrl *__restrict__ ctrl)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i > t.n) return;
  if (i < t.n)
    { const uint32_t bcur = dir_bucket(t.dir, t.keys[i * W]);
      bool first = i == 0;
      if (i > 0)
        { first = dir_bucket(t.dir, t.keys[(i - 1) * W]) != bcur;
          if (!key_lt<W>(load_key<W>(t.keys, i - 1), load_key<W>(t.keys, i))) ctrl->unsorted = 1;
        }
      if (first) bstart[bcur] = (uint32_t) i;
    }
  else bstart[t.dir.nb] = (uint32_t) t.n;
}

// ---- the general path over a table that is cut into prefix shards ON ONE DEVICE (more than 2^32 entries) -----------
// The prefix-side partner of an entry (the k-mer with one of its first p0 bases replaced) may live in another shard:
// the look-up first picks the shard whose k-mer range holds it (<= 16 comparisons with the shards' first k-mers), then
// searches that shard's directory.  Window blocks never straddle a cut, so everything else stays shard local.
#define SET_MAX 16
struct TabSet
{ int ns;
  Tab shard[SET_MAX];
  u64 first[SET_MAX][4];       // first k-mer of shard s (all ones for an empty shard behind the last one)
};

template <int W> SMG_DEV int set_find(const TabSet *set, const Key<W> &y, int64_t &j)
{ int s = 0;
  for (int q = 1; q < set->ns; q++)
    { Key<W> f;
#pragma unroll
      for (int w = 0; w < W; w++) f.w[w] = set->first[q][w];
      if (!key_lt<W>(y, f)) s = q;
    }
  const Tab &t = set->shard[s];
  j = t.n > 0 ? find_key<W>(t.keys, t.dir, y) : -1;
  return s;
}

// ---- pass 1 -------------------------------------------------------------------------------
// One thread per entry.  SYM: scan positions >= p0 inside the window block, write
// deg = S_all, emit a request (rc(x), cnt, S_hi) when S_hi > 0 (or for every entry when
// emit_all), accumulate the fingerprints when want_fp.
// !SYM (general path): additionally resolve positions < p0 by directory look-ups; deg = all.

template <int W, bool SYM> __global__ void __launch_bounds__(TPB)
k_pass1(Tab t, int64_t lo, int64_t hi, int emit_all, int want_fp, u64 *__restrict__ req,
        int64_t req_cap, Ctrl *__restrict__ ctrl, const TabSet *__restrict__ set = NULL)
{ const int64_t i = lo + (int64_t) blockIdx.x * TPB + threadIdx.x;
  const bool live = i < hi;
  const Geo g = t.g;
  unsigned s_all = 0, s_hi = 0;
  Key<W> x;
  unsigned c = 0;
#pragma unroll
  for (int w = 0; w < W; w++) x.w[w] = 0;

  if (live)
    { x = load_key<W>(t.keys, i);
      c = t.cnt[i];
      bool big = false;
      if (i + WIN_LIM < t.n) big |= same_block<W>(x, load_key<W>(t.keys, i + WIN_LIM), g);
      if (i - WIN_LIM >= 0)  big |= same_block<W>(x, load_key<W>(t.keys, i - WIN_LIM), g);
      if (!big)
        { for (int64_t j = i + 1; j < t.n; j++)
            { const Key<W> y = load_key<W>(t.keys, j);
              if (!same_block<W>(x, y, g)) break;
              const int p = pair_pos<W>(x, y);
              if (p >= 0 && c + (unsigned) t.cnt[j] <= SMG_SMAX)
                { s_all++; s_hi += (p != g.k - 1 - p); }
            }
          for (int64_t j = i - 1; j >= 0; j--)
            { const Key<W> y = load_key<W>(t.keys, j);
              if (!same_block<W>(x, y, g)) break;
              const int p = pair_pos<W>(x, y);
              if (p >= 0 && c + (unsigned) t.cnt[j] <= SMG_SMAX)
                { s_all++; s_hi += (p != g.k - 1 - p); }
            }
        }
      else
        { // block bounds by bisection on the (monotone) same_block predicate
          int64_t a = 0, b = i;
          while (a < b)
            { const int64_t m = (a + b) >> 1;
              if (same_block<W>(x, load_key<W>(t.keys, m), g)) b = m; else a = m + 1;
            }
          const int64_t blo = a;
          a = i + 1; b = t.n;
          while (a < b)
            { const int64_t m = (a + b) >> 1;
              if (!same_block<W>(x, load_key<W>(t.keys, m), g)) b = m; else a = m + 1;
            }
          const int64_t bhi = a;
          for (int p = g.p0; p < g.k; p++)
            for (int d = 1; d <= 3; d++)
              { const Key<W> y = flip_base<W>(x, p, d);
                const int64_t j = lower_bound_key<W>(t.keys, blo, bhi, y);
                if (j < bhi && key_eq<W>(load_key<W>(t.keys, j), y)
                    && c + (unsigned) t.cnt[j] <= SMG_SMAX)
                  { s_all++; s_hi += (p != g.k - 1 - p); }
              }
        }
      if (!SYM)
        { for (int p = 0; p < g.p0; p++)
            for (int d = 1; d <= 3; d++)
              { const Key<W> y = flip_base<W>(x, p, d);
                if (set)                      // (the partner may live in another shard of the same device)
                  { int64_t j;
                    const int sh = set_find<W>(set, y, j);
                    if (j >= 0 && c + (unsigned) set->shard[sh].cnt[j] <= SMG_SMAX) s_all++;
                  }
                else
                  { const int64_t j = find_key<W>(t.keys, t.dir, y);
                    if (j >= 0 && c + (unsigned) t.cnt[j] <= SMG_SMAX) s_all++;
                  }
              }
        }
      t.deg[i] = (uint8_t) s_all;
    }

  if (SYM)
    { const bool emit = live && (emit_all || s_hi > 0);
      const u64 mask = __ballot(emit);
      if (mask)
        { const int lane = threadIdx.x & 63;
          u64 base = 0;
          if (lane == __ffsll((long long) mask) - 1)
            base = atomicAdd(&ctrl->nreq, (u64) __popcll(mask));
          base = __shfl(base, __ffsll((long long) mask) - 1, 64);
          if (emit)
            { const u64 slot = base + __popcll(mask & ((1ull << lane) - 1));
              if ((int64_t) slot < req_cap)
                { const Key<W> r = revcomp<W>(x, g.k);
                  u64 *o = req + slot * (W + 1);
#pragma unroll
                  for (int w = 0; w < W; w++) o[w] = r.w[w];
                  o[W] = (u64) c | ((u64) (s_hi & 0xFF) << 16);
                }
            }
        }
      if (want_fp)
        { u64 f0 = 0, f1 = 0, f2 = 0, f3 = 0;
          if (live)
            { const Key<W> r = revcomp<W>(x, g.k);
              f0 = hash_entry<W>(x, c, 0x243f6a8885a308d3ull);
              f1 = hash_entry<W>(x, c, 0x13198a2e03707344ull);
              f2 = hash_entry<W>(r, c, 0x243f6a8885a308d3ull);
              f3 = hash_entry<W>(r, c, 0x13198a2e03707344ull);
            }
          // (XOR, as on the fast path: the entries are strictly increasing, nothing can cancel; shards XOR their residues)
          f0 = wave_xor_u64(f0); f1 = wave_xor_u64(f1);
          f2 = wave_xor_u64(f2); f3 = wave_xor_u64(f3);
          if ((threadIdx.x & 63) == 0)
            { atomicXor((unsigned long long *) &ctrl->fp[0], (unsigned long long) f0); atomicXor((unsigned long long *) &ctrl->fp[1], (unsigned long long) f1);
              atomicXor((unsigned long long *) &ctrl->fp[2], (unsigned long long) f2); atomicXor((unsigned long long *) &ctrl->fp[3], (unsigned long long) f3);
            }
        }
    }
}

// requests -> degrees (the S_hi(rc(x)) term), and the per-request symmetry proof
template <int W> __global__ void __launch_bounds__(TPB)
k_apply(Tab t, const u64 *__restrict__ req, int64_t nreq, Ctrl *__restrict__ ctrl)
{ const int64_t r = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (r >= nreq) return;
  Key<W> y;
  const u64 *q = req + r * (W + 1);
#pragma unroll
  for (int w = 0; w < W; w++) y.w[w] = q[w];
  const unsigned c = (unsigned) (q[W] & 0xFFFF), v = (unsigned) ((q[W] >> 16) & 0xFF);
  const int64_t j = find_key<W>(t.keys, t.dir, y);
  if (j < 0 || t.cnt[j] != c) { if (ctrl->missing == 0) ctrl->missing = 1; return; }
  if (v) deg_add(t.deg, j, v, t.g.wrap);
}

// exact symmetry proof for every entry of [lo,hi) against the local table (single GPU)
template <int W> __global__ void __launch_bounds__(TPB)
k_verify(Tab t, int64_t lo, int64_t hi, Ctrl *__restrict__ ctrl)
{ const int64_t i = lo + (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= hi) return;
  const Key<W> r = revcomp<W>(load_key<W>(t.keys, i), t.g.k);
  const int64_t j = find_key<W>(t.keys, t.dir, r);
  if (j < 0 || t.cnt[j] != t.cnt[i]) { if (ctrl->missing == 0) ctrl->missing = 1; }
}

// ---- pass 2 -------------------------------------------------------------------------------
// Entry i with (wrapped) degree <= 1 looks for its partners j > i; the pair enters the plot
// when deg(j) <= 1 too.  SYM: pairs at p != k-1-p stand for themselves and their complement
// image (weight 2).  General: every position is visited, weight 1.

SMG_DEV void plot_add(u64 *__restrict__ plot, unsigned ci, unsigned cj, unsigned wgt)
{ const unsigned s = ci + cj, m = ci < cj ? ci : cj;
  atomicAdd(plot + (size_t) s * SMG_PLOT_COLS + m, (u64) wgt);
}

template <int W, bool SYM> __global__ void __launch_bounds__(TPB)
k_pass2(Tab t, int64_t lo, int64_t hi, u64 *__restrict__ plot, const TabSet *__restrict__ set = NULL)
{ const int64_t i = lo + (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= hi) return;
  const Geo g = t.g;
  const unsigned di = t.deg[i];
  if (di > 1) return;
  if (di == 0 && !g.wrap) return;            // no wrap possible: degree 0 means no pair at all
  const Key<W> x = load_key<W>(t.keys, i);
  const unsigned c = t.cnt[i];

  bool big = false;
  if (i + WIN_LIM < t.n) big = same_block<W>(x, load_key<W>(t.keys, i + WIN_LIM), g);
  if (!big)
    { for (int64_t j = i + 1; j < t.n; j++)
        { const Key<W> y = load_key<W>(t.keys, j);
          if (!same_block<W>(x, y, g)) break;
          const int p = pair_pos<W>(x, y);
          if (p >= 0)
            { const unsigned cj = t.cnt[j];
              if (c + cj <= SMG_SMAX && t.deg[j] <= 1)
                { const unsigned wgt = (SYM && p != g.k - 1 - p) ? 2 : 1;
                  plot_add(plot, c, cj, wgt);
                }
            }
        }
    }
  else
    { int64_t a = i + 1, b = t.n;
      while (a < b)
        { const int64_t m = (a + b) >> 1;
          if (!same_block<W>(x, load_key<W>(t.keys, m), g)) b = m; else a = m + 1;
        }
      const int64_t bhi = a;
      for (int p = g.p0; p < g.k; p++)
        for (int d = 1; d <= 3; d++)
          { const Key<W> y = flip_base<W>(x, p, d);
            if (!key_lt<W>(x, y)) continue;
            const int64_t j = lower_bound_key<W>(t.keys, i + 1, bhi, y);
            if (j < bhi && key_eq<W>(load_key<W>(t.keys, j), y))
              { const unsigned cj = t.cnt[j];
                if (c + cj <= SMG_SMAX && t.deg[j] <= 1)
                  { const unsigned wgt = (SYM && p != g.k - 1 - p) ? 2 : 1;
                    plot_add(plot, c, cj, wgt);
                  }
              }
          }
    }
  if (!SYM)
    { for (int p = 0; p < g.p0; p++)
        for (int d = 1; d <= 3; d++)
          { const Key<W> y = flip_base<W>(x, p, d);
            if (!key_lt<W>(x, y)) continue;
            if (set)
              { int64_t j;
                const int sh = set_find<W>(set, y, j);
                if (j >= 0)
                  { const unsigned cj = set->shard[sh].cnt[j];
                    if (c + cj <= SMG_SMAX && set->shard[sh].deg[j] <= 1) plot_add(plot, c, cj, 1);
                  }
              }
            else
              { const int64_t j = find_key<W>(t.keys, t.dir, y);
                if (j >= 0)
                  { const unsigned cj = t.cnt[j];
                    if (c + cj <= SMG_SMAX && t.deg[j] <= 1) plot_add(plot, c, cj, 1);
                  }
              }
          }
    }
}

// ---- extract on the counted path (k > 85): the pairs pass 2 counts, as records ---------------------
// The same walk as k_pass2<W, true>; a pair at a labelled pixel is written out like kf_extract writes it (the pair,
// and for p != k-1-p its mirror image at k-1-p).  One global atomic per pair: this path is exact, not fast.
template <int W> __global__ void __launch_bounds__(TPB)
k_extract(Tab t, const uint16_t *__restrict__ labels, u64 *__restrict__ out, u64 capacity, u64 *__restrict__ total)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i >= t.n) return;
  const Geo g = t.g;
  const unsigned di = t.deg[i];
  if (di > 1) return;
  if (di == 0 && !g.wrap) return;
  const Key<W> x = load_key<W>(t.keys, i);
  const unsigned c = t.cnt[i];
  const int k = g.k;

  auto emit = [&](int64_t j, const Key<W> &y, int p)
  { const unsigned cj = t.cnt[j];
    if (c + cj > SMG_SMAX || t.deg[j] > 1) return;
    const unsigned sum = c + cj, mn = c < cj ? c : cj;
    const unsigned lab = labels[(size_t) sum * SMG_PLOT_COLS + mn];
    if (!lab) return;
    const bool w2 = p != k - 1 - p;
    const unsigned bi = base_at<W>(x, p), bj = base_at<W>(y, p);              // bi < bj (i < j)
    const u64 q = atomicAdd(total, (u64) (w2 ? 2 : 1));
    if (q < capacity)
      { const bool pj = c < cj;                                                 // cnt[a] < cnt[b]: print b, alt base of a
        const Key<W> &who = pj ? y : x;
        u64 *o = out + q * (W + 1);
#pragma unroll
        for (int w = 0; w < W; w++) o[w] = who.w[w];
        o[W] = (u64) p | ((u64) (pj ? bi : bj) << 8) | ((u64) lab << 16);
      }
    if (w2 && q + 1 < capacity)
      { const bool pb = cj < c;                                                 // mirror image: a = rc(y), b = rc(x)
        const Key<W> who = revcomp<W>(pb ? x : y, k);
        u64 *o = out + (q + 1) * (W + 1);
#pragma unroll
        for (int w = 0; w < W; w++) o[w] = who.w[w];
        o[W] = (u64) (k - 1 - p) | ((u64) (pb ? 3u - bj : 3u - bi) << 8) | ((u64) lab << 16);
      }
  };

  bool big = false;
  if (i + WIN_LIM < t.n) big = same_block<W>(x, load_key<W>(t.keys, i + WIN_LIM), g);
  if (!big)
    { for (int64_t j = i + 1; j < t.n; j++)
        { const Key<W> y = load_key<W>(t.keys, j);
          if (!same_block<W>(x, y, g)) break;
          const int p = pair_pos<W>(x, y);
          if (p >= 0) emit(j, y, p);
        }
    }
  else
    { int64_t a = i + 1, b = t.n;
      while (a < b)
        { const int64_t m = (a + b) >> 1;
          if (!same_block<W>(x, load_key<W>(t.keys, m), g)) b = m; else a = m + 1;
        }
      const int64_t bhi = a;
      for (int p = g.p0; p < g.k; p++)
        for (int d = 1; d <= 3; d++)
          { const Key<W> y = flip_base<W>(x, p, d);
            if (!key_lt<W>(x, y)) continue;
            const int64_t j = lower_bound_key<W>(t.keys, i + 1, bhi, y);
            if (j < bhi && key_eq<W>(load_key<W>(t.keys, j), y)) emit(j, y, p);
          }
    }
}

// ---- extract on the general path (a table that is not closed under reverse complement): the pairs k_pass2<W, false> counts
// The walk of k_pass2<W, false>: suffix-side partners from the window block, prefix-side partners (p < p0) looked up in the
// table, or over virtual shards in whichever shard holds them (TabSet).  A pair is written ONCE, by its lower member, with the
// printed member and the alt base chosen as k_extract chooses them; no mirror image (if the table holds the complement pair,
// the walk finds it as a pair of its own).  Weight 1 per pair, as in the plot of the general path.
// Without wrap a degree <= 1 means at most one partner: the walk stops at it, and a wave reserves the slots of its records
// with one atomic.  A wrapped degree (k > 85: 0 or 1 mod 256) can stand for hundreds of partners: one atomic per record.
template <int W> __global__ void __launch_bounds__(TPB)
k_extract_general(Tab t, const uint16_t *__restrict__ labels, u64 *__restrict__ out, u64 capacity, u64 *__restrict__ total,
                  const TabSet *__restrict__ set)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  const Geo g = t.g;
  bool has = false;                          // (no wrap) the one record of this lane
  Key<W> rk; u64 rmeta = 0;
#pragma unroll
  for (int w = 0; w < W; w++) rk.w[w] = 0;
  unsigned di = 2;
  if (i < t.n) di = t.deg[i];
  if (di <= 1 && (di == 1 || g.wrap))        // (lanes without work stay for the wave's ballot below)
    { const Key<W> x = load_key<W>(t.keys, i);
      const unsigned c = t.cnt[i];
      bool done = false;
      // a partner y > x with count cj and degree dj: -> true when the walk can stop (no wrap: the one partner was found)
      auto visit = [&](const Key<W> &y, int p, unsigned cj, unsigned dj) -> bool
      { if (c + cj > SMG_SMAX) return false;                                   // not a pair (nor counted in a degree)
        const unsigned sum = c + cj, mn = c < cj ? c : cj;
        const unsigned lab = dj <= 1 ? labels[(size_t) sum * SMG_PLOT_COLS + mn] : 0u;
        if (lab)
          { const bool pj = c < cj;                                               // print the larger count; tie: x (smaller base)
            const Key<W> &who = pj ? y : x;
            const u64 meta = (u64) p | ((u64) (pj ? base_at<W>(x, p) : base_at<W>(y, p)) << 8) | ((u64) lab << 16);
            if (!g.wrap) { rk = who; rmeta = meta; has = true; }
            else
              { const u64 q = atomicAdd(total, (u64) 1);
                if (q < capacity)
                  { u64 *o = out + q * (W + 1);
#pragma unroll
                    for (int w = 0; w < W; w++) o[w] = who.w[w];
                    o[W] = meta;
                  }
              }
          }
        return !g.wrap;
      };

      bool big = false;
      if (i + WIN_LIM < t.n) big = same_block<W>(x, load_key<W>(t.keys, i + WIN_LIM), g);
      if (!big)
        { for (int64_t j = i + 1; j < t.n && !done; j++)
            { const Key<W> y = load_key<W>(t.keys, j);
              if (!same_block<W>(x, y, g)) break;
              const int p = pair_pos<W>(x, y);
              if (p >= 0) done = visit(y, p, t.cnt[j], t.deg[j]);
            }
        }
      else
        { int64_t a = i + 1, b = t.n;
          while (a < b)
            { const int64_t m = (a + b) >> 1;
              if (!same_block<W>(x, load_key<W>(t.keys, m), g)) b = m; else a = m + 1;
            }
          const int64_t bhi = a;
          for (int p = g.p0; p < g.k && !done; p++)
            for (int d = 1; d <= 3 && !done; d++)
              { const Key<W> y = flip_base<W>(x, p, d);
                if (!key_lt<W>(x, y)) continue;
                const int64_t j = lower_bound_key<W>(t.keys, i + 1, bhi, y);
                if (j < bhi && key_eq<W>(load_key<W>(t.keys, j), y)) done = visit(y, p, t.cnt[j], t.deg[j]);
              }
        }
      for (int p = 0; p < g.p0 && !done; p++)
        for (int d = 1; d <= 3 && !done; d++)
          { const Key<W> y = flip_base<W>(x, p, d);
            if (!key_lt<W>(x, y)) continue;
            if (set)
              { int64_t j;
                const int sh = set_find<W>(set, y, j);
                if (j >= 0) done = visit(y, p, set->shard[sh].cnt[j], set->shard[sh].deg[j]);
              }
            else
              { const int64_t j = find_key<W>(t.keys, t.dir, y);
                if (j >= 0) done = visit(y, p, t.cnt[j], t.deg[j]);
              }
          }
    }
  if (g.wrap) return;                        // (uniform over the grid)
  const u64 mask = __ballot(has);
  if (!mask) return;
  const int lead = __ffsll((long long) mask) - 1;
  u64 base = 0;
  if ((int) (threadIdx.x & 63) == lead) base = atomicAdd(total, (u64) __popcll(mask));
  base = __shfl(base, lead, 64);
  if (has)
    { const u64 q = base + __builtin_amdgcn_mbcnt_hi((unsigned) (mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) mask, 0u));
      if (q < capacity)
        { u64 *o = out + q * (W + 1);
#pragma unroll
          for (int w = 0; w < W; w++) o[w] = rk.w[w];
          o[W] = rmeta;
        }
    }
}

// ---- counted path (k > 85, and the general all-positions fallback at any k) ---------------------

static Tab make_tab(smg_engine *e)
{ Tab t;
  t.keys = e->tab.keys; t.cnt = e->tab.cnt; t.deg = e->deg; t.n = e->tab.n; t.g = e->tab.geo; t.dir = e->run.dir;
  return t;
}

static int counted_prepare(smg_engine *e, RunKind kind, char *errbuf, size_t errlen)
{ begin_run(e, kind);
  HIPCHK(hipMemsetAsync(e->ctrl, 0, sizeof(Ctrl), e->stream));
  set_geo(e);
  const int64_t dbytes = ((e->tab.n + 3) & ~3ll) + 4;
  HIPCHK(e->deg.reserve(dbytes));
  HIPCHK(hipMemsetAsync(e->deg, 0, (size_t) dbytes, e->stream));
  const int rc = dir_geometry(e, 8, errbuf, errlen);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(e->bstart, 0xFF, sizeof(uint32_t) * ((size_t) e->run.dir.nb + 2), e->stream));
  Tab t = make_tab(e);
  const unsigned nblk = (unsigned) ((e->tab.n + 1 + TPB - 1) / TPB);
  with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(k_directory<w()>, dim3(nblk), dim3(TPB), 0, e->stream, t, e->bstart, e->ctrl); });
  HIPCHK(hipGetLastError());
  return SMG_OK;
}

__global__ void __launch_bounds__(TPB) kc_fill_u32(uint32_t *__restrict__ p, int64_t n, uint32_t v, uint32_t last)
{ const int64_t i = (int64_t) blockIdx.x * TPB + threadIdx.x;
  if (i < n) p[i] = i == n - 1 ? last : v;
}

// The launches of both paths, each over the whole table, between its pair of events and dispatched on W.  What the
// one-shot run and the phase API do differently (emit_all, the first size of the record list, k_verify) is their callers'.

// k_pass1<W, SYM>: events 2, 3
template <bool SYM> static void launch_pass1(smg_engine *e, int emit_all, int want_fp, u64 *req, int64_t cap, const TabSet *d_set)
{ const unsigned nblk = (unsigned) ((e->tab.n + TPB - 1) / TPB);
  Tab t = make_tab(e);
  hipEventRecord(e->ev[EV_PASS1_BEG], e->stream);
  if (e->tab.n > 0)
    {
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL((k_pass1<w(), SYM>), dim3(nblk), dim3(TPB), 0, e->stream, t,
          (int64_t) 0, e->tab.n, emit_all, want_fp, req, cap, e->ctrl, d_set); });
    }
  hipEventRecord(e->ev[EV_PASS1_END], e->stream);
}

// k_apply<W> over nrec records, then (verify) k_verify<W> over the table: events 4, 5
static void launch_apply(smg_engine *e, const u64 *rec, int64_t nrec, bool verify)
{ Tab t = make_tab(e);
  hipEventRecord(e->ev[EV_LOOKUP_BEG], e->stream);
  if (nrec > 0)
    { const unsigned rb = (unsigned) ((nrec + TPB - 1) / TPB);
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(k_apply<w()>, dim3(rb), dim3(TPB), 0, e->stream, t, rec, nrec, e->ctrl); });
    }
  if (verify && e->tab.n > 0)
    { const unsigned nblk = (unsigned) ((e->tab.n + TPB - 1) / TPB);
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL(k_verify<w()>, dim3(nblk), dim3(TPB), 0, e->stream, t, (int64_t) 0, e->tab.n, e->ctrl); });
    }
  hipEventRecord(e->ev[EV_LOOKUP_END], e->stream);
}

// the plot cleared, then k_pass2<W, SYM>: events 6, 7
template <bool SYM> static int launch_pass2(smg_engine *e, int64_t *d_plot, const TabSet *d_set, char *errbuf, size_t errlen)
{ HIPCHK(hipMemsetAsync(d_plot, 0, sizeof(int64_t) * SMG_PLOT_CELLS, e->stream));
  hipEventRecord(e->ev[EV_PASS2_BEG], e->stream);
  if (e->tab.n > 0)
    { Tab t = make_tab(e);
      const unsigned nblk = (unsigned) ((e->tab.n + TPB - 1) / TPB);
      with_words<4>(e->tab.W, [&](auto w) { hipLaunchKernelGGL((k_pass2<w(), SYM>), dim3(nblk), dim3(TPB), 0, e->stream, t,
          (int64_t) 0, e->tab.n, (u64 *) d_plot, d_set); });
    }
  hipEventRecord(e->ev[EV_PASS2_END], e->stream);
  HIPCHK(hipGetLastError());
  return SMG_OK;
}

// Pass 1 of the symmetric half-scan = k_pass1<W, true>: S_all into deg[], records (rc(x), count | S_hi << 16) from the
// owners of a hi-side pair (emit_all: from every entry) into the flat list e->lists.cur.rec, which holds `cap` records at first and,
// where pass 1 counted more, that many on the second attempt.
static int counted_pass1(smg_engine *e, int emit_all, int symcheck, int64_t cap, char *errbuf, size_t errlen)
{ int rc;
  if ((rc = counted_prepare(e, RUN_COUNTED, errbuf, errlen))) return rc;
  for (int attempt = 0; attempt < 2; attempt++)
    { HIPCHK(e->lists.reserve_flat(cap, e->tab.W + 1));
      launch_pass1<true>(e, emit_all, symcheck == SMG_SYM_HASH, e->lists.cur.rec, cap, NULL);
      if ((rc = read_ctrl(e, errbuf, errlen))) return rc;
      if (e->h_ctrl->unsorted)
        return fail(errbuf, errlen, SMG_EFORMAT, "table entries are not strictly increasing%s");
      if ((int64_t) e->h_ctrl->nreq <= cap) break;
      cap = (int64_t) e->h_ctrl->nreq;
      HIPCHK(hipMemsetAsync(&e->ctrl->nreq, 0, sizeof(u64), e->stream));
      HIPCHK(hipMemsetAsync(e->ctrl->fp, 0, sizeof(u64) * 4, e->stream));
    }
  e->st.ms_pass1 = ms_between(e, EV_PASS1_BEG, EV_PASS1_END);
  e->st.nrequests = (int64_t) e->h_ctrl->nreq;
  return SMG_OK;
}

// symmetric half-scan with counted degrees (exact uint8 wrap emulation), k > 85
static int counted_symmetric(smg_engine *e, int symcheck, int64_t *d_plot, bool *symmetric,
                             char *errbuf, size_t errlen)
{ int rc;
  if ((rc = counted_pass1(e, 0, symcheck, e->tab.n / 4 + 1024, errbuf, errlen))) return rc;
  launch_apply(e, e->lists.cur.rec, e->st.nrequests, symcheck == SMG_SYM_EXACT);
  if ((rc = read_ctrl(e, errbuf, errlen))) return rc;
  e->st.ms_rclookup = ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
  *symmetric = e->h_ctrl->missing == 0;
  if (*symmetric && symcheck == SMG_SYM_HASH)
    *symmetric = e->h_ctrl->fp[0] == e->h_ctrl->fp[2] && e->h_ctrl->fp[1] == e->h_ctrl->fp[3];
  if (!*symmetric) return SMG_OK;
  if ((rc = launch_pass2<true>(e, d_plot, NULL, errbuf, errlen))) return rc;
  if ((rc = plot_sum(e, d_plot, errbuf, errlen))) return rc;
  e->st.ms_pass2 = ms_between(e, EV_PASS2_BEG, EV_PASS2_END);
  e->st.path = 1;
  e->run.completed = true;
  return SMG_OK;
}

// The same in the steps of the phase API (sharded runs): the flat list is presented to the router as full chunks of F_CH
// records; a received record adds S_hi to the degree of its k-mer (the uint8 wrap of PloidyPlot.c:163 emulated by deg_add)
// and proves that the k-mer is there with the same count.  The exact proof emits from every entry instead of k_verify.
static int counted_phase_pass1(smg_engine *e, int symcheck, char *errbuf, size_t errlen)
{ const int emit_all = symcheck == SMG_SYM_EXACT;
  int rc = counted_pass1(e, emit_all, symcheck, (emit_all ? e->tab.n : e->tab.n / 4) + 1024, errbuf, errlen);
  if (rc) return rc;
  e->run.rw = e->tab.W + 1;
  const int64_t nreq = e->st.nrequests;
  for (int i = 0; i < 4; i++) e->run.fp[i] = e->h_ctrl->fp[i];
  const int64_t nc = (nreq + F_CH - 1) / F_CH;
  if (nc >= 0x7FFFFFFFll) return fail(errbuf, errlen, SMG_EINVAL, "shard too large%s");
  HIPCHK(e->lists.reserve_fills(nc));
  if (nc > 0)
    hipLaunchKernelGGL(kc_fill_u32, dim3((unsigned) ((nc + TPB - 1) / TPB)), dim3(TPB), 0, e->stream, e->lists.cur.fill, nc, (uint32_t) F_CH,
                       (uint32_t) (nreq - (nc - 1) * F_CH));
  HIPCHK(hipGetLastError());
  e->run.n_chunks = (unsigned) nc;
  e->st.path = 1; e->st.ms_filter = 0;
  e->run.pass1_done = true;
  return SMG_OK;
}

static int counted_phase_apply(smg_engine *e, const u64 *rec, int64_t nrec, int64_t *missing, char *errbuf, size_t errlen)
{ launch_apply(e, rec, nrec, false);
  HIPCHK(hipGetLastError());
  if (!missing) { e->run.lookup_pending = true; return SMG_OK; }
  const int rc = read_ctrl(e, errbuf, errlen);
  if (rc) return rc;
  e->st.ms_rclookup += ms_between(e, EV_LOOKUP_BEG, EV_LOOKUP_END);
  *missing = (int64_t) e->h_ctrl->missing;
  return SMG_OK;
}

static int counted_phase_pass2(smg_engine *e, int64_t *d_plot, char *errbuf, size_t errlen)
{ const int rc = launch_pass2<true>(e, d_plot, NULL, errbuf, errlen);
  if (rc) return rc;
  e->st.path = 1; e->st.npairs = 0; e->st.ms_pass2 = -1.0;      // (no host wait: smg_engine_stats resolves the events)
  e->run.completed = true;
  return SMG_OK;
}

// general (assumption-free) path: both passes over every position
static int run_general(smg_engine *e, int64_t *d_plot, char *errbuf, size_t errlen)
{ int rc;
  if ((rc = counted_prepare(e, RUN_GENERAL, errbuf, errlen))) return rc;
  launch_pass1<false>(e, 0, 0, NULL, 0, NULL);
  if ((rc = launch_pass2<false>(e, d_plot, NULL, errbuf, errlen))) return rc;
  if ((rc = plot_sum(e, d_plot, errbuf, errlen))) return rc;
  if (e->h_ctrl->unsorted)
    return fail(errbuf, errlen, SMG_EFORMAT, "table entries are not strictly increasing%s");
  e->st.ms_pass1 += ms_between(e, EV_PASS1_BEG, EV_PASS1_END);
  e->st.ms_pass2 = ms_between(e, EV_PASS2_BEG, EV_PASS2_END);
  e->st.path = 2;
  e->run.completed = true;
  return SMG_OK;
}

// the general path of ONE shard of a table whose shards all live on this device (smg_multi.hpp: virtual shards): step 1
// builds the directory and the degree array (then the caller collects the Tabs of all shards into a TabSet on the
// device), step 2 = pass 1 (degrees, over all positions), step 3 = pass 2 -- a barrier between the steps is the caller's.
static int general_shard_prepare(smg_engine *e, Tab *out, char *errbuf, size_t errlen)
{ int rc = counted_prepare(e, RUN_GENERAL, errbuf, errlen);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  *out = make_tab(e);
  return SMG_OK;
}

static int general_shard_pass(smg_engine *e, const TabSet *d_set, int pass, int64_t *d_plot, char *errbuf, size_t errlen)
{ int rc = SMG_OK;
  if (pass == 1) launch_pass1<false>(e, 0, 0, NULL, 0, d_set);
  else rc = launch_pass2<false>(e, d_plot, d_set, errbuf, errlen);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  if ((rc = read_ctrl(e, errbuf, errlen))) return rc;
  if (e->h_ctrl->unsorted) return fail(errbuf, errlen, SMG_EFORMAT, "table entries are not strictly increasing%s");
  if (pass == 1) { e->st.ms_pass1 += ms_between(e, EV_PASS1_BEG, EV_PASS1_END); }
  else { e->st.ms_pass2 = ms_between(e, EV_PASS2_BEG, EV_PASS2_END); e->st.path = 2; e->run.completed = true; }
  return SMG_OK;
}

// out-of-core shards (fast_resume, smg_hetmers.hip) for k > 85: the byte a shard left behind is its array of counted degrees
// (S_all of every entry, uint8 with the reference's wrap); the look-ups of the received requests add S_hi of the complements
// on top (k_apply) and pass 2 reads the sums
static int counted_resume(smg_engine *e, const uint8_t *d_degs, char *errbuf, size_t errlen)
{ HIPCHK(hipSetDevice(e->device));
  int rc = counted_prepare(e, RUN_COUNTED, errbuf, errlen);  // control words, geometry, zeroed degrees, directory
  if (rc) return rc;
  if (e->tab.n > 0) HIPCHK(hipMemcpyAsync(e->deg, d_degs, (size_t) e->tab.n, hipMemcpyDeviceToDevice, e->stream));
  e->run.rw = e->tab.W + 1;
  e->st.nrequests = 0; e->st.ms_rclookup = 0; e->st.path = 1;
  e->run.pass1_done = true;
  return SMG_OK;
}
