// smg_mergepath.hpp -- the merge-path logic of ks_merge<W> (smg_keysort.hpp) as plain C++: the diagonal search and the
// sequential merge of one thread's items.  No HIP type in here, so that the same text compiles for the device and, in
// mergepath_check.cpp, for the host under the address and undefined-behaviour sanitizers.
//
// Two sorted lists A[0 .. na) and B[0 .. nb) merge into na + nb outputs; of equal keys A's comes first.  The first d
// outputs take mp_split(d) items from A and d - mp_split(d) from B, whatever d: tiles and threads cut the output evenly
// and find their inputs with one search each (Green, McColl, Bader: "GPU merge path", ICS 2012).

#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MP_HD __host__ __device__ __forceinline__
#define MP_UNROLL _Pragma("unroll")
#else
#define MP_HD inline
#define MP_UNROLL
#endif

// outputs per workgroup of ks_merge<W> (T), merged by MP_TPB threads of T / MP_TPB items each
#define MP_TPB 256
template <int W> struct KsMergeTile { static constexpr int value = W <= 2 ? 2048 : 1024; };
static inline int ks_merge_tile(int W)
{ return W == 1 ? KsMergeTile<1>::value : W == 2 ? KsMergeTile<2>::value : W == 3 ? KsMergeTile<3>::value : KsMergeTile<4>::value; }

// is the W-word key at a less than the one at b?  (left aligned k-mers: word 0 is the most significant)
template <int W> MP_HD bool mp_key_lt(const unsigned long long *a, const unsigned long long *b)
{ MP_UNROLL
  for (int w = 0; w < W; w++)
    { if (a[w] != b[w]) return a[w] < b[w]; }
  return false;
}

// Items of A among the first `diag` outputs, 0 <= diag <= na + nb.  b_before_a(j, i): is B[j] < A[i]?
// The search looks at A[i] for i < min(diag, na) and at B[j] for j < min(diag, nb) only.
template <class BBeforeA> MP_HD int64_t mp_split(int64_t diag, int64_t na, int64_t nb, BBeforeA b_before_a)
{ int64_t lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
  while (lo < hi)
    { const int64_t mid = (lo + hi) >> 1;                      // are mid items from A enough?  (B[diag - 1 - mid] then goes out before A[mid])
      if (b_before_a(diag - 1 - mid, mid)) hi = mid; else lo = mid + 1;
    }
  return lo;
}

// The next `count` <= IPT outputs from the split (i, j): emit(c, from_a, index) for c = 0 .. count - 1, index into A or B.
// The caller guarantees count <= (na - i) + (nb - j); b_before_a is asked only about items that both exist.  The trip
// count is a constant so that a device caller's IPT outputs stay in registers.
template <int IPT, class BBeforeA, class Emit>
MP_HD void mp_merge_run(int64_t i, int64_t j, int64_t na, int64_t nb, int count, BBeforeA b_before_a, Emit emit)
{ MP_UNROLL
  for (int c = 0; c < IPT; c++)
    if (c < count)
      { const bool from_a = j >= nb || (i < na && !b_before_a(j, i));
        emit(c, from_a, from_a ? i : j);
        if (from_a) i++; else j++;
      }
}
