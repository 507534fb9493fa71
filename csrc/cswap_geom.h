// Geometry of the compare-exchange leaves (cswap_diff, cswap_cross, cswap_apply): one stage
// (k, j) of a bitonic sorting network along the middle axis of an [outer, n, inner] array.
// Plain data and host code only, shared by leaf_cpu.cpp (the CPU twins) and leaf_hip.hip (the
// launchers), in the style of img_geom.h; the kernels keep their own parameter struct.
#pragma once
#include <stdint.h>

#include "img_geom.h"  // slot_cap

namespace mxr {

struct CswapGeom {
  // attributes: element (o, pos, c) lives at (o*n + pos)*inner + c; n, k, j powers of two with
  // j < k <= n; by = -1: every inner index is its own sort, by >= 0: column `by` is the key
  // of all `inner` columns of a row (table mode)
  int64_t outer, n, inner, by, k, j;
  int descending = 0;
  // derived by cswap_geom_check
  int lj;          // log2 j
  int64_t half;    // n / 2: pairs of one sort
  int64_t cols;    // columns that carry a flag: 1 in table mode, else inner
  int64_t n_x;     // outer * n * inner: elements of the array
  int64_t n_pair;  // outer * half * inner: one product per pair and column
  int64_t n_flag;  // outer * half * cols: one difference / flag per pair and flag column
};

inline bool cswap_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// Pair t of [0, n/2): i is t with a zero bit inserted at bit lj, l = i | j; ascending iff
// (i & k) == 0, flipped when the whole sort is descending.
inline int64_t cswap_low(int64_t t, int lj) {
  return ((t >> lj) << (lj + 1)) | (t & (((int64_t)1 << lj) - 1));
}
inline bool cswap_ascending(const CswapGeom& g, int64_t i) {
  return ((i & g.k) == 0) != (g.descending != 0);
}

// Validate g's attributes and fill the derived fields.  Returns the entry points' codes --
// -3 malformed, -2 unsupported element width, 0 nothing to do -- or 1 to go on.
// stride_a / stride_b: the operands' slot strides in elements (0 where there is none).
inline int cswap_geom_check(CswapGeom& g, int elem_bytes, int64_t slots, int64_t stride_a,
                            int64_t stride_b = 0) {
  const int64_t lim = 0x7fffffff;
  if (g.outer < 0 || g.inner < 0 || g.n < 2 || g.outer > lim || g.n > lim || g.inner > lim ||
      !cswap_pow2(g.n) || !cswap_pow2(g.k) || !cswap_pow2(g.j) || g.j >= g.k || g.k > g.n ||
      g.by < -1 || (g.inner > 0 && g.by >= g.inner) || slots < 0 || stride_a < 0 || stride_b < 0)
    return -3;
  if (elem_bytes != 8 && elem_bytes != 16) return -2;
  if (g.outer && g.inner && g.n > ((int64_t)1 << 60) / g.outer / g.inner) return -3;
  g.lj = 0;
  while (((int64_t)1 << g.lj) < g.j) ++g.lj;
  g.half = g.n / 2;
  g.cols = g.by >= 0 ? 1 : g.inner;
  g.n_x = g.outer * g.n * g.inner;
  g.n_pair = g.outer * g.half * g.inner;
  g.n_flag = g.outer * g.half * g.cols;
  if (slots == 0 || g.n_x == 0) return 0;
  // n_x (the largest count of a slot) and the strides within slot_cap: no extent wraps
  const int64_t cap = slot_cap(slots);
  if (g.n_x > cap || stride_a > cap || stride_b > cap) return -3;
  return 1;
}

}  // namespace mxr
