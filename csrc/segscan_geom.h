// Geometry of the prefix-sum leaves (scan, segscan_cross, segscan_apply): a plain prefix sum,
// or one stage j of a segmented Hillis-Steele scan, along the middle axis of an [outer, n,
// inner] array.  Plain data and host code only, shared by leaf_cpu.cpp (the CPU twins and the
// entry points) and leaf_hip.hip (the launchers), in the style of cswap_geom.h; the kernels
// keep their own parameter struct.
#pragma once
#include <stdint.h>

#include "img_geom.h"  // slot_cap

namespace mxr {

// positions of the axis one lane walks with the running sum in registers; an axis longer than
// this is scanned in three phases (chunk sums, their scan, an add pass)
constexpr int64_t kScanChunk = 256;

struct ScanGeom {
  // attributes: element (o, pos, c) lives at (o*n + pos)*inner + c
  int64_t outer, n, inner;
  int exclusive = 0, reverse = 0;
  // derived by scan_geom_check
  int64_t chunks;  // ceil(n / kScanChunk)
  int64_t n_x;     // outer * n * inner: elements of a slot
  int64_t n_sum;   // outer * chunks * inner: chunk sums of a slot (0 where chunks == 1)
  int64_t ws;      // workspace elements of a slot: sums and offsets of every level
};

// workspace of one slot: a level of `chunks` > 1 chunks keeps its sums and their scanned
// offsets, 2 * lines * chunks elements, and the levels below it (the sums are scanned by the
// same rule)
inline int64_t scan_ws_elems(int64_t lines, int64_t n) {
  int64_t ws = 0;
  while (n > kScanChunk) {
    n = (n + kScanChunk - 1) / kScanChunk;
    ws += 2 * lines * n;
  }
  return ws;
}

// Validate g's attributes and fill the derived fields.  Returns the entry points' codes --
// -3 malformed, -2 unsupported element width, 0 nothing to do -- or 1 to go on.
// stride_x: the operand's slot stride in elements.
inline int scan_geom_check(ScanGeom& g, int elem_bytes, int64_t slots, int64_t stride_x) {
  const int64_t lim = 0x7fffffff;
  if (g.outer < 0 || g.n < 0 || g.inner < 0 || g.outer > lim || g.n > lim || g.inner > lim ||
      slots < 0 || stride_x < 0)
    return -3;
  if (elem_bytes != 8 && elem_bytes != 16) return -2;
  if (g.outer && g.inner && g.n > ((int64_t)1 << 60) / g.outer / g.inner) return -3;
  g.chunks = (g.n + kScanChunk - 1) / kScanChunk;
  g.n_x = g.outer * g.n * g.inner;
  g.n_sum = g.chunks > 1 ? g.outer * g.chunks * g.inner : 0;
  g.ws = scan_ws_elems(g.outer * g.inner, g.n);  // below n_x: 2/256 + 2/256^2 + ... of it
  if (slots == 0 || g.n_x == 0) return 0;
  // n_x (the largest count of a slot) and the stride within slot_cap: no extent wraps
  const int64_t cap = slot_cap(slots);
  if (g.n_x > cap || stride_x > cap) return -3;
  return 1;
}

struct SegscanGeom {
  // attributes: the state is [outer, n, inner] with the continuation flag in column inner - 1;
  // stage j reaches back j positions, 1 <= j < n
  int64_t outer, n, inner, j;
  // derived by segscan_geom_check
  int64_t n_x;  // outer * n * inner: elements of the state
  int64_t n_p;  // outer * (n - j) * inner: products of the stage
};

// As scan_geom_check.  stride_a / stride_b: the operands' slot strides in elements (0 where
// there is none).
inline int segscan_geom_check(SegscanGeom& g, int elem_bytes, int64_t slots, int64_t stride_a,
                              int64_t stride_b = 0) {
  const int64_t lim = 0x7fffffff;
  if (g.outer < 0 || g.n < 0 || g.inner < 0 || g.outer > lim || g.n > lim || g.inner > lim ||
      g.j < 1 || g.j >= g.n || slots < 0 || stride_a < 0 || stride_b < 0)
    return -3;
  if (elem_bytes != 8 && elem_bytes != 16) return -2;
  if (g.outer && g.inner && g.n > ((int64_t)1 << 60) / g.outer / g.inner) return -3;
  g.n_x = g.outer * g.n * g.inner;
  g.n_p = g.outer * (g.n - g.j) * g.inner;
  if (slots == 0 || g.n_x == 0) return 0;
  const int64_t cap = slot_cap(slots);
  if (g.n_x > cap || stride_a > cap || stride_b > cap) return -3;
  return 1;
}

}  // namespace mxr
