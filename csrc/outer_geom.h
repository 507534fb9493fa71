// Geometry of the outer-product leaf (outer_cross): per group and row, the A x B products of
// a row of A elements with a row of B elements, trimmed to the first n_out.  Plain data and
// host code only, shared by leaf_cpu.cpp (the CPU twin and the entry point) and leaf_hip.hip
// (the launcher), in the style of segscan_geom.h; the kernel keeps its own parameter struct.
#pragma once
#include <stdint.h>

#include "img_geom.h"  // slot_cap, product_within

namespace mxr {

struct OuterGeom {
  // attributes: L is [groups, rows, A], H is [groups, rows, B] and the output
  // [groups, rows, n_out] with column c = a + A * b, 1 <= n_out <= A * B
  int64_t groups, rows, A, B, n_out;
  // derived by outer_geom_check
  int64_t n_l;  // rows * A: elements of one group of L
  int64_t n_h;  // rows * B: elements of one group of H
  int64_t n_o;  // groups * rows * n_out: elements of an output slot
};

// Validate g's attributes and fill the derived fields.  Returns the entry points' codes --
// -3 malformed, -2 unsupported element width, 0 nothing to do -- or 1 to go on.
// l_slot / h_slot: the operands' slot strides, l_group / h_group: their group strides, in
// elements.  Every extent an index is formed from -- a slot's reach (groups - 1) * group stride
// + rows * A, the strides, the output -- stays within slot_cap.
inline int outer_geom_check(OuterGeom& g, int elem_bytes, int64_t slots, int64_t l_slot,
                            int64_t l_group, int64_t h_slot, int64_t h_group) {
  const int64_t lim = 0x7fffffff;
  if (g.groups < 0 || g.rows < 0 || g.A < 1 || g.B < 1 || g.n_out < 1 || g.groups > lim ||
      g.rows > lim || g.A > lim || g.B > lim || g.n_out > lim || slots < 0 || l_slot < 0 ||
      l_group < 0 || h_slot < 0 || h_group < 0)
    return -3;
  // A and B are within lim here, so their product stays below 2^62
  if (g.n_out > g.A * g.B) return -3;
  if (elem_bytes != 8 && elem_bytes != 16) return -2;
  if (slots == 0 || g.groups == 0 || g.rows == 0) {
    g.n_l = g.n_h = g.n_o = 0;
    return 0;
  }
  const int64_t cap = slot_cap(slots);
  if (!product_within(cap, {g.rows, g.A}) || !product_within(cap, {g.rows, g.B}) ||
      !product_within(cap, {g.groups, g.rows, g.n_out}) || l_slot > cap || h_slot > cap ||
      !product_within(cap, {g.groups, l_group}) || !product_within(cap, {g.groups, h_group}))
    return -3;
  g.n_l = g.rows * g.A;
  g.n_h = g.rows * g.B;
  g.n_o = g.groups * g.rows * g.n_out;
  return 1;
}

}  // namespace mxr
