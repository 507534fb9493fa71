// Geometry of the image leaf kernels (im2col, col2im, resize2d, dwconv): the attributes the
// mx_* entry points take, what is derived from them once, and their range checks.  Plain
// data and host code only, shared by leaf_cpu.cpp (the CPU twins) and leaf_hip.hip (the
// launchers); the kernels keep their own parameter structs, filled from this record.
#pragma once
#include <stdint.h>

#include <initializer_list>

namespace mxr {

// What a slot's element count and a slot stride may be at most, for `slots` > 0 slots: with
// both within it, (slots - 1) * stride + count and slots * count stay below 2^62, so no entry
// point forms an extent that wraps int64_t (and comes out looking small to the index-width
// choice of a launcher).  mx_perm_gather's rule, shared by every leaf.
inline int64_t slot_cap(int64_t slots) { return ((int64_t)1 << 61) / slots; }

// whether the product of non-negative factors is at most cap, without forming a product
// that wraps
inline bool product_within(int64_t cap, std::initializer_list<int64_t> factors) {
  for (int64_t f : factors)
    if (f == 0) return true;
  int64_t p = 1;
  for (int64_t f : factors) {
    if (p > cap / f) return false;
    p *= f;
  }
  return true;
}

struct ImgGeom {
  // attributes (resize2d: OH x OW is the output size and the window is 1 x 1)
  int64_t N, C, H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW;
  int64_t mult = 1;      // dwconv: output channels per input channel
  int wbh = 0, wbw = 0;  // resize2d: bits of the height / width weights
  int nhwc = 0;
  // derived by img_geom_check
  int64_t sN, sH, sW, sC;  // strides of the input image [N, C, H, W] / [N, H, W, C] in elements
  int64_t K, OC;           // C * KH * KW: a patch-matrix row; C * mult
  int64_t n_in;            // elements of the input image
  int64_t rows, inner;     // the leaf's output as rows x inner, inner contiguous
  int64_t n_out;           // rows * inner
};

// What a leaf writes, which says what rows x inner are.  An image of CH channels and h x w
// pixels is (N*h*w) x CH in NHWC and (N*CH*h) x w in NCHW.
enum ImgOut {
  IMG_PATCHES,  // im2col: the patch matrix, (N*OH*OW) x K
  IMG_INPUT,    // col2im: the image [N, C, H, W]
  IMG_OUTPUT,   // resize2d, dwconv: the image [N, OC, OH, OW]
};

// Where the leaves' checks differ.  The kernels hold tap coordinates, channel and tap counts
// in 32 bits, each its own expressions.
enum : unsigned {
  IMG_ARITH_FIRST = 1,  // -2 for an element that is not 8 or 16 bytes, ahead of the 2^31 bounds
                        // (without it the width is left to the dispatch: after the checks here)
  IMG_NEED_PIXELS = 2,  // H and W positive: every output reads a pixel
  IMG_GATHER_TAPS = 4,  // oh*sh + kh*dh - pt and its w twin
  IMG_SCATTER_TAPS = 8, // y + pt - kh*dh and its w twin
  IMG_TAP_COUNT = 16,   // KH * KW
  IMG_CHANNELS = 32,    // C * mult
};

struct ImgLeaf {
  ImgOut out;
  unsigned checks;
};
constexpr ImgLeaf kIm2colLeaf{IMG_PATCHES, IMG_GATHER_TAPS};
constexpr ImgLeaf kCol2imLeaf{IMG_INPUT, IMG_ARITH_FIRST | IMG_SCATTER_TAPS | IMG_TAP_COUNT};
constexpr ImgLeaf kResize2dLeaf{IMG_OUTPUT, IMG_ARITH_FIRST | IMG_NEED_PIXELS};
constexpr ImgLeaf kDwconvLeaf{IMG_OUTPUT, IMG_GATHER_TAPS | IMG_TAP_COUNT | IMG_CHANNELS};

// Validate g's attributes for `leaf` and fill the derived fields.  Returns the entry points'
// codes -- -3 malformed, -2 unsupported element width, 0 nothing to do -- or 1 to go on.
// stride_a / stride_b: the operands' slot strides in elements (0 where there is none).
inline int img_geom_check(ImgGeom& g, ImgLeaf leaf, int elem_bytes, int64_t slots,
                          int64_t stride_a, int64_t stride_b = 0) {
  const unsigned ck = leaf.checks;
  if (g.OH <= 0 || g.OW <= 0 || g.KH <= 0 || g.KW <= 0 || g.sh <= 0 || g.sw <= 0 || g.dh <= 0 ||
      g.dw <= 0 || g.pt < 0 || g.pl < 0 || g.N < 0 || g.C < 0 || g.H < 0 || g.W < 0 ||
      g.mult <= 0 || slots < 0 || stride_a < 0 || stride_b < 0 || g.wbh < 0 || g.wbh > 12 ||
      g.wbw < 0 || g.wbw > 12)
    return -3;
  if ((ck & IMG_NEED_PIXELS) && (g.H == 0 || g.W == 0)) return -3;
  if ((ck & IMG_ARITH_FIRST) && elem_bytes != 8 && elem_bytes != 16) return -2;
  const int64_t lim = 0x7fffffff;
  const int64_t dims[] = {g.N,  g.C,  g.H,  g.W,  g.KH, g.KW, g.sh, g.sw,
                          g.pt, g.pl, g.dh, g.dw, g.OH, g.OW, g.mult};
  for (int64_t d : dims)
    if (d > lim) return -3;
  if ((ck & IMG_GATHER_TAPS) && ((g.OH - 1) * g.sh + (g.KH - 1) * g.dh > lim ||
                                 (g.OW - 1) * g.sw + (g.KW - 1) * g.dw > lim))
    return -3;
  if ((ck & IMG_SCATTER_TAPS) && (g.H + g.pt > lim || g.W + g.pl > lim ||
                                  (g.KH - 1) * g.dh > lim || (g.KW - 1) * g.dw > lim))
    return -3;
  if ((ck & IMG_TAP_COUNT) && g.KH * g.KW > lim) return -3;
  if ((ck & IMG_CHANNELS) && g.C * g.mult > lim) return -3;
  if (slots == 0 || g.N == 0 || g.C == 0) return 0;
  if (leaf.out == IMG_INPUT && (g.H == 0 || g.W == 0)) return 0;
  // Every extent a side forms -- (slots - 1) * stride + a slot's elements, slots * n_out --
  // stays below 2^62: the strides, the input image and the taps of all outputs (which bound
  // the patch matrix, the output image and the weights) are each at most 2^61 / slots.
  const int64_t cap = slot_cap(slots);
  if (stride_a > cap || stride_b > cap || !product_within(cap, {g.N, g.C, g.H, g.W}) ||
      !product_within(cap, {g.N, g.C, g.mult, g.OH, g.OW, g.KH, g.KW}))
    return -3;
  const bool nhwc = g.nhwc != 0;
  g.sN = g.C * g.H * g.W;
  g.sH = nhwc ? g.W * g.C : g.W;
  g.sW = nhwc ? g.C : 1;
  g.sC = nhwc ? 1 : g.H * g.W;
  g.K = g.C * g.KH * g.KW;
  g.OC = g.C * g.mult;
  g.n_in = g.N * g.sN;
  if (leaf.out == IMG_PATCHES) {
    g.rows = g.N * g.OH * g.OW, g.inner = g.K;
  } else {
    const bool in = leaf.out == IMG_INPUT;
    const int64_t ch = in ? g.C : g.OC, h = in ? g.H : g.OH, w = in ? g.W : g.OW;
    g.rows = nhwc ? g.N * h * w : g.N * ch * h, g.inner = nhwc ? ch : w;
  }
  g.n_out = g.rows * g.inner;
  return 1;
}

}  // namespace mxr
