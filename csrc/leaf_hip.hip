// gfx950 leaf kernels of the moosex ring dialect: the image leaves (im2col, dwconv, col2im,
// resize2d), the piecewise-linear and piecewise-polynomial local steps (pwl_cross, pwp_cross),
// the compare-exchange leaves (cswap_diff / _cross / _apply), the permuted row gather of a
// shuffle step (perm_gather), the prefix-sum leaves (scan, segscan_cross / _apply) and the
// outer-product leaf of a demultiplexer level (outer_cross).  Each is a share-wise kernel over
// slots whose geometry and sizes are checked on the host (img_geom.h, cswap_geom.h,
// segscan_geom.h, outer_geom.h, mx_perm_gather) before it gets here.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "moosex.h"
#include "ring_launch.h"

namespace {

// ---------------------------------------------------------------------------
// The image leaves (im2col, dwconv, col2im, resize2d, pwl_cross).  Their kernels are
// templates over <T, I, V>: the element, the index type (32-bit when every extent fits) and
// the elements a lane owns (2 only for u64: every access is 16 bytes).  The host side below is
// shared: the geometry arrives validated in an ImgGeom (img_geom.h), leaf_dispatch picks the
// form, lane_plan and row_grid shape the launch of a rows x inner output.
// ---------------------------------------------------------------------------
using mxr::ImgGeom;

template <class T, int V>
struct alignas(sizeof(T) * V) LaneVec {
  T v[V];
};

template <class T_, class I_, int V_>
struct LeafForm {
  using T = T_;
  using I = I_;
  static constexpr int V = V_;
};

// launch(LeafForm<T, I, V>{}) for elem_bytes (1 only where BYTES; else -2, as any other
// width), 32-bit indices when `small`, two u64 per lane when `two`
template <class T, int V, class F>
static int leaf_index(bool small, F& launch) {
  return small ? launch(LeafForm<T, int32_t, V>{}) : launch(LeafForm<T, int64_t, V>{});
}
template <bool BYTES = false, class F>
static int leaf_dispatch(int elem_bytes, bool small, bool two, F launch) {
  switch (elem_bytes) {
    case 1:
      if constexpr (BYTES) return leaf_index<uint8_t, 1>(small, launch);
      return -2;
    case 8: return two ? leaf_index<u64, 2>(small, launch) : leaf_index<u64, 1>(small, launch);
    case 16: return leaf_index<u128, 1>(small, launch);
    default: return -2;
  }
}

// 32-bit indices serve extents below 2^31 elements less `headroom`, the overshoot of a lane's
// last loop step
static bool fits32(int64_t headroom, std::initializer_list<int64_t> extents) {
  for (int64_t e : extents)
    if (e >= (1ll << 31) - headroom) return false;
  return true;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// A block of 256 lanes over a rows x inner output: bx inner lanes of V elements, no more
// than the inner extent needs (and at most max_bx), by 256 / bx rows; `tiles` blocks cover
// the inner extent.
struct LanePlan {
  int bx, by;
  int64_t tiles;
};
static LanePlan lane_plan(int64_t inner, int V, int max_bx = 64) {
  int bx = max_bx;
  while (bx > 1 && (bx / 2) * V >= inner) bx /= 2;
  return {bx, 256 / bx, (inner + (int64_t)bx * V - 1) / ((int64_t)bx * V)};
}

// the row grid is capped at 65,536 rows; a lane strides over the rest
static int64_t row_grid(int64_t rows, int by) {
  return std::min<int64_t>((rows + by - 1) / by, 65536 / by);
}

// the input strides and the window attributes of a kernel's parameter struct
template <class P>
static void set_strides(P& p, const ImgGeom& g) {
  using I = decltype(p.sN);
  p.sN = (I)g.sN, p.sH = (I)g.sH, p.sW = (I)g.sW, p.sC = (I)g.sC;
}
template <class P>
static void set_window(P& p, const ImgGeom& g) {
  p.H = (int)g.H, p.W = (int)g.W, p.KH = (int)g.KH, p.KW = (int)g.KW, p.sh = (int)g.sh;
  p.sw = (int)g.sw, p.pt = (int)g.pt, p.pl = (int)g.pl, p.dh = (int)g.dh, p.dw = (int)g.dw;
  p.OH = (int)g.OH, p.OW = (int)g.OW, p.nhwc = g.nhwc;
}

// im2col: the patch gather that turns a 2-D convolution into a GEMM over shares.  Output-
// stationary: a lane owns V adjacent output columns of one row, so stores are coalesced
// (V = 2 for u64 with an even row length: one 16-byte store; u128 moves 16 bytes per lane as
// is).  Block = 64 columns x 4 rows: a wave walks one output row, reading contiguous c runs
// (NHWC) or kw runs (NCHW, dw == 1).  The column (c, kh, kw) is decomposed once per lane and
// kept while the lane strides over rows; a row (n, oh, ow) once per visit.  A tap in the
// padding stores zero without a load.  Slots (share slots of a stacked buffer) are
// blockIdx.z, read at in_slot_stride and written densely.  I is the index type: 32-bit when
// both extents are below 2^31.
template <class I>
struct Im2colP {
  I in_slot_stride, sN, sH, sW, sC;  // input strides in elements (format-dependent)
  I K, rows;
  int C, H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW, nhwc;
};

template <class T, class I, int V>
__global__ void __launch_bounds__(256) k_im2col(const T* __restrict__ in, T* __restrict__ out,
                                                Im2colP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  const I col0 = (I)((blockIdx.x * (I)64 + threadIdx.x) * V);
  if (col0 >= p.K) return;
  I coff[V];
  int dy[V], dx[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const U col = (U)(col0 + j);
    U c, kh, kw;
    if (p.nhwc) {
      const U t = col / (U)p.C;
      c = col - t * (U)p.C;
      kh = t / (U)p.KW;
      kw = t - kh * (U)p.KW;
    } else {
      const U kk = (U)(p.KH * p.KW);
      c = col / kk;
      const U r = col - c * kk;
      kh = r / (U)p.KW;
      kw = r - kh * (U)p.KW;
    }
    coff[j] = (I)c * p.sC;
    dy[j] = (int)kh * p.dh - p.pt;
    dx[j] = (int)kw * p.dw - p.pl;
  }
  const T* __restrict__ src = in + (I)blockIdx.z * p.in_slot_stride;
  T* __restrict__ dst = out + (I)blockIdx.z * p.rows * p.K;
  for (I row = (I)(blockIdx.y * blockDim.y + threadIdx.y); row < p.rows;
       row += (I)(gridDim.y * blockDim.y)) {
    const U q = (U)row / (U)p.OW;
    const int ow = (int)((U)row - q * (U)p.OW);
    const U n = q / (U)p.OH;
    const int oh = (int)(q - n * (U)p.OH);
    const I base = (I)n * p.sN;
    const int y0 = oh * p.sh, x0 = ow * p.sw;
    LaneVec<T, V> o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int iy = y0 + dy[j], ix = x0 + dx[j];
      T v = (T)0;
      if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
        v = src[base + coff[j] + (I)iy * p.sH + (I)ix * p.sW];
      o.v[j] = v;
    }
    *reinterpret_cast<LaneVec<T, V>*>(dst + row * p.K + col0) = o;
  }
}

template <class T, class I, int V>
static int im2col_launch(const void* in, void* out, int64_t slots, int64_t in_slot_stride,
                         const ImgGeom& g, void* stream) {
  Im2colP<I> p;
  p.in_slot_stride = (I)in_slot_stride;
  set_strides(p, g);
  set_window(p, g);
  p.K = (I)g.K, p.rows = (I)g.rows, p.C = (int)g.C;
  const int64_t gx = (g.K + 64 * V - 1) / (64 * V);  // the kernel's block is 64 x 4
  hipLaunchKernelGGL((k_im2col<T, I, V>),
                     dim3((unsigned)gx, (unsigned)row_grid(g.rows, 4), (unsigned)slots),
                     dim3(64, 4), 0, S(stream), (const T*)in, (T*)out, p);
  MX_LAUNCH_CHECK();
  return 0;
}

// Depthwise convolution over shares (moosex.h mx_dwconv): a memory-bound stencil, output-
// stationary like k_im2col.  The output is rows x inner: inner = the C*mult channels (NHWC,
// rows (n, oh, ow)) or the OW columns of one channel (NCHW, rows (n, oh)); a lane owns V
// adjacent inner outputs of a row (V = 2 for u64 with an even inner extent: every store is 16
// bytes), adjacent lanes are adjacent in c (NHWC) or ow (NCHW), and the lane strides over
// rows.  A block is blockDim.x inner lanes x 256 / blockDim.x rows; blockIdx.x picks its
// inner tile: a run of blockDim.x * V channels (NHWC), or one channel and a run of OW (NCHW).
// The weights of the block's channels -- all KH*KW taps, in cross mode w0 + w1 (formed here,
// once per element) and w0 -- are staged in LDS once, laid out [tap][channel] so a lane's
// read is its own 16 bytes (NHWC) or a broadcast (NCHW).  Per output: KH*KW wrapping
// multiply-adds (two in cross mode, x0.(w0 + w1) + x1.w0) on inputs read once; a tap in the
// padding is skipped without a load.  Slots are blockIdx.z.  I: the index type, 32-bit when
// every extent is below 2^31.
template <class I>
struct DwconvP {
  I x_slot, w_slot, o_slot;  // slot strides in elements
  I sN, sH, sW, sC;          // input strides in elements (format-dependent)
  I rows;
  int H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW, OC, mult, nhwc;
  int tiles;  // NCHW: inner tiles per channel
};

template <class T, class I, int V, bool CROSS>
__global__ void __launch_bounds__(256) k_dwconv(const T* __restrict__ x0,
                                                const T* __restrict__ x1,
                                                const T* __restrict__ w0,
                                                const T* __restrict__ w1, T* __restrict__ out,
                                                DwconvP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  extern __shared__ __align__(16) unsigned char dwconv_lds[];
  T* __restrict__ wl = reinterpret_cast<T*>(dwconv_lds);
  const int taps = p.KH * p.KW;
  const int bx = (int)blockDim.x, by = (int)blockDim.y;
  const int cw = p.nhwc ? bx * V : 1;  // channels of this block
  int oc_base, ow_base = 0;
  if (p.nhwc) {
    oc_base = (int)blockIdx.x * cw;
  } else {
    oc_base = (int)(blockIdx.x / (unsigned)p.tiles);
    ow_base = (int)(blockIdx.x - (unsigned)oc_base * (unsigned)p.tiles) * bx * V;
  }
  {
    const int nch = min(cw, p.OC - oc_base);
    const I woff = (I)blockIdx.z * p.w_slot + (I)oc_base * (I)taps;
    const int nw = nch * taps;
    for (int i = (int)(threadIdx.y * bx + threadIdx.x); i < nw; i += bx * by) {
      const int cl = i / taps, tap = i - cl * taps;
      const T a = w0[woff + i];
      if (CROSS) {
        wl[tap * cw + cl] = a + w1[woff + i];
        wl[(taps + tap) * cw + cl] = a;
      } else {
        wl[tap * cw + cl] = a;
      }
    }
  }
  __syncthreads();
  const int l0 = (int)threadIdx.x * V;
  // V == 2 only with an even inner extent: both outputs are inside, or neither
  if ((p.nhwc ? oc_base + l0 >= p.OC : ow_base + l0 >= p.OW)) return;
  I coff[V];  // the input channel's offset
  int wcol[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int oc = p.nhwc ? oc_base + l0 + j : oc_base;
    coff[j] = (I)(oc / p.mult) * p.sC;
    wcol[j] = p.nhwc ? l0 + j : 0;
  }
  const T* __restrict__ xs0 = x0 + (I)blockIdx.z * p.x_slot;
  const T* __restrict__ xs1 = CROSS ? x1 + (I)blockIdx.z * p.x_slot : nullptr;
  T* __restrict__ dst = out + (I)blockIdx.z * p.o_slot;
  for (I row = (I)(blockIdx.y * by + threadIdx.y); row < p.rows; row += (I)(gridDim.y * by)) {
    U n;
    int oh, ow;
    I oidx;
    if (p.nhwc) {
      const U q = (U)row / (U)p.OW;
      ow = (int)((U)row - q * (U)p.OW);
      n = q / (U)p.OH;
      oh = (int)(q - n * (U)p.OH);
      oidx = row * (I)p.OC + (I)(oc_base + l0);
    } else {
      n = (U)row / (U)p.OH;
      oh = (int)((U)row - n * (U)p.OH);
      ow = ow_base + l0;
      oidx = (((I)n * (I)p.OC + (I)oc_base) * (I)p.OH + (I)oh) * (I)p.OW + (I)ow;
    }
    const I base = (I)n * p.sN;
    const int y0 = oh * p.sh - p.pt;
    LaneVec<T, V> acc;
#pragma unroll
    for (int j = 0; j < V; ++j) acc.v[j] = (T)0;
    for (int kh = 0; kh < p.KH; ++kh) {
      const int iy = y0 + kh * p.dh;
      if (iy < 0 || iy >= p.H) continue;
      const I rbase = base + (I)iy * p.sH;
      for (int kw = 0; kw < p.KW; ++kw) {
        const int tap = kh * p.KW + kw;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const int ix = (p.nhwc ? ow : ow + j) * p.sw - p.pl + kw * p.dw;
          if (ix < 0 || ix >= p.W) continue;
          const I xi = rbase + coff[j] + (I)ix * p.sW;
          acc.v[j] += xs0[xi] * wl[tap * cw + wcol[j]];
          if (CROSS) acc.v[j] += xs1[xi] * wl[(taps + tap) * cw + wcol[j]];
        }
      }
    }
    *reinterpret_cast<LaneVec<T, V>*>(dst + oidx) = acc;
  }
}

template <class T, class I, int V, bool CROSS>
static int dwconv_launch(const void* x0, const void* x1, const void* w0, const void* w1,
                         void* out, int64_t slots, int64_t x_slot_stride, int64_t w_slot_stride,
                         const ImgGeom& g, void* stream) {
  const bool nhwc = g.nhwc;
  // NCHW: the channel is part of blockIdx.x, the rows are (n, oh)
  const int64_t rows = nhwc ? g.rows : g.N * g.OH;
  // inner lanes of a block: few enough that the block's weights fit 64 KB of LDS (NHWC: bx * V
  // channels; NCHW: one channel)
  const int64_t per = g.KH * g.KW * (int64_t)sizeof(T) * (CROSS ? 2 : 1);
  int max_bx = 64;
  while (max_bx > 1 && nhwc && per * max_bx * V > 65536) max_bx /= 2;
  const LanePlan b = lane_plan(g.inner, V, max_bx);
  const int64_t lds = per * (nhwc ? b.bx * V : 1);
  if (lds > 65536) return -3;
  const int64_t gx = nhwc ? b.tiles : g.OC * b.tiles;
  if (gx > 0x7fffffff) return -3;
  // rows per lane: one visit while that leaves the grid small, up to 8 on a large one (the
  // staged weights serve them all)
  const int64_t gy_full = (rows + b.by - 1) / b.by;
  const int64_t visits = std::max<int64_t>(1, std::min<int64_t>(8, gx * slots * gy_full / 4096));
  const int64_t gy = std::min<int64_t>((gy_full + visits - 1) / visits, 65536 / b.by);
  DwconvP<I> p;
  p.x_slot = (I)x_slot_stride, p.w_slot = (I)w_slot_stride, p.o_slot = (I)g.n_out;
  set_strides(p, g);
  set_window(p, g);
  p.rows = (I)rows, p.OC = (int)g.OC, p.mult = (int)g.mult, p.tiles = (int)b.tiles;
  hipLaunchKernelGGL((k_dwconv<T, I, V, CROSS>), dim3((unsigned)gx, (unsigned)gy, (unsigned)slots),
                     dim3(b.bx, b.by), (size_t)lds, S(stream), (const T*)x0, (const T*)x1,
                     (const T*)w0, (const T*)w1, (T*)out, p);
  MX_LAUNCH_CHECK();
  return 0;
}

// col2im (moosex.h mx_col2im): the adjoint of k_im2col, as an output-stationary gather -- no
// atomics and no scatter, so the wrapping sums equal the CPU twin's bit for bit.  The output
// image is rows x inner: inner = the C channels (NHWC, rows (n, y, x)) or the W columns of one
// channel (NCHW, rows (n, c, y)); a lane owns V adjacent inner outputs of a row (V = 2 for u64
// with an even inner extent: every store is 16 bytes), adjacent lanes are adjacent in c (NHWC)
// or x (NCHW), and the lane strides over rows.  Per output the lane walks the KH*KW taps: a
// tap contributes when y + pt - kh*dh is a non-negative multiple of sh whose quotient oh is
// below OH (and its w twin).  NHWC: a wave reads contiguous channel runs of one patch-matrix
// row, 16 bytes per lane; NCHW lanes read K elements apart (correct, uncoalesced).  A block is
// blockDim.x inner lanes x 256 / blockDim.x rows.  Slots are blockIdx.z, read at in_slot and
// written densely.  I: the index type, 32-bit when every extent is below 2^31.
template <class I>
struct Col2imP {
  I in_slot, o_slot;  // slot strides in elements
  I K, rows;          // patch-matrix row length; output rows
  int C, H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW, nhwc;
};

template <class T, class I, int V>
__global__ void __launch_bounds__(256) k_col2im(const T* __restrict__ in, T* __restrict__ out,
                                                Col2imP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  const unsigned bx = blockDim.x, by = blockDim.y;
  const unsigned inner = (unsigned)(p.nhwc ? p.C : p.W);
  // V == 2 only with an even inner extent: both outputs are inside, or neither
  const unsigned i0 = (blockIdx.x * bx + threadIdx.x) * V;
  if (i0 >= inner) return;
  const T* __restrict__ src = in + (I)blockIdx.z * p.in_slot;
  T* __restrict__ dst = out + (I)blockIdx.z * p.o_slot;
  for (I row = (I)(blockIdx.y * by + threadIdx.y); row < p.rows; row += (I)(gridDim.y * by)) {
    U n;
    int y, x, c = 0;
    if (p.nhwc) {
      const U q = (U)row / (U)p.W;
      x = (int)((U)row - q * (U)p.W);
      n = q / (U)p.H;
      y = (int)(q - n * (U)p.H);
    } else {
      const U q = (U)row / (U)p.H;
      y = (int)((U)row - q * (U)p.H);
      n = q / (U)p.C;
      c = (int)(q - n * (U)p.C);
      x = (int)i0;
    }
    const I nbase = (I)n * (I)p.OH * (I)p.OW;
    LaneVec<T, V> acc;
#pragma unroll
    for (int j = 0; j < V; ++j) acc.v[j] = (T)0;
    for (int kh = 0; kh < p.KH; ++kh) {
      const int ty = y + p.pt - kh * p.dh;
      if (ty < 0) break;  // ty only falls with kh
      const unsigned oh = (unsigned)ty / (unsigned)p.sh;
      if (oh * (unsigned)p.sh != (unsigned)ty || oh >= (unsigned)p.OH) continue;
      const I rbase = nbase + (I)oh * (I)p.OW;
      if (p.nhwc) {
        for (int kw = 0; kw < p.KW; ++kw) {
          const int tx = x + p.pl - kw * p.dw;
          if (tx < 0) break;
          const unsigned ow = (unsigned)tx / (unsigned)p.sw;
          if (ow * (unsigned)p.sw != (unsigned)tx || ow >= (unsigned)p.OW) continue;
          const I si = (rbase + (I)ow) * p.K + (I)(kh * p.KW + kw) * (I)p.C + (I)i0;
          const LaneVec<T, V> r = *reinterpret_cast<const LaneVec<T, V>*>(src + si);
#pragma unroll
          for (int j = 0; j < V; ++j) acc.v[j] += r.v[j];
        }
      } else {
        const I cbase = ((I)c * (I)p.KH + (I)kh) * (I)p.KW;
        for (int kw = 0; kw < p.KW; ++kw) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const int tx = x + j + p.pl - kw * p.dw;
            if (tx < 0) continue;
            const unsigned ow = (unsigned)tx / (unsigned)p.sw;
            if (ow * (unsigned)p.sw != (unsigned)tx || ow >= (unsigned)p.OW) continue;
            acc.v[j] += src[(rbase + (I)ow) * p.K + cbase + (I)kw];
          }
        }
      }
    }
    *reinterpret_cast<LaneVec<T, V>*>(dst + row * (I)inner + (I)i0) = acc;
  }
}

template <class T, class I, int V>
static int col2im_launch(const void* in, void* out, int64_t slots, int64_t in_slot_stride,
                         const ImgGeom& g, void* stream) {
  const LanePlan b = lane_plan(g.inner, V);
  Col2imP<I> p;
  p.in_slot = (I)in_slot_stride, p.o_slot = (I)g.n_out;
  set_window(p, g);
  p.K = (I)g.K, p.rows = (I)g.rows, p.C = (int)g.C;
  hipLaunchKernelGGL((k_col2im<T, I, V>),
                     dim3((unsigned)b.tiles, (unsigned)row_grid(g.rows, b.by), (unsigned)slots),
                     dim3(b.bx, b.by), 0, S(stream), (const T*)in, (T*)out, p);
  MX_LAUNCH_CHECK();
  return 0;
}

// image resize (moosex.h mx_resize2d), on k_col2im's plan: output-stationary, no atomics, so
// the wrapping sums equal the CPU twin's bit for bit.  The output image is rows x inner: inner
// = the C channels (NHWC, rows (n, oy, ox)) or the OW columns of one channel (NCHW, rows (n, c,
// oy)); a lane owns V adjacent inner outputs of a row (V = 2 only for u64 in NHWC with an even
// C: both outputs share their taps, every load and store is 16 bytes), adjacent lanes are
// adjacent in c (NHWC: a wave reads contiguous channel runs of four input pixels) or in ox
// (NCHW: a wave reads two input rows at the columns its width taps name -- neighbouring when
// upsampling, strided when downsampling), and the lane strides over rows.  The tables th / tw
// are int32 [3, O] (i0, i1, w1): NHWC reads both once per row, the same entries for all lanes
// of the row; NCHW reads the width entries of its column once and the height entries per row.
// The four weights wh_a * ww_b < 2^24 are 32-bit; with both weight widths 0 the lane copies its
// one tap.  Indices are clamped to the image: a bad table reads a wrong pixel, never outside.
// Slots are blockIdx.z, read at in_slot and written densely.  I: the index type, 32-bit when
// every extent is below 2^31.
template <class I>
struct Resize2dP {
  I in_slot, o_slot;  // slot strides in elements
  I sN, sH, sW, sC;   // input strides in elements (format-dependent)
  I rows;             // output rows
  int C, H, W, OH, OW, wbh, wbw, nhwc;
};

template <class T, class I, int V>
__global__ void __launch_bounds__(256) k_resize2d(const T* __restrict__ in, T* __restrict__ out,
                                                  const int32_t* __restrict__ th,
                                                  const int32_t* __restrict__ tw,
                                                  Resize2dP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  using Vec = LaneVec<T, V>;
  const unsigned bx = blockDim.x, by = blockDim.y;
  const unsigned inner = (unsigned)(p.nhwc ? p.C : p.OW);
  // V == 2 only with an even inner extent: both outputs are inside, or neither
  const unsigned i0 = (blockIdx.x * bx + threadIdx.x) * V;
  if (i0 >= inner) return;
  const bool nearest = (p.wbh | p.wbw) == 0;
  const unsigned hmax = (unsigned)p.H - 1u, wmax = (unsigned)p.W - 1u;
  const T* __restrict__ src = in + (I)blockIdx.z * p.in_slot;
  T* __restrict__ dst = out + (I)blockIdx.z * p.o_slot;
  unsigned xa = 0, xb = 0, w1 = 0;
  if (!p.nhwc) {  // the lane's column, and so its width taps, are fixed
    xa = min((unsigned)tw[i0], wmax);
    xb = min((unsigned)tw[(unsigned)p.OW + i0], wmax);
    w1 = (unsigned)tw[2u * (unsigned)p.OW + i0];
  }
  for (I row = (I)(blockIdx.y * by + threadIdx.y); row < p.rows; row += (I)(gridDim.y * by)) {
    unsigned oy;
    I base;
    if (p.nhwc) {
      const U q = (U)row / (U)p.OW;
      const unsigned ox = (unsigned)((U)row - q * (U)p.OW);
      const U n = q / (U)p.OH;
      oy = (unsigned)(q - n * (U)p.OH);
      xa = min((unsigned)tw[ox], wmax);
      xb = min((unsigned)tw[(unsigned)p.OW + ox], wmax);
      w1 = (unsigned)tw[2u * (unsigned)p.OW + ox];
      base = (I)n * p.sN + (I)i0;
    } else {
      const U q = (U)row / (U)p.OH;
      oy = (unsigned)((U)row - q * (U)p.OH);
      const U n = q / (U)p.C;
      base = (I)n * p.sN + (I)(q - n * (U)p.C) * p.sC;
    }
    const unsigned ya = min((unsigned)th[oy], hmax);
    const I ra = base + (I)ya * p.sH;
    Vec acc = *reinterpret_cast<const Vec*>(src + ra + (I)xa * p.sW);
    if (!nearest) {
      const unsigned yb = min((unsigned)th[(unsigned)p.OH + oy], hmax);
      const unsigned h1 = (unsigned)th[2u * (unsigned)p.OH + oy];
      const unsigned h0 = (1u << p.wbh) - h1, w0 = (1u << p.wbw) - w1;
      const I rb = base + (I)yb * p.sH;
      const Vec r01 = *reinterpret_cast<const Vec*>(src + ra + (I)xb * p.sW);
      const Vec r10 = *reinterpret_cast<const Vec*>(src + rb + (I)xa * p.sW);
      const Vec r11 = *reinterpret_cast<const Vec*>(src + rb + (I)xb * p.sW);
      const uint32_t c00 = h0 * w0, c01 = h0 * w1, c10 = h1 * w0, c11 = h1 * w1;
#pragma unroll
      for (int j = 0; j < V; ++j)
        acc.v[j] = acc.v[j] * (T)c00 + r01.v[j] * (T)c01 + r10.v[j] * (T)c10 +
                   r11.v[j] * (T)c11;
    }
    *reinterpret_cast<Vec*>(dst + row * (I)inner + (I)i0) = acc;
  }
}

template <class T, class I, int V>
static int resize2d_launch(const void* in, void* out, int64_t slots, int64_t in_slot_stride,
                           const ImgGeom& g, const int32_t* th, const int32_t* tw,
                           void* stream) {
  const LanePlan b = lane_plan(g.inner, V);
  Resize2dP<I> p;
  p.in_slot = (I)in_slot_stride, p.o_slot = (I)g.n_out;
  set_strides(p, g);
  p.rows = (I)g.rows;
  p.C = (int)g.C, p.H = (int)g.H, p.W = (int)g.W, p.OH = (int)g.OH, p.OW = (int)g.OW;
  p.wbh = g.wbh, p.wbw = g.wbw, p.nhwc = g.nhwc;
  hipLaunchKernelGGL((k_resize2d<T, I, V>),
                     dim3((unsigned)b.tiles, (unsigned)row_grid(g.rows, b.by), (unsigned)slots),
                     dim3(b.bx, b.by), 0, S(stream), (const T*)in, (T*)out, th, tw, p);
  MX_LAUNCH_CHECK();
  return 0;
}

// piecewise-linear local step (moosex.h mx_pwl_cross), on k_col2im's plan with one row per
// slot: a lane owns V adjacent outputs (one u128, or two u64 when n is even and every buffer
// is 16-byte aligned, so every load and store is 16 bytes), adjacent lanes are adjacent in
// memory, the lane strides over the slot by the grid, and slots are blockIdx.z, read at their
// strides and written densely.  Per output: 2k + 2 reads (k + 1 in plain mode) and one write;
// the flag planes of a slot are n elements apart.  The public tables arrive in the kernel's
// arguments (scalar registers, no table in memory); the loop over the k planes is unrolled to
// MX_PWL_MAX with a uniform exit.  Wrapping sums in the CPU twin's order, so the results
// are equal bit for bit.  I: the index type, 32-bit when every extent is below 2^31.
template <class T, class I>
struct PwlP {
  T da[MX_PWL_MAX], db[MX_PWL_MAX], ak;
  I s_slot, x_slot, n;  // slot strides and slot length in elements
  int k, cross;
};

template <class T, class I, int V>
__global__ void __launch_bounds__(256) k_pwl_cross(const T* __restrict__ s0,
                                                   const T* __restrict__ s1,
                                                   const T* __restrict__ x0,
                                                   const T* __restrict__ x1, T* __restrict__ out,
                                                   PwlP<T, I> p) {
  using Vec = LaneVec<T, V>;
  const I sb = (I)blockIdx.z * p.s_slot, xb = (I)blockIdx.z * p.x_slot;
  T* __restrict__ dst = out + (I)blockIdx.z * p.n;
  const I step = (I)(gridDim.x * 256u) * V;
  // V == 2 only with an even n: both outputs are inside, or neither
  for (I i = (I)(blockIdx.x * 256u + threadIdx.x) * V; i < p.n; i += step) {
    const Vec a0 = *reinterpret_cast<const Vec*>(x0 + xb + i);
    Vec g0, g1, h, a;
#pragma unroll
    for (int v = 0; v < V; ++v) g0.v[v] = g1.v[v] = h.v[v] = (T)0, a.v[v] = a0.v[v];
    if (p.cross) {
      const Vec a1 = *reinterpret_cast<const Vec*>(x1 + xb + i);
#pragma unroll
      for (int v = 0; v < V; ++v) a.v[v] += a1.v[v];
    }
#pragma unroll
    for (int j = 0; j < MX_PWL_MAX; ++j) {
      if (j >= p.k) break;
      const I fi = sb + (I)j * p.n + i;
      const Vec f0 = *reinterpret_cast<const Vec*>(s0 + fi);
#pragma unroll
      for (int v = 0; v < V; ++v) g0.v[v] += p.da[j] * f0.v[v], h.v[v] += p.db[j] * f0.v[v];
      if (p.cross) {
        const Vec f1 = *reinterpret_cast<const Vec*>(s1 + fi);
#pragma unroll
        for (int v = 0; v < V; ++v) g1.v[v] += p.da[j] * f1.v[v];
      }
    }
    Vec o;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      o.v[v] = g0.v[v] * a.v[v] + p.ak * a0.v[v] + h.v[v];
      if (p.cross) o.v[v] += g1.v[v] * a0.v[v];
    }
    *reinterpret_cast<Vec*>(dst + i) = o;
  }
}

template <class T, class I, int V>
static int pwl_cross_launch(const void* s0, const void* s1, const void* x0, const void* x1,
                            void* out, int64_t slots, int64_t s_slot_stride,
                            int64_t x_slot_stride, int64_t n, int k, const uint64_t* da,
                            const uint64_t* db, const uint64_t* ak, void* stream) {
  PwlP<T, I> p;
  std::memset(&p, 0, sizeof(p));
  std::memcpy(p.da, da, sizeof(T) * k);
  std::memcpy(p.db, db, sizeof(T) * k);
  std::memcpy(&p.ak, ak, sizeof(T));
  p.s_slot = (I)s_slot_stride, p.x_slot = (I)x_slot_stride, p.n = (I)n;
  p.k = k, p.cross = x1 != nullptr;
  const int64_t lanes = (n + V - 1) / V;
  // the grid is capped at 256 CUs x 8 blocks per slot; a lane strides over the rest
  const int64_t gx = std::min<int64_t>((lanes + 255) / 256, 256 * 8);
  hipLaunchKernelGGL((k_pwl_cross<T, I, V>), dim3((unsigned)gx, 1, (unsigned)slots), dim3(256), 0,
                     S(stream), (const T*)s0, (const T*)s1, (const T*)x0, (const T*)x1, (T*)out,
                     p);
  MX_LAUNCH_CHECK();
  return 0;
}

// piecewise-polynomial local step (moosex.h mx_pwp_cross), on k_pwl_cross's plan: a lane owns V
// adjacent outputs (one u128, or two u64 when n is even and every buffer is 16-byte aligned),
// strides over the slot by the grid, slots are blockIdx.z.  Per output: 2k + 2D reads of 16
// bytes per lane (k + D in plain mode) and one write; each power is read through its own
// pointer pair at its own slot stride, where its multiplication wrote it.  The (D + 1) x k
// difference tables, the D last-piece coefficients and the power pointers arrive in the
// kernel's arguments and every index into them is a compile-time constant once the loops are
// unrolled, so they are scalar operands and nothing is a table in memory.  The loop over the
// planes is unrolled to MX_PWP_MAX with a uniform exit.  g0[0] is the constant's sum H.
// Wrapping sums, so the results equal the CPU twin's bit for bit.
template <class T, class I, int D>
struct PwpP {
  T dt[D + 1][MX_PWP_MAX], ck[D];
  const T* p0[D];
  const T* p1[D];
  I p_slot[D];  // slot strides of the powers in elements
  I s_slot, n;  // the flags' slot stride and the slot length
  int k, cross;
};

template <class T, class I, int V, int D>
__global__ void __launch_bounds__(256) k_pwp_cross(const T* __restrict__ s0,
                                                   const T* __restrict__ s1, T* __restrict__ out,
                                                   PwpP<T, I, D> p) {
  using Vec = LaneVec<T, V>;
  const I sb = (I)blockIdx.z * p.s_slot;
  T* __restrict__ dst = out + (I)blockIdx.z * p.n;
  const I step = (I)(gridDim.x * 256u) * V;
  // V == 2 only with an even n: both outputs are inside, or neither
  for (I i = (I)(blockIdx.x * 256u + threadIdx.x) * V; i < p.n; i += step) {
    Vec g0[D + 1], g1[D + 1];
#pragma unroll
    for (int q = 0; q <= D; ++q)
#pragma unroll
      for (int v = 0; v < V; ++v) g0[q].v[v] = g1[q].v[v] = (T)0;
#pragma unroll
    for (int j = 0; j < MX_PWP_MAX; ++j) {
      if (j >= p.k) break;
      const I fi = sb + (I)j * p.n + i;
      const Vec f0 = *reinterpret_cast<const Vec*>(s0 + fi);
#pragma unroll
      for (int q = 0; q <= D; ++q)
#pragma unroll
        for (int v = 0; v < V; ++v) g0[q].v[v] += p.dt[q][j] * f0.v[v];
      if (p.cross) {
        const Vec f1 = *reinterpret_cast<const Vec*>(s1 + fi);
#pragma unroll
        for (int q = 1; q <= D; ++q)
#pragma unroll
          for (int v = 0; v < V; ++v) g1[q].v[v] += p.dt[q][j] * f1.v[v];
      }
    }
    Vec o = g0[0];
#pragma unroll
    for (int q = 1; q <= D; ++q) {
      const I pi = (I)blockIdx.z * p.p_slot[q - 1] + i;
      const Vec a0 = *reinterpret_cast<const Vec*>(p.p0[q - 1] + pi);
      Vec a = a0;
      if (p.cross) {
        const Vec a1 = *reinterpret_cast<const Vec*>(p.p1[q - 1] + pi);
#pragma unroll
        for (int v = 0; v < V; ++v) a.v[v] += a1.v[v];
      }
#pragma unroll
      for (int v = 0; v < V; ++v) {
        o.v[v] += g0[q].v[v] * a.v[v] + p.ck[q - 1] * a0.v[v];
        if (p.cross) o.v[v] += g1[q].v[v] * a0.v[v];
      }
    }
    *reinterpret_cast<Vec*>(dst + i) = o;
  }
}

template <class T, class I, int V, int D>
static int pwp_cross_launch(const void* s0, const void* s1, const void* const* p0,
                            const void* const* p1, void* out, int64_t slots,
                            int64_t s_slot_stride, const int64_t* p_slot_stride, int64_t n, int k,
                            const uint64_t* dt, const uint64_t* ck, void* stream) {
  PwpP<T, I, D> p;
  std::memset(&p, 0, sizeof(p));
  for (int q = 0; q <= D; ++q) std::memcpy(p.dt[q], (const T*)dt + (int64_t)q * k, sizeof(T) * k);
  std::memcpy(p.ck, ck, sizeof(T) * D);
  for (int q = 0; q < D; ++q) {
    p.p0[q] = (const T*)p0[q];
    p.p1[q] = p1 ? (const T*)p1[q] : nullptr;
    p.p_slot[q] = (I)p_slot_stride[q];
  }
  p.s_slot = (I)s_slot_stride, p.n = (I)n;
  p.k = k, p.cross = p1 != nullptr;
  const int64_t lanes = (n + V - 1) / V;
  // the grid is capped at 256 CUs x 8 blocks per slot; a lane strides over the rest
  const int64_t gx = std::min<int64_t>((lanes + 255) / 256, 256 * 8);
  hipLaunchKernelGGL((k_pwp_cross<T, I, V, D>), dim3((unsigned)gx, 1, (unsigned)slots), dim3(256),
                     0, S(stream), (const T*)s0, (const T*)s1, (T*)out, p);
  MX_LAUNCH_CHECK();
  return 0;
}

// The compare-exchange leaves (moosex.h mx_cswap_diff / _cross / _apply).  A stage (k, j)
// pairs position i with i | j, so in memory it is a butterfly over blocks of 2r contiguous
// elements, r = j * inner: run index e of a block's low half meets run index e of its high
// half, and the pair-major arrays (differences, flags, products) are dense at b*r + e.  A lane
// owns a pair and loads both of its elements; adjacent lanes are adjacent in both runs and in
// the pair-major array, a lane strides over the slot by the grid, slots are blockIdx.z, read at
// their strides and written densely.  Forms F: 0 one pair per lane (any u128: every access is
// 16 bytes as it is); 1 two adjacent pairs of a run per lane (u64, r even, 16-byte aligned
// operands: every access is 16 bytes); 2 r = 1 (j = 1, inner = 1), where the two elements of
// a pair are adjacent: one 16-byte load takes both (u64).  The table-mode difference reads
// the key column only: run index q is element q*unit + off with unit = inner, off = by and
// r = j.  The stage travels in the kernel's arguments: nothing is uploaded.  Ring arithmetic
// wraps, so the results equal the CPU twins' bit for bit.  Every output element has one
// writer.  I: the index type, 32-bit when every extent is below 2^31.
template <class I>
struct CswapP {
  I x_slot, a_slot;  // slot strides of x and of the other operand (flags / products)
  I total;           // pairs (times columns) of a slot
  I r, unit, off;    // run length; element of run index q: q*unit + off
  I sdiv;            // cross: the flag of product g is g / sdiv (inner in table mode, else 1)
  I amask, k;        // block b is ascending iff (((b & amask) << lj1) & k) == 0, ...
  I n_x;             // apply: elements of an output slot
  int rs;            // log2 r where r is a power of two, else -1
  int lj1, desc, cross;
};

template <class T_, class I_, int F_>
struct CswapForm {
  using T = T_;
  using I = I_;
  static constexpr int F = F_;
};

// block b and the low element of pair g
template <class I>
__device__ __forceinline__ I cswap_low_of(const CswapP<I>& p, I g, I& b) {
  using U = typename std::make_unsigned<I>::type;
  b = p.rs >= 0 ? (I)((U)g >> p.rs) : (I)((U)g / (U)p.r);
  return (b * p.r + g) * p.unit + p.off;  // (b*2r + e) with e = g - b*r
}

template <class T, class I, int F>
__global__ void __launch_bounds__(256) k_cswap_diff(const T* __restrict__ x, T* __restrict__ out,
                                                    CswapP<I> p) {
  constexpr int V = F == 1 ? 2 : 1;
  using Vec = LaneVec<T, 2>;
  const T* __restrict__ src = x + (I)blockIdx.z * p.x_slot;
  T* __restrict__ dst = out + (I)blockIdx.z * p.total;
  const I step = (I)(gridDim.x * 256u) * V;
  for (I g = (I)(blockIdx.x * 256u + threadIdx.x) * V; g < p.total; g += step) {
    I b;
    const I lo = cswap_low_of(p, g, b);
    const bool asc = ((((b & p.amask) << p.lj1) & p.k) == 0) != (p.desc != 0);
    if constexpr (F == 0) {
      const T a = src[lo], c = src[lo + p.r * p.unit];
      dst[g] = asc ? c - a : a - c;
    } else if constexpr (F == 1) {  // r even: both pairs are in block b
      const Vec a = *reinterpret_cast<const Vec*>(src + lo);
      const Vec c = *reinterpret_cast<const Vec*>(src + lo + p.r);
      Vec o;
#pragma unroll
      for (int v = 0; v < 2; ++v) o.v[v] = asc ? c.v[v] - a.v[v] : a.v[v] - c.v[v];
      *reinterpret_cast<Vec*>(dst + g) = o;
    } else {  // r == 1: the pair is one vector
      const Vec a = *reinterpret_cast<const Vec*>(src + lo);
      dst[g] = asc ? a.v[1] - a.v[0] : a.v[0] - a.v[1];
    }
  }
}

template <class T, class I, int F>
__global__ void __launch_bounds__(256) k_cswap_cross(const T* __restrict__ s0,
                                                     const T* __restrict__ s1,
                                                     const T* __restrict__ x0,
                                                     const T* __restrict__ x1,
                                                     T* __restrict__ out, CswapP<I> p) {
  constexpr int V = F == 1 ? 2 : 1;
  using Vec = LaneVec<T, 2>;
  using U = typename std::make_unsigned<I>::type;
  const I xb = (I)blockIdx.z * p.x_slot, sb = (I)blockIdx.z * p.a_slot;
  T* __restrict__ dst = out + (I)blockIdx.z * p.total;
  const I step = (I)(gridDim.x * 256u) * V;
  for (I g = (I)(blockIdx.x * 256u + threadIdx.x) * V; g < p.total; g += step) {
    I b;
    const I lo = xb + cswap_low_of(p, g, b);
    T d0[V], d[V], f0[V], f1[V];
    if constexpr (F == 0) {
      d0[0] = x0[lo] - x0[lo + p.r];
      if (p.cross) d[0] = d0[0] + (x1[lo] - x1[lo + p.r]);
    } else if constexpr (F == 1) {
      const Vec a = *reinterpret_cast<const Vec*>(x0 + lo);
      const Vec c = *reinterpret_cast<const Vec*>(x0 + lo + p.r);
#pragma unroll
      for (int v = 0; v < 2; ++v) d0[v] = a.v[v] - c.v[v];
      if (p.cross) {
        const Vec a1 = *reinterpret_cast<const Vec*>(x1 + lo);
        const Vec c1 = *reinterpret_cast<const Vec*>(x1 + lo + p.r);
#pragma unroll
        for (int v = 0; v < 2; ++v) d[v] = d0[v] + (a1.v[v] - c1.v[v]);
      }
    } else {
      const Vec a = *reinterpret_cast<const Vec*>(x0 + lo);
      d0[0] = a.v[0] - a.v[1];
      if (p.cross) {
        const Vec a1 = *reinterpret_cast<const Vec*>(x1 + lo);
        d[0] = d0[0] + (a1.v[0] - a1.v[1]);
      }
    }
    bool flag_vec = false;
    if constexpr (F == 1) {
      flag_vec = p.sdiv == 1;
      if (flag_vec) {  // a flag per product: the two are one vector
        const Vec f = *reinterpret_cast<const Vec*>(s0 + sb + g);
        f0[0] = f.v[0], f0[1] = f.v[1];
        if (p.cross) {
          const Vec h = *reinterpret_cast<const Vec*>(s1 + sb + g);
          f1[0] = h.v[0], f1[1] = h.v[1];
        }
      }
    }
    if (!flag_vec) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const I fi = sb + (p.sdiv == 1 ? g + v : (I)((U)(g + v) / (U)p.sdiv));
        f0[v] = s0[fi];
        if (p.cross) f1[v] = s1[fi];
      }
    }
    T o[V];
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = p.cross ? f0[v] * d[v] + f1[v] * d0[v] : f0[v] * d0[v];
    if constexpr (F == 1) {
      Vec w;
      w.v[0] = o[0], w.v[1] = o[1];
      *reinterpret_cast<Vec*>(dst + g) = w;
    } else {
      dst[g] = o[0];
    }
  }
}

template <class T, class I, int F>
__global__ void __launch_bounds__(256) k_cswap_apply(const T* __restrict__ x,
                                                     const T* __restrict__ pr,
                                                     T* __restrict__ out, CswapP<I> p) {
  constexpr int V = F == 1 ? 2 : 1;
  using Vec = LaneVec<T, 2>;
  const T* __restrict__ src = x + (I)blockIdx.z * p.x_slot;
  const T* __restrict__ q = pr + (I)blockIdx.z * p.a_slot;
  T* __restrict__ dst = out + (I)blockIdx.z * p.n_x;
  const I step = (I)(gridDim.x * 256u) * V;
  for (I g = (I)(blockIdx.x * 256u + threadIdx.x) * V; g < p.total; g += step) {
    I b;
    const I lo = cswap_low_of(p, g, b);
    if constexpr (F == 0) {
      const T d = q[g];
      dst[lo] = src[lo] - d;
      dst[lo + p.r] = src[lo + p.r] + d;
    } else if constexpr (F == 1) {
      const Vec d = *reinterpret_cast<const Vec*>(q + g);
      Vec a = *reinterpret_cast<const Vec*>(src + lo);
      Vec c = *reinterpret_cast<const Vec*>(src + lo + p.r);
#pragma unroll
      for (int v = 0; v < 2; ++v) a.v[v] -= d.v[v], c.v[v] += d.v[v];
      *reinterpret_cast<Vec*>(dst + lo) = a;
      *reinterpret_cast<Vec*>(dst + lo + p.r) = c;
    } else {
      const T d = q[g];
      Vec a = *reinterpret_cast<const Vec*>(src + lo);
      a.v[0] -= d, a.v[1] += d;
      *reinterpret_cast<Vec*>(dst + lo) = a;
    }
  }
}

// the parameters of a stage: `key_only` walks the key column's pairs (the table-mode difference)
template <class I>
static CswapP<I> cswap_params(const mxr::CswapGeom& g, bool key_only, int64_t x_slot,
                              int64_t a_slot, bool cross) {
  CswapP<I> p;
  std::memset(&p, 0, sizeof(p));
  const int64_t r = key_only ? g.j : g.j * g.inner;
  p.x_slot = (I)x_slot, p.a_slot = (I)a_slot;
  p.total = (I)(key_only ? g.outer * g.half : g.n_pair);
  p.r = (I)r, p.unit = (I)(key_only ? g.inner : 1), p.off = (I)(key_only ? g.by : 0);
  p.sdiv = (I)(g.by >= 0 ? g.inner : 1);
  p.amask = (I)(g.n / (2 * g.j) - 1), p.k = (I)g.k, p.n_x = (I)g.n_x;
  p.rs = -1;
  if ((r & (r - 1)) == 0)
    for (p.rs = 0; ((int64_t)1 << p.rs) < r;) ++p.rs;
  p.lj1 = g.lj + 1, p.desc = g.descending, p.cross = cross;
  return p;
}

// launch(CswapForm<T, I, F>{}): u64 takes form 2 when r == 1 and form 1 when r is even, where
// `wide` (unit stride, every operand and slot stride on 16 bytes) allows; u128 form 0
template <class L>
static int cswap_dispatch(int elem_bytes, bool small, bool wide, int64_t r, L launch) {
#define MX_CSWAP_FORM(T, F)                                 \
  return small ? launch(CswapForm<T, int32_t, F>{}) : launch(CswapForm<T, int64_t, F>{})
  switch (elem_bytes) {
    case 8:
      if (wide && r == 1) {
        MX_CSWAP_FORM(u64, 2);
      }
      if (wide && r % 2 == 0) {
        MX_CSWAP_FORM(u64, 1);
      }
      MX_CSWAP_FORM(u64, 0);
    case 16: MX_CSWAP_FORM(u128, 0);
    default: return -2;
  }
#undef MX_CSWAP_FORM
}

// the grid is capped at 256 CUs x 8 blocks per slot; a lane strides over the rest
static dim3 cswap_grid(int64_t total, int F, int64_t slots) {
  const int64_t lanes = F == 1 ? total / 2 : total;
  return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((lanes + 255) / 256, 256 * 8)), 1,
              (unsigned)slots);
}

// permuted row gather (moosex.h mx_perm_gather), on k_resize2d's plan: the output is rows x
// inner with rows = outer * n; a lane owns V adjacent inner outputs of a row (V = 2 only for
// u64 with an even inner extent and aligned buffers: every load and store is 16 bytes; u128
// moves 16 bytes per lane as is), adjacent lanes are adjacent in the row -- a gathered row is
// read as one contiguous run, the masks and the output are read and written in order -- and
// the lane strides over rows.  perm[r] is read once per row, the same entry for all lanes of
// the row, and clamped to [0, n): a bad perm gathers a wrong row, never outside.  The optional
// operands are uniform null tests.  Slots are blockIdx.z, read at their strides and written
// densely.  I: the index type, 32-bit when every extent is below 2^31.
template <class I>
struct PermGatherP {
  I a_slot, b_slot, p_slot, m_slot, o_slot;  // slot strides in elements
  I rows, n, inner;
};

template <class T, class I, int V>
__global__ void __launch_bounds__(256) k_perm_gather(const T* __restrict__ a,
                                                     const T* __restrict__ b,
                                                     const T* __restrict__ pl,
                                                     const T* __restrict__ mi,
                                                     const int64_t* __restrict__ perm,
                                                     T* __restrict__ out, PermGatherP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  using Vec = LaneVec<T, V>;
  const unsigned by = blockDim.y;
  // V == 2 only with an even inner extent: both outputs are inside, or neither
  const I c0 = ((I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x) * V;
  if (c0 >= p.inner) return;
  const I z = (I)blockIdx.z;
  const T* __restrict__ sa = a + z * p.a_slot;
  const T* __restrict__ sb = b ? b + z * p.b_slot : nullptr;
  const T* __restrict__ sp = pl ? pl + z * p.p_slot : nullptr;
  const T* __restrict__ sm = mi ? mi + z * p.m_slot : nullptr;
  T* __restrict__ dst = out + z * p.o_slot;
  const uint64_t last = (uint64_t)p.n - 1u;
  for (I row = (I)(blockIdx.y * by + threadIdx.y); row < p.rows; row += (I)(gridDim.y * by)) {
    const U o = (U)row / (U)p.n;
    const I r = row - (I)o * p.n;
    const uint64_t want = (uint64_t)perm[r];  // a negative entry wraps above `last`
    const I src = (I)(want < last ? want : last);
    const I si = ((I)o * p.n + src) * p.inner + c0, di = row * p.inner + c0;
    Vec v = *reinterpret_cast<const Vec*>(sa + si);
    if (sb) {
      const Vec w = *reinterpret_cast<const Vec*>(sb + si);
#pragma unroll
      for (int j = 0; j < V; ++j) v.v[j] += w.v[j];
    }
    if (sp) {
      const Vec w = *reinterpret_cast<const Vec*>(sp + di);
#pragma unroll
      for (int j = 0; j < V; ++j) v.v[j] += w.v[j];
    }
    if (sm) {
      const Vec w = *reinterpret_cast<const Vec*>(sm + di);
#pragma unroll
      for (int j = 0; j < V; ++j) v.v[j] -= w.v[j];
    }
    *reinterpret_cast<Vec*>(dst + di) = v;
  }
}

template <class T, class I, int V>
static int perm_gather_launch(const void* a, const void* b, const void* pl, const void* mi,
                              const int64_t* perm, void* out, int64_t slots, int64_t a_slot,
                              int64_t b_slot, int64_t p_slot, int64_t m_slot, int64_t outer,
                              int64_t n, int64_t inner, void* stream) {
  const LanePlan lp = lane_plan(inner, V);
  const int64_t rows = outer * n;
  PermGatherP<I> p;
  p.a_slot = (I)a_slot, p.b_slot = (I)b_slot, p.p_slot = (I)p_slot, p.m_slot = (I)m_slot;
  p.o_slot = (I)(rows * inner), p.rows = (I)rows, p.n = (I)n, p.inner = (I)inner;
  hipLaunchKernelGGL((k_perm_gather<T, I, V>),
                     dim3((unsigned)lp.tiles, (unsigned)row_grid(rows, lp.by), (unsigned)slots),
                     dim3(lp.bx, lp.by), 0, S(stream), (const T*)a, (const T*)b, (const T*)pl,
                     (const T*)mi, perm, (T*)out, p);
  MX_LAUNCH_CHECK();
  return 0;
}

// The prefix-sum leaves (moosex.h mx_scan, mx_segscan_cross / _apply), on k_perm_gather's plan:
// a rows x inner index space, a lane owns V adjacent inner elements of a row (V = 2 only for
// u64 with an even inner extent and aligned buffers: every access is 16 bytes; u128 moves 16
// bytes per lane as is, its carry between the limbs is the compiler's 128-bit add), adjacent
// lanes are adjacent in memory, a lane strides over rows, slots are blockIdx.z, read at their
// strides and written densely.  I: the index type, 32-bit when every extent is below 2^31.
//
// k_scan: a row is (o, chunk k) -- positions [k * kScanChunk, ...) of line o -- and the lane
// walks them with the running sum in registers.  SUMS: the chunk's sum goes to sums[o, k, c].
// Else the scan proper: the sum starts at off[o, k, c] (null: 0; the exclusive scan of the
// chunk sums, in the same direction) and every position is written once.  The three phases
// are three launches on one stream: no workgroup waits for another.
template <class I>
struct ScanP {
  I x_slot, o_slot, s_slot;  // slot strides of x, out and the sums / offsets
  I rows, chunks, n, inner;  // rows = outer * chunks
  int excl, rev;
};

template <class T, class I, int V, bool SUMS>
__global__ void __launch_bounds__(256) k_scan(const T* __restrict__ x, const T* __restrict__ off,
                                              T* __restrict__ out, ScanP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  using Vec = LaneVec<T, V>;
  const unsigned by = blockDim.y;
  const I c0 = ((I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x) * V;
  if (c0 >= p.inner) return;
  const I z = (I)blockIdx.z;
  const T* __restrict__ src = x + z * p.x_slot;
  const T* __restrict__ so = off ? off + z * p.s_slot : nullptr;
  T* __restrict__ dst = out + z * (SUMS ? p.s_slot : p.o_slot);
  constexpr I chunk = (I)mxr::kScanChunk;
  for (I row = (I)(blockIdx.y * by + threadIdx.y); row < p.rows; row += (I)(gridDim.y * by)) {
    const I o = (I)((U)row / (U)p.chunks), k = row - o * p.chunks;
    const I p0 = k * chunk, len = p.n - p0 < chunk ? p.n - p0 : chunk;
    const I base = (o * p.n + p0) * p.inner + c0;
    Vec acc;
#pragma unroll
    for (int e = 0; e < V; ++e) acc.v[e] = 0;
    if constexpr (SUMS) {
#pragma unroll 4
      for (I t = 0; t < len; ++t) {
        const Vec v = *reinterpret_cast<const Vec*>(src + base + t * p.inner);
#pragma unroll
        for (int e = 0; e < V; ++e) acc.v[e] += v.v[e];
      }
      *reinterpret_cast<Vec*>(dst + row * p.inner + c0) = acc;
    } else {
      if (so) acc = *reinterpret_cast<const Vec*>(so + row * p.inner + c0);
      const I step = p.rev ? -p.inner : p.inner;
      const I first = p.rev ? base + (len - 1) * p.inner : base;
#pragma unroll 4
      for (I t = 0; t < len; ++t) {
        const I i = first + t * step;
        const Vec v = *reinterpret_cast<const Vec*>(src + i);
        Vec w = acc;
#pragma unroll
        for (int e = 0; e < V; ++e) acc.v[e] += v.v[e];
        if (!p.excl) w = acc;
        *reinterpret_cast<Vec*>(dst + i) = w;
      }
    }
  }
}

// a block of bx x by lanes for a rows x inner space: lane_plan's, its rows halved down to one
// wavefront while the grid would stay below 512 blocks (a long axis of few lines has few rows)
static dim3 scan_block(const LanePlan& lp, int64_t rows, int64_t slots, int* by_out) {
  int by = lp.by;
  while (by > 1 && lp.bx * by > 64 && lp.tiles * ((rows + by - 1) / by) * slots < 512) by /= 2;
  *by_out = by;
  return dim3(lp.bx, by);
}

template <class T, class I, int V, bool SUMS>
static int scan_launch(const void* x, const void* off, void* out, int64_t slots, int64_t x_slot,
                       int64_t outer, int64_t n, int64_t inner, int excl, int rev,
                       void* stream) {
  const LanePlan lp = lane_plan(inner, V);
  const int64_t chunks = (n + mxr::kScanChunk - 1) / mxr::kScanChunk, rows = outer * chunks;
  ScanP<I> p;
  p.x_slot = (I)x_slot, p.o_slot = (I)(outer * n * inner), p.s_slot = (I)(rows * inner);
  p.rows = (I)rows, p.chunks = (I)chunks, p.n = (I)n, p.inner = (I)inner;
  p.excl = excl, p.rev = rev;
  int by;
  const dim3 block = scan_block(lp, rows, slots, &by);
  hipLaunchKernelGGL((k_scan<T, I, V, SUMS>),
                     dim3((unsigned)lp.tiles, (unsigned)row_grid(rows, by), (unsigned)slots),
                     block, 0, S(stream), (const T*)x, (const T*)off, (T*)out, p);
  MX_LAUNCH_CHECK();
  return 0;
}

// One level of the scan: an axis of one chunk in one launch; a longer one through its chunk
// sums, which are scanned (exclusive, same direction) by this function again.  ws: this
// level's sums and offsets, slots * outer * chunks * inner elements each, then the levels below.
static int scan_level(int elem_bytes, const void* x, int64_t x_slot, void* out, char* ws,
                      int64_t slots, int64_t outer, int64_t n, int64_t inner, int excl, int rev,
                      void* stream) {
  const int64_t chunks = (n + mxr::kScanChunk - 1) / mxr::kScanChunk;
  const int64_t n_x = outer * n * inner, n_sum = outer * chunks * inner;
  char* sums = ws;
  char* offs = ws + slots * n_sum * elem_bytes;
  const bool small = fits32(1 << 17, {(slots - 1) * x_slot + n_x, slots * n_x});
  const bool two = inner % 2 == 0 && aligned16(x) && aligned16(out) && aligned16(ws) &&
                   x_slot % 2 == 0;
  auto phase = [&](bool sums_only, const void* off, void* dst) {
    return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
      using F = decltype(f);
      using T = typename F::T;
      using I = typename F::I;
      return sums_only ? scan_launch<T, I, F::V, true>(x, nullptr, dst, slots, x_slot, outer, n,
                                                       inner, excl, rev, stream)
                       : scan_launch<T, I, F::V, false>(x, off, dst, slots, x_slot, outer, n,
                                                        inner, excl, rev, stream);
    });
  };
  if (chunks <= 1) return phase(false, nullptr, out);
  int rc = phase(true, nullptr, sums);
  if (rc) return rc;
  rc = scan_level(elem_bytes, sums, n_sum, offs, offs + slots * n_sum * elem_bytes, slots, outer,
                  chunks, inner, 1, rev, stream);
  if (rc) return rc;
  return phase(false, offs, out);
}

// k_segscan_cross: a row is (o, pos - j) of the products; the flag of the row -- column
// inner - 1 at pos -- is one load, the same for all lanes of the row.
template <class I>
struct SegscanP {
  I a_slot, b_slot, o_slot;  // slot strides: state (cross: both components), products, output
  I rows, n, nj, j, inner;   // nj = n - j
};

template <class T, class I, int V>
__global__ void __launch_bounds__(256) k_segscan_cross(const T* __restrict__ a,
                                                       const T* __restrict__ b,
                                                       T* __restrict__ out, SegscanP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  using Vec = LaneVec<T, V>;
  const unsigned by = blockDim.y;
  const I c0 = ((I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x) * V;
  if (c0 >= p.inner) return;
  const I z = (I)blockIdx.z;
  const T* __restrict__ sa = a + z * p.a_slot;
  const T* __restrict__ sb = b ? b + z * p.a_slot : nullptr;
  T* __restrict__ dst = out + z * p.o_slot;
  for (I row = (I)(blockIdx.y * by + threadIdx.y); row < p.rows; row += (I)(gridDim.y * by)) {
    const I o = (I)((U)row / (U)p.nj), t = row - o * p.nj;
    const I ti = (o * p.n + t) * p.inner + c0;
    const I fi = (o * p.n + t + p.j) * p.inner + p.inner - 1;
    const T ga = sa[fi];
    const Vec ta = *reinterpret_cast<const Vec*>(sa + ti);
    Vec v;
    if (sb) {
      const T gb = sb[fi];
      const Vec tb = *reinterpret_cast<const Vec*>(sb + ti);
#pragma unroll
      for (int e = 0; e < V; ++e) v.v[e] = ga * (ta.v[e] + tb.v[e]) + gb * ta.v[e];
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) v.v[e] = ga * ta.v[e];
    }
    *reinterpret_cast<Vec*>(dst + row * p.inner + c0) = v;
  }
}

// k_segscan_apply: a row is (o, pos) of the state; below j it is copied, from j on the values
// take the product of pos - j and the flag column is replaced by it.
template <class T, class I, int V>
__global__ void __launch_bounds__(256) k_segscan_apply(const T* __restrict__ x,
                                                       const T* __restrict__ pr,
                                                       T* __restrict__ out, SegscanP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  using Vec = LaneVec<T, V>;
  const unsigned by = blockDim.y;
  const I c0 = ((I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x) * V;
  if (c0 >= p.inner) return;
  const I z = (I)blockIdx.z;
  const T* __restrict__ src = x + z * p.a_slot;
  const T* __restrict__ q = pr + z * p.b_slot;
  T* __restrict__ dst = out + z * p.o_slot;
  for (I row = (I)(blockIdx.y * by + threadIdx.y); row < p.rows; row += (I)(gridDim.y * by)) {
    const I o = (I)((U)row / (U)p.n), pos = row - o * p.n;
    const I si = row * p.inner + c0;
    Vec v = *reinterpret_cast<const Vec*>(src + si);
    if (pos >= p.j) {
      const Vec w = *reinterpret_cast<const Vec*>(q + (o * p.nj + pos - p.j) * p.inner + c0);
#pragma unroll
      for (int e = 0; e < V; ++e) v.v[e] = c0 + e == p.inner - 1 ? w.v[e] : v.v[e] + w.v[e];
    }
    *reinterpret_cast<Vec*>(dst + si) = v;
  }
}

template <class I>
static SegscanP<I> segscan_params(const mxr::SegscanGeom& g, int64_t a_slot, int64_t b_slot,
                                  int64_t o_slot, int64_t rows) {
  SegscanP<I> p;
  p.a_slot = (I)a_slot, p.b_slot = (I)b_slot, p.o_slot = (I)o_slot, p.rows = (I)rows;
  p.n = (I)g.n, p.nj = (I)(g.n - g.j), p.j = (I)g.j, p.inner = (I)g.inner;
  return p;
}

// k_outer_cross (moosex.h mx_outer_cross), on the segscan leaves' plan: a (groups * rows) x
// n_out index space, a lane owns V adjacent output columns and strides over the lines.  The
// lane's columns are fixed, so its b = c / A and a = c % A are formed once, outside the loop,
// for any A (a block's columns span several b where A is small).  V = 2 only where A is even:
// then both columns lie in one run of A and take one H element.  Per line a lane loads one
// vector of L and one element of H (per component); the lanes of a run read the same H
// address.  L and H are read at their own slot and group strides, the output is dense.
template <class I>
struct OuterP {
  I l_slot, l_group, h_slot, h_group, o_slot;
  I lines, rows, A, B, n_out;  // lines = groups * rows
};

template <class T, class I, int V>
__global__ void __launch_bounds__(256) k_outer_cross(const T* __restrict__ la,
                                                     const T* __restrict__ lb,
                                                     const T* __restrict__ ha,
                                                     const T* __restrict__ hb,
                                                     T* __restrict__ out, OuterP<I> p) {
  using U = typename std::make_unsigned<I>::type;
  using Vec = LaneVec<T, V>;
  const unsigned by = blockDim.y;
  const I c0 = ((I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x) * V;
  if (c0 >= p.n_out) return;
  const I b = (I)((U)c0 / (U)p.A), a0 = c0 - b * p.A;
  const I z = (I)blockIdx.z;
  const T* __restrict__ sla = la + z * p.l_slot + a0;
  const T* __restrict__ sha = ha + z * p.h_slot + b;
  const T* __restrict__ slb = lb ? lb + z * p.l_slot + a0 : nullptr;
  const T* __restrict__ shb = lb ? hb + z * p.h_slot + b : nullptr;
  T* __restrict__ dst = out + z * p.o_slot + c0;
  for (I q = (I)(blockIdx.y * by + threadIdx.y); q < p.lines; q += (I)(gridDim.y * by)) {
    const I gi = (I)((U)q / (U)p.rows), r = q - gi * p.rows;
    const I li = gi * p.l_group + r * p.A, hi = gi * p.h_group + r * p.B;
    const Vec xa = *reinterpret_cast<const Vec*>(sla + li);
    const T ya = sha[hi];
    Vec v;
    if (slb) {
      const Vec xb = *reinterpret_cast<const Vec*>(slb + li);
      const T ys = ya + shb[hi];
#pragma unroll
      for (int e = 0; e < V; ++e) v.v[e] = xa.v[e] * ys + xb.v[e] * ya;
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) v.v[e] = xa.v[e] * ya;
    }
    *reinterpret_cast<Vec*>(dst + q * p.n_out) = v;
  }
}

}  // namespace

extern "C" {

int mxh_outer_cross(int elem_bytes, const void* la, const void* lb, const void* ha,
                    const void* hb, void* out, int64_t slots, int64_t l_slot_stride,
                    int64_t l_group_stride, int64_t h_slot_stride, int64_t h_group_stride,
                    const mxr::OuterGeom& g, void* stream) {
  if (slots > 65535) return -3;
  // outer_geom_check kept every term within slot_cap, so neither sum wraps
  const int64_t l_reach = (slots - 1) * l_slot_stride + (g.groups - 1) * l_group_stride + g.n_l;
  const int64_t h_reach = (slots - 1) * h_slot_stride + (g.groups - 1) * h_group_stride + g.n_h;
  const bool small = fits32(1 << 17, {l_reach, h_reach, slots * g.n_o});
  // the vector accesses are L's and the output's; H is read one element at a time
  const bool two = g.A % 2 == 0 && g.n_out % 2 == 0 && aligned16(la) && aligned16(lb) &&
                   aligned16(out) && l_slot_stride % 2 == 0 && l_group_stride % 2 == 0;
  const int64_t lines = g.groups * g.rows;
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    using T = typename F::T;
    using I = typename F::I;
    const LanePlan lp = lane_plan(g.n_out, F::V);
    OuterP<I> p;
    p.l_slot = (I)l_slot_stride, p.l_group = (I)l_group_stride, p.h_slot = (I)h_slot_stride;
    p.h_group = (I)h_group_stride, p.o_slot = (I)g.n_o, p.lines = (I)lines, p.rows = (I)g.rows;
    p.A = (I)g.A, p.B = (I)g.B, p.n_out = (I)g.n_out;
    hipLaunchKernelGGL((k_outer_cross<T, I, F::V>),
                       dim3((unsigned)lp.tiles, (unsigned)row_grid(lines, lp.by), (unsigned)slots),
                       dim3(lp.bx, lp.by), 0, S(stream), (const T*)la, (const T*)lb,
                       (const T*)ha, (const T*)hb, (T*)out, p);
    MX_LAUNCH_CHECK();
    return 0;
  });
}

int mxh_scan(int elem_bytes, const void* x, void* out, void* ws, int64_t slots,
             int64_t x_slot_stride, const mxr::ScanGeom& g, void* stream) {
  if (slots > 65535) return -3;
  return scan_level(elem_bytes, x, x_slot_stride, out, (char*)ws, slots, g.outer, g.n, g.inner,
                    g.exclusive, g.reverse, stream);
}

int mxh_segscan_cross(int elem_bytes, const void* a, const void* b, void* out, int64_t slots,
                      int64_t slot_stride, const mxr::SegscanGeom& g, void* stream) {
  if (slots > 65535) return -3;
  const bool small = fits32(1 << 17, {(slots - 1) * slot_stride + g.n_x, slots * g.n_p});
  const bool two = g.inner % 2 == 0 && aligned16(a) && aligned16(b) && aligned16(out) &&
                   slot_stride % 2 == 0;
  const int64_t rows = g.outer * (g.n - g.j);
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    using T = typename F::T;
    const LanePlan lp = lane_plan(g.inner, F::V);
    const auto p = segscan_params<typename F::I>(g, slot_stride, 0, g.n_p, rows);
    hipLaunchKernelGGL((k_segscan_cross<T, typename F::I, F::V>),
                       dim3((unsigned)lp.tiles, (unsigned)row_grid(rows, lp.by), (unsigned)slots),
                       dim3(lp.bx, lp.by), 0, S(stream), (const T*)a, (const T*)b, (T*)out, p);
    MX_LAUNCH_CHECK();
    return 0;
  });
}

int mxh_segscan_apply(int elem_bytes, const void* x, const void* pr, void* out, int64_t slots,
                      int64_t x_slot_stride, int64_t p_slot_stride, const mxr::SegscanGeom& g,
                      void* stream) {
  if (slots > 65535) return -3;
  const bool small = fits32(1 << 17, {(slots - 1) * x_slot_stride + g.n_x,
                                      (slots - 1) * p_slot_stride + g.n_p, slots * g.n_x});
  const bool two = g.inner % 2 == 0 && aligned16(x) && aligned16(pr) && aligned16(out) &&
                   x_slot_stride % 2 == 0 && p_slot_stride % 2 == 0;
  const int64_t rows = g.outer * g.n;
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    using T = typename F::T;
    const LanePlan lp = lane_plan(g.inner, F::V);
    const auto p = segscan_params<typename F::I>(g, x_slot_stride, p_slot_stride, g.n_x, rows);
    hipLaunchKernelGGL((k_segscan_apply<T, typename F::I, F::V>),
                       dim3((unsigned)lp.tiles, (unsigned)row_grid(rows, lp.by), (unsigned)slots),
                       dim3(lp.bx, lp.by), 0, S(stream), (const T*)x, (const T*)pr, (T*)out, p);
    MX_LAUNCH_CHECK();
    return 0;
  });
}

int mxh_perm_gather(int elem_bytes, const void* a, const void* b, const void* p, const void* m,
                    const int64_t* perm, void* out, int64_t slots, int64_t a_slot_stride,
                    int64_t b_slot_stride, int64_t p_slot_stride, int64_t m_slot_stride,
                    int64_t outer, int64_t n, int64_t inner, void* stream) {
  if (slots <= 0 || outer <= 0 || n <= 0 || inner <= 0) return 0;
  if (slots > 65535 || !a || !perm || !out || a_slot_stride < 0 || b_slot_stride < 0 ||
      p_slot_stride < 0 || m_slot_stride < 0)
    return -3;
  // mx_perm_gather bounded n_x, the strides and their products with `slots` below 2^62
  const int64_t n_x = outer * n * inner;
  const bool small = fits32(1 << 17, {(slots - 1) * a_slot_stride + n_x,
                                      b ? (slots - 1) * b_slot_stride + n_x : 0,
                                      p ? (slots - 1) * p_slot_stride + n_x : 0,
                                      m ? (slots - 1) * m_slot_stride + n_x : 0, slots * n_x});
  // two outputs per lane: every row, slot and buffer has to start on 16 bytes
  const bool two = inner % 2 == 0 && aligned16(a) && aligned16(b) && aligned16(p) &&
                   aligned16(m) && aligned16(out) && a_slot_stride % 2 == 0 &&
                   b_slot_stride % 2 == 0 && p_slot_stride % 2 == 0 && m_slot_stride % 2 == 0;
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    return perm_gather_launch<typename F::T, typename F::I, F::V>(
        a, b, p, m, perm, out, slots, a_slot_stride, b_slot_stride, p_slot_stride, m_slot_stride,
        outer, n, inner, stream);
  });
}

// The image leaves: g comes validated from mx_* (img_geom_check); what is left here is what
// only a launch is bound by -- slots are blockIdx.z -- and each leaf's choice of form.
int mxh_im2col(int elem_bytes, const void* in, void* out, int64_t slots, int64_t in_slot_stride,
               const ImgGeom& g, void* stream) {
  if (slots > 65535 || (g.K + 63) / 64 > 0x7fffffff) return -3;
  const int64_t in_extent = (slots - 1) * in_slot_stride + g.n_in;
  const bool small = fits32(1 << 17, {in_extent, slots * g.n_out});
  const bool two = g.K % 2 == 0 && aligned16(out);
  return leaf_dispatch<true>(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    return im2col_launch<typename F::T, typename F::I, F::V>(in, out, slots, in_slot_stride, g,
                                                             stream);
  });
}

int mxh_col2im(int elem_bytes, const void* in, void* out, int64_t slots, int64_t in_slot_stride,
               const ImgGeom& g, void* stream) {
  if (slots > 65535) return -3;
  const int64_t in_extent = (slots - 1) * in_slot_stride + g.N * g.OH * g.OW * g.K;
  const bool small = fits32(1 << 23, {in_extent, slots * g.n_out});
  // 16-byte stores need an even inner extent; NHWC's 16-byte loads an aligned input too
  const bool two = g.inner % 2 == 0 && aligned16(out) &&
                   (!g.nhwc || (aligned16(in) && in_slot_stride % 2 == 0));
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    return col2im_launch<typename F::T, typename F::I, F::V>(in, out, slots, in_slot_stride, g,
                                                             stream);
  });
}

int mxh_resize2d(int elem_bytes, const void* in, void* out, int64_t slots,
                 int64_t in_slot_stride, const ImgGeom& g, const int32_t* th,
                 const int32_t* tw, void* stream) {
  if (slots > 65535) return -3;
  const int64_t in_extent = (slots - 1) * in_slot_stride + g.n_in;
  const bool small = fits32(1 << 23, {in_extent, slots * g.n_out});
  // two outputs per lane share their taps only in NHWC; 16-byte accesses need an even C and
  // aligned buffers
  const bool two = g.nhwc && g.C % 2 == 0 && aligned16(out) && aligned16(in) &&
                   in_slot_stride % 2 == 0;
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    return resize2d_launch<typename F::T, typename F::I, F::V>(in, out, slots, in_slot_stride,
                                                               g, th, tw, stream);
  });
}

int mxh_pwl_cross(int elem_bytes, const void* s0, const void* s1, const void* x0, const void* x1,
                  void* out, int64_t slots, int64_t s_slot_stride, int64_t x_slot_stride,
                  int64_t n, int k, const uint64_t* da, const uint64_t* db, const uint64_t* ak,
                  void* stream) {
  if (slots <= 0 || n <= 0) return 0;
  if (k < 0 || k > MX_PWL_MAX || slots > 65535 || s_slot_stride < 0 || x_slot_stride < 0 || !ak ||
      (k && (!da || !db)) || (s1 == nullptr) != (x1 == nullptr))
    return -3;
  const int64_t s_extent = (slots - 1) * s_slot_stride + (int64_t)k * n;
  const int64_t x_extent = (slots - 1) * x_slot_stride + n;
  const bool small = fits32(1 << 23, {s_extent, x_extent, slots * n});
  // two outputs per lane: every plane, slot and buffer has to start on 16 bytes
  const bool two = n % 2 == 0 && aligned16(s0) && aligned16(s1) && aligned16(x0) &&
                   aligned16(x1) && aligned16(out) && s_slot_stride % 2 == 0 &&
                   x_slot_stride % 2 == 0;
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    return pwl_cross_launch<typename F::T, typename F::I, F::V>(
        s0, s1, x0, x1, out, slots, s_slot_stride, x_slot_stride, n, k, da, db, ak, stream);
  });
}

int mxh_pwp_cross(int elem_bytes, const void* s0, const void* s1, const void* const* p0,
                  const void* const* p1, void* out, int64_t slots, int64_t s_slot_stride,
                  const int64_t* p_slot_stride, int64_t n, int k, int d, const uint64_t* dt,
                  const uint64_t* ck, void* stream) {
  if (slots <= 0 || n <= 0) return 0;
  if (k < 1 || k > MX_PWP_MAX || d < 1 || d > MX_PWP_DEG || slots > 65535 || s_slot_stride < 0 ||
      !s0 || !out || !p0 || !p_slot_stride || !dt || !ck || (s1 == nullptr) != (p1 == nullptr))
    return -3;
  bool small = fits32(1 << 23, {(slots - 1) * s_slot_stride + (int64_t)k * n, slots * n});
  // two outputs per lane: every plane, slot and buffer has to start on 16 bytes
  bool two = n % 2 == 0 && aligned16(s0) && aligned16(s1) && aligned16(out) &&
             s_slot_stride % 2 == 0;
  for (int q = 0; q < d; ++q) {
    if (p_slot_stride[q] < 0 || !p0[q] || (p1 && !p1[q])) return -3;
    small = small && fits32(1 << 23, {(slots - 1) * p_slot_stride[q] + n});
    two = two && aligned16(p0[q]) && (!p1 || aligned16(p1[q])) && p_slot_stride[q] % 2 == 0;
  }
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    using T = typename F::T;
    using I = typename F::I;
#define MX_PWP(D)                                                                              \
  case D:                                                                                      \
    return pwp_cross_launch<T, I, F::V, D>(s0, s1, p0, p1, out, slots, s_slot_stride,          \
                                           p_slot_stride, n, k, dt, ck, stream)
    switch (d) {
      MX_PWP(1);
      MX_PWP(2);
      MX_PWP(3);
      default: return -3;
    }
#undef MX_PWP
  });
}

int mxh_cswap_diff(int elem_bytes, const void* x, void* out, int64_t slots, int64_t x_slot_stride,
                   const mxr::CswapGeom& g, void* stream) {
  if (slots > 65535) return -3;
  const bool key_only = g.by >= 0;
  const int64_t r = key_only ? g.j : g.j * g.inner;
  const bool small = fits32(1 << 23, {(slots - 1) * x_slot_stride + g.n_x, slots * g.n_flag});
  const bool wide = (!key_only || g.inner == 1) && aligned16(x) && aligned16(out) &&
                    x_slot_stride % 2 == 0;
  return cswap_dispatch(elem_bytes, small, wide, r, [&](auto f) {
    using F = decltype(f);
    using T = typename F::T;
    const auto p = cswap_params<typename F::I>(g, key_only, x_slot_stride, 0, false);
    hipLaunchKernelGGL((k_cswap_diff<T, typename F::I, F::F>), cswap_grid(g.n_flag, F::F, slots),
                       dim3(256), 0, S(stream), (const T*)x, (T*)out, p);
    MX_LAUNCH_CHECK();
    return 0;
  });
}

int mxh_cswap_cross(int elem_bytes, const void* s0, const void* s1, const void* x0,
                    const void* x1, void* out, int64_t slots, int64_t s_slot_stride,
                    int64_t x_slot_stride, const mxr::CswapGeom& g, void* stream) {
  if (slots > 65535 || (s1 == nullptr) != (x1 == nullptr)) return -3;
  const bool small = fits32(1 << 23, {(slots - 1) * x_slot_stride + g.n_x,
                                      (slots - 1) * s_slot_stride + g.n_flag, slots * g.n_pair});
  const bool wide = aligned16(s0) && aligned16(s1) && aligned16(x0) && aligned16(x1) &&
                    aligned16(out) && s_slot_stride % 2 == 0 && x_slot_stride % 2 == 0;
  return cswap_dispatch(elem_bytes, small, wide, g.j * g.inner, [&](auto f) {
    using F = decltype(f);
    using T = typename F::T;
    const auto p =
        cswap_params<typename F::I>(g, false, x_slot_stride, s_slot_stride, x1 != nullptr);
    hipLaunchKernelGGL((k_cswap_cross<T, typename F::I, F::F>),
                       cswap_grid(g.n_pair, F::F, slots), dim3(256), 0, S(stream), (const T*)s0,
                       (const T*)s1, (const T*)x0, (const T*)x1, (T*)out, p);
    MX_LAUNCH_CHECK();
    return 0;
  });
}

int mxh_cswap_apply(int elem_bytes, const void* x, const void* pr, void* out, int64_t slots,
                    int64_t x_slot_stride, int64_t p_slot_stride, const mxr::CswapGeom& g,
                    void* stream) {
  if (slots > 65535) return -3;
  const bool small = fits32(1 << 23, {(slots - 1) * x_slot_stride + g.n_x,
                                      (slots - 1) * p_slot_stride + g.n_pair, slots * g.n_x});
  const bool wide = aligned16(x) && aligned16(pr) && aligned16(out) && x_slot_stride % 2 == 0 &&
                    p_slot_stride % 2 == 0;
  return cswap_dispatch(elem_bytes, small, wide, g.j * g.inner, [&](auto f) {
    using F = decltype(f);
    using T = typename F::T;
    const auto p = cswap_params<typename F::I>(g, false, x_slot_stride, p_slot_stride, false);
    hipLaunchKernelGGL((k_cswap_apply<T, typename F::I, F::F>),
                       cswap_grid(g.n_pair, F::F, slots), dim3(256), 0, S(stream), (const T*)x,
                       (const T*)pr, (T*)out, p);
    MX_LAUNCH_CHECK();
    return 0;
  });
}

int mxh_dwconv(int elem_bytes, const void* x0, const void* x1, const void* w0, const void* w1,
               void* out, int64_t slots, int64_t x_slot_stride, int64_t w_slot_stride,
               const ImgGeom& g, void* stream) {
  if (slots > 65535) return -3;
  const int64_t x_extent = (slots - 1) * x_slot_stride + g.n_in;
  const int64_t w_extent = (slots - 1) * w_slot_stride + g.OC * g.KH * g.KW;
  const bool small = fits32(1 << 23, {x_extent, w_extent, slots * g.n_out});
  const bool two = g.inner % 2 == 0 && aligned16(out);
  const bool cross = x1 != nullptr;
  return leaf_dispatch(elem_bytes, small, two, [&](auto f) {
    using F = decltype(f);
    using T = typename F::T;
    using I = typename F::I;
    return cross ? dwconv_launch<T, I, F::V, true>(x0, x1, w0, w1, out, slots, x_slot_stride,
                                                   w_slot_stride, g, stream)
                 : dwconv_launch<T, I, F::V, false>(x0, x1, w0, w1, out, slots, x_slot_stride,
                                                    w_slot_stride, g, stream);
  });
}

}  // extern "C"
