// Host (CPU) twins of the leaf kernels of leaf_hip.hip -- the image leaves, the piecewise-
// linear local step, the compare-exchange leaves, the permuted row gather, the prefix-sum
// leaves and the outer-product leaf -- and their mx_* entry points, which check the geometry
// (img_geom.h, cswap_geom.h, segscan_geom.h, outer_geom.h) and the sizes for both sides.  Plain
// loops: the oracle.
#include <algorithm>
#include <cstring>
#include <vector>

#include "moosex.h"
#include "ring_common.h"
#include "ring_host.h"

namespace {

using mxr::ImgGeom;

// The image leaves take the record img_geom_check (img_geom.h) filled; their loops read its
// attributes, strides and counts under the names of moosex.h.
template <class T>
void im2col_cpu(const T* in, T* out, int64_t slots, int64_t in_slot_stride, const ImgGeom& geom) {
  const int64_t C = geom.C, H = geom.H, W = geom.W, KH = geom.KH, KW = geom.KW, sh = geom.sh, sw = geom.sw;
  const int64_t pt = geom.pt, pl = geom.pl, dh = geom.dh, dw = geom.dw, OH = geom.OH, OW = geom.OW;
  const int64_t K = geom.K, rows = geom.rows, sN = geom.sN, sH = geom.sH, sW = geom.sW, sC = geom.sC;
  const bool nhwc = geom.nhwc;
  parallel_for(slots * rows, std::max<int64_t>(1, 4096 / K), [=](int64_t b, int64_t e) {
    for (int64_t g = b; g < e; ++g) {
      const int64_t s = g / rows, row = g - s * rows;
      const int64_t ow = row % OW, oh = (row / OW) % OH, n = row / (OW * OH);
      const T* src = in + s * in_slot_stride + n * sN;
      T* dst = out + g * K;
      for (int64_t c = 0; c < C; ++c)
        for (int64_t kh = 0; kh < KH; ++kh)
          for (int64_t kw = 0; kw < KW; ++kw) {
            const int64_t iy = oh * sh + kh * dh - pt, ix = ow * sw + kw * dw - pl;
            const int64_t col = nhwc ? (kh * KW + kw) * C + c : (c * KH + kh) * KW + kw;
            const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
            dst[col] = inside ? src[c * sC + iy * sH + ix * sW] : (T)0;
          }
    }
  });
}

// col2im (moosex.h mx_col2im): every image pixel gathers the patch-matrix entries whose tap
// lands on it; parallel over the image rows (s, n, y)
template <class T>
void col2im_cpu(const T* in, T* out, int64_t slots, int64_t in_slot_stride, const ImgGeom& geom) {
  const int64_t N = geom.N, C = geom.C, H = geom.H, W = geom.W, KH = geom.KH, KW = geom.KW, sh = geom.sh, sw = geom.sw;
  const int64_t pt = geom.pt, pl = geom.pl, dh = geom.dh, dw = geom.dw, OH = geom.OH, OW = geom.OW;
  const int64_t K = geom.K, sN = geom.sN, sH = geom.sH, sW = geom.sW, sC = geom.sC;
  const bool nhwc = geom.nhwc;
  parallel_for(slots * N * H, std::max<int64_t>(1, 4096 / (W * K)), [=](int64_t b, int64_t e) {
    for (int64_t g = b; g < e; ++g) {
      const int64_t y = g % H, n = (g / H) % N, s = g / (H * N);
      const T* src = in + s * in_slot_stride + n * OH * OW * K;
      T* dst = out + (s * N + n) * sN + y * sH;
      for (int64_t x = 0; x < W; ++x)
        for (int64_t c = 0; c < C; ++c) {
          T acc = 0;
          for (int64_t kh = 0; kh < KH; ++kh) {
            const int64_t ty = y + pt - kh * dh;
            if (ty < 0 || ty % sh || ty / sh >= OH) continue;
            for (int64_t kw = 0; kw < KW; ++kw) {
              const int64_t tx = x + pl - kw * dw;
              if (tx < 0 || tx % sw || tx / sw >= OW) continue;
              const int64_t col = nhwc ? (kh * KW + kw) * C + c : (c * KH + kh) * KW + kw;
              acc += src[(ty / sh * OW + tx / sw) * K + col];
            }
          }
          dst[x * sW + c * sC] = acc;
        }
    }
  });
}

// image resize (moosex.h mx_resize2d): every output pixel is the integer-weighted sum of its
// four taps (one tap without a multiply when both weight widths are 0); parallel over the
// output rows (s, n, oy)
template <class T>
void resize2d_cpu(const T* in, T* out, int64_t slots, int64_t in_slot_stride, const ImgGeom& geom,
                  const int32_t* th, const int32_t* tw) {
  const int64_t N = geom.N, C = geom.C, H = geom.H, W = geom.W, OH = geom.OH, OW = geom.OW;
  const int64_t sH = geom.sH, sW = geom.sW, sC = geom.sC;
  const int wbh = geom.wbh, wbw = geom.wbw;
  const bool nhwc = geom.nhwc;
  const int64_t oH = nhwc ? OW * C : OW, oW = nhwc ? C : 1, oC = nhwc ? 1 : OH * OW;
  const bool nearest = wbh == 0 && wbw == 0;
  parallel_for(slots * N * OH, std::max<int64_t>(1, 4096 / (OW * C)), [=](int64_t b, int64_t e) {
    for (int64_t g = b; g < e; ++g) {
      const int64_t oy = g % OH, n = (g / OH) % N, s = g / (OH * N);
      const T* src = in + s * in_slot_stride + n * C * H * W;
      T* dst = out + (s * N + n) * C * OH * OW + oy * oH;
      const int64_t y0 = th[oy], y1 = th[OH + oy];
      const uint32_t h1 = (uint32_t)th[2 * OH + oy], h0 = (1u << wbh) - h1;
      for (int64_t ox = 0; ox < OW; ++ox) {
        const int64_t x0 = tw[ox], x1 = tw[OW + ox];
        const uint32_t w1 = (uint32_t)tw[2 * OW + ox], w0 = (1u << wbw) - w1;
        for (int64_t c = 0; c < C; ++c) {
          const T* p = src + c * sC;
          T acc;
          if (nearest)
            acc = p[y0 * sH + x0 * sW];
          else
            acc = p[y0 * sH + x0 * sW] * (T)(h0 * w0) + p[y0 * sH + x1 * sW] * (T)(h0 * w1) +
                  p[y1 * sH + x0 * sW] * (T)(h1 * w0) + p[y1 * sH + x1 * sW] * (T)(h1 * w1);
          dst[ox * oW + c * oC] = acc;
        }
      }
    }
  });
}

// depthwise convolution (moosex.h mx_dwconv): the arithmetic of k_dwconv in plain loops; the
// cross mode's w0 + w1 is formed once per weight element
template <class T>
void dwconv_cpu(const T* x0, const T* x1, const T* w0, const T* w1, T* out, int64_t slots,
                int64_t x_slot_stride, int64_t w_slot_stride, const ImgGeom& geom) {
  const int64_t H = geom.H, W = geom.W, mult = geom.mult, KH = geom.KH, KW = geom.KW, sh = geom.sh, sw = geom.sw;
  const int64_t pt = geom.pt, pl = geom.pl, dh = geom.dh, dw = geom.dw, OH = geom.OH, OW = geom.OW;
  const int64_t OC = geom.OC, taps = KH * KW, rows = geom.N * OH * OW;
  const int64_t sN = geom.sN, sH = geom.sH, sW = geom.sW, sC = geom.sC;
  const bool nhwc = geom.nhwc;
  const bool cross = x1 != nullptr;
  std::vector<T> wsum;
  if (cross) {
    const int64_t wslots = w_slot_stride ? slots : 1;
    wsum.resize((size_t)(wslots * OC * taps));
    for (int64_t s = 0; s < wslots; ++s)
      for (int64_t i = 0; i < OC * taps; ++i)
        wsum[s * OC * taps + i] = w0[s * w_slot_stride + i] + w1[s * w_slot_stride + i];
  }
  const T* ws = wsum.data();
  parallel_for(slots * rows, std::max<int64_t>(1, 4096 / (OC * taps)), [=](int64_t b, int64_t e) {
    for (int64_t g = b; g < e; ++g) {
      const int64_t s = g / rows, row = g - s * rows;
      const int64_t ow = row % OW, oh = (row / OW) % OH, n = row / (OW * OH);
      const int64_t xb = s * x_slot_stride + n * sN;
      const T* wa = w0 + s * w_slot_stride;
      const T* wb = cross ? ws + (w_slot_stride ? s * OC * taps : 0) : nullptr;
      for (int64_t oc = 0; oc < OC; ++oc) {
        const int64_t c = oc / mult;
        T acc = 0;
        for (int64_t kh = 0; kh < KH; ++kh) {
          const int64_t iy = oh * sh + kh * dh - pt;
          if (iy < 0 || iy >= H) continue;
          for (int64_t kw = 0; kw < KW; ++kw) {
            const int64_t ix = ow * sw + kw * dw - pl;
            if (ix < 0 || ix >= W) continue;
            const int64_t xi = xb + c * sC + iy * sH + ix * sW, wi = (oc * KH + kh) * KW + kw;
            if (cross)
              acc += x0[xi] * wb[wi] + x1[xi] * wa[wi];
            else
              acc += x0[xi] * wa[wi];
          }
        }
        const int64_t oi = nhwc ? row * OC + oc : ((n * OC + oc) * OH + oh) * OW + ow;
        out[s * rows * OC + oi] = acc;
      }
    }
  });
}

// piecewise-linear local step (moosex.h mx_pwl_cross): the arithmetic of k_pwl_cross in plain
// loops, one output element at a time
template <class T>
void pwl_cross_cpu(const T* s0, const T* s1, const T* x0, const T* x1, T* out, int64_t slots,
                   int64_t s_slot_stride, int64_t x_slot_stride, int64_t n, int k,
                   const uint64_t* da, const uint64_t* db, const uint64_t* ak) {
  T DA[MX_PWL_MAX], DB[MX_PWL_MAX], AK;
  std::memcpy(DA, da, sizeof(T) * k);
  std::memcpy(DB, db, sizeof(T) * k);
  std::memcpy(&AK, ak, sizeof(T));
  const bool cross = x1 != nullptr;
  parallel_for(slots * n, 1 << 12, [&](int64_t b, int64_t e) {
    for (int64_t g = b; g < e; ++g) {
      const int64_t s = g / n, i = g - s * n;
      const T* f0 = s0 + s * s_slot_stride + i;
      const T* f1 = cross ? s1 + s * s_slot_stride + i : nullptr;
      const T a0 = x0[s * x_slot_stride + i];
      T g0 = 0, g1 = 0, h = 0;
      for (int j = 0; j < k; ++j) {
        g0 += DA[j] * f0[j * n];
        h += DB[j] * f0[j * n];
        if (cross) g1 += DA[j] * f1[j * n];
      }
      T v = g0 * (cross ? a0 + x1[s * x_slot_stride + i] : a0) + AK * a0 + h;
      if (cross) v += g1 * a0;
      out[g] = v;
    }
  });
}

// piecewise-polynomial local step (moosex.h mx_pwp_cross): the arithmetic of k_pwp_cross in
// plain loops, one output element at a time.  G[0] is the constant's sum H.
template <class T>
void pwp_cross_cpu(const T* s0, const T* s1, const void* const* p0, const void* const* p1, T* out,
                   int64_t slots, int64_t s_slot_stride, const int64_t* p_slot_stride, int64_t n,
                   int k, int d, const uint64_t* dt, const uint64_t* ck) {
  T D[MX_PWP_DEG + 1][MX_PWP_MAX], CK[MX_PWP_DEG + 1];
  for (int i = 0; i <= d; ++i) std::memcpy(D[i], (const T*)dt + (int64_t)i * k, sizeof(T) * k);
  std::memcpy(CK + 1, ck, sizeof(T) * d);
  const bool cross = p1 != nullptr;
  parallel_for(slots * n, 1 << 12, [&](int64_t b, int64_t e) {
    for (int64_t g = b; g < e; ++g) {
      const int64_t s = g / n, i = g - s * n;
      const T* f0 = s0 + s * s_slot_stride + i;
      const T* f1 = cross ? s1 + s * s_slot_stride + i : nullptr;
      T g0[MX_PWP_DEG + 1] = {0, 0, 0, 0}, g1[MX_PWP_DEG + 1] = {0, 0, 0, 0};
      for (int j = 0; j < k; ++j) {
        for (int q = 0; q <= d; ++q) g0[q] += D[q][j] * f0[j * n];
        if (cross)
          for (int q = 1; q <= d; ++q) g1[q] += D[q][j] * f1[j * n];
      }
      T v = 0;
      for (int q = 1; q <= d; ++q) {
        const int64_t pi = s * p_slot_stride[q - 1] + i;
        const T a0 = ((const T*)p0[q - 1])[pi];
        v += g0[q] * (cross ? a0 + ((const T*)p1[q - 1])[pi] : a0) + CK[q] * a0;
        if (cross) v += g1[q] * a0;
      }
      out[g] = v + g0[0];
    }
  });
}

using mxr::CswapGeom;

// The compare-exchange leaves (moosex.h mx_cswap_*): one (slot, row, pair) at a time, the
// pairing as cswap_geom.h words it.  f(s, o, t, i, l): i, l the two positions of pair t.
template <class F>
void cswap_pairs(int64_t slots, const CswapGeom& g, F f) {
  const int64_t per = g.outer * g.half;
  parallel_for(slots * per, std::max<int64_t>(1, 4096 / g.inner), [&](int64_t b, int64_t e) {
    for (int64_t q = b; q < e; ++q) {
      const int64_t s = q / per, r = q - s * per, o = r / g.half, t = r - o * g.half;
      const int64_t i = mxr::cswap_low(t, g.lj);
      f(s, o, t, i, i | g.j);
    }
  });
}

template <class T>
void cswap_diff_cpu(const T* x, T* out, int64_t slots, int64_t x_slot_stride,
                    const CswapGeom& g) {
  const int64_t c0 = g.by >= 0 ? g.by : 0;
  cswap_pairs(slots, g, [&](int64_t s, int64_t o, int64_t t, int64_t i, int64_t l) {
    const T* xi = x + s * x_slot_stride + (o * g.n + i) * g.inner + c0;
    const T* xl = x + s * x_slot_stride + (o * g.n + l) * g.inner + c0;
    T* dst = out + s * g.n_flag + (o * g.half + t) * g.cols;
    const bool asc = mxr::cswap_ascending(g, i);
    for (int64_t c = 0; c < g.cols; ++c) dst[c] = asc ? xl[c] - xi[c] : xi[c] - xl[c];
  });
}

template <class T>
void cswap_cross_cpu(const T* s0, const T* s1, const T* x0, const T* x1, T* out, int64_t slots,
                     int64_t s_slot_stride, int64_t x_slot_stride, const CswapGeom& g) {
  const bool cross = x1 != nullptr;
  cswap_pairs(slots, g, [&](int64_t s, int64_t o, int64_t t, int64_t i, int64_t l) {
    const int64_t xi = s * x_slot_stride + (o * g.n + i) * g.inner;
    const int64_t xl = s * x_slot_stride + (o * g.n + l) * g.inner;
    const int64_t f = s * s_slot_stride + (o * g.half + t) * g.cols;
    T* dst = out + s * g.n_pair + (o * g.half + t) * g.inner;
    for (int64_t c = 0; c < g.inner; ++c) {
      const int64_t fc = f + (g.by >= 0 ? 0 : c);
      const T d0 = x0[xi + c] - x0[xl + c];
      T v = s0[fc] * (cross ? d0 + (x1[xi + c] - x1[xl + c]) : d0);
      if (cross) v += s1[fc] * d0;
      dst[c] = v;
    }
  });
}

template <class T>
void cswap_apply_cpu(const T* x, const T* p, T* out, int64_t slots, int64_t x_slot_stride,
                     int64_t p_slot_stride, const CswapGeom& g) {
  cswap_pairs(slots, g, [&](int64_t s, int64_t o, int64_t t, int64_t i, int64_t l) {
    const int64_t ri = (o * g.n + i) * g.inner, rl = (o * g.n + l) * g.inner;
    const T* src = x + s * x_slot_stride;
    const T* pp = p + s * p_slot_stride + (o * g.half + t) * g.inner;
    T* dst = out + s * g.n_x;
    for (int64_t c = 0; c < g.inner; ++c) {
      dst[ri + c] = src[ri + c] - pp[c];
      dst[rl + c] = src[rl + c] + pp[c];
    }
  });
}

// The permuted row gather (moosex.h mx_perm_gather): one (slot, row) at a time.
template <class T>
void perm_gather_cpu(const T* a, const T* b, const T* p, const T* m, const int64_t* perm, T* out,
                     int64_t slots, int64_t a_slot, int64_t b_slot, int64_t p_slot,
                     int64_t m_slot, int64_t outer, int64_t n, int64_t inner) {
  const int64_t rows = outer * n;
  parallel_for(slots * rows, std::max<int64_t>(1, 4096 / inner), [=](int64_t q0, int64_t q1) {
    for (int64_t q = q0; q < q1; ++q) {
      const int64_t s = q / rows, row = q - s * rows, o = row / n, r = row - o * n;
      const int64_t si = (o * n + perm[r]) * inner, di = row * inner;
      T* dst = out + q * inner;
      for (int64_t c = 0; c < inner; ++c) {
        T v = a[s * a_slot + si + c];
        if (b) v += b[s * b_slot + si + c];
        if (p) v += p[s * p_slot + di + c];
        if (m) v -= m[s * m_slot + di + c];
        dst[c] = v;
      }
    }
  });
}

using mxr::ScanGeom;
using mxr::SegscanGeom;

// The prefix sum (moosex.h mx_scan): one (slot, row, column) line at a time, front to back or
// back to front.  The plain walk is the oracle of the kernel's three phases: sums in the ring
// are the same in any grouping.
template <class T>
void scan_cpu(const T* x, T* out, int64_t slots, int64_t x_slot_stride, const ScanGeom& g) {
  const int64_t lines = g.outer * g.inner;
  parallel_for(slots * lines, std::max<int64_t>(1, 4096 / g.n), [&](int64_t b, int64_t e) {
    for (int64_t q = b; q < e; ++q) {
      const int64_t s = q / lines, r = q - s * lines, o = r / g.inner, c = r - o * g.inner;
      const T* src = x + s * x_slot_stride + o * g.n * g.inner + c;
      T* dst = out + s * g.n_x + o * g.n * g.inner + c;
      T acc = 0;
      for (int64_t t = 0; t < g.n; ++t) {
        const int64_t i = (g.reverse ? g.n - 1 - t : t) * g.inner;
        const T v = src[i];
        if (g.exclusive) {
          dst[i] = acc;
          acc += v;
        } else {
          acc += v;
          dst[i] = acc;
        }
      }
    }
  });
}

// The segmented-scan stage (moosex.h mx_segscan_cross / _apply): one (slot, row, position) at
// a time.
template <class T>
void segscan_cross_cpu(const T* a, const T* b, T* out, int64_t slots, int64_t slot_stride,
                       const SegscanGeom& g) {
  const int64_t nj = g.n - g.j, rows = g.outer * nj;
  parallel_for(slots * rows, std::max<int64_t>(1, 4096 / g.inner), [&](int64_t q0, int64_t q1) {
    for (int64_t q = q0; q < q1; ++q) {
      const int64_t s = q / rows, row = q - s * rows, o = row / nj, t = row - o * nj;
      const int64_t ti = s * slot_stride + (o * g.n + t) * g.inner;
      const int64_t fi = s * slot_stride + (o * g.n + t + g.j) * g.inner + g.inner - 1;
      T* dst = out + q * g.inner;
      for (int64_t c = 0; c < g.inner; ++c)
        dst[c] = b ? a[fi] * (a[ti + c] + b[ti + c]) + b[fi] * a[ti + c] : a[fi] * a[ti + c];
    }
  });
}

template <class T>
void segscan_apply_cpu(const T* x, const T* p, T* out, int64_t slots, int64_t x_slot_stride,
                       int64_t p_slot_stride, const SegscanGeom& g) {
  const int64_t nj = g.n - g.j, rows = g.outer * g.n;
  parallel_for(slots * rows, std::max<int64_t>(1, 4096 / g.inner), [&](int64_t q0, int64_t q1) {
    for (int64_t q = q0; q < q1; ++q) {
      const int64_t s = q / rows, row = q - s * rows, o = row / g.n, pos = row - o * g.n;
      const T* src = x + s * x_slot_stride + row * g.inner;
      T* dst = out + q * g.inner;
      if (pos < g.j) {
        for (int64_t c = 0; c < g.inner; ++c) dst[c] = src[c];
        continue;
      }
      const T* pp = p + s * p_slot_stride + (o * nj + pos - g.j) * g.inner;
      for (int64_t c = 0; c + 1 < g.inner; ++c) dst[c] = src[c] + pp[c];
      dst[g.inner - 1] = pp[g.inner - 1];
    }
  });
}

using mxr::OuterGeom;

// The outer-product leaf (moosex.h mx_outer_cross): one (slot, group, row) at a time, the run
// of A columns of every b.
template <class T>
void outer_cross_cpu(const T* la, const T* lb, const T* ha, const T* hb, T* out, int64_t slots,
                     int64_t l_slot, int64_t l_group, int64_t h_slot, int64_t h_group,
                     const OuterGeom& g) {
  const int64_t lines = g.groups * g.rows;
  parallel_for(slots * lines, std::max<int64_t>(1, 4096 / g.n_out), [&](int64_t q0, int64_t q1) {
    for (int64_t q = q0; q < q1; ++q) {
      const int64_t s = q / lines, line = q - s * lines, gi = line / g.rows, r = line - gi * g.rows;
      const int64_t li = s * l_slot + gi * l_group + r * g.A;
      const int64_t hi = s * h_slot + gi * h_group + r * g.B;
      T* dst = out + q * g.n_out;
      for (int64_t c = 0; c < g.n_out; ++c) {
        const int64_t b = c / g.A, a = c - b * g.A;
        dst[c] = lb ? la[li + a] * (ha[hi + b] + hb[hi + b]) + lb[li + a] * ha[hi + b]
                    : la[li + a] * ha[hi + b];
      }
    }
  });
}

}  // namespace

extern "C" {

int mx_outer_cross(int dev, int elem_bytes, const void* la, const void* lb, const void* ha,
                   const void* hb, void* out, int64_t slots, int64_t l_slot_stride,
                   int64_t l_group_stride, int64_t h_slot_stride, int64_t h_group_stride,
                   int64_t groups, int64_t rows, int64_t A, int64_t B, int64_t n_out,
                   void* stream) {
  OuterGeom g{groups, rows, A, B, n_out};
  const int rc = mxr::outer_geom_check(g, elem_bytes, slots, l_slot_stride, l_group_stride,
                                       h_slot_stride, h_group_stride);
  if (rc <= 0) return rc;
  if (!la || !ha || !out || (lb == nullptr) != (hb == nullptr)) return -3;
  if (dev)
    return mxh_outer_cross(elem_bytes, la, lb, ha, hb, out, slots, l_slot_stride, l_group_stride,
                           h_slot_stride, h_group_stride, g, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    outer_cross_cpu((const T*)la, (const T*)lb, (const T*)ha, (const T*)hb, (T*)out, slots,
                    l_slot_stride, l_group_stride, h_slot_stride, h_group_stride, g);
    return 0;
  });
}

int64_t mx_scan_chunk(void) { return mxr::kScanChunk; }

int64_t mx_scan_ws_elems(int64_t slots, int64_t outer, int64_t n, int64_t inner) {
  ScanGeom g{outer, n, inner};
  const int rc = mxr::scan_geom_check(g, 8, slots, 0);
  return rc < 0 ? rc : slots * g.ws;
}

int mx_scan(int dev, int elem_bytes, const void* x, void* out, void* ws, int64_t ws_elems,
            int64_t slots, int64_t x_slot_stride, int64_t outer, int64_t n, int64_t inner,
            int exclusive, int reverse, void* stream) {
  ScanGeom g{outer, n, inner, exclusive != 0, reverse != 0};
  const int rc = mxr::scan_geom_check(g, elem_bytes, slots, x_slot_stride);
  if (rc <= 0) return rc;
  // both sides take the same workspace, so both refuse the same calls
  if (g.ws && (!ws || ws_elems < slots * g.ws)) return -3;
  if (!x || !out) return -3;
  if (dev) return mxh_scan(elem_bytes, x, out, ws, slots, x_slot_stride, g, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    scan_cpu((const T*)x, (T*)out, slots, x_slot_stride, g);
    return 0;
  });
}

int mx_segscan_cross(int dev, int elem_bytes, const void* a, const void* b, void* out,
                     int64_t slots, int64_t slot_stride, int64_t outer, int64_t n,
                     int64_t inner, int64_t j, void* stream) {
  SegscanGeom g{outer, n, inner, j};
  const int rc = mxr::segscan_geom_check(g, elem_bytes, slots, slot_stride);
  if (rc <= 0) return rc;
  if (!a || !out) return -3;
  if (dev) return mxh_segscan_cross(elem_bytes, a, b, out, slots, slot_stride, g, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    segscan_cross_cpu((const T*)a, (const T*)b, (T*)out, slots, slot_stride, g);
    return 0;
  });
}

int mx_segscan_apply(int dev, int elem_bytes, const void* x, const void* p, void* out,
                     int64_t slots, int64_t x_slot_stride, int64_t p_slot_stride, int64_t outer,
                     int64_t n, int64_t inner, int64_t j, void* stream) {
  SegscanGeom g{outer, n, inner, j};
  const int rc = mxr::segscan_geom_check(g, elem_bytes, slots, x_slot_stride, p_slot_stride);
  if (rc <= 0) return rc;
  if (!x || !p || !out) return -3;
  if (dev)
    return mxh_segscan_apply(elem_bytes, x, p, out, slots, x_slot_stride, p_slot_stride, g,
                             stream);
  DISPATCH_ELEM(elem_bytes, T, {
    segscan_apply_cpu((const T*)x, (const T*)p, (T*)out, slots, x_slot_stride, p_slot_stride, g);
    return 0;
  });
}

int mx_perm_gather(int dev, int elem_bytes, const void* a, const void* b, const void* p,
                   const void* m, const int64_t* perm, void* out, int64_t slots,
                   int64_t a_slot_stride, int64_t b_slot_stride, int64_t p_slot_stride,
                   int64_t m_slot_stride, int64_t outer, int64_t n, int64_t inner, void* stream) {
  const int64_t lim = 0x7fffffff;
  if (slots < 0 || outer < 0 || n < 0 || inner < 0 || outer > lim || n > lim || inner > lim ||
      a_slot_stride < 0 || b_slot_stride < 0 || p_slot_stride < 0 || m_slot_stride < 0)
    return -3;
  if (elem_bytes != 8 && elem_bytes != 16) return -2;
  if (slots == 0 || outer == 0 || n == 0 || inner == 0) return 0;
  if (n > ((int64_t)1 << 60) / outer / inner) return -3;
  // every extent a side forms -- (slots - 1) * stride + n_x and slots * n_x -- stays below 2^62
  const int64_t n_x = outer * n * inner, cap = mxr::slot_cap(slots);
  if (n_x > cap || a_slot_stride > cap || b_slot_stride > cap || p_slot_stride > cap ||
      m_slot_stride > cap)
    return -3;
  if (!a || !perm || !out) return -3;
  if (dev)
    return mxh_perm_gather(elem_bytes, a, b, p, m, perm, out, slots, a_slot_stride,
                           b_slot_stride, p_slot_stride, m_slot_stride, outer, n, inner, stream);
  std::vector<bool> seen(n, false);  // a permutation: every index once
  for (int64_t r = 0; r < n; ++r) {
    if (perm[r] < 0 || perm[r] >= n || seen[perm[r]]) return -3;
    seen[perm[r]] = true;
  }
  DISPATCH_ELEM(elem_bytes, T, {
    perm_gather_cpu((const T*)a, (const T*)b, (const T*)p, (const T*)m, perm, (T*)out, slots,
                    a_slot_stride, b_slot_stride, p_slot_stride, m_slot_stride, outer, n, inner);
    return 0;
  });
}

int mx_im2col(int dev, int elem_bytes, const void* in, void* out, int64_t slots,
              int64_t in_slot_stride, int64_t N, int64_t C, int64_t H, int64_t W, int64_t KH,
              int64_t KW, int64_t sh, int64_t sw, int64_t pt, int64_t pl, int64_t dh,
              int64_t dw, int64_t OH, int64_t OW, int nhwc, void* stream) {
  ImgGeom g{N, C, H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW};
  g.nhwc = nhwc;
  const int rc = mxr::img_geom_check(g, mxr::kIm2colLeaf, elem_bytes, slots, in_slot_stride);
  if (rc <= 0) return rc;
  if (dev) return mxh_im2col(elem_bytes, in, out, slots, in_slot_stride, g, stream);
  if (elem_bytes == 1) {  // bit tensors: the one leaf that moves them
    im2col_cpu((const uint8_t*)in, (uint8_t*)out, slots, in_slot_stride, g);
    return 0;
  }
  DISPATCH_ELEM(elem_bytes, T, {
    im2col_cpu((const T*)in, (T*)out, slots, in_slot_stride, g);
    return 0;
  });
}

int mx_col2im(int dev, int elem_bytes, const void* in, void* out, int64_t slots,
              int64_t in_slot_stride, int64_t N, int64_t C, int64_t H, int64_t W, int64_t KH,
              int64_t KW, int64_t sh, int64_t sw, int64_t pt, int64_t pl, int64_t dh,
              int64_t dw, int64_t OH, int64_t OW, int nhwc, void* stream) {
  ImgGeom g{N, C, H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW};
  g.nhwc = nhwc;
  const int rc = mxr::img_geom_check(g, mxr::kCol2imLeaf, elem_bytes, slots, in_slot_stride);
  if (rc <= 0) return rc;
  if (dev) return mxh_col2im(elem_bytes, in, out, slots, in_slot_stride, g, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    col2im_cpu((const T*)in, (T*)out, slots, in_slot_stride, g);
    return 0;
  });
}

int mx_resize2d(int dev, int elem_bytes, const void* in, void* out, int64_t slots,
                int64_t in_slot_stride, int64_t N, int64_t C, int64_t H, int64_t W, int64_t OH,
                int64_t OW, const int32_t* th, const int32_t* tw, int wbh, int wbw, int nhwc,
                void* stream) {
  ImgGeom g{N, C, H, W, 1, 1, 1, 1, 0, 0, 1, 1, OH, OW};  // a 1 x 1 window
  g.wbh = wbh, g.wbw = wbw, g.nhwc = nhwc;
  const int rc = mxr::img_geom_check(g, mxr::kResize2dLeaf, elem_bytes, slots, in_slot_stride);
  if (rc <= 0) return rc;
  if (!th || !tw) return -3;
  if (dev) return mxh_resize2d(elem_bytes, in, out, slots, in_slot_stride, g, th, tw, stream);
  // the tables are checked on the host only: the kernel clamps what it reads from them
  for (int64_t o = 0; o < OH; ++o)
    if (th[o] < 0 || th[o] >= H || th[OH + o] < 0 || th[OH + o] >= H || th[2 * OH + o] < 0 ||
        th[2 * OH + o] > (wbh ? 1 << wbh : 0))
      return -3;
  for (int64_t o = 0; o < OW; ++o)
    if (tw[o] < 0 || tw[o] >= W || tw[OW + o] < 0 || tw[OW + o] >= W || tw[2 * OW + o] < 0 ||
        tw[2 * OW + o] > (wbw ? 1 << wbw : 0))
      return -3;
  DISPATCH_ELEM(elem_bytes, T, {
    resize2d_cpu((const T*)in, (T*)out, slots, in_slot_stride, g, th, tw);
    return 0;
  });
}

int mx_dwconv(int dev, int elem_bytes, const void* x0, const void* x1, const void* w0,
              const void* w1, void* out, int64_t slots, int64_t x_slot_stride,
              int64_t w_slot_stride, int64_t N, int64_t C, int64_t H, int64_t W, int64_t mult,
              int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t pt, int64_t pl,
              int64_t dh, int64_t dw, int64_t OH, int64_t OW, int nhwc, void* stream) {
  ImgGeom g{N, C, H, W, KH, KW, sh, sw, pt, pl, dh, dw, OH, OW, mult};
  g.nhwc = nhwc;
  if ((x1 == nullptr) != (w1 == nullptr)) return -3;  // cross mode takes both second components
  const int rc = mxr::img_geom_check(g, mxr::kDwconvLeaf, elem_bytes, slots, x_slot_stride,
                                     w_slot_stride);
  if (rc <= 0) return rc;
  if (dev)
    return mxh_dwconv(elem_bytes, x0, x1, w0, w1, out, slots, x_slot_stride, w_slot_stride, g,
                      stream);
  DISPATCH_ELEM(elem_bytes, T, {
    dwconv_cpu((const T*)x0, (const T*)x1, (const T*)w0, (const T*)w1, (T*)out, slots,
               x_slot_stride, w_slot_stride, g);
    return 0;
  });
}

int mx_pwl_cross(int dev, int elem_bytes, const void* s0, const void* s1, const void* x0,
                 const void* x1, void* out, int64_t slots, int64_t s_slot_stride,
                 int64_t x_slot_stride, int64_t n, int k, const uint64_t* da, const uint64_t* db,
                 const uint64_t* ak, void* stream) {
  if (slots < 0 || n < 0 || k < 0 || k > MX_PWL_MAX || s_slot_stride < 0 || x_slot_stride < 0)
    return -3;
  if ((s1 == nullptr) != (x1 == nullptr)) return -3;  // cross mode takes both next components
  if (elem_bytes != 8 && elem_bytes != 16) return -2;
  if (slots == 0 || n == 0) return 0;
  // the flags' k * n elements of a slot (the largest count) and the strides within slot_cap
  const int64_t cap = mxr::slot_cap(slots);
  if (n > cap / std::max(k, 1) || s_slot_stride > cap || x_slot_stride > cap) return -3;
  if (!ak || (k && (!da || !db))) return -3;
  if (dev)
    return mxh_pwl_cross(elem_bytes, s0, s1, x0, x1, out, slots, s_slot_stride, x_slot_stride, n,
                         k, da, db, ak, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    pwl_cross_cpu((const T*)s0, (const T*)s1, (const T*)x0, (const T*)x1, (T*)out, slots,
                  s_slot_stride, x_slot_stride, n, k, da, db, ak);
    return 0;
  });
}

int mx_pwp_cross(int dev, int elem_bytes, const void* s0, const void* s1, const void* const* p0,
                 const void* const* p1, void* out, int64_t slots, int64_t s_slot_stride,
                 const int64_t* p_slot_stride, int64_t n, int k, int d, const uint64_t* dt,
                 const uint64_t* ck, void* stream) {
  if (slots < 0 || n < 0 || k < 1 || k > MX_PWP_MAX || d < 1 || d > MX_PWP_DEG ||
      s_slot_stride < 0 || !p0 || !p_slot_stride || !dt || !ck)
    return -3;
  if ((s1 == nullptr) != (p1 == nullptr)) return -3;  // cross mode takes both next components
  if (elem_bytes != 8 && elem_bytes != 16) return -2;
  for (int i = 0; i < d; ++i)
    if (p_slot_stride[i] < 0) return -3;
  if (slots == 0 || n == 0) return 0;
  // the flags' k * n elements of a slot (the largest count) and the strides within slot_cap
  const int64_t cap = mxr::slot_cap(slots);
  if (n > cap / k || s_slot_stride > cap) return -3;
  for (int i = 0; i < d; ++i)
    if (p_slot_stride[i] > cap || !p0[i] || (p1 && !p1[i])) return -3;
  if (!s0 || !out) return -3;
  if (dev)
    return mxh_pwp_cross(elem_bytes, s0, s1, p0, p1, out, slots, s_slot_stride, p_slot_stride, n,
                         k, d, dt, ck, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    pwp_cross_cpu((const T*)s0, (const T*)s1, p0, p1, (T*)out, slots, s_slot_stride,
                  p_slot_stride, n, k, d, dt, ck);
    return 0;
  });
}

int mx_cswap_diff(int dev, int elem_bytes, const void* x, void* out, int64_t slots,
                  int64_t x_slot_stride, int64_t outer, int64_t n, int64_t inner, int64_t by,
                  int64_t k, int64_t j, int descending, void* stream) {
  CswapGeom g{outer, n, inner, by, k, j, descending};
  const int rc = mxr::cswap_geom_check(g, elem_bytes, slots, x_slot_stride);
  if (rc <= 0) return rc;
  if (dev) return mxh_cswap_diff(elem_bytes, x, out, slots, x_slot_stride, g, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    cswap_diff_cpu((const T*)x, (T*)out, slots, x_slot_stride, g);
    return 0;
  });
}

int mx_cswap_cross(int dev, int elem_bytes, const void* s0, const void* s1, const void* x0,
                   const void* x1, void* out, int64_t slots, int64_t s_slot_stride,
                   int64_t x_slot_stride, int64_t outer, int64_t n, int64_t inner, int64_t by,
                   int64_t k, int64_t j, int descending, void* stream) {
  CswapGeom g{outer, n, inner, by, k, j, descending};
  if ((s1 == nullptr) != (x1 == nullptr)) return -3;  // cross mode takes both next components
  const int rc = mxr::cswap_geom_check(g, elem_bytes, slots, s_slot_stride, x_slot_stride);
  if (rc <= 0) return rc;
  if (dev)
    return mxh_cswap_cross(elem_bytes, s0, s1, x0, x1, out, slots, s_slot_stride, x_slot_stride,
                           g, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    cswap_cross_cpu((const T*)s0, (const T*)s1, (const T*)x0, (const T*)x1, (T*)out, slots,
                    s_slot_stride, x_slot_stride, g);
    return 0;
  });
}

int mx_cswap_apply(int dev, int elem_bytes, const void* x, const void* p, void* out,
                   int64_t slots, int64_t x_slot_stride, int64_t p_slot_stride, int64_t outer,
                   int64_t n, int64_t inner, int64_t by, int64_t k, int64_t j, int descending,
                   void* stream) {
  CswapGeom g{outer, n, inner, by, k, j, descending};
  const int rc = mxr::cswap_geom_check(g, elem_bytes, slots, x_slot_stride, p_slot_stride);
  if (rc <= 0) return rc;
  if (dev)
    return mxh_cswap_apply(elem_bytes, x, p, out, slots, x_slot_stride, p_slot_stride, g, stream);
  DISPATCH_ELEM(elem_bytes, T, {
    cswap_apply_cpu((const T*)x, (const T*)p, (T*)out, slots, x_slot_stride, p_slot_stride, g);
    return 0;
  });
}

}  // extern "C"
