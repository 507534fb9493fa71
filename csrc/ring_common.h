// Element-level ring semantics shared by the host and device kernels.
#pragma once
#include <stdint.h>
#include <string.h>

#include "aes_core.h"
#include "cswap_geom.h"
#include "img_geom.h"
#include "outer_geom.h"
#include "segscan_geom.h"
#include "moosex.h"

namespace mxr {

using u64 = uint64_t;
using u128 = unsigned __int128;
using i128 = __int128;

template <class T>
struct Bits {
  static constexpr int value = 8 * sizeof(T);
};

template <class T>
MX_HD inline T binop(int op, T a, T b) {
  if constexpr (sizeof(T) == 1) {  // bit tensors: Z_2 (0/1 bytes)
    switch (op) {
      case MX_ADD:
      case MX_SUB:
      case MX_XOR: return (T)((a ^ b) & 1);
      case MX_MUL:
      case MX_AND: return (T)(a & b & 1);
      case MX_OR: return (T)((a | b) & 1);
    }
    return 0;
  } else {
    switch (op) {
      case MX_ADD: return a + b;
      case MX_SUB: return a - b;
      case MX_MUL: return a * b;
      case MX_AND: return a & b;
      case MX_OR: return a | b;
      case MX_XOR: return a ^ b;
    }
    return 0;
  }
}

template <class T>
MX_HD inline T unop(int op, T a, int k) {
  constexpr int W = Bits<T>::value;
  if constexpr (sizeof(T) == 1) {
    switch (op) {
      case MX_NEG: return (T)(a & 1);
      case MX_NOT: return (T)((a ^ 1) & 1);
      default: return k == 0 ? (T)(a & 1) : (T)0;
    }
  } else {
    switch (op) {
      case MX_NEG: return (T)0 - a;
      case MX_NOT: return ~a;
      case MX_SHL: return k >= W ? (T)0 : (T)(a << k);
      case MX_SHR: return k >= W ? (T)0 : (T)(a >> k);
      case MX_SAR: {
        if constexpr (sizeof(T) == 8) {
          int64_t s = (int64_t)a;
          return (T)(k >= 64 ? (s >> 63) : (s >> k));
        } else {
          i128 s = (i128)a;
          return (T)(k >= 128 ? (s >> 127) : (s >> k));
        }
      }
    }
    return 0;
  }
}

template <class T>
MX_HD inline uint8_t cmpop(int op, T a, T b) {
  if constexpr (sizeof(T) == 1) {
    switch (op) {
      case MX_LT: return a < b;
      case MX_GT: return a > b;
      case MX_EQ: return a == b;
      default: return a & 1;
    }
  } else if constexpr (sizeof(T) == 8) {
    int64_t x = (int64_t)a, y = (int64_t)b;
    switch (op) {
      case MX_LT: return x < y;
      case MX_GT: return x > y;
      case MX_EQ: return x == y;
      default: return (uint8_t)(a >> 63);
    }
  } else {
    i128 x = (i128)a, y = (i128)b;
    switch (op) {
      case MX_LT: return x < y;
      case MX_GT: return x > y;
      case MX_EQ: return x == y;
      default: return (uint8_t)(a >> 127);
    }
  }
}

template <class T>
MX_HD inline T cross(int kind, T x0, T x1, T y0, T y1, bool has_x1, bool has_y1) {
  if (kind == MX_CROSS_BOOL) {
    T v = x0 & y0;
    if (has_y1) v ^= x0 & y1;
    if (has_x1) v ^= x1 & y0;
    return v;
  }
  T v = x0 * y0;
  if (has_y1) v += x0 * y1;
  if (has_x1) v += x1 * y0;
  return v;
}

template <class T>
MX_HD inline T zs_combine(int kind, T v, T ra, T rb) {
  if (kind == MX_CROSS_BOOL) return (T)(v ^ ra ^ rb);
  return (T)(v + ra - rb);
}

// Fixed-point conversions follow Rust's numeric `as` casts, which the reference applies at
// the ring's own width:
//   double -> Z_2^64  is `x as i64 as u64`:   truncates toward zero, saturates at
//                     [-2^63, 2^63 - 1], NaN -> 0;
//   double -> Z_2^128 is `x as i128 as u128`: the same at [-2^127, 2^127 - 1];
//   Z_2^w  -> double  is `x as iW as f64`:    the nearest double of the signed value, ties
//                     to even, one rounding.
// Kernels encode through f64_to_ring<T> only, so the stand-alone encode and the share
// kernels that encode their input cannot drift apart.

// double -> i128, truncating toward zero, saturating at the limits of i128; NaN -> 0
MX_HD inline i128 f64_to_i128(double x) {
  uint64_t bits;
  memcpy(&bits, &x, 8);
  int neg = (int)(bits >> 63);
  int e = (int)((bits >> 52) & 0x7ff);
  uint64_t mant = bits & ((1ull << 52) - 1);
  if (e == 0x7ff) return mant ? (i128)0 : (neg ? (i128)((u128)1 << 127) : ~(i128)((u128)1 << 127));
  if (e == 0) return 0;  // subnormals truncate to 0
  mant |= (1ull << 52);
  int sh = e - 1075;  // value = mant * 2^sh
  u128 mag;
  if (sh >= 0) {
    if (sh > 127 - 53) return neg ? (i128)((u128)1 << 127) : ~(i128)((u128)1 << 127);
    mag = (u128)mant << sh;
  } else if (sh <= -53) {
    mag = 0;
  } else {
    mag = (u128)(mant >> (-sh));
  }
  return neg ? -(i128)mag : (i128)mag;
}

// double -> element of the ring T (u64 or u128), saturating at the signed range of T
template <class T>
MX_HD inline T f64_to_ring(double x) {
  if constexpr (sizeof(T) == 8) {
    if (x >= 9223372036854775808.0) return (T)0x7fffffffffffffffull;
    if (x > -9223372036854775808.0) return (T)(int64_t)x;  // in range: the cast truncates
    return x != x ? (T)0 : (T)1 << 63;
  } else {
    return (T)f64_to_i128(x);
  }
}

// signed value of a Z_2^128 element -> nearest double (ties to even).  The magnitude is taken
// in unsigned arithmetic (-2^127 has no signed negation) and rounded once: its top 64 bits,
// with a sticky bit for whatever lies below them, convert in one correctly rounded step, and
// the scaling back by a power of two is exact.
MX_HD inline double i128_to_f64(u128 v) {
  const bool neg = (v >> 127) != 0;
  const u128 m = neg ? (u128)0 - v : v;
  const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
  double r;
  if (hi == 0) {
    r = (double)lo;
  } else {
    const int s = 64 - __builtin_clzll(hi);  // 1..64 bits of m lie above the low limb
    const uint64_t lost = s == 64 ? lo : lo & ((1ull << s) - 1);
    const uint64_t top = (uint64_t)(m >> s) | (uint64_t)(lost != 0);  // bit 63 is set
    const uint64_t pbits = (uint64_t)(1023 + s) << 52;                // 2^s as a double
    double p;
    memcpy(&p, &pbits, 8);
    r = (double)top * p;
  }
  return neg ? -r : r;
}

// signed value of a ring element (u64 or u128) -> nearest double: the decode of an opening
template <class T>
MX_HD inline double signed_to_f64(T v) {
  if constexpr (sizeof(T) == 8)
    return (double)(int64_t)v;
  else
    return i128_to_f64(v);
}

}  // namespace mxr

// Device launchers (ring_hip.hip, leaf_hip.hip, gemm_valu.hip, gemm_mfma.hip)
extern "C" {
int mxh_ew_binary(int op, int words, const void* a, int64_t na, const void* b, int64_t nb,
                  void* out, int64_t n, void* stream);
int mxh_ew_unary(int op, int words, const void* a, void* out, int64_t n, int64_t param,
                 void* stream);
int mxh_ew_compare(int op, int words, const void* a, int64_t na, const void* b, int64_t nb,
                   uint8_t* out, int64_t n, void* stream);
int mxh_bit_extract(int words, const void* a, uint8_t* out, int64_t n, int bit, void* stream);
int mxh_ring_inject(int words, const uint8_t* bits, void* out, int64_t n, int bit,
                    void* stream);
int mxh_encode(int words, const double* x, void* out, int64_t n, int frac, void* stream);
int mxh_decode(int words, const void* x, double* out, int64_t n, int frac, void* stream);
int mxh_addn_decode(int words, const void* a, const void* b, const void* c, const void* d,
                    double* out, int64_t n, int frac, void* stream);
int mxh_fill(int words, void* out, int64_t n, uint64_t lo, uint64_t hi, void* stream);
int mxh_bit_planes(int words, const void* a, uint8_t* out, int64_t outer, int64_t inner,
                   int start, int count, void* stream);
int mxh_weighted_sum(int words, const void* a, const void* w, void* out, int64_t outer,
                     int64_t k, int64_t inner, void* stream);
int mxh_sum_axis(int words, const void* a, void* out, int64_t outer, int64_t red, int64_t inner,
                 void* stream);
int mxh_prg(const uint8_t* key16, uint64_t nonce, uint64_t ctr0, void* out, int64_t nbytes,
            void* stream);
int mxh_rss_cross(int kind, int words, const void* x0, const void* x1, const void* y0,
                  const void* y1, void* out, int64_t n, int nparties, const uint8_t* keys16,
                  uint64_t nonce, void* stream);
int mxh_prf_expand(int words, void* out, int64_t n, int nkeys, const uint8_t* keys16,
                   uint64_t nonce, void* stream);
int mxh_rss_cross_kp(int kind, int words, const void* x0, const void* x1, const void* y0,
                     const void* y1, void* out, int64_t n, int nparties,
                     const uint32_t* const* slot_ptrs, uint64_t nonce, void* stream);
int mxh_rss_cross_k(int kind, int words, const void* x0, const void* x1, const void* y0,
                    const void* y1, void* out, int64_t n, int nparties, const uint32_t* slots,
                    int nslots, uint64_t nonce, void* stream);
int mxh_rss_mul3_kv(int kind, int words, const void* x0, const void* x1, const void* y0,
                    const void* y1, void* out0, void* out1, int64_t n, const uint32_t* slots,
                    uint64_t nonce, const int64_t* views, void* stream);
int mxh_rss_mul3_k(int kind, int words, const void* x0, const void* x1, const void* y0,
                   const void* y1, void* out0, void* out1, int64_t n, const uint32_t* slots,
                   uint64_t nonce, void* stream);
int mxh_ew_binary_slot(int op, int words, const void* a, const void* b, int64_t nb, void* out,
                       int64_t m, int nparties, int which, void* stream);
int mxh_add_zs3(int words, const void* v, const void* r, void* out0, void* out1, int64_t n,
                void* stream);
int mxh_ew_binary2(int op, int words, const void* a0, const void* b0, void* out0,
                   const void* a1, const void* b1, void* out1, int64_t na, int64_t nb, int64_t n,
                   void* stream);
int mxh_mul_add2(int words, const void* a0, const void* a1, const void* f, const void* c,
                 int add0, int add1, void* out0, void* out1, int64_t n, void* stream);
int mxh_ew_add3(int words, const void* a, const void* b, const void* c, void* out, int64_t n,
                void* stream);
int mxh_lincomb2(int words, int nin, const void* const* ins, const int64_t* coef, const void* b,
                 int64_t nb, void* out0, void* out1, int64_t m, int nparties, int which0,
                 int which1, void* stream);
int mxh_sum_views2(int words, const void* base0, const void* base1, int64_t is0, int64_t is1,
                   int64_t ps0, int64_t ps1, int k, void* out0, void* out1, int64_t m,
                   int nparties, void* stream);
int mxh_slot_place2(int words, const void* x0, const void* x1, void* out0, void* out1,
                    int64_t m, int nparties, int which0, int which1, void* stream);
int mxh_mul_trunc3_kv(int words, const void* x0, const void* x1, const void* y0, const void* y1,
                      void* out0, void* out1, int64_t n, int64_t ostride, const uint32_t* slots,
                      uint64_t nmul, int m, const uint64_t* nn, const int64_t* views,
                      void* stream);
int mxh_mul_trunc3_open(int words, const void* x, int64_t xstride, double* out, int64_t n,
                        const uint32_t* slots, uint64_t nmul, int m, const uint64_t* nn, int frac,
                        void* stream);
// gemm_crt.hip: mxh_mul_trunc3_open of a product still held as the CRT GEMM's residues
int mxh_crt_recon_open(int words, const int64_t* crt, double* out, int64_t n,
                       const uint32_t* slots, int m, const uint64_t* nn, int frac, void* stream);
int mxh_ew_unary2(int op, int words, const void* a0, void* out0, const void* a1, void* out1,
                  int64_t n, int64_t param, void* stream);
int mxh_transpose2(int words, const void* a0, void* out0, const void* a1, void* out1,
                   int64_t rows, int64_t cols, void* stream);
int mxh_ew_binary_slot2(int op, int words, const void* a0, const void* a1, const void* b,
                        int64_t nb, void* out0, void* out1, int64_t m, int nparties, int which0,
                        int which1, void* stream);
// the image leaves: g is validated and filled by img_geom_check (img_geom.h)
int mxh_im2col(int elem_bytes, const void* in, void* out, int64_t slots, int64_t in_slot_stride,
               const mxr::ImgGeom& g, void* stream);
int mxh_col2im(int elem_bytes, const void* in, void* out, int64_t slots, int64_t in_slot_stride,
               const mxr::ImgGeom& g, void* stream);
int mxh_resize2d(int elem_bytes, const void* in, void* out, int64_t slots,
                 int64_t in_slot_stride, const mxr::ImgGeom& g, const int32_t* th,
                 const int32_t* tw, void* stream);
int mxh_pwl_cross(int elem_bytes, const void* s0, const void* s1, const void* x0, const void* x1,
                  void* out, int64_t slots, int64_t s_slot_stride, int64_t x_slot_stride,
                  int64_t n, int k, const uint64_t* da, const uint64_t* db, const uint64_t* ak,
                  void* stream);
int mxh_pwp_cross(int elem_bytes, const void* s0, const void* s1, const void* const* p0,
                  const void* const* p1, void* out, int64_t slots, int64_t s_slot_stride,
                  const int64_t* p_slot_stride, int64_t n, int k, int d, const uint64_t* dt,
                  const uint64_t* ck, void* stream);
int mxh_dwconv(int elem_bytes, const void* x0, const void* x1, const void* w0, const void* w1,
               void* out, int64_t slots, int64_t x_slot_stride, int64_t w_slot_stride,
               const mxr::ImgGeom& g, void* stream);
// the compare-exchange leaves: g is validated and filled by cswap_geom_check (cswap_geom.h)
int mxh_cswap_diff(int elem_bytes, const void* x, void* out, int64_t slots, int64_t x_slot_stride,
                   const mxr::CswapGeom& g, void* stream);
int mxh_cswap_cross(int elem_bytes, const void* s0, const void* s1, const void* x0,
                    const void* x1, void* out, int64_t slots, int64_t s_slot_stride,
                    int64_t x_slot_stride, const mxr::CswapGeom& g, void* stream);
int mxh_cswap_apply(int elem_bytes, const void* x, const void* p, void* out, int64_t slots,
                    int64_t x_slot_stride, int64_t p_slot_stride, const mxr::CswapGeom& g,
                    void* stream);
// the permuted row gather: sizes and strides checked by mx_perm_gather, rows = outer * n
int mxh_perm_gather(int elem_bytes, const void* a, const void* b, const void* p, const void* m,
                    const int64_t* perm, void* out, int64_t slots, int64_t a_slot_stride,
                    int64_t b_slot_stride, int64_t p_slot_stride, int64_t m_slot_stride,
                    int64_t outer, int64_t n, int64_t inner, void* stream);
// the prefix-sum leaves: g is validated and filled by scan_geom_check / segscan_geom_check
// (segscan_geom.h); ws holds slots * g.ws elements (mx_scan checked it)
int mxh_scan(int elem_bytes, const void* x, void* out, void* ws, int64_t slots,
             int64_t x_slot_stride, const mxr::ScanGeom& g, void* stream);
int mxh_segscan_cross(int elem_bytes, const void* a, const void* b, void* out, int64_t slots,
                      int64_t slot_stride, const mxr::SegscanGeom& g, void* stream);
int mxh_segscan_apply(int elem_bytes, const void* x, const void* p, void* out, int64_t slots,
                      int64_t x_slot_stride, int64_t p_slot_stride, const mxr::SegscanGeom& g,
                      void* stream);
// the outer-product leaf: g is validated and filled by outer_geom_check (outer_geom.h); lb and
// hb are both null (plain) or both set (cross)
int mxh_outer_cross(int elem_bytes, const void* la, const void* lb, const void* ha,
                    const void* hb, void* out, int64_t slots, int64_t l_slot_stride,
                    int64_t l_group_stride, int64_t h_slot_stride, int64_t h_group_stride,
                    const mxr::OuterGeom& g, void* stream);
int mxh_ks_cross1(int words, const void* g0, const void* g1, const void* p0, const void* p1,
                  void* z, int64_t n, int d, int both, const uint8_t* keys16, uint64_t nonce,
                  void* stream);
int mxh_ks_cross1_s(int words, const void* g0, const void* g1, const void* p0, const void* p1,
                    void* z, int64_t n, int d, int both, const uint32_t* const* slots,
                    uint64_t nonce, void* stream);
int mxh_ks_cross1x_s(int words, const void* g0, const void* g1, const void* t0, const void* t1,
                     void* go0, void* go1, const void* p0, const void* p1, void* z, int64_t n,
                     int d, int both, const uint32_t* const* slots, uint64_t nonce,
                     void* stream);
int mxh_ks_sum2(int words, const void* p0, const void* p1, const void* g0, const void* g1,
                const void* t0, const void* t1, void* o0, void* o1, int64_t n, void* stream);
int mxh_ks_adder3_k(int words, const void* g0, const void* g1, const void* p0, const void* p1,
                    void* og0, void* og1, int64_t n, int nlev, const uint32_t* slots,
                    const uint64_t* nonces, void* stream);
int mxh_ks_level3_k(int words, const void* g0, const void* g1, const void* p0, const void* p1,
                    void* og0, void* og1, void* op0, void* op1, int64_t n, int d, int both,
                    const uint32_t* slots, uint64_t nonce, void* stream);
int mxh_prf_expand_k(int words, void* out, int64_t n, int nkeys, const uint32_t* slots,
                     uint64_t nonce, void* stream);
int mxh_gemm(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
             const void* A1, const void* B0, const void* B1, int mode, void* C, int accumulate,
             void* stream);
}
