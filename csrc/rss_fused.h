// Fused single-pass kernels for a stacked 3-party session (all parties on one device).
//
// They compute exactly the same shares as the generic protocol code in
// moose_amd/protocols/replicated.py (same PRF keys, nonces and element->keystream
// mapping), but do every party's local work of a whole protocol in ONE pass over
// memory: TruncPr (dealer masks, masked openings, additive->replicated) and Share.
#pragma once
#include <stdint.h>

#include "aes_core.h"
#include "moosex.h"
#include "ring_common.h"

namespace mxf {

template <class T>
MX_HD inline T shl(T x, int k) {
  constexpr int W = 8 * sizeof(T);
  return k >= W ? (T)0 : (T)(x << k);
}
template <class T>
MX_HD inline T shr(T x, int k) {
  constexpr int W = 8 * sizeof(T);
  return k >= W ? (T)0 : (T)(x >> k);
}

// inputs: slots x0, x1, x2 and the six PRF values (dealer key k0: r0, rt0, rm0, z0;
// dealer key k2: r1, z2).  Returns the new slots z0, z1, z2 (z0, z2 are the PRF values).
template <class T>
MX_HD inline T trunc_pr_z1(T x0, T x1, T x2, T r0, T r1, T rt0, T rm0, T z0, T z2, int m) {
  constexpr int W = 8 * sizeof(T);
  const int k = W - 1;
  T r = r0 + r1;
  T r_msb = shr<T>(r, W - 1);
  T r_top = shr<T>(shl<T>(r, 1), m + 1);
  T rt1 = r_top - rt0;
  T rm1 = r_msb - rm0;
  T mk0 = x0 + x1 + shl<T>((T)1, k - 1) + r0;
  T mk1 = x2 + r1;
  T c = mk0 + mk1;
  T c_msb = shr<T>(c, W - 1);
  T c_top = shr<T>(shl<T>(c, 1), m + 1);
  T ov0 = rm0 - shl<T>(c_msb * rm0, 1) + c_msb;
  T y0 = shl<T>(ov0, k - m) - rt0 + c_top - shl<T>((T)1, k - 1 - m);
  T ov1 = rm1 - shl<T>(c_msb * rm1, 1);
  T y1 = shl<T>(ov1, k - m) - rt1;
  return (y0 - z0) + (y1 - z2);
}

// z0 + trunc_pr_z1(x0, x1, x2, r0, r1, rt0, rm0, z0, z2, m) + z2 -- the opened value of the
// new sharing -- from x = x0 + x1 + x2 and r = r0 + r1 alone.  The sum is y0 + y1 of
// trunc_pr_z1, and in Z_2^w (shl and the products by c_msb are linear there)
//   ov0 + ov1 = r_msb - 2 c_msb r_msb + c_msb,      rt0 + rt1 = r_top,
// so the dealer's split of r_top and r_msb (rt0, rm0) and the output masks z0, z2 cancel
// bit for bit; c itself reads the slots only through their sum, so a zero share added to
// them (k_p - k_{p+1} on slot p) cancels as well.  An opening therefore needs two of the
// tail's nine keystreams and one sum of the three local products.
template <class T>
MX_HD inline T trunc_pr_open(T x, T r, int m) {
  constexpr int W = 8 * sizeof(T);
  const int k = W - 1;
  T r_msb = shr<T>(r, W - 1);
  T r_top = shr<T>(shl<T>(r, 1), m + 1);
  T c = x + shl<T>((T)1, k - 1) + r;
  T c_msb = shr<T>(c, W - 1);
  T c_top = shr<T>(shl<T>(c, 1), m + 1);
  T ov = r_msb - shl<T>(c_msb * r_msb, 1) + c_msb;
  return shl<T>(ov, k - m) - r_top + c_top - shl<T>((T)1, k - 1 - m);
}

// ---------------------------------------------------------------------------------------
// Input sharing by the member P_j0 (k_share3, its host twin, and the sharing CRT operand prep
// of gemm_crt.hip): slot j0 = r (one PRF draw), slot j0 + 1 = x - r, slot j0 + 2 = 0;
// mirrored (MX_SHARE_MIRROR) the first two are swapped.  ``kind`` is without the mirror flag.
// ---------------------------------------------------------------------------------------
// the plain element i: ring data, or a float64 encoded as RingFixedpointEncode (scale = 2^frac)
template <class T>
MX_HD inline T share_plain(int kind, const void* xv, int64_t i, double scale) {
  return kind == MX_SHARE_F64 ? mxr::f64_to_ring<T>(((const double*)xv)[i] * scale)
                              : ((const T*)xv)[i];
}
template <class T>
MX_HD inline T share_masked(int kind, T x, T r) {
  return kind == MX_CROSS_BOOL ? (T)(x ^ r) : (T)(x - r);
}
// the slots that hold r and the masked value (the third one is zero)
MX_HD inline void share_place(int j0, bool mir, int* jr, int* jv) {
  *jr = mir ? (j0 + 1) % 3 : j0;
  *jv = mir ? j0 : (j0 + 1) % 3;
}
template <class T>
MX_HD inline void share_slots(int kind, T x, T r, int j0, bool mir, T (&slot)[3]) {
  const T v = share_masked<T>(kind, x, r);
  slot[j0] = mir ? v : r;
  slot[(j0 + 1) % 3] = mir ? r : v;
  slot[(j0 + 2) % 3] = 0;
}

// ---------------------------------------------------------------------------------------
// Ring extension Z_2^64 -> Z_2^128 of a replicated sharing (dealer P2), exact for
// -2^62 <= x < 2^62: TruncPr's overflow trick without the truncation.  With x' = x + 2^62 in
// [0, 2^63) and c = x' + r (mod 2^64) opened, the integer sum x' + r wraps exactly when
// r_msb = 1 and c_msb = 0, so x' = c - R + 2^64 r_msb (1 - c_msb) over Z_2^128 (R = r
// zero-extended).  The dealer shares R and r_msb additively between P0 and P1; the share of
// r_msb only matters modulo 2^64 (it is shifted left by 64) and travels as a u64.
// ---------------------------------------------------------------------------------------
using u128_t = unsigned __int128;

// launches of at most this many elements take the latency form of the device kernel
constexpr int64_t kRingExtendLatMax = 8192;

// dealer P2: r = r0 + r1 -> (R1, M1) for P1
MX_HD inline void ring_extend_dealer(uint64_t r0, uint64_t r1, u128_t R0, uint64_t M0, u128_t* R1,
                                     uint64_t* M1) {
  const uint64_t r = r0 + r1;
  *R1 = (u128_t)r - R0;
  *M1 = (r >> 63) - M0;
}

// P0's masked opening share: x0 + x1 + 2^62 + r0 (P1's is x2 + r1)
MX_HD inline uint64_t ring_extend_mask0(uint64_t x0, uint64_t x1, uint64_t r0) {
  return x0 + x1 + ((uint64_t)1 << 62) + r0;
}

// P0's (first) / P1's additive share of the widened value from the opened c
MX_HD inline u128_t ring_extend_y(uint64_t c, u128_t R, uint64_t M, bool first) {
  const uint64_t nc = 1 - (c >> 63);
  const u128_t y = ((u128_t)(uint64_t)(nc * M) << 64) - R;
  return first ? y + (u128_t)c - ((u128_t)1 << 62) : y;
}

// inputs: slots x0, x1, x2 and the six PRF values (dealer key k0: r0, R0, M0, z0; dealer key
// k2: r1, z2).  Returns the new slot z1 (z0, z2 are the PRF values).
MX_HD inline u128_t ring_extend_z1(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t r0, uint64_t r1,
                                   u128_t R0, uint64_t M0, u128_t z0, u128_t z2) {
  u128_t R1;
  uint64_t M1;
  ring_extend_dealer(r0, r1, R0, M0, &R1, &M1);
  const uint64_t c = ring_extend_mask0(x0, x1, r0) + (x2 + r1);
  const u128_t y0 = ring_extend_y(c, R0, M0, true);
  const u128_t y1 = ring_extend_y(c, R1, M1, false);
  return (y0 - z0) + (y1 - z2);
}

}  // namespace mxf

// ---------------------------------------------------------------------------------------
// Per-party TruncPr rounds (one party per stacked component, parties on different GPUs;
// see rss_party.hip).  Same arithmetic as trunc_pr_z1, split at the two message rounds.
// The dealer's msb-mask share only matters modulo 2^(m+1) (it is shifted left by k - m),
// so it travels as a u64 (m <= 63).
// ---------------------------------------------------------------------------------------
namespace mxf {

// dealer P2: r = r0 + r1 -> (rt1, rm1) for P1
template <class T>
MX_HD inline void trunc_dealer(T r0, T r1, T rt0, T rm0, int m, T* rt1, uint64_t* rm1) {
  constexpr int W = 8 * sizeof(T);
  const T r = r0 + r1;
  *rt1 = shr<T>(shl<T>(r, 1), m + 1) - rt0;
  *rm1 = (uint64_t)(shr<T>(r, W - 1) - rm0);
}

// P0's masked opening share: x0 + x1 + 2^(k-1) + r0
template <class T>
MX_HD inline T trunc_mask0(T x0, T x1, T r0) {
  constexpr int W = 8 * sizeof(T);
  return x0 + x1 + shl<T>((T)1, W - 2) + r0;
}

// P0's (first) / P1's truncated additive share from the opened c
template <class T>
MX_HD inline T trunc_y(T c, T rt, T rm, int m, bool first) {
  constexpr int W = 8 * sizeof(T);
  const int k = W - 1;
  const T c_msb = shr<T>(c, W - 1);
  T ov = rm - shl<T>(c_msb * rm, 1);
  if (!first) return shl<T>(ov, k - m) - rt;
  ov = ov + c_msb;
  const T c_top = shr<T>(shl<T>(c, 1), m + 1);
  return shl<T>(ov, k - m) - rt + c_top - shl<T>((T)1, k - 1 - m);
}

// ---------------------------------------------------------------------------------------
// The rounds of one element as a party in ``role`` computes them: the ONE statement of the
// per-party protocol for the device kernels (party_rounds.h) and their host twins
// (party_rounds_cpu.h).  PRF streams (key of the drawing party):
//   r0, t, m, z0 under k0 (P0 own, P2 next);  r1, z2 under k2 (P1 next, P2 own)
// ---------------------------------------------------------------------------------------

// The dot tail's zero-share form of a party's local product x: P0 a = f(k0), P1 b = f(k2),
// P2 both (f = PRF at the zero-share nonce); a stream the role does not draw is 0.
template <class T>
MX_HD inline T zero_masked(T x, T a, T b) {
  return x + a - b;
}

// Round 0: what P0 / P1 / P2 send of their additive part v of the value (TruncPr: P0's
// x0 + x1, P1's x2; dot tail: zero_masked) under the opening mask r (P0 r0, P1 r1).
template <class T>
MX_HD inline T trunc_open_msg(int role, T v, T r) {
  return role == 0 ? trunc_mask0<T>(v, (T)0, r) : role == 1 ? (T)(v + r) : v;
}

// Round 0, dealer P2: the messages for P1 and its own new share (s0, s1) = (z2, z0).
template <class T>
struct TruncDeal {
  T rt1;
  uint64_t rm1;
  T s0, s1;
};
template <class T>
MX_HD inline TruncDeal<T> trunc_deal(T r0, T r1, T t, T mm, T z0, T z2, int m) {
  TruncDeal<T> d;
  trunc_dealer<T>(r0, r1, t, mm, m, &d.rt1, &d.rm1);
  d.s0 = z2;
  d.s1 = z0;
  return d;
}

// Round 1, P0 / P1: w = y - z from the opened c; (rt, rm) are P0's own draws t, m or what
// P1 received from the dealer; z (P0 z0, P1 z2) is the party's new share s0 / s1.
template <class T>
MX_HD inline T trunc_round1_w(int role, T c, T rt, T rm, T z, int m) {
  return trunc_y<T>(c, rt, rm, m, role == 0) - z;
}

// The same two for the ring extension; every draw is a 128-bit lane, r0, r1 and M0 its low
// 64 bits.
struct RingExtendDeal {
  u128_t R1;
  uint64_t M1;
  u128_t s0, s1;
};
MX_HD inline RingExtendDeal ring_extend_deal(u128_t r0, u128_t r1, u128_t R0, u128_t M0, u128_t z0,
                                             u128_t z2) {
  RingExtendDeal d;
  ring_extend_dealer((uint64_t)r0, (uint64_t)r1, R0, (uint64_t)M0, &d.R1, &d.M1);
  d.s0 = z2;
  d.s1 = z0;
  return d;
}
MX_HD inline u128_t ring_extend_round1_w(int role, uint64_t c, u128_t R, uint64_t M, u128_t z) {
  return ring_extend_y(c, R, M, role == 0) - z;
}

}  // namespace mxf
