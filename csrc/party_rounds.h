// The per-party TruncPr / dot-tail rounds as the device kernels of rss_party.hip (stacked
// components, dense rows or per-component pointers) and rss_jobs.hip (job rows) walk them.
// The arithmetic of one element is in rss_fused.h (trunc_open_msg, trunc_deal,
// trunc_round1_w, ...); here are the keystream walk, the PRF streams a role draws and the
// round bodies, written once and parameterised by where an element is read and written.
//
// TruncPr (dealer P2, reference additive/trunc.rs:114-170), rounds:
//   r0: P0 mk0 = x0 + x1 + 2^(k-2) + r0          -> P1
//       P1 mk1 = x2 + r1                          -> P0
//       P2 rt1, rm1 (dealer shares for P1)        -> P1;  P2's new shares (z2, z0)
//   r1: P0 c = mk0 + mk1, y0, w0 = y0 - z0        -> P1;  P0's s0 = z0
//       P1 c = mk1 + mk0, y1, w1 = y1 - z2        -> P0;  P1's s1 = z2
//   r2: z1 = w0 + w1 (elementwise)
// Fixed-point dot tail (rep.dot_trunc): the reshare of rep.dot is folded into round 0.  P_p's
// local product masked by the zero share is z_p (3-out-of-3 additive), and the opening
// c = x + r + 2^(k-2) is assembled from
//   P0: m0 = z0 + 2^(k-2) + r0   -> P1
//   P1: m1 = z1 + r1              -> P0
//   P2: z2                        -> P0 and P1        (+ the dealer's rt1, rm1 -> P1)
// so P0 and P1 get c = m0 + m1 + z2 in ONE round (the generic path needs the reshare round
// plus the P0 <-> P1 round).  c is the same value and every output share depends on the input
// only through c, so the shares are bitwise equal to reshare + TruncPr and to the stacked
// fused kernel.  Zero share: P0 f(k0), P1 -f(k2), P2 f(k2) - f(k0) (f = PRF at nonce n_a; sums
// to zero).  z2 is masked by f(k2) against P0 and f(k0) against P1, m0 / m1 by the opening
// masks: every view is as with the textbook alpha_p = f(k_p) - f(k_{p+1}), with one PRF
// stream less at P0 and at P1.
// Keys: a party in role p holds own = k_p and nxt = k_{p+1}.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "prf_dev.h"
#include "rss_fused.h"

// The walk bodies and element functors are lambdas called once per unrolled element; kept out
// of line they would pin the ChaCha blocks they capture in scratch memory.
#define MX_LAMBDA_INLINE __attribute__((always_inline))

namespace mxp {

using u64 = uint64_t;
using u128 = unsigned __int128;

// keystream chunks of n elements of T
template <class T>
__host__ __device__ constexpr int64_t chunks_of(int64_t n) {
  return (n + mxd::Lane<T>::kPer - 1) / mxd::Lane<T>::kPer;
}

// element j of the chunk in part ``part`` of ChaCha block w
template <class T>
__device__ __forceinline__ T draw(const uint32_t (&w)[16], int part, int j) {
  uint64_t lo, hi;
  mx::part_u64(w, part, &lo, &hi);
  return mxd::pick<T>(lo, hi, j);
}

// body(part, j, i) for the elements i < n of ChaCha block B's four chunks (< nb), P
// elements per chunk, in increasing i.  ``part`` and ``j`` arrive as std::integral_constant
// (the body is a generic lambda), so the block's words are picked by constants and stay in
// registers whatever the unroller decides.
template <int P, int kPart, int kJ = 0, class Body>
__device__ __forceinline__ void walk_chunk(int64_t i0, int64_t n, Body& body) {
  if (i0 + kJ >= n) return;
  body(std::integral_constant<int, kPart>{}, std::integral_constant<int, kJ>{}, i0 + kJ);
  if constexpr (kJ + 1 < P) walk_chunk<P, kPart, kJ + 1>(i0, n, body);
}
template <int P, int kPart = 0, class Body>
__device__ __forceinline__ void walk_block(uint64_t B, int64_t nb, int64_t n, Body&& body) {
  const int64_t b = (int64_t)mx::ks_chunk(B, kPart);
  if (b >= nb) return;
  walk_chunk<P, kPart>(b * P, n, body);
  if constexpr (kPart < 3) walk_block<P, kPart + 1>(B, nb, n, body);
}

// The dealer P2's six streams in nonce order nn = (r0, r1, t, m, z0, z2): k0 is its nxt, k2
// its own.
struct DealerBlocks {
  uint32_t r0[16], r1[16], t[16], m[16], z0[16], z2[16];
};
__device__ __forceinline__ void draw_dealer(const uint32_t* own, const uint32_t* nxt,
                                            const uint64_t (&nn)[6], uint64_t B, DealerBlocks& w) {
  mx::chacha_block(nxt, nn[0], B, w.r0);
  mx::chacha_block(own, nn[1], B, w.r1);
  mx::chacha_block(nxt, nn[2], B, w.t);
  mx::chacha_block(nxt, nn[3], B, w.m);
  mx::chacha_block(nxt, nn[4], B, w.z0);
  mx::chacha_block(own, nn[5], B, w.z2);
}

// Round 0 of the dealer over block B: sink(i, d) gets element i's TruncDeal.
template <class T, class Sink>
__device__ __forceinline__ void dealer_r0(const uint32_t* own, const uint32_t* nxt,
                                          const uint64_t (&nn)[6], int m, uint64_t B, int64_t nb,
                                          int64_t n, Sink&& sink) {
  DealerBlocks w;
  draw_dealer(own, nxt, nn, B, w);
  walk_block<mxd::Lane<T>::kPer>(B, nb, n, [&](auto part, auto j, int64_t i) MX_LAMBDA_INLINE {
    sink(i, mxf::trunc_deal<T>(draw<T>(w.r0, part, j), draw<T>(w.r1, part, j),
                               draw<T>(w.t, part, j), draw<T>(w.m, part, j),
                               draw<T>(w.z0, part, j), draw<T>(w.z2, part, j), m));
  });
}

// Round 0 of P0 / P1 / P2 (role) over block B: msg(i) = the opening message of value(i).
// kZero: the dot tail's form, value(i) masked by the zero share at nonce n_a; TruncPr's own
// form (P0, P1 only) draws the opening mask alone.  nr = (r0, r1).
template <class T, bool kZero, class Value, class Msg>
__device__ __forceinline__ void main_r0(int role, const uint32_t* own, const uint32_t* nxt,
                                        uint64_t n_a, const uint64_t (&nr)[2], uint64_t B,
                                        int64_t nb, int64_t n, Value&& value, Msg&& msg) {
  uint32_t wa[16], wb[16], wr[16];
  if (kZero && role != 1) mx::chacha_block(own, n_a, B, wa);
  if (kZero && role != 0) mx::chacha_block(nxt, n_a, B, wb);
  if (role == 0) mx::chacha_block(own, nr[0], B, wr);
  if (role == 1) mx::chacha_block(nxt, nr[1], B, wr);
  walk_block<mxd::Lane<T>::kPer>(B, nb, n, [&](auto part, auto j, int64_t i) MX_LAMBDA_INLINE {
    const T a = kZero && role != 1 ? draw<T>(wa, part, j) : (T)0;
    const T b = kZero && role != 0 ? draw<T>(wb, part, j) : (T)0;
    const T r = role != 2 ? draw<T>(wr, part, j) : (T)0;
    msg(i) = mxf::trunc_open_msg<T>(role, mxf::zero_masked<T>(value(i), a, b), r);
  });
}

// Round 1 of P0 / P1 (role) over block B: c = opened(i); recv(i, &rt, &rm) reads what P1
// received from the dealer; sink(i, w, z) gets w and the new share z (P0's s0, P1's s1).
// nn = (t, m, z0, z2): P0 draws t, m, z0 under its own k0, P1 z2 under its nxt k2.
template <class T, int kRole, class Opened, class Recv, class Sink>
__device__ __forceinline__ void round1_as(const uint32_t* own, const uint32_t* nxt,
                                          const uint64_t (&nn)[4], int m, uint64_t B, int64_t nb,
                                          int64_t n, Opened&& opened, Recv&& recv, Sink&& sink) {
  uint32_t wt[16], wm[16], wz[16];
  if (kRole == 0) {
    mx::chacha_block(own, nn[0], B, wt);
    mx::chacha_block(own, nn[1], B, wm);
    mx::chacha_block(own, nn[2], B, wz);
  } else {
    mx::chacha_block(nxt, nn[3], B, wz);
  }
  walk_block<mxd::Lane<T>::kPer>(B, nb, n, [&](auto part, auto j, int64_t i) MX_LAMBDA_INLINE {
    T rt, rm;
    if (kRole == 0) {
      rt = draw<T>(wt, part, j);
      rm = draw<T>(wm, part, j);
    } else {
      recv(i, &rt, &rm);
    }
    const T z = draw<T>(wz, part, j);
    sink(i, mxf::trunc_round1_w<T>(kRole, opened(i), rt, rm, z, m), z);
  });
}
template <class T, class Opened, class Recv, class Sink>
__device__ __forceinline__ void round1(int role, const uint32_t* own, const uint32_t* nxt,
                                       const uint64_t (&nn)[4], int m, uint64_t B, int64_t nb,
                                       int64_t n, Opened&& opened, Recv&& recv, Sink&& sink) {
  if (role == 0)
    round1_as<T, 0>(own, nxt, nn, m, B, nb, n, opened, recv, sink);
  else
    round1_as<T, 1>(own, nxt, nn, m, B, nb, n, opened, recv, sink);
}

// ---- launches ----
inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -100 - (int)e;
}

// launch(T{}) for the ring width of ``words`` (1: u64, 2: u128), then the launch status
template <class Launch>
inline int for_width(int words, Launch&& launch) {
  if (words == 1)
    launch(u64{});
  else if (words == 2)
    launch(u128{});
  else
    return -2;
  return launch_status();
}

}  // namespace mxp
