// Per-party protocol kernels for layouts where the three parties of a session sit on
// DIFFERENT GPUs (moose_amd/parallel/cyclic.py): a GPU stacks one party of each of up to
// three sessions, component c playing role roles[c].  Each kernel does every stacked
// role's local work of one protocol round in one pass; the messages between rounds go
// over RCCL.  Same PRF keys / nonces / counters as the generic protocol code, so the shares
// are bitwise equal to it (and to the single-GPU fused kernels of rss_fused.hip).
//
// The TruncPr and dot-tail rounds, the streams each role draws and the round bodies are in
// party_rounds.h (one element's arithmetic: rss_fused.h); the kernels here say where a
// component's elements are read and written.  Share by member j: one kernel computing every
// role's two slots (the owner's masked x_j is then sent to P_{j+2}).
// Key slots: component c passes (own k_p, next k_{p+1}[, k_all]) of its session.
#include <hip/hip_runtime.h>

#include "moosex.h"
#include "party_abi.h"
#include "party_batch.h"
#include "party_rounds.h"
#include "prf_dev.h"
#include "ring_common.h"
#include "rss_fused.h"

using u64 = uint64_t;
using u128 = unsigned __int128;

namespace {

struct Roles {
  int r[3];
};

// Each thread walks ChaCha blocks (prf_dev.h) of one component: g = c * nblk + B, and the
// body runs for the block's chunks b = ks_chunk(B, part).
#define MX_PARTY_WALK(NB, NCOMP)                                                    \
  const int64_t nblk = (int64_t)mx::ks_blocks_for((uint64_t)(NB));               \
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < nblk * (NCOMP); \
       g += (int64_t)gridDim.x * blockDim.x)

template <class T>
__device__ __forceinline__ void d_trunc_party_r0(int64_t n, int m, const Roles& roles,
                                                 const T* __restrict__ s0, const T* __restrict__ s1,
                                                 T* __restrict__ msg, u64* __restrict__ msg_rm,
                                                 T* __restrict__ out0, T* __restrict__ out1,
                                                 const mxd::KeySrc& keys, uint64_t n_r0,
                                                 uint64_t n_r1, uint64_t n_t, uint64_t n_m,
                                                 uint64_t n_z0, uint64_t n_z2, int ncomp) {
  __shared__ uint32_t rks[mxd::kMaxKeySlots][mxd::kKeyWords];
  mxd::stage_keys(rks, keys, 2 * ncomp);
  const int64_t nb = mxp::chunks_of<T>(n);
  const uint64_t nn[6] = {n_r0, n_r1, n_t, n_m, n_z0, n_z2}, nr[2] = {n_r0, n_r1};
  MX_PARTY_WALK(nb, ncomp) {
    const int c = (int)(g / nblk);
    const uint64_t B = (uint64_t)(g - c * nblk);
    const int role = roles.r[c];
    const uint32_t* own = rks[2 * c];
    const uint32_t* nxt = rks[2 * c + 1];
    const int64_t base = (int64_t)c * n;
    if (role == 0 || role == 1) {  // P0's part of the value is x0 + x1, P1's x2
      mxp::main_r0<T, false>(
          role, own, nxt, 0, nr, B, nb, n,
          [&](int64_t i) MX_LAMBDA_INLINE {
            return role == 0 ? (T)(s0[base + i] + s1[base + i]) : s1[base + i];
          },
          [&](int64_t i) MX_LAMBDA_INLINE -> T& { return msg[base + i]; });
    } else if (role == 2) {
      mxp::dealer_r0<T>(own, nxt, nn, m, B, nb, n,
                        [&](int64_t i, const mxf::TruncDeal<T>& d) MX_LAMBDA_INLINE {
                          msg[base + i] = d.rt1;
                          msg_rm[base + i] = d.rm1;
                          out0[base + i] = d.s0;
                          out1[base + i] = d.s1;
                        });
    }
  }
}

template <class T>
__global__ void __launch_bounds__(256) k_trunc_party_r0(int64_t n, int m, Roles roles,
                                                        const T* __restrict__ s0,
                                                        const T* __restrict__ s1,
                                                        T* __restrict__ msg,
                                                        u64* __restrict__ msg_rm,
                                                        T* __restrict__ out0, T* __restrict__ out1,
                                                        mxd::KeySrc keys, uint64_t n_r0,
                                                        uint64_t n_r1, uint64_t n_t, uint64_t n_m,
                                                        uint64_t n_z0, uint64_t n_z2, int ncomp) {
  d_trunc_party_r0<T>(n, m, roles, s0, s1, msg, msg_rm, out0, out1, keys, n_r0, n_r1, n_t, n_m,
                      n_z0, n_z2, ncomp);
}

// Round 1 of every stacked component in role 0 / 1.  at(c): the component's R1Args; a null
// z2m is TruncPr's own two-term opening c = mine + other, else the dot tail's three-term one.
template <class T>
struct R1Args {
  const T* mine;
  const T* other;
  const T* z2m;
  const T* rt;
  const u64* rm;
  T* w;
  T* o0;
  T* o1;
};

template <class T, class At>
__device__ __forceinline__ void party_round1(int64_t n, int m, const Roles& roles,
                                             const mxd::KeySrc& keys, uint64_t n_t, uint64_t n_m,
                                             uint64_t n_z0, uint64_t n_z2, int ncomp, At&& at) {
  __shared__ uint32_t rks[mxd::kMaxKeySlots][mxd::kKeyWords];
  mxd::stage_keys(rks, keys, 2 * ncomp);
  const int64_t nb = mxp::chunks_of<T>(n);
  const uint64_t nn[4] = {n_t, n_m, n_z0, n_z2};
  MX_PARTY_WALK(nb, ncomp) {
    const int c = (int)(g / nblk);
    const uint64_t B = (uint64_t)(g - c * nblk);
    const int role = roles.r[c];
    if (role != 0 && role != 1) continue;
    const R1Args<T> a = at(c);
    T* o = role == 0 ? a.o0 : a.o1;
    mxp::round1<T>(
        role, rks[2 * c], rks[2 * c + 1], nn, m, B, nb, n,
        [&](int64_t i) MX_LAMBDA_INLINE {
          T cc = a.mine[i] + a.other[i];
          if (a.z2m != nullptr) cc += a.z2m[i];
          return cc;
        },
        [&](int64_t i, T* rt, T* rm) MX_LAMBDA_INLINE {
          *rt = a.rt[i];
          *rm = (T)a.rm[i];
        },
        [&](int64_t i, T w, T z) MX_LAMBDA_INLINE {
          a.w[i] = w;
          o[i] = z;
        });
  }
}

template <class T>
__device__ __forceinline__ void d_trunc_party_r1(int64_t n, int m, const Roles& roles,
                                                 const T* __restrict__ msg,
                                                 const T* __restrict__ rmk,
                                                 const T* __restrict__ rrt,
                                                 const u64* __restrict__ rrm, T* __restrict__ w,
                                                 T* __restrict__ out0, T* __restrict__ out1,
                                                 const mxd::KeySrc& keys, uint64_t n_t,
                                                 uint64_t n_m, uint64_t n_z0, uint64_t n_z2,
                                                 int ncomp) {
  party_round1<T>(n, m, roles, keys, n_t, n_m, n_z0, n_z2, ncomp, [&](int c) {
    const int64_t base = (int64_t)c * n;
    return R1Args<T>{msg + base, rmk + base, nullptr,     rrt + base,
                     rrm + base, w + base,   out0 + base, out1 + base};
  });
}

template <class T>
__global__ void __launch_bounds__(256) k_trunc_party_r1(int64_t n, int m, Roles roles,
                                                        const T* __restrict__ msg,
                                                        const T* __restrict__ rmk,
                                                        const T* __restrict__ rrt,
                                                        const u64* __restrict__ rrm,
                                                        T* __restrict__ w, T* __restrict__ out0,
                                                        T* __restrict__ out1, mxd::KeySrc keys,
                                                        uint64_t n_t, uint64_t n_m, uint64_t n_z0,
                                                        uint64_t n_z2, int ncomp) {
  d_trunc_party_r1<T>(n, m, roles, msg, rmk, rrt, rrm, w, out0, out1, keys, n_t, n_m, n_z0, n_z2,
                      ncomp);
}

// Ring extension Z_2^64 -> Z_2^128 (dealer P2; rss_fused.h: ring_extend_deal / _mask0 /
// _round1_w), rounds and streams as TruncPr's:
//   r0: P0 msg = x0 + x1 + 2^62 + r0 (u64)        -> P1
//       P1 msg = x2 + r1 (u64)                     -> P0
//       P2 R1 (u128), M1 (u64)                     -> P1;  P2's new shares (z2, z0)
//   r1: P0 c = msg + rmk, w0 = y0 - z0             -> P1;  P0's s0 = z0
//       P1 c = msg + rmk, w1 = y1 - z2             -> P0;  P1's s1 = z2
//   r2: z1 = w0 + w1 (elementwise, host side)
// All six streams are drawn at 128-bit lane width, one chunk per element, as k_ring_extend3
// and additive.ring_extend draw them (r0, r1, M0 use the low 64 bits of their lane): the
// walk is over n chunks although the input is u64.
__device__ __forceinline__ void d_ring_extend_party_r0(
    int64_t n, const Roles& roles, const u64* __restrict__ s0, const u64* __restrict__ s1,
    u64* __restrict__ msg, u128* __restrict__ msg_R, u64* __restrict__ msg_M,
    u128* __restrict__ out0, u128* __restrict__ out1, const mxd::KeySrc& keys, uint64_t n_r0,
    uint64_t n_r1, uint64_t n_R, uint64_t n_M, uint64_t n_z0, uint64_t n_z2, int ncomp) {
  __shared__ uint32_t rks[mxd::kMaxKeySlots][mxd::kKeyWords];
  mxd::stage_keys(rks, keys, 2 * ncomp);
  const uint64_t nn[6] = {n_r0, n_r1, n_R, n_M, n_z0, n_z2};
  MX_PARTY_WALK(n, ncomp) {
    const int c = (int)(g / nblk);
    const uint64_t B = (uint64_t)(g - c * nblk);
    const int role = roles.r[c];
    const uint32_t* own = rks[2 * c];
    const uint32_t* nxt = rks[2 * c + 1];
    const int64_t base = (int64_t)c * n;
    if (role == 0 || role == 1) {  // r0 under k0 = P0's own, r1 under k2 = P1's next
      uint32_t wa[16];
      mx::chacha_block(role == 0 ? own : nxt, role == 0 ? n_r0 : n_r1, B, wa);
      mxp::walk_block<1>(B, n, n, [&](auto part, auto, int64_t i) MX_LAMBDA_INLINE {
        const u64 r = (u64)mxp::draw<u128>(wa, part, 0);
        msg[base + i] = role == 0 ? mxf::ring_extend_mask0(s0[base + i], s1[base + i], r)
                                  : s1[base + i] + r;
      });
    } else if (role == 2) {
      mxp::DealerBlocks w;
      mxp::draw_dealer(own, nxt, nn, B, w);
      mxp::walk_block<1>(B, n, n, [&](auto part, auto, int64_t i) MX_LAMBDA_INLINE {
        const mxf::RingExtendDeal d = mxf::ring_extend_deal(
            mxp::draw<u128>(w.r0, part, 0), mxp::draw<u128>(w.r1, part, 0),
            mxp::draw<u128>(w.t, part, 0), mxp::draw<u128>(w.m, part, 0),
            mxp::draw<u128>(w.z0, part, 0), mxp::draw<u128>(w.z2, part, 0));
        msg_R[base + i] = d.R1;
        msg_M[base + i] = d.M1;
        out0[base + i] = d.s0;
        out1[base + i] = d.s1;
      });
    }
  }
}

__global__ void __launch_bounds__(256) k_ring_extend_party_r0(
    int64_t n, Roles roles, const u64* __restrict__ s0, const u64* __restrict__ s1,
    u64* __restrict__ msg, u128* __restrict__ msg_R, u64* __restrict__ msg_M,
    u128* __restrict__ out0, u128* __restrict__ out1, mxd::KeySrc keys, uint64_t n_r0,
    uint64_t n_r1, uint64_t n_R, uint64_t n_M, uint64_t n_z0, uint64_t n_z2, int ncomp) {
  d_ring_extend_party_r0(n, roles, s0, s1, msg, msg_R, msg_M, out0, out1, keys, n_r0, n_r1, n_R,
                         n_M, n_z0, n_z2, ncomp);
}

__device__ __forceinline__ void d_ring_extend_party_r1(
    int64_t n, const Roles& roles, const u64* __restrict__ msg, const u64* __restrict__ rmk,
    const u128* __restrict__ rR, const u64* __restrict__ rM, u128* __restrict__ w,
    u128* __restrict__ out0, u128* __restrict__ out1, const mxd::KeySrc& keys, uint64_t n_R,
    uint64_t n_M, uint64_t n_z0, uint64_t n_z2, int ncomp) {
  __shared__ uint32_t rks[mxd::kMaxKeySlots][mxd::kKeyWords];
  mxd::stage_keys(rks, keys, 2 * ncomp);
  MX_PARTY_WALK(n, ncomp) {
    const int c = (int)(g / nblk);
    const uint64_t B = (uint64_t)(g - c * nblk);
    const int role = roles.r[c];
    const int64_t base = (int64_t)c * n;
    if (role == 0) {  // R0, M0, z0 under its own k0
      const uint32_t* k0 = rks[2 * c];
      uint32_t wR[16], wM[16], wz[16];
      mx::chacha_block(k0, n_R, B, wR);
      mx::chacha_block(k0, n_M, B, wM);
      mx::chacha_block(k0, n_z0, B, wz);
      mxp::walk_block<1>(B, n, n, [&](auto part, auto, int64_t i) MX_LAMBDA_INLINE {
        const int64_t k = base + i;
        const u64 cc = msg[k] + rmk[k];
        uint64_t Rl, Rh, ml, mh, zl, zh;
        mx::part_u64(wR, part, &Rl, &Rh);
        mx::part_u64(wM, part, &ml, &mh);
        mx::part_u64(wz, part, &zl, &zh);
        const u128 z0 = mxd::pick<u128>(zl, zh, 0);
        w[k] = mxf::ring_extend_round1_w(0, cc, mxd::pick<u128>(Rl, Rh, 0), ml, z0);
        out0[k] = z0;
      });
    } else if (role == 1) {  // z2 under its next k2
      uint32_t wz[16];
      mx::chacha_block(rks[2 * c + 1], n_z2, B, wz);
      mxp::walk_block<1>(B, n, n, [&](auto part, auto, int64_t i) MX_LAMBDA_INLINE {
        const int64_t k = base + i;
        const u64 cc = msg[k] + rmk[k];
        const u128 z2 = mxp::draw<u128>(wz, part, 0);
        w[k] = mxf::ring_extend_round1_w(1, cc, rR[k], rM[k], z2);
        out1[k] = z2;
      });
    }
  }
}

__global__ void __launch_bounds__(256) k_ring_extend_party_r1(
    int64_t n, Roles roles, const u64* __restrict__ msg, const u64* __restrict__ rmk,
    const u128* __restrict__ rR, const u64* __restrict__ rM, u128* __restrict__ w,
    u128* __restrict__ out0, u128* __restrict__ out1, mxd::KeySrc keys, uint64_t n_R,
    uint64_t n_M, uint64_t n_z0, uint64_t n_z2, int ncomp) {
  d_ring_extend_party_r1(n, roles, msg, rmk, rR, rM, w, out0, out1, keys, n_R, n_M, n_z0, n_z2,
                         ncomp);
}

template <class T>
__device__ __forceinline__ void d_share_party(int kind, int64_t n, const Roles& rel,
                                              const void* __restrict__ xv, T* __restrict__ out0,
                                              T* __restrict__ out1, const mxd::KeySrc& keys,
                                              uint64_t n1, uint64_t na, int ncomp) {
  const bool mir = kind & MX_SHARE_MIRROR;
  kind &= ~MX_SHARE_MIRROR;
  const T* x = (const T*)xv;
  const double* xf = (const double*)xv;  // kind MX_SHARE_F64: encode in the kernel
  const double scale = kind == MX_SHARE_F64 ? ldexp(1.0, (int)na) : 0.0;
  __shared__ uint32_t rks[mxd::kMaxKeySlots][mxd::kKeyWords];
  // keys: 2 per component, the first used: k_j of the owner j (rel 0: own, rel 2: next).
  // As the reference (replicated/convert.rs:74-90): slot j = PRF(k_j), slot j+1 = x - slot j
  // (sent to P_{j+1}), slot j+2 = 0, so rel 1 draws nothing.  Mirrored (MX_SHARE_MIRROR):
  // slot j+1 = PRF(k_{j+1}) (rel 0: next, rel 1: own), slot j = x - slot j+1 (sent to
  // P_{j+2}), slot j+2 = 0, so rel 2 draws nothing
  mxd::stage_keys(rks, keys, 2 * ncomp);
  const int64_t nb = mxp::chunks_of<T>(n);
  MX_PARTY_WALK(nb, ncomp) {
    const int c = (int)(g / nblk);
    const uint64_t B = (uint64_t)(g - c * nblk);
    // rel code: the role relative to the owner (0..2) + 4 * (1 + the component of the
    // recipient P_{j+1}, mirrored P_{j+2}) when the owner's masked share stays on this device
    // (written straight into its s0, mirrored its s1)
    const int code = rel.r[c];
    if (code < 0) continue;
    const int r = code & 3, fwd = (code >> 2) - 1;
    const int64_t base = (int64_t)c * n;
    if (r > 2) continue;
    const bool draws = mir ? r != 2 : r != 1;
    uint32_t wa[16];
    if (draws) mx::chacha_block(rks[2 * c], n1, B, wa);
    constexpr int P = mxd::Lane<T>::kPer;
    mxp::walk_block<P>(B, nb, n, [&](auto part, auto j, int64_t i) MX_LAMBDA_INLINE {
      const T rr = draws ? mxp::draw<T>(wa, part, j) : (T)0;
      if (r == 0) {  // owner: (PRF(k_j), x - PRF(k_j)); mirrored (x - PRF(k_{j+1}), PRF)
        const T xi = kind == MX_SHARE_F64 ? mxr::f64_to_ring<T>(xf[i] * scale) : x[i];
        const T v = kind == MX_CROSS_BOOL ? (T)(xi ^ rr) : (T)(xi - rr);
        out0[base + i] = mir ? v : rr;
        out1[base + i] = mir ? rr : v;
        if (fwd >= 0) (mir ? out1 : out0)[(int64_t)fwd * n + i] = v;
      } else if (r == 1) {  // P_{j+1}: (received, 0); mirrored (PRF(k_{j+1}), 0)
        if (mir) out0[base + i] = rr;
        out1[base + i] = 0;
      } else {  // P_{j+2}: (0, PRF(k_j)); mirrored (0, received)
        out0[base + i] = 0;
        if (!mir) out1[base + i] = rr;
      }
    });
  }
}

template <class T>
__global__ void __launch_bounds__(256) k_share_party(int kind, int64_t n, Roles rel,
                                                     const void* __restrict__ xv,
                                                     T* __restrict__ out0, T* __restrict__ out1,
                                                     mxd::KeySrc keys, uint64_t n1, uint64_t na,
                                                     int ncomp) {
  d_share_party<T>(kind, n, rel, xv, out0, out1, keys, n1, na, ncomp);
}

// ---------------------------------------------------------------------------------------
// Fixed-point dot tail (rep.dot_trunc; party_rounds.h) for parties on different GPUs.
// Input: each party's local cross products (the RSS dot's GEMM output).  Round 1 is
// TruncPr's with the three-term c; round 2 adds the exchanged w's.  Every array argument is
// a per-component pointer triple (component slots need not be adjacent: rows of a larger
// stack, buffers received from other GPUs, or -- one party per process at N = 1 -- the
// sender's buffer).
// ---------------------------------------------------------------------------------------
struct CP3 {
  const void* p[3];
};
struct WP3 {
  void* p[3];
};

template <class T>
__device__ __forceinline__ const T* cp(const CP3& a, int c) {
  return (const T*)a.p[c];
}
template <class T>
__device__ __forceinline__ T* wp(const WP3& a, int c) {
  return (T*)a.p[c];
}

template <class T>
__device__ __forceinline__ void d_dot_tail_r0(int64_t n, int m, const Roles& roles,
                                              const CP3& cross, const WP3& msg, const WP3& msg_rt,
                                              const WP3& msg_rm, const WP3& out0, const WP3& out1,
                                              const mxd::KeySrc& keys, uint64_t n_a, uint64_t n_r0,
                                              uint64_t n_r1, uint64_t n_t, uint64_t n_m,
                                              uint64_t n_z0, uint64_t n_z2, int ncomp) {
  __shared__ uint32_t rks[mxd::kMaxKeySlots][mxd::kKeyWords];
  mxd::stage_keys(rks, keys, 2 * ncomp);
  const int64_t nb = mxp::chunks_of<T>(n);
  const uint64_t nn[6] = {n_r0, n_r1, n_t, n_m, n_z0, n_z2}, nr[2] = {n_r0, n_r1};
  MX_PARTY_WALK(nb, ncomp) {
    const int c = (int)(g / nblk);
    const uint64_t B = (uint64_t)(g - c * nblk);
    const int role = roles.r[c];
    if (role < 0 || role > 2) continue;
    const uint32_t* own = rks[2 * c];
    const uint32_t* nxt = rks[2 * c + 1];
    const T* x = cp<T>(cross, c);
    T* mo = wp<T>(msg, c);
    // no cross (null): the dealer part only, launched before the product exists, so P2's
    // rt1 / rm1 travel while the GEMM runs; no msg_rt (null): no dealer part
    if (x != nullptr)
      mxp::main_r0<T, true>(
          role, own, nxt, n_a, nr, B, nb, n, [&](int64_t i) MX_LAMBDA_INLINE { return x[i]; },
          [&](int64_t i) MX_LAMBDA_INLINE -> T& { return mo[i]; });
    if (role == 2 && msg_rt.p[c] != nullptr) {
      T* rt = wp<T>(msg_rt, c);
      u64* rm = wp<u64>(msg_rm, c);
      T* o0 = wp<T>(out0, c);
      T* o1 = wp<T>(out1, c);
      mxp::dealer_r0<T>(own, nxt, nn, m, B, nb, n,
                        [&](int64_t i, const mxf::TruncDeal<T>& d) MX_LAMBDA_INLINE {
                          rt[i] = d.rt1;
                          rm[i] = d.rm1;
                          o0[i] = d.s0;
                          o1[i] = d.s1;
                        });
    }
  }
}

template <class T>
__global__ void __launch_bounds__(256) k_dot_tail_r0(int64_t n, int m, Roles roles, CP3 cross,
                                                     WP3 msg, WP3 msg_rt, WP3 msg_rm, WP3 out0,
                                                     WP3 out1, mxd::KeySrc keys, uint64_t n_a,
                                                     uint64_t n_r0, uint64_t n_r1, uint64_t n_t,
                                                     uint64_t n_m, uint64_t n_z0, uint64_t n_z2,
                                                     int ncomp) {
  d_dot_tail_r0<T>(n, m, roles, cross, msg, msg_rt, msg_rm, out0, out1, keys, n_a, n_r0, n_r1, n_t,
                   n_m, n_z0, n_z2, ncomp);
}

// P0 / P1: c = own message + the other's + z2 (a null rz component: the two-term opening)
template <class T>
__device__ __forceinline__ void d_dot_tail_r1(int64_t n, int m, const Roles& roles, const CP3& msg,
                                              const CP3& rmk, const CP3& rz, const CP3& rrt,
                                              const CP3& rrm, const WP3& w, const WP3& out0,
                                              const WP3& out1, const mxd::KeySrc& keys,
                                              uint64_t n_t, uint64_t n_m, uint64_t n_z0,
                                              uint64_t n_z2, int ncomp) {
  party_round1<T>(n, m, roles, keys, n_t, n_m, n_z0, n_z2, ncomp, [&](int c) {
    return R1Args<T>{cp<T>(msg, c),   cp<T>(rmk, c), cp<T>(rz, c),   cp<T>(rrt, c),
                     cp<u64>(rrm, c), wp<T>(w, c),   wp<T>(out0, c), wp<T>(out1, c)};
  });
}

template <class T>
__global__ void __launch_bounds__(256) k_dot_tail_r1(int64_t n, int m, Roles roles, CP3 msg,
                                                     CP3 rmk, CP3 rz, CP3 rrt, CP3 rrm, WP3 w,
                                                     WP3 out0, WP3 out1, mxd::KeySrc keys,
                                                     uint64_t n_t, uint64_t n_m, uint64_t n_z0,
                                                     uint64_t n_z2, int ncomp) {
  d_dot_tail_r1<T>(n, m, roles, msg, rmk, rz, rrt, rrm, w, out0, out1, keys, n_t, n_m, n_z0, n_z2,
                   ncomp);
}

// out[c] = a[c] + b[c] for the components in role 0 or 1 (P0's s1, P1's s0 = w0 + w1)
template <class T>
__device__ __forceinline__ void d_dot_tail_r2(int64_t n, const Roles& roles, const CP3& a,
                                              const CP3& b, const WP3& out, int ncomp) {
  const int64_t total = n * ncomp;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < total;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(g / n);
    const int64_t i = g - (int64_t)c * n;
    const int role = roles.r[c];
    if (role != 0 && role != 1) continue;
    wp<T>(out, c)[i] = cp<T>(a, c)[i] + cp<T>(b, c)[i];
  }
}

template <class T>
__global__ void __launch_bounds__(256) k_dot_tail_r2(int64_t n, Roles roles, CP3 a, CP3 b, WP3 out,
                                                     int ncomp) {
  d_dot_tail_r2<T>(n, roles, a, b, out, ncomp);
}

// party-batched twins for the composed one-GPU replay (party_batch.h)
MX_X3(k_trunc_party_r0<u64>, d_trunc_party_r0<u64>);
MX_X3(k_trunc_party_r0<u128>, d_trunc_party_r0<u128>);
MX_X3(k_trunc_party_r1<u64>, d_trunc_party_r1<u64>);
MX_X3(k_trunc_party_r1<u128>, d_trunc_party_r1<u128>);
MX_X3(k_ring_extend_party_r0, d_ring_extend_party_r0);
MX_X3(k_ring_extend_party_r1, d_ring_extend_party_r1);
MX_X3(k_share_party<u64>, d_share_party<u64>);
MX_X3(k_share_party<u128>, d_share_party<u128>);
MX_X3(k_dot_tail_r0<u64>, d_dot_tail_r0<u64>);
MX_X3(k_dot_tail_r0<u128>, d_dot_tail_r0<u128>);
MX_X3(k_dot_tail_r1<u64>, d_dot_tail_r1<u64>);
MX_X3(k_dot_tail_r1<u128>, d_dot_tail_r1<u128>);
MX_X3(k_dot_tail_r2<u64>, d_dot_tail_r2<u64>);
MX_X3(k_dot_tail_r2<u128>, d_dot_tail_r2<u128>);

inline CP3 cp3(const void* const* a, int ncomp) {
  CP3 o{{nullptr, nullptr, nullptr}};
  if (a)
    for (int c = 0; c < ncomp; ++c) o.p[c] = a[c];
  return o;
}
inline WP3 wp3(void* const* a, int ncomp) {
  WP3 o{{nullptr, nullptr, nullptr}};
  if (a)
    for (int c = 0; c < ncomp; ++c) o.p[c] = a[c];
  return o;
}

// The head of every entry point: the launch's roles and key source (slots may be null: a
// kernel without PRF).  False: the entry point returns *rc (nothing to do, bad ncomp).
inline bool party_args(int64_t n, int ncomp, const int* roles, const uint32_t* const* slots,
                       Roles* rr, mxd::KeySrc* keys, int* rc) {
  *rc = n == 0 ? 0 : -3;
  if (n == 0 || ncomp < 1 || ncomp > 3) return false;
  if (slots != nullptr) *keys = mxd::keysrc_slots(slots, 2 * ncomp);
  for (int c = 0; c < 3; ++c) rr->r[c] = c < ncomp ? roles[c] : -1;
  return true;
}

// grid of a walk over the chunks of n elements of T for ncomp stacked components
template <class T>
inline dim3 party_grid(int64_t n, int ncomp) {
  return dim3(mxd::grid_for_chunks(mxp::chunks_of<T>(n)) * ncomp);
}

}  // namespace

extern "C" {

int mxh_trunc_party_r0(int words, int64_t n, int m, int ncomp, const int* roles,
                       const void* s0, const void* s1, void* msg, void* msg_rm, void* out0,
                       void* out1, const uint32_t* const* slots, const uint64_t* nn,
                       void* stream) {
  Roles rr;
  mxd::KeySrc k;
  int rc;
  if (!party_args(n, ncomp, roles, slots, &rr, &k, &rc)) return rc;
  return mxp::for_width(words, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_trunc_party_r0<T>, party_grid<T>(n, ncomp), dim3(256), 0,
                       (hipStream_t)stream, n, m, rr, (const T*)s0, (const T*)s1, (T*)msg,
                       (u64*)msg_rm, (T*)out0, (T*)out1, k, nn[0], nn[1], nn[2], nn[3], nn[4],
                       nn[5], ncomp);
  });
}

int mxh_trunc_party_r1(int words, int64_t n, int m, int ncomp, const int* roles,
                       const void* msg, const void* rmk, const void* rrt, const void* rrm,
                       void* w, void* out0, void* out1, const uint32_t* const* slots,
                       const uint64_t* nn, void* stream) {
  Roles rr;
  mxd::KeySrc k;
  int rc;
  if (!party_args(n, ncomp, roles, slots, &rr, &k, &rc)) return rc;
  return mxp::for_width(words, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_trunc_party_r1<T>, party_grid<T>(n, ncomp), dim3(256), 0,
                       (hipStream_t)stream, n, m, rr, (const T*)msg, (const T*)rmk,
                       (const T*)rrt, (const u64*)rrm, (T*)w, (T*)out0, (T*)out1, k, nn[2], nn[3],
                       nn[4], nn[5], ncomp);
  });
}

int mxh_ring_extend_party_r0(int64_t n, int ncomp, const int* roles, const void* s0,
                             const void* s1, void* msg, void* msg_R, void* msg_M, void* out0,
                             void* out1, const uint32_t* const* slots, const uint64_t* nn,
                             void* stream) {
  Roles rr;
  mxd::KeySrc k;
  int rc;
  if (!party_args(n, ncomp, roles, slots, &rr, &k, &rc)) return rc;
  hipLaunchKernelGGL(k_ring_extend_party_r0, party_grid<u128>(n, ncomp), dim3(256), 0,
                     (hipStream_t)stream, n, rr, (const u64*)s0, (const u64*)s1, (u64*)msg,
                     (u128*)msg_R, (u64*)msg_M, (u128*)out0, (u128*)out1, k, nn[0], nn[1], nn[2],
                     nn[3], nn[4], nn[5], ncomp);
  return mxp::launch_status();
}

int mxh_ring_extend_party_r1(int64_t n, int ncomp, const int* roles, const void* msg,
                             const void* rmk, const void* rR, const void* rM, void* w,
                             void* out0, void* out1, const uint32_t* const* slots,
                             const uint64_t* nn, void* stream) {
  Roles rr;
  mxd::KeySrc k;
  int rc;
  if (!party_args(n, ncomp, roles, slots, &rr, &k, &rc)) return rc;
  hipLaunchKernelGGL(k_ring_extend_party_r1, party_grid<u128>(n, ncomp), dim3(256), 0,
                     (hipStream_t)stream, n, rr, (const u64*)msg, (const u64*)rmk,
                     (const u128*)rR, (const u64*)rM, (u128*)w, (u128*)out0, (u128*)out1, k,
                     nn[2], nn[3], nn[4], nn[5], ncomp);
  return mxp::launch_status();
}

int mxh_share_party(int kind, int words, int64_t n, int ncomp, const int* rel, const void* x,
                    void* out0, void* out1, const uint32_t* const* slots, uint64_t n1,
                    uint64_t na, void* stream) {
  Roles rr;
  mxd::KeySrc k;
  int rc;
  if (!party_args(n, ncomp, rel, slots, &rr, &k, &rc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (words == 0) {  // bits: no u64 / u128 pair
    hipLaunchKernelGGL(k_share_party<uint8_t>, party_grid<uint8_t>(n, ncomp), dim3(256), 0, st,
                       kind, n, rr, x, (uint8_t*)out0, (uint8_t*)out1, k, n1, na, ncomp);
    return mxp::launch_status();
  }
  return mxp::for_width(words, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_share_party<T>, party_grid<T>(n, ncomp), dim3(256), 0, st, kind, n, rr,
                       x, (T*)out0, (T*)out1, k, n1, na, ncomp);
  });
}

int mxh_dot_tail_r0(int words, int64_t n, int m, int ncomp, const int* roles,
                    const void* const* cross, void* const* msg, void* const* msg_rt,
                    void* const* msg_rm, void* const* out0, void* const* out1,
                    const uint32_t* const* slots, const uint64_t* nn, void* stream) {
  Roles rr;
  mxd::KeySrc k;
  int rc;
  if (!party_args(n, ncomp, roles, slots, &rr, &k, &rc)) return rc;
  const CP3 x = cp3(cross, ncomp);
  const WP3 mo = wp3(msg, ncomp), rt = wp3(msg_rt, ncomp), rm = wp3(msg_rm, ncomp),
            o0 = wp3(out0, ncomp), o1 = wp3(out1, ncomp);
  return mxp::for_width(words, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_dot_tail_r0<T>, party_grid<T>(n, ncomp), dim3(256), 0,
                       (hipStream_t)stream, n, m, rr, x, mo, rt, rm, o0, o1, k, nn[0], nn[1],
                       nn[2], nn[3], nn[4], nn[5], nn[6], ncomp);
  });
}

int mxh_dot_tail_r1(int words, int64_t n, int m, int ncomp, const int* roles,
                    const void* const* msg, const void* const* rmk, const void* const* rz,
                    const void* const* rrt, const void* const* rrm, void* const* w,
                    void* const* out0, void* const* out1, const uint32_t* const* slots,
                    const uint64_t* nn, void* stream) {
  Roles rr;
  mxd::KeySrc k;
  int rc;
  if (!party_args(n, ncomp, roles, slots, &rr, &k, &rc)) return rc;
  const CP3 a = cp3(msg, ncomp), b = cp3(rmk, ncomp), z = cp3(rz, ncomp), t = cp3(rrt, ncomp),
            r = cp3(rrm, ncomp);
  const WP3 wo = wp3(w, ncomp), o0 = wp3(out0, ncomp), o1 = wp3(out1, ncomp);
  return mxp::for_width(words, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(k_dot_tail_r1<T>, party_grid<T>(n, ncomp), dim3(256), 0,
                       (hipStream_t)stream, n, m, rr, a, b, z, t, r, wo, o0, o1, k, nn[3], nn[4],
                       nn[5], nn[6], ncomp);
  });
}

int mxh_dot_tail_r2(int words, int64_t n, int ncomp, const int* roles, const void* const* a,
                    const void* const* b, void* const* out, void* stream) {
  Roles rr;
  int rc;
  if (!party_args(n, ncomp, roles, nullptr, &rr, nullptr, &rc)) return rc;
  const CP3 x = cp3(a, ncomp), y = cp3(b, ncomp);
  const WP3 o = wp3(out, ncomp);
  return mxp::for_width(words, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_dot_tail_r2<T>, dim3(mxd::grid_for(n * ncomp)), dim3(256), 0,
                       (hipStream_t)stream, n, rr, x, y, o, ncomp);
  });
}

}  // extern "C"
