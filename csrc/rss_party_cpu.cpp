// Host versions of the per-party protocol kernels (rss_party.hip) and the C ABI entry
// points that dispatch host / device.  Key slots are MX_KEY_SLOT_WORDS-word images whose
// first four words are the raw AES key.
#include <cmath>

#include "moosex.h"
#include "party_abi.h"
#include "party_rounds_cpu.h"
#include "ring_common.h"
#include "rss_fused.h"

namespace {

using u64 = uint64_t;
using u128 = unsigned __int128;
using mxc::for_chunks;
using mxc::prf;

// the dealer's outputs of one component
template <class T>
auto deal_out(T* rt, u64* rm, T* o0, T* o1) {
  return [=](int64_t i, const mxf::TruncDeal<T>& d) {
    rt[i] = d.rt1;
    rm[i] = d.rm1;
    o0[i] = d.s0;
    o1[i] = d.s1;
  };
}

template <class T>
int trunc_r0(int64_t n, int m, int ncomp, const int* roles, const T* s0, const T* s1, T* msg,
             u64* msg_rm, T* out0, T* out1, const uint32_t* const* slots, const uint64_t* nn) {
  for (int c = 0; c < ncomp; ++c) {
    const int role = roles[c];
    const uint32_t* own = slots[2 * c];
    const uint32_t* nxt = slots[2 * c + 1];
    const int64_t base = (int64_t)c * n;
    for_chunks(n, [&](int64_t i0, int64_t len) {
      if (role == 0 || role == 1)  // P0's part of the value is x0 + x1, P1's x2
        mxc::main_r0<T>(
            false, role, own, nxt, 0, nn, i0, len,
            [&](int64_t i) { return role == 0 ? (T)(s0[base + i] + s1[base + i]) : s1[base + i]; },
            [&](int64_t i) -> T& { return msg[base + i]; });
      else if (role == 2)
        mxc::dealer_r0<T>(own, nxt, nn, m, i0, len,
                          deal_out<T>(msg + base, msg_rm + base, out0 + base, out1 + base));
    });
  }
  return 0;
}

// Round 1 of every component in role 0 / 1 (rss_party.hip party_round1): a null z2m is
// TruncPr's own two-term opening, else the dot tail's three-term one.
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
int party_round1(int64_t n, int m, int ncomp, const int* roles, const uint32_t* const* slots,
                 const uint64_t* nn, At&& at) {
  for (int c = 0; c < ncomp; ++c) {
    const int role = roles[c];
    if (role != 0 && role != 1) continue;
    const R1Args<T> a = at(c);
    T* o = role == 0 ? a.o0 : a.o1;
    for_chunks(n, [&](int64_t i0, int64_t len) {
      mxc::round1<T>(
          role, slots[2 * c], slots[2 * c + 1], nn, m, i0, len,
          [&](int64_t i) { return (T)(a.mine[i] + a.other[i] + (a.z2m ? a.z2m[i] : (T)0)); },
          [&](int64_t i, T* rt, T* rm) {
            *rt = a.rt[i];
            *rm = (T)a.rm[i];
          },
          [&](int64_t i, T w, T z) {
            a.w[i] = w;
            o[i] = z;
          });
    });
  }
  return 0;
}

template <class T>
int trunc_r1(int64_t n, int m, int ncomp, const int* roles, const T* msg, const T* rmk,
             const T* rrt, const u64* rrm, T* w, T* out0, T* out1,
             const uint32_t* const* slots, const uint64_t* nn) {
  return party_round1<T>(n, m, ncomp, roles, slots, nn + 2, [&](int c) {
    const int64_t base = (int64_t)c * n;
    return R1Args<T>{msg + base, rmk + base, nullptr,     rrt + base,
                     rrm + base, w + base,   out0 + base, out1 + base};
  });
}

// Ring extension Z_2^64 -> Z_2^128 (k_ring_extend_party_r0 / r1): every stream at 128-bit
// width (element i = the composed protocol's 128-bit draw); r0, r1, M0 use the low 64 bits
int ring_extend_r0(int64_t n, int ncomp, const int* roles, const u64* s0, const u64* s1, u64* msg,
                   u128* msg_R, u64* msg_M, u128* out0, u128* out1,
                   const uint32_t* const* slots, const uint64_t* nn) {
  for (int c = 0; c < ncomp; ++c) {
    const int role = roles[c];
    const uint32_t* own = slots[2 * c];
    const uint32_t* nxt = slots[2 * c + 1];
    const int64_t base = (int64_t)c * n;
    for_chunks(n, [&](int64_t i0, int64_t len) {
      if (role == 0 || role == 1) {  // r0 under k0 = P0's own, r1 under k2 = P1's next
        const std::vector<u128> r = prf<u128>(role == 0 ? own : nxt, nn[role], i0, len);
        for (int64_t q = 0; q < len; ++q) {
          const int64_t i = base + i0 + q;
          msg[i] = role == 0 ? mxf::ring_extend_mask0(s0[i], s1[i], (u64)r[q]) : s1[i] + (u64)r[q];
        }
      } else if (role == 2) {
        const mxc::DealerDraws<u128> w(own, nxt, nn, i0, len);
        for (int64_t q = 0; q < len; ++q) {
          const int64_t i = base + i0 + q;
          const mxf::RingExtendDeal d =
              mxf::ring_extend_deal(w.r0[q], w.r1[q], w.t[q], w.m[q], w.z0[q], w.z2[q]);
          msg_R[i] = d.R1;
          msg_M[i] = d.M1;
          out0[i] = d.s0;
          out1[i] = d.s1;
        }
      }
    });
  }
  return 0;
}

int ring_extend_r1(int64_t n, int ncomp, const int* roles, const u64* msg, const u64* rmk,
                   const u128* rR, const u64* rM, u128* w, u128* out0, u128* out1,
                   const uint32_t* const* slots, const uint64_t* nn) {
  for (int c = 0; c < ncomp; ++c) {
    const int role = roles[c];
    if (role != 0 && role != 1) continue;
    const int64_t base = (int64_t)c * n;
    u128* o = role == 0 ? out0 : out1;
    for_chunks(n, [&](int64_t i0, int64_t len) {
      const mxc::Round1Draws<u128> k(role, slots[2 * c], slots[2 * c + 1], nn + 2, i0, len);
      for (int64_t q = 0; q < len; ++q) {
        const int64_t i = base + i0 + q;
        const u128 R = role == 0 ? k.t[q] : rR[i];
        const u64 M = role == 0 ? (u64)k.m[q] : rM[i];
        w[i] = mxf::ring_extend_round1_w(role, msg[i] + rmk[i], R, M, k.z[q]);
        o[i] = k.z[q];
      }
    });
  }
  return 0;
}

template <class T>
int share_party(int kind, int64_t n, int ncomp, const int* rel, const void* xp, T* out0, T* out1,
                const uint32_t* const* slots, uint64_t n1, uint64_t na) {
  const bool mir = kind & MX_SHARE_MIRROR;
  kind &= ~MX_SHARE_MIRROR;
  const T* x = (const T*)xp;
  const double* xf = (const double*)xp;  // kind MX_SHARE_F64 (moosex.h)
  const double scale = kind == MX_SHARE_F64 ? std::ldexp(1.0, (int)na) : 0.0;
  for (int c = 0; c < ncomp; ++c) {
    const int code = rel[c];  // as k_share_party: role + 4 * (1 + local P_{j+1} component)
    if (code < 0) continue;
    const int r = code & 3, fwd = (code >> 2) - 1;
    const int64_t base = (int64_t)c * n;
    if (r > 2) continue;
    for_chunks(n, [&](int64_t i0, int64_t len) {
      std::vector<T> a(len);
      if (mir ? r != 2 : r != 1) mxc::prf_into<T>(slots[2 * c], n1, i0, len, a.data());
      for (int64_t q = 0; q < len; ++q) {
        const int64_t i = base + i0 + q;
        if (r == 0) {
          const T xv =
              kind == MX_SHARE_F64 ? mxr::f64_to_ring<T>(xf[i0 + q] * scale) : x[i0 + q];
          const T v = kind == MX_CROSS_BOOL ? (T)(xv ^ a[q]) : (T)(xv - a[q]);
          out0[i] = mir ? v : a[q];
          out1[i] = mir ? a[q] : v;
          if (fwd >= 0) (mir ? out1 : out0)[(int64_t)fwd * n + i0 + q] = v;
        } else if (r == 1) {
          if (mir) out0[i] = a[q];
          out1[i] = 0;  // s0 arrives from the owner (mirrored: zero slot j+2)
        } else {
          out0[i] = 0;
          if (!mir) out1[i] = a[q];  // mirrored: s1 arrives from the owner
        }
      }
    });
  }
  return 0;
}


// ---- fixed-point dot tail (see rss_party.hip: reshare folded into TruncPr round A) ----
template <class T>
int dot_tail_r0(int64_t n, int m, int ncomp, const int* roles, const void* const* cross,
                void* const* msg, void* const* msg_rt, void* const* msg_rm, void* const* out0,
                void* const* out1, const uint32_t* const* slots, const uint64_t* nn) {
  for (int c = 0; c < ncomp; ++c) {
    const int role = roles[c];
    if (role < 0 || role > 2) continue;
    const uint32_t* own = slots[2 * c];
    const uint32_t* nxt = slots[2 * c + 1];
    const T* x = (const T*)cross[c];
    T* mo = (T*)msg[c];
    // as k_dot_tail_r0: no cross -> the dealer part only; no msg_rt -> no dealer part
    const bool dealer = role == 2 && msg_rt[c] != nullptr;
    for_chunks(n, [&](int64_t i0, int64_t len) {
      if (x != nullptr)
        mxc::main_r0<T>(
            true, role, own, nxt, nn[0], nn + 1, i0, len, [&](int64_t i) { return x[i]; },
            [&](int64_t i) -> T& { return mo[i]; });
      if (dealer)
        mxc::dealer_r0<T>(own, nxt, nn + 1, m, i0, len,
                          deal_out<T>((T*)msg_rt[c], (u64*)msg_rm[c], (T*)out0[c], (T*)out1[c]));
    });
  }
  return 0;
}

template <class T>
int dot_tail_r1(int64_t n, int m, int ncomp, const int* roles, const void* const* msg,
                const void* const* rmk, const void* const* rz, const void* const* rrt,
                const void* const* rrm, void* const* w, void* const* out0, void* const* out1,
                const uint32_t* const* slots, const uint64_t* nn) {
  return party_round1<T>(n, m, ncomp, roles, slots, nn + 3, [&](int c) {
    return R1Args<T>{(const T*)msg[c],   (const T*)rmk[c], rz ? (const T*)rz[c] : nullptr,
                     (const T*)rrt[c],   (const u64*)rrm[c], (T*)w[c],
                     (T*)out0[c],        (T*)out1[c]};
  });
}

template <class T>
int dot_tail_r2(int64_t n, int ncomp, const int* roles, const void* const* a,
                const void* const* b, void* const* out) {
  for (int c = 0; c < ncomp; ++c) {
    if (roles[c] != 0 && roles[c] != 1) continue;
    const T* x = (const T*)a[c];
    const T* y = (const T*)b[c];
    T* o = (T*)out[c];
    mx_cpu_parallel_for(n, 1 << 14, [&](int64_t s, int64_t e) {
      for (int64_t i = s; i < e; ++i) o[i] = x[i] + y[i];
    });
  }
  return 0;
}

}  // namespace

extern "C" {

int mx_trunc_party_r0(int dev, int words, int64_t n, int m, int ncomp, const int* roles,
                      const void* s0, const void* s1, void* msg, void* msg_rm, void* out0,
                      void* out1, const uint32_t* const* slots, const uint64_t* nn,
                      void* stream) {
  if (m < 1 || m > 63) return -3;
  if (dev)
    return mxh_trunc_party_r0(words, n, m, ncomp, roles, s0, s1, msg, msg_rm, out0, out1,
                              slots, nn, stream);
  if (words == 1)
    return trunc_r0<u64>(n, m, ncomp, roles, (const u64*)s0, (const u64*)s1, (u64*)msg,
                         (u64*)msg_rm, (u64*)out0, (u64*)out1, slots, nn);
  if (words == 2)
    return trunc_r0<u128>(n, m, ncomp, roles, (const u128*)s0, (const u128*)s1, (u128*)msg,
                          (u64*)msg_rm, (u128*)out0, (u128*)out1, slots, nn);
  return -2;
}

int mx_trunc_party_r1(int dev, int words, int64_t n, int m, int ncomp, const int* roles,
                      const void* msg, const void* rmk, const void* rrt, const void* rrm,
                      void* w, void* out0, void* out1, const uint32_t* const* slots,
                      const uint64_t* nn, void* stream) {
  if (m < 1 || m > 63) return -3;
  if (dev)
    return mxh_trunc_party_r1(words, n, m, ncomp, roles, msg, rmk, rrt, rrm, w, out0, out1,
                              slots, nn, stream);
  if (words == 1)
    return trunc_r1<u64>(n, m, ncomp, roles, (const u64*)msg, (const u64*)rmk,
                         (const u64*)rrt, (const u64*)rrm, (u64*)w, (u64*)out0, (u64*)out1,
                         slots, nn);
  if (words == 2)
    return trunc_r1<u128>(n, m, ncomp, roles, (const u128*)msg, (const u128*)rmk,
                          (const u128*)rrt, (const u64*)rrm, (u128*)w, (u128*)out0,
                          (u128*)out1, slots, nn);
  return -2;
}

int mx_ring_extend_party_r0(int dev, int64_t n, int ncomp, const int* roles, const void* s0,
                            const void* s1, void* msg, void* msg_R, void* msg_M, void* out0,
                            void* out1, const uint32_t* const* slots, const uint64_t* nn,
                            void* stream) {
  if (n == 0) return 0;
  if (ncomp < 1 || ncomp > 3) return -3;
  if (dev)
    return mxh_ring_extend_party_r0(n, ncomp, roles, s0, s1, msg, msg_R, msg_M, out0, out1,
                                    slots, nn, stream);
  return ring_extend_r0(n, ncomp, roles, (const u64*)s0, (const u64*)s1, (u64*)msg, (u128*)msg_R,
                        (u64*)msg_M, (u128*)out0, (u128*)out1, slots, nn);
}

int mx_ring_extend_party_r1(int dev, int64_t n, int ncomp, const int* roles, const void* msg,
                            const void* rmk, const void* rR, const void* rM, void* w, void* out0,
                            void* out1, const uint32_t* const* slots, const uint64_t* nn,
                            void* stream) {
  if (n == 0) return 0;
  if (ncomp < 1 || ncomp > 3) return -3;
  if (dev)
    return mxh_ring_extend_party_r1(n, ncomp, roles, msg, rmk, rR, rM, w, out0, out1, slots, nn,
                                    stream);
  return ring_extend_r1(n, ncomp, roles, (const u64*)msg, (const u64*)rmk, (const u128*)rR,
                        (const u64*)rM, (u128*)w, (u128*)out0, (u128*)out1, slots, nn);
}

int mx_share_party(int dev, int kind, int words, int64_t n, int ncomp, const int* rel,
                   const void* x, void* out0, void* out1, const uint32_t* const* slots,
                   uint64_t n1, uint64_t na, void* stream) {
  if (dev)
    return mxh_share_party(kind, words, n, ncomp, rel, x, out0, out1, slots, n1, na, stream);
  switch (words) {
    case 0:
      return share_party<uint8_t>(kind, n, ncomp, rel, (const uint8_t*)x, (uint8_t*)out0,
                                  (uint8_t*)out1, slots, n1, na);
    case 1:
      return share_party<u64>(kind, n, ncomp, rel, (const u64*)x, (u64*)out0, (u64*)out1,
                              slots, n1, na);
    case 2:
      return share_party<u128>(kind, n, ncomp, rel, (const u128*)x, (u128*)out0, (u128*)out1,
                               slots, n1, na);
    default:
      return -2;
  }
}


int mx_dot_tail_r0(int dev, int words, int64_t n, int m, int ncomp, const int* roles,
                   const void* const* cross, void* const* msg, void* const* msg_rt,
                   void* const* msg_rm, void* const* out0, void* const* out1,
                   const uint32_t* const* slots, const uint64_t* nn, void* stream) {
  if (m < 1 || m > 63) return -3;
  if (ncomp < 1 || ncomp > 3) return -3;
  if (dev)
    return mxh_dot_tail_r0(words, n, m, ncomp, roles, cross, msg, msg_rt, msg_rm, out0, out1,
                           slots, nn, stream);
  if (words == 1)
    return dot_tail_r0<u64>(n, m, ncomp, roles, cross, msg, msg_rt, msg_rm, out0, out1, slots,
                            nn);
  if (words == 2)
    return dot_tail_r0<u128>(n, m, ncomp, roles, cross, msg, msg_rt, msg_rm, out0, out1, slots,
                             nn);
  return -2;
}

int mx_dot_tail_r1(int dev, int words, int64_t n, int m, int ncomp, const int* roles,
                   const void* const* msg, const void* const* rmk, const void* const* rz,
                   const void* const* rrt, const void* const* rrm, void* const* w,
                   void* const* out0, void* const* out1, const uint32_t* const* slots,
                   const uint64_t* nn, void* stream) {
  if (m < 1 || m > 63) return -3;
  if (ncomp < 1 || ncomp > 3) return -3;
  if (dev)
    return mxh_dot_tail_r1(words, n, m, ncomp, roles, msg, rmk, rz, rrt, rrm, w, out0, out1,
                           slots, nn, stream);
  if (words == 1)
    return dot_tail_r1<u64>(n, m, ncomp, roles, msg, rmk, rz, rrt, rrm, w, out0, out1, slots,
                            nn);
  if (words == 2)
    return dot_tail_r1<u128>(n, m, ncomp, roles, msg, rmk, rz, rrt, rrm, w, out0, out1, slots,
                             nn);
  return -2;
}

int mx_dot_tail_r2(int dev, int words, int64_t n, int ncomp, const int* roles,
                   const void* const* a, const void* const* b, void* const* out, void* stream) {
  if (ncomp < 1 || ncomp > 3) return -3;
  if (dev) return mxh_dot_tail_r2(words, n, ncomp, roles, a, b, out, stream);
  if (words == 1) return dot_tail_r2<u64>(n, ncomp, roles, a, b, out);
  if (words == 2) return dot_tail_r2<u128>(n, ncomp, roles, a, b, out);
  return -2;
}

}  // extern "C"
