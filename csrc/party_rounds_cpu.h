// Host twins of the round bodies of party_rounds.h, shared by rss_party_cpu.cpp and
// rss_jobs_cpu.cpp: per chunk of elements [i0, i0 + len) the PRF ranges a role draws and the
// element loop over rss_fused.h's round functions, parameterised by where an element is read
// and written.  Same streams, same element order as the device kernels.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>

#include "rss_fused.h"

void mx_cpu_prf_range(const uint8_t* key, uint64_t nonce, int words, int64_t i0, int64_t n,
                      void* out);
void mx_cpu_parallel_for(int64_t n, int64_t grain,
                         const std::function<void(int64_t, int64_t)>& f);

namespace mxc {

// f(i0, len) over [0, n) in chunks, in parallel
template <class F>
void for_chunks(int64_t n, F&& f) {
  mx_cpu_parallel_for(n, 1 << 12, [&](int64_t s, int64_t e) {
    const int64_t CH = 512;
    for (int64_t c = s; c < e; c += CH) f(c, std::min(CH, e - c));
  });
}

// elements [i0, i0 + len) of PRF(key slot, nonce) at the lane width of T
template <class T>
void prf_into(const uint32_t* slot, uint64_t nonce, int64_t i0, int64_t len, T* out) {
  const int words = sizeof(T) == 1 ? 0 : (int)(sizeof(T) / 8);
  mx_cpu_prf_range((const uint8_t*)slot, nonce, words, i0, len, out);
}
template <class T>
std::vector<T> prf(const uint32_t* slot, uint64_t nonce, int64_t i0, int64_t len) {
  std::vector<T> out(len);
  prf_into<T>(slot, nonce, i0, len, out.data());
  return out;
}

// The dealer P2's six streams in nonce order nn = (r0, r1, t, m, z0, z2): k0 is its nxt, k2
// its own.
template <class T>
struct DealerDraws {
  std::vector<T> r0, r1, t, m, z0, z2;
  DealerDraws(const uint32_t* own, const uint32_t* nxt, const uint64_t* nn, int64_t i0,
              int64_t len)
      : r0(prf<T>(nxt, nn[0], i0, len)), r1(prf<T>(own, nn[1], i0, len)),
        t(prf<T>(nxt, nn[2], i0, len)), m(prf<T>(nxt, nn[3], i0, len)),
        z0(prf<T>(nxt, nn[4], i0, len)), z2(prf<T>(own, nn[5], i0, len)) {}
};

// Round 0 of the dealer: sink(i, d) gets element i's TruncDeal.
template <class T, class Sink>
void dealer_r0(const uint32_t* own, const uint32_t* nxt, const uint64_t* nn, int m, int64_t i0,
               int64_t len, Sink&& sink) {
  const DealerDraws<T> w(own, nxt, nn, i0, len);
  for (int64_t q = 0; q < len; ++q)
    sink(i0 + q, mxf::trunc_deal<T>(w.r0[q], w.r1[q], w.t[q], w.m[q], w.z0[q], w.z2[q], m));
}

// Round 0 of P0 / P1 / P2 (role): msg(i) = the opening message of value(i).  zero: the dot
// tail's form, value(i) masked by the zero share at nonce n_a; TruncPr's own form (P0, P1
// only) draws the opening mask alone.  nr = (r0, r1).
template <class T, class Value, class Msg>
void main_r0(bool zero, int role, const uint32_t* own, const uint32_t* nxt, uint64_t n_a,
             const uint64_t* nr, int64_t i0, int64_t len, Value&& value, Msg&& msg) {
  // a stream the role does not draw stays 0
  std::vector<T> a(len, (T)0), b(len, (T)0), r(len, (T)0);
  if (zero && role != 1) prf_into<T>(own, n_a, i0, len, a.data());
  if (zero && role != 0) prf_into<T>(nxt, n_a, i0, len, b.data());
  if (role == 0) prf_into<T>(own, nr[0], i0, len, r.data());
  if (role == 1) prf_into<T>(nxt, nr[1], i0, len, r.data());
  for (int64_t q = 0; q < len; ++q) {
    const int64_t i = i0 + q;
    msg(i) = mxf::trunc_open_msg<T>(role, mxf::zero_masked<T>(value(i), a[q], b[q]), r[q]);
  }
}

// Round 1's streams, nn = (t, m, z0, z2): P0 t, m, z0 under its own k0; P1 z2 (into z) under
// its nxt k2.
template <class T>
struct Round1Draws {
  std::vector<T> t, m, z;
  Round1Draws(int role, const uint32_t* own, const uint32_t* nxt, const uint64_t* nn, int64_t i0,
              int64_t len) {
    if (role == 0) {
      t = prf<T>(own, nn[0], i0, len);
      m = prf<T>(own, nn[1], i0, len);
      z = prf<T>(own, nn[2], i0, len);
    } else {
      z = prf<T>(nxt, nn[3], i0, len);
    }
  }
};

// Round 1 of P0 / P1 (role): c = opened(i); recv(i, &rt, &rm) reads what P1 received from the
// dealer; sink(i, w, z) gets w and the new share z (P0's s0, P1's s1).
template <class T, class Opened, class Recv, class Sink>
void round1(int role, const uint32_t* own, const uint32_t* nxt, const uint64_t* nn, int m,
            int64_t i0, int64_t len, Opened&& opened, Recv&& recv, Sink&& sink) {
  const Round1Draws<T> w(role, own, nxt, nn, i0, len);
  for (int64_t q = 0; q < len; ++q) {
    const int64_t i = i0 + q;
    T rt, rm;
    if (role == 0) {
      rt = w.t[q];
      rm = w.m[q];
    } else {
      recv(i, &rt, &rm);
    }
    sink(i, mxf::trunc_round1_w<T>(role, opened(i), rt, rm, w.z[q], m), w.z[q]);
  }
}

}  // namespace mxc
