// Host (CPU) twins of the stacked boolean kernels of ring_hip.hip: the Kogge-Stone adder's levels, chains and per-party
// cross terms (mx_ks_*).  Plain loops over the keystream of ring_cpu.cpp (mx_cpu_prf_range):
// the oracle.
#include <string.h>

#include <vector>

#include "moosex.h"
#include "ring_common.h"
#include "ring_host.h"

extern "C" {

int mx_ks_cross1(int dev, int words, const void* g0, const void* g1, const void* p0,
                 const void* p1, void* z, int64_t n, int d, int both, const uint8_t* keys16,
                 uint64_t nonce, void* stream) {
  if (dev) return mxh_ks_cross1(words, g0, g1, p0, p1, z, n, d, both, keys16, nonce, stream);
  if (words != 1 && words != 2) return -2;
  DISPATCH_WORDS(words, T, {
    const int64_t m = both ? 2 * n : n;
    std::vector<T> r0(m), r1(m);
    mx_cpu_prf_range(keys16, nonce, words, 0, m, r0.data());
    mx_cpu_prf_range(keys16 + 16, nonce, words, 0, m, r1.data());
    const T *G0 = (const T*)g0, *G1 = (const T*)g1, *A0 = (const T*)p0, *A1 = (const T*)p1;
    T* Z = (T*)z;
    parallel_for(n, 4096, [&](int64_t lo, int64_t hi) {
      for (int64_t e = lo; e < hi; ++e) {
        const T s0 = G0[e] << d, s1 = G1[e] << d;
        Z[e] = (A0[e] & s0) ^ (A0[e] & s1) ^ (A1[e] & s0) ^ r0[e] ^ r1[e];
        if (both) {
          const T u0 = A0[e] << d, u1 = A1[e] << d;
          Z[n + e] = (A0[e] & u0) ^ (A0[e] & u1) ^ (A1[e] & u0) ^ r0[n + e] ^ r1[n + e];
        }
      }
    });
    return 0;
  });
}

int mx_ks_cross1_s(int dev, int words, const void* g0, const void* g1, const void* p0,
                   const void* p1, void* z, int64_t n, int d, int both,
                   const uint32_t* const* slots, uint64_t nonce, void* stream) {
  if (dev) return mxh_ks_cross1_s(words, g0, g1, p0, p1, z, n, d, both, slots, nonce, stream);
  uint8_t keys16[32];  // host slots: the raw key is the slot's first 16 bytes
  memcpy(keys16, slots[0], 16);
  memcpy(keys16 + 16, slots[1], 16);
  return mx_ks_cross1(0, words, g0, g1, p0, p1, z, n, d, both, keys16, nonce, stream);
}

int mx_ks_cross1x_s(int dev, int words, const void* g0, const void* g1, const void* t0,
                    const void* t1, void* go0, void* go1, const void* p0, const void* p1,
                    void* z, int64_t n, int d, int both, const uint32_t* const* slots,
                    uint64_t nonce, void* stream) {
  if (dev)
    return mxh_ks_cross1x_s(words, g0, g1, t0, t1, go0, go1, p0, p1, z, n, d, both, slots,
                            nonce, stream);
  if (t0 != nullptr) {  // g ^ t first, then the plain level on it
    if (words != 1 && words != 2) return -2;
    DISPATCH_WORDS(words, T, {
      const T *G0 = (const T*)g0, *G1 = (const T*)g1, *A = (const T*)t0, *B = (const T*)t1;
      T *O0 = (T*)go0, *O1 = (T*)go1;
      for (int64_t e = 0; e < n; ++e) {
        O0[e] = G0[e] ^ A[e];
        O1[e] = G1[e] ^ B[e];
      }
      return mx_ks_cross1_s(0, words, go0, go1, p0, p1, z, n, d, both, slots, nonce, stream);
    });
  }
  return mx_ks_cross1_s(0, words, g0, g1, p0, p1, z, n, d, both, slots, nonce, stream);
}

int mx_ks_sum2(int dev, int words, const void* p0, const void* p1, const void* g0,
               const void* g1, const void* t0, const void* t1, void* o0, void* o1, int64_t n,
               void* stream) {
  if (dev) return mxh_ks_sum2(words, p0, p1, g0, g1, t0, t1, o0, o1, n, stream);
  if (words != 1 && words != 2) return -2;
  DISPATCH_WORDS(words, T, {
    const T* P[2] = {(const T*)p0, (const T*)p1};
    const T* G[2] = {(const T*)g0, (const T*)g1};
    const T* X[2] = {(const T*)t0, (const T*)t1};
    T* O[2] = {(T*)o0, (T*)o1};
    for (int s = 0; s < 2; ++s)
      for (int64_t e = 0; e < n; ++e) O[s][e] = P[s][e] ^ (T)((G[s][e] ^ X[s][e]) << 1);
    return 0;
  });
}

int mx_ks_adder3_k(int dev, int words, const void* g0, const void* g1, const void* p0,
                   const void* p1, void* og0, void* og1, int64_t n, int nlev,
                   const uint32_t* slots, const uint64_t* nonces, void* stream) {
  if (dev)
    return mxh_ks_adder3_k(words, g0, g1, p0, p1, og0, og1, n, nlev, slots, nonces, stream);
  // host: the per-level chain (mx_ks_level3_k), ping-ponging through temporaries
  if (words != 1 && words != 2) return -2;
  const size_t es = 8 * (size_t)words, sz = 3 * (size_t)n * es;
  std::vector<uint8_t> G0(sz), G1(sz), A0(sz), A1(sz), NG0(sz), NG1(sz), NA0(sz), NA1(sz);
  memcpy(G0.data(), g0, sz);
  memcpy(G1.data(), g1, sz);
  memcpy(A0.data(), p0, sz);
  memcpy(A1.data(), p1, sz);
  int d = 1;
  for (int l = 0; l < nlev; ++l, d *= 2) {
    const int both = 2 * d < 64 * words;
    const int rc = mx_ks_level3_k(0, words, G0.data(), G1.data(), A0.data(), A1.data(),
                                  NG0.data(), NG1.data(), NA0.data(), NA1.data(), n, d, both,
                                  slots, nonces[l], stream);
    if (rc) return rc;
    G0.swap(NG0);
    G1.swap(NG1);
    if (both) {
      A0.swap(NA0);
      A1.swap(NA1);
    }
  }
  memcpy(og0, G0.data(), sz);
  memcpy(og1, G1.data(), sz);
  return 0;
}

int mx_ks_level3_k(int dev, int words, const void* g0, const void* g1, const void* p0,
                   const void* p1, void* og0, void* og1, void* op0, void* op1, int64_t n,
                   int d, int both, const uint32_t* slots, uint64_t nonce, void* stream) {
  if (dev)
    return mxh_ks_level3_k(words, g0, g1, p0, p1, og0, og1, op0, op1, n, d, both, slots, nonce,
                           stream);
  if (words != 1 && words != 2) return -2;
  DISPATCH_WORDS(words, T, {
    const int64_t m = both ? 2 * n : n;
    std::vector<T> r[3];
    for (int k = 0; k < 3; ++k) {
      r[k].resize(m);
      mx_cpu_prf_range((const uint8_t*)(slots + MX_KEY_SLOT_WORDS * k), nonce, words, 0, m,
                       r[k].data());
    }
    const T *G0 = (const T*)g0, *G1 = (const T*)g1, *A0 = (const T*)p0, *A1 = (const T*)p1;
    T *OG0 = (T*)og0, *OG1 = (T*)og1, *OP0 = (T*)op0, *OP1 = (T*)op1;
    parallel_for(n, 4096, [&](int64_t lo, int64_t hi) {
      for (int64_t e = lo; e < hi; ++e) {
        T t[3], q[3];
        for (int p = 0; p < 3; ++p) {
          const int64_t i = p * n + e;
          const int pn = (p + 1) % 3;
          const T s0 = G0[i] << d, s1 = G1[i] << d;
          t[p] = (A0[i] & s0) ^ (A0[i] & s1) ^ (A1[i] & s0) ^ r[p][e] ^ r[pn][e];
          if (both) {
            const T u0 = A0[i] << d, u1 = A1[i] << d;
            q[p] = (A0[i] & u0) ^ (A0[i] & u1) ^ (A1[i] & u0) ^ r[p][n + e] ^ r[pn][n + e];
          }
        }
        for (int p = 0; p < 3; ++p) {
          const int64_t i = p * n + e;
          const int pn = (p + 1) % 3;
          OG0[i] = G0[i] ^ t[p];
          OG1[i] = G1[i] ^ t[pn];
          if (both) {
            OP0[i] = q[p];
            OP1[i] = q[pn];
          }
        }
      }
    });
    return 0;
  });
}

}  // extern "C"
