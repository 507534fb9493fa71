// Host (CPU) twins of the stacked product kernels of ring_hip.hip: the RSS local step with its zero share, the PRF
// expansion and the small multiply-add forms, with their mx_* entry points.  Plain loops over
// the keystream of ring_cpu.cpp (mx_cpu_prf_range): the oracle.
#include <string.h>

#include <algorithm>

#include "moosex.h"
#include "ring_common.h"
#include "ring_host.h"

namespace {

// the keystream of one 16-byte key at the width of T (ring_cpu.cpp holds the PRF)
template <class T>
void prf_elements(const uint8_t* key, uint64_t nonce, int64_t i0, int64_t n, T* out) {
  mx_cpu_prf_range(key, nonce, sizeof(T) == 1 ? 0 : (int)(sizeof(T) / 8), i0, n, out);
}

template <class T>
int rss_cross_t(int kind, const T* x0, const T* x1, const T* y0, const T* y1, T* out, int64_t n,
                int nparties, const uint8_t* keys, uint64_t nonce) {
  for (int p = 0; p < nparties; ++p) {
    const int64_t off = (int64_t)p * n;
    const uint8_t* ka = keys ? keys + 16 * p : nullptr;
    const uint8_t* kb = keys ? keys + 16 * (p + 1) : nullptr;
    parallel_for(n, 1 << 14, [&](int64_t s, int64_t e) {
      const int64_t CH = 1024;
      T ra[CH], rb[CH];
      for (int64_t c = s; c < e; c += CH) {
        int64_t m = std::min(CH, e - c);
        if (ka) {
          prf_elements<T>(ka, nonce, c, m, ra);
          prf_elements<T>(kb, nonce, c, m, rb);
        }
        for (int64_t j = 0; j < m; ++j) {
          int64_t i = off + c + j;
          T v;
          if (x0 && y0) {
            v = mxr::cross<T>(kind, x0[i], x1 ? x1[i] : (T)0, y0[i], y1 ? y1[i] : (T)0,
                              x1 != nullptr, y1 != nullptr);
          } else if (x0) {
            v = x0[i];  // add-zero-share mode
          } else {
            v = 0;
          }
          if (ka) v = mxr::zs_combine<T>(kind, v, ra[j], rb[j]);
          out[i] = v;
        }
      }
    });
  }
  return 0;
}

template <class T>
int prf_expand_t(T* out, int64_t n, int nkeys, const uint8_t* keys, uint64_t nonce) {
  for (int p = 0; p < nkeys; ++p) {
    const uint8_t* k = keys + 16 * p;
    parallel_for(n, 1 << 14, [&](int64_t s, int64_t e) {
      prf_elements<T>(k, nonce, s, e - s, out + (int64_t)p * n + s);
    });
  }
  return 0;
}

}  // namespace

extern "C" {

int mx_rss_cross(int dev, int kind, int words, const void* x0, const void* x1,
                 const void* y0, const void* y1, void* out, int64_t n, int nparties,
                 const uint8_t* keys16, uint64_t nonce, void* stream) {
  if (dev)
    return mxh_rss_cross(kind, words, x0, x1, y0, y1, out, n, nparties, keys16, nonce, stream);
  DISPATCH_WORDS(words, T,
                 return rss_cross_t<T>(kind, (const T*)x0, (const T*)x1, (const T*)y0,
                                       (const T*)y1, (T*)out, n, nparties, keys16, nonce));
}

int mx_zero_share(int dev, int kind, int words, void* out, int64_t n, int nparties,
                  const uint8_t* keys16, uint64_t nonce, void* stream) {
  return mx_rss_cross(dev, kind, words, nullptr, nullptr, nullptr, nullptr, out, n, nparties,
                      keys16, nonce, stream);
}

int mx_prf_expand(int dev, int words, void* out, int64_t n, int nkeys, const uint8_t* keys16,
                  uint64_t nonce, void* stream) {
  if (dev) return mxh_prf_expand(words, out, n, nkeys, keys16, nonce, stream);
  DISPATCH_WORDS(words, T, return prf_expand_t<T>((T*)out, n, nkeys, keys16, nonce));
}

int mx_rss_cross_k(int dev, int kind, int words, const void* x0, const void* x1,
                   const void* y0, const void* y1, void* out, int64_t n, int nparties,
                   const uint32_t* slots, int nslots, uint64_t nonce, void* stream) {
  if (nslots < 1 || nparties < 1 || nparties > 3) return -3;
  if (dev)
    return mxh_rss_cross_k(kind, words, x0, x1, y0, y1, out, n, nparties, slots, nslots, nonce,
                           stream);
  uint8_t keys[16 * 4];  // host slots: the raw keys lead each slot
  for (int i = 0; i <= nparties; ++i)
    memcpy(keys + 16 * i, slots + MX_KEY_SLOT_WORDS * (i % nslots), 16);
  DISPATCH_WORDS(words, T,
                 return rss_cross_t<T>(kind, (const T*)x0, (const T*)x1, (const T*)y0,
                                       (const T*)y1, (T*)out, n, nparties, keys, nonce));
}

int mx_rss_cross_kp(int dev, int kind, int words, const void* x0, const void* x1,
                    const void* y0, const void* y1, void* out, int64_t n, int nparties,
                    const uint32_t* const* slot_ptrs, uint64_t nonce, void* stream) {
  if (nparties < 1 || nparties > 3) return -3;
  if (dev)
    return mxh_rss_cross_kp(kind, words, x0, x1, y0, y1, out, n, nparties, slot_ptrs, nonce,
                            stream);
  const int64_t es = words == 0 ? 1 : 8 * words;
  auto at = [&](const void* b, int p) -> const void* {
    return b ? (const uint8_t*)b + (int64_t)p * n * es : nullptr;
  };
  for (int p = 0; p < nparties; ++p) {
    uint8_t keys[32];
    memcpy(keys, slot_ptrs[2 * p], 16);
    memcpy(keys + 16, slot_ptrs[2 * p + 1], 16);
    void* o = (uint8_t*)out + (int64_t)p * n * es;
    int rc = -2;
    if (words == 0)
      rc = rss_cross_t<uint8_t>(kind, (const uint8_t*)at(x0, p), (const uint8_t*)at(x1, p),
                                (const uint8_t*)at(y0, p), (const uint8_t*)at(y1, p),
                                (uint8_t*)o, n, 1, keys, nonce);
    else if (words == 1)
      rc = rss_cross_t<u64>(kind, (const u64*)at(x0, p), (const u64*)at(x1, p),
                            (const u64*)at(y0, p), (const u64*)at(y1, p), (u64*)o, n, 1, keys,
                            nonce);
    else if (words == 2)
      rc = rss_cross_t<u128>(kind, (const u128*)at(x0, p), (const u128*)at(x1, p),
                             (const u128*)at(y0, p), (const u128*)at(y1, p), (u128*)o, n, 1,
                             keys, nonce);
    if (rc) return rc;
  }
  return 0;
}

int mx_rss_mul3_k(int dev, int kind, int words, const void* x0, const void* x1, const void* y0,
                  const void* y1, void* out0, void* out1, int64_t n, const uint32_t* slots,
                  uint64_t nonce, void* stream) {
  if (dev)
    return mxh_rss_mul3_k(kind, words, x0, x1, y0, y1, out0, out1, n, slots, nonce, stream);
  int rc = mx_rss_cross_k(0, kind, words, x0, x1, y0, y1, out0, n, 3, slots, 3, nonce, stream);
  if (rc) return rc;
  const int64_t bytes = n * (words == 0 ? 1 : 8 * words);
  for (int p = 0; p < 3; ++p)  // out1[p] = out0[p + 1]
    memcpy((uint8_t*)out1 + p * bytes, (const uint8_t*)out0 + ((p + 1) % 3) * bytes, bytes);
  return 0;
}

int mx_rss_mul3_kv(int dev, int kind, int words, const void* x0, const void* x1, const void* y0,
                   const void* y1, void* out0, void* out1, int64_t n, const uint32_t* slots,
                   uint64_t nonce, const int64_t* views, void* stream) {
  if (!dev) return -2;  // device only: host callers pass contiguous operands
  return mxh_rss_mul3_kv(kind, words, x0, x1, y0, y1, out0, out1, n, slots, nonce, views, stream);
}

int mx_mul_trunc3_kv(int dev, int words, const void* x0, const void* x1, const void* y0,
                     const void* y1, void* out0, void* out1, int64_t n, int64_t ostride,
                     const uint32_t* slots, uint64_t nmul, int m, const uint64_t* nonces,
                     const int64_t* views, void* stream) {
  if (!mx_trunc_shift_ok(words, m)) return -3;  // moosex.h: 0 <= m <= w - 2
  if (dev)
    return mxh_mul_trunc3_kv(words, x0, x1, y0, y1, out0, out1, n, ostride, slots, nmul, m,
                             nonces, views, stream);
  return 1;  // host: the caller composes mx_rss_mul3 and mx_trunc_pr3
}

int mx_mul_add2(int dev, int words, const void* a0, const void* a1, const void* f,
                const void* c, int add0, int add1, void* out0, void* out1, int64_t n,
                void* stream) {
  if (dev) return mxh_mul_add2(words, a0, a1, f, c, add0, add1, out0, out1, n, stream);
  DISPATCH_WORDS(words, T, {
    const T* fs = (const T*)f;
    const T cv = *(const T*)c;
    for (int y = 0; y < 2; ++y) {
      const T* a = (const T*)(y ? a1 : a0);
      T* o = (T*)(y ? out1 : out0);
      const T add = (y ? add1 : add0) ? cv : (T)0;
      for (int64_t i = 0; i < n; ++i) o[i] = a[i] * fs[i] + add;
    }
    return 0;
  });
}

int mx_prf_expand_k(int dev, int words, void* out, int64_t n, int nkeys, const uint32_t* slots,
                    uint64_t nonce, void* stream) {
  if (nkeys < 1 || nkeys > 4) return -3;
  if (dev) return mxh_prf_expand_k(words, out, n, nkeys, slots, nonce, stream);
  uint8_t keys[16 * 4];
  for (int i = 0; i < nkeys; ++i) memcpy(keys + 16 * i, slots + MX_KEY_SLOT_WORDS * i, 16);
  DISPATCH_WORDS(words, T, return prf_expand_t<T>((T*)out, n, nkeys, keys, nonce));
}

}  // extern "C"
