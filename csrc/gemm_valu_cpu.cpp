// Host (CPU) ring GEMM: the oracle of gemm_valu.hip and of the MFMA paths behind mxh_gemm.
#include <algorithm>
#include <vector>

#include "moosex.h"
#include "ring_common.h"
#include "ring_host.h"

namespace {

template <class T>
void gemm_plain(const T* A, const T* B, T* C, int64_t M, int64_t N, int64_t K, bool acc) {
  parallel_for(M, 4, [&](int64_t s, int64_t e) {
    std::vector<T> row(N);
    for (int64_t i = s; i < e; ++i) {
      std::fill(row.begin(), row.end(), (T)0);
      const T* a = A + i * K;
      for (int64_t k = 0; k < K; ++k) {
        T av = a[k];
        const T* b = B + k * N;
        for (int64_t j = 0; j < N; ++j) row[j] += av * b[j];
      }
      T* c = C + i * N;
      if (acc)
        for (int64_t j = 0; j < N; ++j) c[j] += row[j];
      else
        for (int64_t j = 0; j < N; ++j) c[j] = row[j];
    }
  });
}

template <class T>
int gemm_t(int64_t batch, int64_t M, int64_t N, int64_t K, const T* A0, const T* A1,
           const T* B0, const T* B1, int mode, T* C, int accumulate) {
  for (int64_t b = 0; b < batch; ++b) {
    const T* a0 = A0 + b * M * K;
    const T* b0 = B0 + b * K * N;
    T* c = C + b * M * N;
    if (mode == 0) {
      gemm_plain(a0, b0, c, M, N, K, accumulate != 0);
    } else {
      const T* a1 = A1 + b * M * K;
      const T* b1 = B1 + b * K * N;
      std::vector<T> bs(K * N);
      for (int64_t i = 0; i < K * N; ++i) bs[i] = b0[i] + b1[i];
      gemm_plain(a0, bs.data(), c, M, N, K, accumulate != 0);
      gemm_plain(a1, b0, c, M, N, K, true);
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int mx_gemm(int dev, int words, int64_t batch, int64_t M, int64_t N, int64_t K,
            const void* A0, const void* A1, const void* B0, const void* B1, int mode, void* C,
            int accumulate, void* stream) {
  if (dev) return mxh_gemm(words, batch, M, N, K, A0, A1, B0, B1, mode, C, accumulate, stream);
  if (words == 1)
    return gemm_t<u64>(batch, M, N, K, (const u64*)A0, (const u64*)A1, (const u64*)B0,
                       (const u64*)B1, mode, (u64*)C, accumulate);
  if (words == 2)
    return gemm_t<u128>(batch, M, N, K, (const u128*)A0, (const u128*)A1, (const u128*)B0,
                        (const u128*)B1, mode, (u128*)C, accumulate);
  return -2;
}

}  // extern "C"
