// gfx950 VALU ring GEMM / GEMV: the reference product for small and skinny shapes, and the
// entry points mxh_gemm / mxh_gemm_bs that send a large product on to the MFMA paths
// (gemm_mfma.hip, gemm_crt.hip).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <cstdlib>

#include "moosex.h"
#include "party_batch.h"
#include "ring_launch.h"

namespace {

// Reference (VALU) ring GEMM: 16x16 output tile per block, K staged through LDS.
// a_bs / b_bs: batch strides in elements (0: one operand broadcast over the batch).
template <class T, int TS>
__device__ __forceinline__ void d_gemm_valu(int64_t M, int64_t N, int64_t K,
                                            const T* __restrict__ A0, const T* __restrict__ A1,
                                            const T* __restrict__ B0, const T* __restrict__ B1,
                                            int mode, T* __restrict__ C, int accumulate,
                                            int64_t a_bs, int64_t b_bs, int zb) {
  __shared__ T As[TS][TS + 1];
  __shared__ T Bs[TS][TS + 1];
  const int64_t b = zb >= 0 ? zb : blockIdx.z;  // zb >= 0: an unbatched launch's only product
  const int64_t row = blockIdx.y * TS + threadIdx.y;
  const int64_t col = blockIdx.x * TS + threadIdx.x;
  const T* a0 = A0 + b * a_bs;
  const T* b0 = B0 + b * b_bs;
  const T* a1 = mode ? A1 + b * a_bs : nullptr;
  const T* b1 = mode ? B1 + b * b_bs : nullptr;
  T acc = 0;
  const int passes = mode ? 2 : 1;
  for (int pass = 0; pass < passes; ++pass) {
    for (int64_t k0 = 0; k0 < K; k0 += TS) {
      int64_t ka = k0 + threadIdx.x, kb = k0 + threadIdx.y;
      T av = 0, bv = 0;
      if (row < M && ka < K) av = (pass == 0 ? a0 : a1)[row * K + ka];
      if (col < N && kb < K) {
        bv = b0[kb * N + col];
        if (mode && pass == 0) bv += b1[kb * N + col];
      }
      As[threadIdx.y][threadIdx.x] = av;
      Bs[threadIdx.y][threadIdx.x] = bv;
      __syncthreads();
#pragma unroll
      for (int k = 0; k < TS; ++k) acc += As[threadIdx.y][k] * Bs[k][threadIdx.x];
      __syncthreads();
    }
  }
  if (row < M && col < N) {
    T* c = C + b * M * N + row * N + col;
    *c = accumulate ? (T)(*c + acc) : acc;
  }
}

template <class T, int TS>
__global__ void __launch_bounds__(256) k_gemm_valu(int64_t M, int64_t N, int64_t K,
                                                   const T* __restrict__ A0,
                                                   const T* __restrict__ A1,
                                                   const T* __restrict__ B0,
                                                   const T* __restrict__ B1, int mode,
                                                   T* __restrict__ C, int accumulate,
                                                   int64_t a_bs, int64_t b_bs, int zb) {
  d_gemm_valu<T, TS>(M, N, K, A0, A1, B0, B1, mode, C, accumulate, a_bs, b_bs, zb);
}

// an unbatched product (grid z = 1, zb = 0) of several parties: one party-batched launch
MX_X3((k_gemm_valu<u64, 16>), (d_gemm_valu<u64, 16>));
MX_X3((k_gemm_valu<u128, 16>), (d_gemm_valu<u128, 16>));

// Skinny products (N <= 4: a matrix times a vector or a few columns -- the per-party
// LogReg and LR dots): one wave per output row, its lanes splitting K, then a butterfly over
// whole ring elements.  One pass of coalesced loads instead of the tiled kernel's serial
// k-tiles with two barriers each (a 100 x 128 by 128 x 1 product: ~25 us there).  The same
// ring sums (addition mod 2^w is associative), so the same products.
template <class T>
__device__ __forceinline__ T shfl_xor_wave(T v, int m) {
  constexpr int W = (int)(sizeof(T) / 4);
  uint32_t w[W];
#pragma unroll
  for (int q = 0; q < W; ++q) w[q] = (uint32_t)(v >> (32 * q));
#pragma unroll
  for (int q = 0; q < W; ++q) w[q] = (uint32_t)__shfl_xor((int)w[q], m, 64);
  T r = 0;
#pragma unroll
  for (int q = 0; q < W; ++q) r |= (T)w[q] << (32 * q);
  return r;
}

template <class T>
__device__ __forceinline__ void d_gemv_valu(int64_t M, int64_t N, int64_t K,
                                            const T* __restrict__ A0, const T* __restrict__ A1,
                                            const T* __restrict__ B0, const T* __restrict__ B1,
                                            int mode, T* __restrict__ C, int accumulate,
                                            int64_t a_bs, int64_t b_bs, int zb) {
  const int64_t b = zb >= 0 ? zb : blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= M) return;  // uniform per wave: the butterfly below sees whole waves
  const T* a0 = A0 + b * a_bs + row * K;
  const T* a1 = mode ? A1 + b * a_bs + row * K : nullptr;
  const T* b0 = B0 + b * b_bs;
  const T* b1 = mode ? B1 + b * b_bs : nullptr;
  for (int64_t n = 0; n < N; ++n) {
    T acc = 0;
    for (int64_t k = lane; k < K; k += 64) {
      const T y0 = b0[k * N + n];
      if (mode) {
        acc += a0[k] * (y0 + b1[k * N + n]) + a1[k] * y0;
      } else {
        acc += a0[k] * y0;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += shfl_xor_wave(acc, m);
    if (lane == 0) {
      T* c = C + b * M * N + row * N + n;
      *c = accumulate ? (T)(*c + acc) : acc;
    }
  }
}

template <class T>
__global__ void __launch_bounds__(256) k_gemv_valu(int64_t M, int64_t N, int64_t K,
                                                   const T* __restrict__ A0,
                                                   const T* __restrict__ A1,
                                                   const T* __restrict__ B0,
                                                   const T* __restrict__ B1, int mode,
                                                   T* __restrict__ C, int accumulate,
                                                   int64_t a_bs, int64_t b_bs, int zb) {
  d_gemv_valu<T>(M, N, K, A0, A1, B0, B1, mode, C, accumulate, a_bs, b_bs, zb);
}

MX_X3(k_gemv_valu<u64>, d_gemv_valu<u64>);
MX_X3(k_gemv_valu<u128>, d_gemv_valu<u128>);

// MOOSEX_GEMV=0: skinny products on the tiled kernel too
bool gemv_on() {
  static const bool on = [] {
    const char* e = std::getenv("MOOSEX_GEMV");
    return !(e && e[0] == '0');
  }();
  return on;
}

template <class T>
int launch_gemm_valu(int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                     const void* A1, const void* B0, const void* B1, int mode, void* C,
                     int accumulate, hipStream_t st, int64_t a_bs = -1, int64_t b_bs = -1) {
  if (N <= 4 && gemv_on()) {
    const dim3 grid((unsigned)((M + 3) / 4), 1, (unsigned)batch);
    hipLaunchKernelGGL((k_gemv_valu<T>), grid, dim3(256), 0, st, M, N, K, (const T*)A0,
                       (const T*)A1, (const T*)B0, (const T*)B1, mode, (T*)C, accumulate,
                       a_bs < 0 ? M * K : a_bs, b_bs < 0 ? K * N : b_bs, batch == 1 ? 0 : -1);
    MX_LAUNCH_CHECK();
    return 0;
  }
  constexpr int TS = 16;
  dim3 grid((unsigned)((N + TS - 1) / TS), (unsigned)((M + TS - 1) / TS), (unsigned)batch);
  dim3 block(TS, TS);
  hipLaunchKernelGGL((k_gemm_valu<T, TS>), grid, block, 0, st, M, N, K, (const T*)A0,
                     (const T*)A1, (const T*)B0, (const T*)B1, mode, (T*)C, accumulate,
                     a_bs < 0 ? M * K : a_bs, b_bs < 0 ? K * N : b_bs, batch == 1 ? 0 : -1);
  MX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// from gemm_mfma.hip
extern "C" int mxh_gemm_mfma(int words, int64_t batch, int64_t M, int64_t N, int64_t K,
                             const void* A0, const void* A1, const void* B0, const void* B1,
                             int mode, void* C, int accumulate, void* stream);

static int g_gemm_impl = 0;

extern "C" {

void mx_set_gemm_impl(int impl) { g_gemm_impl = impl; }

int mxh_gemm(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
             const void* A1, const void* B0, const void* B1, int mode, void* C, int accumulate,
             void* stream) {
  if (M == 0 || N == 0 || batch == 0) return 0;
  bool big = M >= 64 && N >= 64 && K >= 32;
  if ((g_gemm_impl == 2 || (g_gemm_impl == 0 && big)) && (words == 1 || words == 2))
    return mxh_gemm_mfma(words, batch, M, N, K, A0, A1, B0, B1, mode, C, accumulate, stream);
  if (words == 1)
    return launch_gemm_valu<u64>(batch, M, N, K, A0, A1, B0, B1, mode, C, accumulate,
                                 S(stream));
  if (words == 2)
    return launch_gemm_valu<u128>(batch, M, N, K, A0, A1, B0, B1, mode, C, accumulate,
                                  S(stream));
  return -2;
}

// Plain batched product with explicit batch strides (elements; 0 broadcasts an operand):
// the small-product (VALU) kernel, or the strided MFMA/CRT GEMM for large ones.
extern "C" int mx_gemm_strided(int words, int64_t batch, int64_t M, int64_t N, int64_t K,
                               const void* A0, const void* A1, int64_t a_bstride, const void* B0,
                               const void* B1, int64_t b_bstride, int mode, void* C,
                               int accumulate, void* stream);

int mxh_gemm_bs(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                int64_t a_bs, const void* B0, int64_t b_bs, void* C, void* stream) {
  if (M == 0 || N == 0 || batch == 0) return 0;
  const bool big = M >= 64 && N >= 64 && K >= 32;
  if (big && g_gemm_impl != 1)
    return mx_gemm_strided(words, batch, M, N, K, A0, nullptr, a_bs, B0, nullptr, b_bs, 0, C, 0,
                           stream);
  if (words == 1)
    return launch_gemm_valu<u64>(batch, M, N, K, A0, nullptr, B0, nullptr, 0, C, 0, S(stream),
                                 a_bs, b_bs);
  if (words == 2)
    return launch_gemm_valu<u128>(batch, M, N, K, A0, nullptr, B0, nullptr, 0, C, 0, S(stream),
                                  a_bs, b_bs);
  return -2;
}

}  // extern "C"
