// What the host (CPU) twins of the ring kernels share (ring_cpu.cpp, rss_mul3_cpu.cpp,
// rss_bits3_cpu.cpp, leaf_cpu.cpp, gemm_valu_cpu.cpp): the element types, the small thread
// pool, the dispatch over element widths and the keystream of ring_cpu.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <thread>
#include <vector>

// ring_cpu.cpp: elements [i0, i0 + n) of PRF(key, nonce) at `words` ring words (0: bits)
void mx_cpu_prf_range(const uint8_t* key, uint64_t nonce, int words, int64_t i0, int64_t n,
                      void* out);

#define DISPATCH_WORDS(words, T, ...)                 \
  switch (words) {                                    \
    case 0: { using T = uint8_t; __VA_ARGS__; }        \
    case 1: { using T = u64; __VA_ARGS__; }            \
    case 2: { using T = u128; __VA_ARGS__; }           \
    default: return -2;                               \
  }

// the arithmetic element widths of the image leaves (moosex.h): 8 or 16 bytes
#define DISPATCH_ELEM(elem_bytes, T, ...)      \
  switch (elem_bytes) {                        \
    case 8: { using T = u64; __VA_ARGS__; }    \
    case 16: { using T = u128; __VA_ARGS__; }  \
    default: return -2;                        \
  }

namespace {

using u64 = uint64_t;
using u128 = unsigned __int128;
using i128 = __int128;

inline int num_threads() {
  static int n = [] {
    const char* e = getenv("MOOSEX_CPU_THREADS");
    int v = e ? atoi(e) : (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(v, 32));
  }();
  return n;
}

template <class F>
void parallel_for(int64_t n, int64_t grain, F f) {
  int nt = num_threads();
  if (n <= grain || nt == 1) {
    if (n > 0) f(0, n);
    return;
  }
  int64_t chunks = std::min<int64_t>(nt, (n + grain - 1) / grain);
  int64_t per = (n + chunks - 1) / chunks;
  std::vector<std::thread> ts;
  ts.reserve(chunks - 1);
  for (int64_t c = 1; c < chunks; ++c) {
    int64_t b = c * per, e = std::min(n, b + per);
    if (b < e) ts.emplace_back([=] { f(b, e); });
  }
  f(0, std::min(n, per));
  for (auto& t : ts) t.join();
}

}  // namespace
