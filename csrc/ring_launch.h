// What the launches of the ring kernel translation units share (ring_hip.hip, leaf_hip.hip,
// gemm_valu.hip): the element types, the block size, the stream cast, the last-error check, the
// dispatch over element widths, the PRF names of prf_dev.h and the share-pair argument block.
// The one grid rule is mxd::grid_for (prf_dev.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "prf_dev.h"
#include "ring_common.h"

using mxr::u128;
using u64 = uint64_t;

using mxd::grid_for;  // blocks of 256 threads over n items, at most 256 CUs x 8 blocks
using mxd::KeySrc;
using mxd::Lane;
using mxd::pick;
using mxd::stage_keys;
using mxd::prf_chunk;
using mxd::kKeyWords;

// a launcher returns -100 - e for the HIP error e its launch left behind
#define MX_LAUNCH_CHECK()                               \
  do {                                                  \
    hipError_t _e = hipGetLastError();                  \
    if (_e != hipSuccess) return -100 - (int)_e;        \
  } while (0)

// run the statement with T = the element of `words` ring words (0: a bit per byte)
#define DEV_DISPATCH(words, T, ...)            \
  switch (words) {                             \
    case 0: { using T = uint8_t; __VA_ARGS__; } \
    case 1: { using T = u64; __VA_ARGS__; }     \
    case 2: { using T = u128; __VA_ARGS__; }    \
    default: return -2;                        \
  }

// Unnamed like the kernels' own namespace: a kernel that takes a Pair by value is internal to
// its translation unit, and so is its argument type.
namespace {

constexpr int kBlock = 256;

inline hipStream_t S(void* s) { return (hipStream_t)s; }

// Share-pair forms: both replicated share vectors (s0, s1) of a share-wise op in ONE launch,
// blockIdx.y picks the pair member.
template <class T>
struct Pair {
  const T* a[2];
  const T* b[2];
  T* o[2];
  int which[2];
};

}  // namespace
