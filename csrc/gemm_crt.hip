// Exact ring GEMM over Z_2^64 / Z_2^128 by multi-modular (CRT) int8 MFMA products.
//
// The limb GEMM (gemm_mfma.hip) splits every ring element into L 8-bit limbs and needs the
// L(L+1)/2 limb-pair products on or below the anti-diagonal: 136 int8 GEMMs for Z_2^128,
// 36 for Z_2^64.  Here the exact INTEGER product is computed instead, in residues:
//
//   * every ring element x is read as its signed representative X in [-2^(w-1), 2^(w-1));
//     the integer product Z = sum_k X_k Y_k then satisfies |Z| <= K' 2^(2w-2);
//   * n pairwise-coprime moduli p_i <= 256 (256, 253, 251, 249, ...) with product
//     M > |Z| / 0.45 are chosen -- 36 for Z_2^128 at K' = 8192, 18 for Z_2^64;
//   * each operand is reduced to centered int8 residues (prep kernels, one udot4 per 4 bytes
//     of the element + one fp32 rounding), and ONE int8 GEMM per modulus gives
//     acc_i = Z mod p_i exactly in i32 (K' <= 2^15 keeps the epilogue's fp32 rounding exact);
//   * the CRT reconstruction  Z = sum_i c_i (M/p_i) - q M,  c_i = Z (M/p_i)^-1 mod p_i,
//     q = round(sum_i c_i / p_i), is evaluated mod 2^w:  z = sum_i c_i W_i - q (M mod 2^w)
//     with W_i = (M/p_i) mod 2^w.  The inverse (M/p_i)^-1 is folded into A's residues, so
//     the GEMM epilogue only reduces acc_i mod p_i (centered, stored as one byte).
//
// So a Z_2^128 product costs 36 int8 GEMMs instead of 136 (3.8x fewer MFMAs), Z_2^64 18
// instead of 36, at the price of wider operand prep and one reconstruction pass.  (The same
// idea as the Ozaki-II / multi-modular emulation of high-precision GEMM on integer matrix
// units; here the target is modular rather than floating-point arithmetic.)
//
// Kernels:
//   k_crt_prep<T, TRANS>  operand -> n residue planes in a blocked, swizzled int8 image
//                         [g = batch*n + i][tile][k-step][256 rows][64 bytes] (one 16 KB
//                         image per (tile, k-step), LDS-DMA ready, ds_read_b128 conflict free)
//   k_crt_prep_src        the same images of an operand that is still the plain input of its
//                         sharing: the three share slots are formed in registers
//   k_crt_gemm16          v_mfma_i32_16x16x64_i8 on a 256 x BN block tile (BN = 256 or 128), 8
//                         or 4 waves, K-step 64, LDS-DMA ring of 3 or 5 stages; the variants
//                         (kVariants, MOOSEX_CRT_KERNEL) differ in tile, waves and schedule.
//                         The epilogue reduces the i32 accumulators mod p_i and stores one byte
//                         per output element in MFMA register order (4 B per lane per 16x16
//                         block)
//   k_crt_recon16<T>      n residue bytes per element -> ring element (sum c_i W_i - q Mw),
//                         optionally accumulated into C; by v_dot4_i32_i8 or multiply-adds
//   k_crt_recon16d_open   the reconstruction of a product that is only revealed, inside the
//                         opening of its TruncPr tail
// Mode 1 (RSS cross GEMM, as in gemm_mfma.hip): A' = [A0 | A1], B' = [B0 + B1 ; B0].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "gemm_ws.h"
#include "hip_attr.h"
#include "moosex.h"
#include "prf_dev.h"
#include "rss_fused.h"

namespace {

using u64 = uint64_t;
using u128 = unsigned __int128;
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kMaxMod = 48;
// pairwise coprime, descending: 2^8, 3*5*17, 11*23, 13*19, primes, 7*31, primes
// Pairwise coprime, in the order they are used (a call takes the shortest prefix whose
// product is large enough).  The first 36 are the product-maximising set of 36 coprime
// integers <= 256 (exhaustive branch-and-bound over 61..256): 268.2 bits, just enough for an
// exact Z_2^128 product at K' = 8192 (268.15 bits), where the greedy descending set
// (256, 255, 253, ...) needs 37.  Their first 18 also cover Z_2^64 at K' = 8192.
constexpr int kModuli[kMaxMod] = {256, 253, 251, 249, 247, 241, 239, 235, 233, 229, 227, 223,
                                  217, 211, 199, 197, 193, 191, 181, 179, 173, 167, 163, 157,
                                  151, 149, 139, 137, 131, 127, 113, 109, 107, 103, 101, 97,
                                  89,  79,  73,  71,  67,  61,  59,  53,  43,  41,  37,  17};

constexpr int BM = 256;          // block tile rows (A side); the cols BN are 256 or 128
constexpr int BK = 64;           // k bytes per stage
constexpr int kImg = BM * BK;    // one A operand image per (tile, k-step): 16 KB
constexpr int kStages = 3;       // LDS ring depth

// byte offset of 16-byte chunk c (0..3) of image row r: chunks XOR-swizzled by
// f((r >> 2) & 3), f = [0, 2, 3, 1], so that the 16 lanes of each ds_read_b128 lane group hit
// 16 distinct 16-byte bank slots for the 16x16x64 fragments (lane l: row l & 15, chunk l >> 4).
__device__ __host__ inline int swz(int q) { return (0x78 >> (2 * (q & 3))) & 3; }
__device__ __host__ inline int img_off(int r, int c) { return r * BK + 16 * (c ^ swz(r >> 2)); }

// --- tables ---------------------------------------------------------------------------------
struct PrepTab {  // operand residues
  int n;
  int p[kMaxMod];
  float rcp[kMaxMod];
  uint32_t w[kMaxMod][4];  // weight of byte j of the element = byte j%4 of word j/4
  uint32_t neg[kMaxMod];   // added when the element is negative: (p - 2^w mod p) [* inv] mod p
  uint32_t mul0;           // p = 256: residue = (byte0 * mul0) mod 256
};
struct EpiTab {  // GEMM epilogue
  int n;
  int p[kMaxMod];
  float pf[kMaxMod];
  float rcp[kMaxMod];
  int t16[kMaxMod];  // 2^16 mod p
};
struct RecTab {  // reconstruction
  int n;
  float rcp[kMaxMod];
  uint16_t W[kMaxMod][8];  // (M / p_i) mod 2^w, 16-bit words
  uint16_t Mw[8];          // M mod 2^w
};

// Reconstruction by v_dot4_i32_i8 over groups of 4 moduli: W_i and R_i = round(2^24 / p_i)
// as signed base-256 digits, packed per (group, digit) with modulus 4g + u in byte u, so one
// dot4 of an element's 4 residues with one (uniform, SGPR) word adds that digit's 4 terms.
struct RecTab4 {
  int groups;
  uint32_t wd[kMaxMod / 4][16];
  uint32_t rd[kMaxMod / 4][3];
};

struct Tables {
  int words = 0, n = 0;
  PrepTab pa, pb;
  EpiTab ep;
  RecTab rc;
  RecTab4 r4;
};

int modinv(int a, int m) {
  int t = 0, nt = 1, r = m, nr = ((a % m) + m) % m;
  while (nr) {
    int q = r / nr, x;
    x = t - q * nt; t = nt; nt = x;
    x = r - q * nr; r = nr; nr = x;
  }
  return r == 1 ? (t % m + m) % m : -1;
}

// smallest n with prod p_i >= |Z|max / 0.45, |Z| <= K' 2^(2w-2)
int moduli_needed(int words, int64_t kprime) {
  const double need = 2.0 * 64 * words - 2 + std::log2((double)std::max<int64_t>(kprime, 1)) +
                      std::log2(1 / 0.45);
  double have = 0;
  for (int i = 0; i < kMaxMod; ++i) {
    have += std::log2((double)kModuli[i]);
    if (have >= need) return i + 1;
  }
  return -1;
}

void build_tables(int words, int n, Tables& t) {
  t.words = words;
  t.n = n;
  const int wbits = 64 * words;
  const int nbytes = 8 * words;
  u128 Mw = 1;
  for (int i = 0; i < n; ++i) Mw *= (u128)kModuli[i];
  if (words == 1) Mw &= ~(u64)0;
  std::memset(&t.pa, 0, sizeof t.pa);
  std::memset(&t.pb, 0, sizeof t.pb);
  std::memset(&t.ep, 0, sizeof t.ep);
  std::memset(&t.rc, 0, sizeof t.rc);
  t.pa.n = t.pb.n = t.ep.n = t.rc.n = n;
  for (int i = 0; i < n; ++i) {
    const int p = kModuli[i];
    u128 W = 1;
    int rest = 1;  // (M / p) mod p
    for (int j = 0; j < n; ++j)
      if (j != i) {
        W *= (u128)kModuli[j];
        rest = (int)((int64_t)rest * kModuli[j] % p);
      }
    const int inv = modinv(rest, p);
    for (int k = 0; k < 8; ++k) t.rc.W[i][k] = (uint16_t)(W >> (16 * k));
    t.rc.rcp[i] = 1.0f / (float)p;
    t.ep.p[i] = p;
    t.ep.pf[i] = (float)p;
    t.ep.rcp[i] = 1.0f / (float)p;
    t.ep.t16[i] = (int)((1 << 16) % p);
    t.pa.p[i] = t.pb.p[i] = p;
    t.pa.rcp[i] = t.pb.rcp[i] = 1.0f / (float)p;
    int pw = 1 % p;  // 256^j mod p
    for (int j = 0; j < nbytes; ++j) {
      const int wb = pw, wa = (int)((int64_t)pw * inv % p);
      t.pb.w[i][j / 4] |= (uint32_t)wb << (8 * (j % 4));
      t.pa.w[i][j / 4] |= (uint32_t)wa << (8 * (j % 4));
      pw = pw * 256 % p;
    }
    // pw = 2^w mod p now; element negative => subtract 2^w, i.e. add p - 2^w mod p
    const int negb = (p - pw) % p;
    t.pb.neg[i] = (uint32_t)negb;
    t.pa.neg[i] = (uint32_t)((int64_t)negb * inv % p);
    if (i == 0) {
      t.pa.mul0 = (uint32_t)inv;
      t.pb.mul0 = 1;
    }
  }
  for (int k = 0; k < 8; ++k) t.rc.Mw[k] = (uint16_t)(Mw >> (16 * k));
  std::memset(&t.r4, 0, sizeof t.r4);
  t.r4.groups = (n + 3) / 4;
  for (int i = 0; i < n; ++i) {
    u128 W = 0;
    for (int k = 0; k < 8; ++k) W |= (u128)t.rc.W[i][k] << (16 * k);
    int carry = 0;
    for (int d = 0; d < nbytes; ++d) {  // W mod 2^w in signed digits (carry out dropped)
      int b = (int)((W >> (8 * d)) & 0xff) + carry;
      carry = b >= 128;
      b -= 256 * carry;
      t.r4.wd[i / 4][d] |= (uint32_t)(uint8_t)(int8_t)b << (8 * (i % 4));
    }
    int R = (int)std::lround(16777216.0 / kModuli[i]);
    for (int d = 0; d < 3; ++d) {  // R < 2^24: exact in three signed digits
      int b = (R & 0xff);
      R >>= 8;
      if (b >= 128) {
        b -= 256;
        R += 1;
      }
      t.r4.rd[i / 4][d] |= (uint32_t)(uint8_t)(int8_t)b << (8 * (i % 4));
    }
  }
  (void)wbits;
}

const Tables& tables_for(int words, int n) {
  static std::mutex mu;
  static Tables cache[3][kMaxMod + 1];
  std::lock_guard<std::mutex> lk(mu);
  Tables& t = cache[words][n];
  if (t.n != n || t.words != words) build_tables(words, n, t);
  return t;
}

// --- device helpers ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) {
  const uint32_t lo = __builtin_amdgcn_perm((uint32_t)b, (uint32_t)a, 0x0c0c0400u);
  const uint32_t hi = __builtin_amdgcn_perm((uint32_t)d, (uint32_t)c, 0x0c0c0400u);
  return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}
__device__ __forceinline__ v4i pack16(const int (&q)[16]) {
  v4i o;
#pragma unroll
  for (int u = 0; u < 4; ++u) o[u] = (int)pack4(q[4 * u], q[4 * u + 1], q[4 * u + 2], q[4 * u + 3]);
  return o;
}

template <class T>
struct Words;
template <>
struct Words<u64> {
  static constexpr int N = 2;
};
template <>
struct Words<u128> {
  static constexpr int N = 4;
};

// centered residue of the signed element whose little-endian 32-bit words are x[0..NW-1]
template <int NW>
__device__ __forceinline__ float residue_f(const uint32_t (&x)[NW], const uint32_t (&w)[4],
                                           uint32_t neg, float p, float rcp) {
  uint32_t s = (x[NW - 1] >> 31) * neg;
#pragma unroll
  for (int q = 0; q < NW; ++q) s = __builtin_amdgcn_udot4(x[q], w[q], s, false);
  const float fs = (float)s;  // < 2^20: exact
  const float qt = __builtin_rintf(fs * rcp);  // p odd: s/p is never within 1/(2p) of k + 1/2
  return __builtin_fmaf(-qt, p, fs);           // in [-(p-1)/2, (p-1)/2]
}
template <int NW>
__device__ __forceinline__ int residue(const uint32_t (&x)[NW], const uint32_t (&w)[4],
                                       uint32_t neg, float p, float rcp) {
  return (int)residue_f<NW>(x, w, neg, p, rcp);
}

// Two residues at once: the fp32 scaling and the multiply-subtract as packed instructions
// (v_pk_mul_f32, v_pk_fma_f32: one issue for both elements); the same values as residue().
typedef float f2 __attribute__((ext_vector_type(2)));
template <int NW>
__device__ __forceinline__ f2 residue2_f(const uint32_t (&xa)[NW], const uint32_t (&xb)[NW],
                                         const uint32_t (&w)[4], uint32_t neg, float p,
                                         float rcp) {
  uint32_t sa = 0, sb = 0;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    sa = __builtin_amdgcn_udot4(xa[q], w[q], sa, false);
    sb = __builtin_amdgcn_udot4(xb[q], w[q], sb, false);
  }
  // the negative-element correction as one packed fma (the signs are per element, hoisted
  // out of the modulus loop): exact, the sum stays below 2^21
  const f2 sg = {(float)(xa[NW - 1] >> 31), (float)(xb[NW - 1] >> 31)};
  const float nf = (float)neg;
  const f2 fs = __builtin_elementwise_fma(sg, (f2){nf, nf}, (f2){(float)sa, (float)sb});
  f2 qt = fs * (f2){rcp, rcp};
  qt.x = __builtin_rintf(qt.x);
  qt.y = __builtin_rintf(qt.y);
  return __builtin_elementwise_fma(-qt, (f2){p, p}, fs);
}
template <int NW>
__device__ __forceinline__ void residue2(const uint32_t (&xa)[NW], const uint32_t (&xb)[NW],
                                         const uint32_t (&w)[4], uint32_t neg, float p,
                                         float rcp, int& ra, int& rb) {
  const f2 r = residue2_f<NW>(xa, xb, w, neg, p, rcp);
  ra = (int)r.x;
  rb = (int)r.y;
}

// The residue of a sum of two ring elements from the two elements' residues.  With S(.) the
// signed representative the residues are taken of, S(a + b mod 2^w) = S(a) + S(b) + kappa 2^w,
// kappa = top(a) + top(b) - carry - top(a + b) in {-1, 0, 1} (the carry out of bit w - 1
// minus the carry into it), and 2^w = -neg (mod p) (PrepTab::neg, A's with the folded inverse).
// So the sum's centred residue is that of ra + rb - kappa neg: an add, one fma and the
// rounding of residue(), about half a residue pass; |ra + rb - kappa neg| <= 2 (p - 1) keeps
// s/p at least 1/(2p) - 2^-21 from k + 1/2 for odd p.  p = 256 (neg = 0): a tie rounds to
// either neighbour, both the same byte.
__host__ __device__ inline int crt_sum_kappa(uint32_t ta, uint32_t tb, uint32_t ts) {  // top words
  const uint32_t carry = ((ta & tb) | ((ta | tb) & ~ts)) >> 31;
  return (int)(ta >> 31) + (int)(tb >> 31) - (int)carry - (int)(ts >> 31);
}
__host__ __device__ inline float crt_combine_f(float ra, float rb, float kappa, float neg,
                                               float p, float rcp) {
  const float fs = __builtin_fmaf(kappa, -neg, ra + rb);
  const float qt = __builtin_rintf(fs * rcp);
  return __builtin_fmaf(-qt, p, fs);
}
__host__ __device__ inline int crt_combine(int ra, int rb, int kappa, uint32_t neg, float p,
                                           float rcp) {
  return (int)crt_combine_f((float)ra, (float)rb, (float)kappa, (float)neg, p, rcp);
}
// two elements in packed instructions (the PK instance); the same values
__host__ __device__ inline f2 crt_combine2(f2 ra, f2 rb, f2 kappa, float neg, float p,
                                           float rcp) {
  const f2 fs = __builtin_elementwise_fma(kappa, (f2){-neg, -neg}, ra + rb);
  f2 qt = fs * (f2){rcp, rcp};
  qt.x = __builtin_rintf(qt.x);
  qt.y = __builtin_rintf(qt.y);
  return __builtin_elementwise_fma(-qt, (f2){p, p}, fs);
}

// One thread = (tile, k-step, image row r, 16-byte chunk c) of every residue plane.
// TRANS = false: A' rows are M rows of A0 (mode 0), [A0 | A1] (mode 1) or A0 + A1 (mode 2)
// (row-major [R][K] per batch, batch stride xs elements).  TRANS = true: B' rows are the N
// columns ([K][R]) of B0 (mode 0), [B0 + B1 ; B0] (1), [B0 ; B1] (2) or B0 + B1 (3).
// nkb k-steps are generated; the image is laid out with nkb_s k-steps per tile (>= nkb: a
// shorter operand placed in a longer operand's slot).
// src.n > 0: batch entry b takes its operands and mode from src instead (one launch for a
// set of images of different forms, e.g. run_crt_asym's sums beside plain shares).
// dual[b] != 0 (mode 0 only): the thread then adds x1 to the elements it holds and writes
// the sum's image too, at byte offset dual[b] from entry b's own image -- a share's image
// and the image of its sum with the next share from one read of the share.
struct PrepSrcs {
  int n = 0;
  int mode[6];
  const void* x0[6];
  const void* x1[6];
  int64_t dual[6];
};

template <class T, bool TRANS, int ROWS, bool PK = true>
__global__ void __launch_bounds__(256)
    k_crt_prep(const T* __restrict__ X0, const T* __restrict__ X1, int64_t R, int64_t K,
               int64_t xs, int mode_all, int8_t* __restrict__ out, int64_t tiles, int64_t nkb,
               int64_t nkb_s, const PrepTab tab, const PrepSrcs src) {
  constexpr int NW = Words<T>::N;
  const int64_t total = tiles * nkb * (ROWS * 4);
  const int64_t b = blockIdx.y;
  const int mode = src.n > 0 ? src.mode[b] : mode_all;
  const T* x0 = src.n > 0 ? (const T*)src.x0[b] : X0 + b * xs;
  const T* x1 = src.n > 0 ? (const T*)src.x1[b] : (mode ? X1 + b * xs : x0);
  const int n = tab.n;
  const int64_t plane = tiles * nkb_s * (int64_t)(ROWS * BK);
  int8_t* ob = out + b * n * plane;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < total;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(g & 3);
    const int r = (int)((g >> 2) & (ROWS - 1));
    const int64_t q = g / (ROWS * 4);
    const int64_t kb = q % nkb, t = q / nkb;
    const int64_t row = t * ROWS + r;
    const int64_t k0 = kb * BK + c * 16;
    uint32_t v[16][NW];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int64_t k = k0 + j;
      T e = 0;
      if (row < R) {
        if (!TRANS) {
          if (k < K) e = mode == 2 ? (T)(x0[row * K + k] + x1[row * K + k]) : x0[row * K + k];
          else if (mode == 1 && k < 2 * K) e = x1[row * K + (k - K)];
        } else {
          if (k < K)
            e = (mode & 1) ? (T)(x0[k * R + row] + x1[k * R + row]) : x0[k * R + row];
          else if (mode == 1 && k < 2 * K) e = x0[(k - K) * R + row];
          else if (mode == 2 && k < 2 * K) e = x1[(k - K) * R + row];
        }
      }
#pragma unroll
      for (int w = 0; w < NW; ++w) v[j][w] = (uint32_t)(e >> (32 * w));
    }
    const int64_t boff = (t * nkb_s + kb) * (int64_t)(ROWS * BK) + img_off(r, c);
    auto emit = [&](int8_t* base) __attribute__((always_inline)) {
    {  // p = 256: the low byte (times the folded inverse)
      int rr[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) rr[j] = (int)(v[j][0] * tab.mul0);
      *(v4i*)base = pack16(rr);
    }
    for (int i = 1; i < n; ++i) {
      const uint32_t w[4] = {tab.w[i][0], tab.w[i][1], tab.w[i][2], tab.w[i][3]};
      const uint32_t neg = tab.neg[i];
      const float p = (float)tab.p[i], rcp = tab.rcp[i];
      int rr[16];
      if constexpr (PK) {
#pragma unroll
        for (int j = 0; j < 16; j += 2)
          residue2<NW>(v[j], v[j + 1], w, neg, p, rcp, rr[j], rr[j + 1]);
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) rr[j] = residue<NW>(v[j], w, neg, p, rcp);
      }
      *(v4i*)(base + i * plane) = pack16(rr);
    }
    };
    emit(ob + boff);
    if (src.n > 0 && src.dual[b]) {  // + x1: the sum's image from the same read of x0
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int64_t k = k0 + j;
        if (row < R && k < K) {
          T e = 0;
#pragma unroll
          for (int w = 0; w < NW; ++w) e |= (T)v[j][w] << (32 * w);
          e += TRANS ? x1[k * R + row] : x1[row * K + k];
#pragma unroll
          for (int w = 0; w < NW; ++w) v[j][w] = (uint32_t)(e >> (32 * w));
        }
      }
      emit(ob + src.dual[b] + boff);
    }
  }
}

// A share source: an operand of run_crt_asym that is still the plain input of its sharing
// (k_share3 has not run).  The prep forms the three slots itself (mxf::share_plain /
// share_masked: slot jr = r, slot jv = x - r, the third 0) and writes the side's four images.
struct ShareSrc {
  const void* x = nullptr;  // plain operand: float64 (MX_SHARE_F64) or ring data
  int kind = 0;             // MX_CROSS_ARITH or MX_SHARE_F64, | MX_SHARE_MIRROR
  int frac = 0;             // MX_SHARE_F64: fractional bits
  int j0 = 0;               // owner slot
  uint64_t nonce = 0;
  mxd::KeySrc key;          // one key: the stream of r
};
// Kernel form.  Image e of the side (byte offset off[e]) holds phase ph[e]: 0 = r, 1 = x - r,
// 2 = the sum of the two, 3 = zero; a sum with the zero slot is its other slot.  A phase may
// belong to several images or to none.
// strip != 0: the zero phase has no image (its entries' ph is -1: nothing stored) -- every
// (modulus, tile) strip of it would be the same nkb * ROWS * BK zero bytes, so the side holds
// that strip once, at byte offset zoff, and k_crt_gemm16 reads it for every modulus and tile
// (map entry kZeroStrip).
struct SrcPlan {
  const void* x;
  int kind, strip;
  double scale;
  uint64_t nonce;
  int ph[4];
  int64_t off[4];
  int64_t zoff;
};
constexpr int kZeroStrip = 7;  // amap / bmap entry: the side's zero strip (images: 0..4)

// k_crt_prep for a share source over Z_2^128, every image of the side from one thread.
// Element i draws keystream chunk i = part (i >> 6) & 3 of ChaCha block ((i >> 8) << 6) |
// (i & 63) (prf_core.h), so a thread's 16 elements lie in 16 blocks, of which it needs one
// quarter each; the other quarters belong to the elements 64, 128 and 192 further on: the
// next three k-steps of the row (A', K % 256 == 0) or the columns +64, +128, +192 (B',
// N % 256 == 0).  The four owners are the lanes of one quad (p = lane & 3): each generates 4
// of the 16 blocks and the quad trades quarters through a wave-private LDS slice (no
// workgroup barrier: a wave's LDS operations complete in order), so every block is
// generated once.  A wave is 4 rows x 4 chunks x 4 owners: per modulus it stores four 256 B
// runs (k_crt_prep: one of 1 KB).  Rows past R hold zeros, as k_crt_prep's.
// The thread holds r and v = x - r (the plain operand is read once) and walks the moduli
// once: the residues of r and of v are full passes, the sum image's are combined from the
// two (crt_combine, with the element's kappa), the zero image's are zero bytes; each goes
// to every image of its phase.  s.strip: the zero phase is one strip instead (SrcPlan).
template <bool TRANS, int ROWS, bool PK>
__global__ void __launch_bounds__(256)
    k_crt_prep_src(const SrcPlan s, const mxd::KeySrc keys, int64_t R, int64_t K,
                   int8_t* __restrict__ out, int64_t tiles, int64_t nkb, const PrepTab tab) {
  using T = u128;
  constexpr int NW = 4;
  __shared__ uint32_t rks[1][mxd::kKeyWords];
  __shared__ uint4 xch[4][4][64];  // [wave][part][lane ^ part]: conflict-free both ways
  mxd::stage_keys(rks, keys, 1);
  const int lane = threadIdx.x & 63;
  const int p = lane & 3;
  uint4(*xw)[64] = xch[threadIdx.x >> 6];
  const int n = tab.n;
  const int64_t plane = tiles * nkb * (int64_t)(ROWS * BK);
  const int64_t total = tiles * ROWS * nkb * 4;  // a multiple of 64: waves stay whole
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < total;
       g += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)((g >> 2) & 3);
    const int rlow = (int)((g >> 4) & 3);
    const int64_t rest = g >> 6;
    int64_t row, kb, i0, istep;  // element j: i0 + j * istep, + 64 p for the thread's own
    if (!TRANS) {
      const int64_t q = rest / (ROWS / 4);
      kb = 4 * (q % (nkb / 4)) + p;
      row = (q / (nkb / 4)) * ROWS + (rest % (ROWS / 4)) * 4 + rlow;
      i0 = row * K + (kb - p) * BK + c * 16;
      istep = 1;
    } else {
      const int64_t q = rest >> 4;
      kb = q % nkb;
      row = (q / nkb) * 256 + 64 * p + (rest & 15) * 4 + rlow;
      i0 = (kb * BK + c * 16) * R + (row - 64 * p);
      istep = R;
    }
    const bool live = row < R;
    const int64_t t = row / ROWS;
    const int r = (int)(row % ROWS);
    uint32_t rr[16][NW], v[16][NW];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {  // blocks of elements 4 jj + (0..3), one per lane of the quad
      uint32_t w[16];
      mx::chacha_block(rks[0], s.nonce, mx::ks_block_of((uint64_t)(i0 + (4 * jj + p) * istep)), w);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        xw[q][lane ^ q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint4 e = xw[p][((lane & ~3) | u) ^ p];
        rr[4 * jj + u][0] = live ? e.x : 0u;
        rr[4 * jj + u][1] = live ? e.y : 0u;
        rr[4 * jj + u][2] = live ? e.z : 0u;
        rr[4 * jj + u][3] = live ? e.w : 0u;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // the other slot v = x - r (r and x - r are each other's mask) and the kappa of r + v
    // (the 16 plain values are loaded before any is encoded: the loads are in flight together)
    float kf[16];
    T xp[16];
    if (s.kind == MX_SHARE_F64) {
      double d[16];
#pragma unroll
      for (int j = 0; j < 16; ++j)
        d[j] = live ? ((const double*)s.x)[i0 + 64 * p + j * istep] : 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) xp[j] = mxf::share_plain<T>(MX_SHARE_F64, d, j, s.scale);
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        xp[j] = live ? mxf::share_plain<T>(s.kind, s.x, i0 + 64 * p + j * istep, s.scale) : (T)0;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      T h = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) h |= (T)rr[j][w] << (32 * w);
      const T x = xp[j];
      const T other = mxf::share_masked<T>(s.kind, x, h);
#pragma unroll
      for (int w = 0; w < NW; ++w) v[j][w] = (uint32_t)(other >> (32 * w));
      kf[j] = (float)crt_sum_kappa(rr[j][NW - 1], v[j][NW - 1],
                                   (uint32_t)((T)(h + other) >> (32 * (NW - 1))));
    }
    const int64_t boff = (t * nkb + kb) * (int64_t)(ROWS * BK) + img_off(r, c);
    bool has[4];  // the phases some image takes
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
      has[ph] = s.ph[0] == ph || s.ph[1] == ph || s.ph[2] == ph || s.ph[3] == ph;
    const bool do_r = has[0] || has[2], do_v = has[1] || has[2];
    auto put = [&](int ph, int64_t ioff, const v4i o) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (s.ph[e] == ph) *(v4i*)(out + s.off[e] + ioff + boff) = o;
    };
    const v4i zero = {0, 0, 0, 0};
    {  // p = 256: the low byte (times the folded inverse); the sum's is the low bytes' sum
      int q[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) q[j] = (int)(rr[j][0] * tab.mul0);
      put(0, 0, pack16(q));
#pragma unroll
      for (int j = 0; j < 16; ++j) q[j] = (int)(v[j][0] * tab.mul0);
      put(1, 0, pack16(q));
#pragma unroll
      for (int j = 0; j < 16; ++j) q[j] = (int)((rr[j][0] + v[j][0]) * tab.mul0);
      put(2, 0, pack16(q));
      put(3, 0, zero);
      // the zero strip: tile 0's threads, here only (boff is their offset in the strip); the
      // workspace is shared with other products, so it is written by every call
      if (s.strip && t == 0) *(v4i*)(out + s.zoff + boff) = zero;
    }
    for (int i = 1; i < n; ++i) {
      const uint32_t w[4] = {tab.w[i][0], tab.w[i][1], tab.w[i][2], tab.w[i][3]};
      const uint32_t neg = tab.neg[i];
      const float pf = (float)tab.p[i], rcp = tab.rcp[i];
      const int64_t ioff = i * plane;
      const float nf = (float)neg;
      auto res4 = [&](const uint32_t (&x)[16][NW], int u, float (&f)[4])
                      __attribute__((always_inline)) {
        if constexpr (PK) {
#pragma unroll
          for (int j = 0; j < 4; j += 2) {
            const f2 g = residue2_f<NW>(x[4 * u + j], x[4 * u + j + 1], w, neg, pf, rcp);
            f[j] = g.x;
            f[j + 1] = g.y;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) f[j] = residue_f<NW>(x[4 * u + j], w, neg, pf, rcp);
        }
      };
      // four elements at a time through all three, so that only their residues are held
      v4i o_r, o_v, o_s;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float fr[4], fv[4], fs[4];
        if (do_r) {
          res4(rr, u, fr);
          o_r[u] = (int)pack4((int)fr[0], (int)fr[1], (int)fr[2], (int)fr[3]);
        }
        if (do_v) {
          res4(v, u, fv);
          o_v[u] = (int)pack4((int)fv[0], (int)fv[1], (int)fv[2], (int)fv[3]);
        }
        if (has[2]) {  // both residues are at hand
          if constexpr (PK) {
#pragma unroll
            for (int j = 0; j < 4; j += 2) {
              const f2 g = crt_combine2((f2){fr[j], fr[j + 1]}, (f2){fv[j], fv[j + 1]},
                                        (f2){kf[4 * u + j], kf[4 * u + j + 1]}, nf, pf, rcp);
              fs[j] = g.x;
              fs[j + 1] = g.y;
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              fs[j] = crt_combine_f(fr[j], fv[j], kf[4 * u + j], nf, pf, rcp);
          }
          o_s[u] = (int)pack4((int)fs[0], (int)fs[1], (int)fs[2], (int)fs[3]);
        }
      }
      put(0, ioff, o_r);
      put(1, ioff, o_v);
      put(2, ioff, o_s);
      put(3, ioff, zero);
    }
  }
}

// o = a + b over n ring elements (run_crt_asym's party-0 A' sum, written once so that its
// residue image streams one operand: the two-operand prep ran at ~2.4 plain images)
template <class T>
__global__ void __launch_bounds__(256)
    k_add_pair(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ o, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    o[i] = a[i] + b[i];
}

// XCD-aware remap (as gemm_mfma.hip): consecutive tile ids land on one XCD
__device__ inline int64_t xcd_remap(int64_t bid, int64_t nwg) {
  const int64_t q = nwg / 8, r = nwg % 8;
  const int64_t x = bid % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
}

// s_waitcnt vmcnt(N) lgkmcnt(0) expcnt(7), gfx9 encoding (vmcnt split 4 + 2 bits)
constexpr int waitcnt_vm_lgkm0(int vm) { return (vm & 15) | ((vm >> 4) << 14) | (7 << 4); }

__device__ __forceinline__ int centered_mod(int acc, float pf, float rcp, int t16) {
  // acc = hi 2^16 + lo; s = hi (2^16 mod p) + lo is exact in fp32 (|s| < 2^24)
  const int hi = acc >> 16, lo = acc & 0xffff;
  const int s = __mul24(hi, t16) + lo;
  const float fs = (float)s;
  const float qt = __builtin_rintf(fs * rcp);
  return (int)__builtin_fmaf(-qt, pf, fs);
}

// The GEMM: one v_mfma_i32_16x16x64_i8 covers a whole 64-byte k-step, lane l reads
// row l & 15, chunk l >> 4 of the image.  WR x WC waves, wave tile (BM/WR) x (BN/WC) =
// MI x NJ MFMA blocks of 16x16 (4 accumulator registers each): <2,4> is 8 waves of 128x64
// (two waves per SIMD, so one wave's LDS reads, address arithmetic and barrier waits hide
// behind its partner's MFMAs), <2,2> 4 waves.  IL == 0: fragments of stage kb+1 are
// read right after the step's barrier into the second register set (the k-loop is unrolled
// by two so the sets swap without moves), while the second half of stage kb's MFMAs runs.
// Output bytes: 16x16 block (bi, bj) at ((bi * BN / 16 + bj) * 64 + lane) * 4 of the tile.
template <int WR, int WC, int BN, int MINW, int STG = kStages, int IL = 0>
__global__ void __launch_bounds__(64 * WR * WC, MINW)
    k_crt_gemm16(const int8_t* __restrict__ RA, const int8_t* __restrict__ RB,
                 int8_t* __restrict__ CR, int tiles_m, int tiles_n, int nkb_all, int gM,
                 const EpiTab ep, int bcast, int a_nkb, int roll, int amap, int bmap) {
  constexpr int NW = WR * WC;
  constexpr int MI = BM / WR / 16, NJ = BN / WC / 16;
  constexpr int NM = MI * NJ;                    // MFMAs per wave per k-step
  constexpr int kImgB = BN * BK;
  constexpr int kStageBytes = kImg + kImgB;
  constexpr int NPIECE = kStageBytes / 1024;
  constexpr int PPW = NPIECE / NW;
  static_assert(PPW * NW == NPIECE, "stage pieces must split evenly over the waves");
  extern __shared__ __attribute__((aligned(16))) int8_t smem[];
  const int ntiles = tiles_m * tiles_n;
  const int tid_flat = (int)xcd_remap(blockIdx.x, ntiles);
  const int group = tid_flat / (gM * tiles_n);
  const int first_m = group * gM;
  const int gm = tiles_m - first_m < gM ? tiles_m - first_m : gM;
  const int in_group = tid_flat % (gM * tiles_n);
  const int tm = first_m + in_group % gm, tn = in_group / gm;
  // amap < 0 (bit 31): the asymmetric three-party product (run_crt_asym) -- the parties with
  // the full K' (1 and 2) are dispatched first, party 0's half-length blocks fill the tail
  const int g = amap < 0 ? (int)((blockIdx.y + ep.n) % gridDim.y) : (int)blockIdx.y;
  const int mi = g % ep.n;
  int nkb = nkb_all;
  const int8_t* ga = RA + ((int64_t)((bcast & 1) ? mi : g) * tiles_m + tm) * a_nkb * (int64_t)kImg;
  const int8_t* gb = RB + ((int64_t)((bcast & 2) ? mi : g) * tiles_n + tn) * nkb_all * (int64_t)kImgB;
  // roll != 0: A' = [x_b | x_{b+roll}] (an RSS pair whose second share is the next party's
  // first) -- the image holds each batch entry's K residues once; k-blocks from a_nkb on
  // read entry b + roll's image (ga2 is biased so that ga2 + kb * kImg addresses it)
  const int8_t* ga2 = ga;
  const int8_t* gb2 = gb;
  int khalf = 1 << 30;
  if (roll) {
    const int nbt = (int)gridDim.y / ep.n;
    const int b2 = (g / ep.n + roll) % nbt;
    ga2 = RA + ((int64_t)(b2 * ep.n + mi) * tiles_m + tm) * a_nkb * (int64_t)kImg -
          (int64_t)a_nkb * kImg;
    khalf = a_nkb;
  } else if (amap < 0) {
    // party b reads A' = [entry e1 | entry e2] of the K-residue A image and
    // B' = [entry f1 ; entry f2] of the K-residue B image (bmap), or only (e1, f1)'s K
    // (k-steps [0, a_nkb): party 0's one-GEMM product) when its half bit is set
    const int sh = 8 * (g / ep.n);
    const int e1 = (amap >> sh) & 7, e2 = (amap >> (sh + 3)) & 7;
    const int f1 = (bmap >> sh) & 7, f2 = (bmap >> (sh + 3)) & 7;
    // Entry kZeroStrip: an all-zero image, held as one (modulus, tile) strip of a_nkb
    // k-steps right below the side's images and read for every modulus and tile (a fresh
    // sharing's zero slot, run_crt_asym); ga2 / gb2 keep their bias of a_nkb k-steps.
    const int64_t sa_ = (int64_t)a_nkb * kImg, sb_ = (int64_t)a_nkb * kImgB;
    ga = e1 == kZeroStrip ? RA - sa_ : RA + ((int64_t)(e1 * ep.n + mi) * tiles_m + tm) * sa_;
    ga2 = (e2 == kZeroStrip ? RA - sa_ : RA + ((int64_t)(e2 * ep.n + mi) * tiles_m + tm) * sa_) -
          sa_;
    gb = f1 == kZeroStrip ? RB - sb_ : RB + ((int64_t)(f1 * ep.n + mi) * tiles_n + tn) * sb_;
    gb2 = (f2 == kZeroStrip ? RB - sb_ : RB + ((int64_t)(f2 * ep.n + mi) * tiles_n + tn) * sb_) -
          sb_;
    khalf = a_nkb;
    if ((amap >> (sh + 6)) & 1) nkb = a_nkb;
  }

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave / WC, wc = wave % WC;
  const int co = 16 * ((lane >> 4) ^ swz((lane & 15) >> 2));
  const int rowa = (wr * (BM / WR) + (lane & 15)) * BK + co;
  const int rowb = kImg + (wc * (BN / WC) + (lane & 15)) * BK + co;

  const int8_t* srcs[PPW];
  const int8_t* srcs2[PPW];
  int dsts[PPW], steps[PPW];
#pragma unroll
  for (int t = 0; t < PPW; ++t) {
    const int pc = wave + NW * t;
    const bool is_b = pc >= 16;
    const int pp = is_b ? pc - 16 : pc;
    srcs[t] = (is_b ? gb : ga) + pp * 1024 + lane * 16;
    srcs2[t] = (is_b ? gb2 : ga2) + pp * 1024 + lane * 16;
    dsts[t] = (is_b ? kImg : 0) + pp * 1024;
    steps[t] = is_b ? kImgB : kImg;
  }
  auto dma = [&](int kb, int t, int8_t* dst_stage) {
    const int8_t* src = kb >= khalf ? srcs2[t] : srcs[t];
    __builtin_amdgcn_global_load_lds((const void*)(src + (int64_t)kb * steps[t]),
                                     (__attribute__((address_space(3))) void*)(dst_stage + dsts[t]),
                                     16, 0, 0);
  };

  v4i acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = v4i{0, 0, 0, 0};

  v4i fa0[MI], fb0[NJ], fa1[MI], fb1[NJ];
  auto frags = [&](const int8_t* st, v4i(&fa)[MI], v4i(&fb)[NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i) fa[i] = *(const v4i*)(st + rowa + i * 16 * BK);
#pragma unroll
    for (int j = 0; j < NJ; ++j) fb[j] = *(const v4i*)(st + rowb + j * 16 * BK);
  };

  // IL == 3 (STG == 5): one barrier per TWO k-steps; the prologue issues stages 0..3 and
  // waits for 0..2 (stage 3 may still be in flight)
  constexpr int PRO = IL == 3 ? 4 : STG;
#pragma unroll
  for (int s = 0; s < PRO; ++s)
#pragma unroll
    for (int t = 0; t < PPW; ++t) dma(s < nkb ? s : nkb - 1, t, smem + s * kStageBytes);
  __builtin_amdgcn_s_waitcnt(waitcnt_vm_lgkm0((PRO - 1) * PPW));
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  frags(smem, fa0, fb0);

  // one k-step: MFMAs of the stage in registers (fa, fb); after the first half, the barrier
  // (stage kb+1 landed everywhere, stage kb no longer read) and the reads of stage kb+1 into
  // (na, nb); the DMA of stage kb+3 into the freed buffer runs beside the second half
  auto step = [&](int kb, int8_t* cur, int8_t* nxt, v4i(&fa)[MI], v4i(&fb)[NJ], v4i(&na)[MI],
                  v4i(&nbf)[NJ]) __attribute__((always_inline)) {
    const int kn = kb + STG < nkb ? kb + STG : nkb - 1;
#pragma unroll MI
    for (int i = 0; i < MI; ++i) {
      if (i == MI / 2) {
        __builtin_amdgcn_s_waitcnt(waitcnt_vm_lgkm0((STG - 2) * PPW));
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        frags(nxt, na, nbf);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll NJ
      for (int j = 0; j < NJ; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        const int h = (i - MI / 2) * NJ + j;  // MFMA index in the second half
#pragma unroll PPW
        for (int t = 0; t < PPW; ++t)
          if (h == (t + 1) * (NM / 2) / PPW - 1) {
            dma(kn, t, cur);
            __builtin_amdgcn_sched_barrier(0);
          }
      }
    }
  };

  // IL: one barrier at the START of each k-step (stage kb+1 landed everywhere, stage kb's
  // buffer no longer read), then the step's MFMAs with the next stage's fragment reads
  // spread one per GAP MFMAs and the DMAs of stage kb+STG in the last gaps -- instead of
  // every wave bursting its 12 fragment reads into the LDS right after a mid-step barrier
  auto rd_frag = [&](const int8_t* st, int q, v4i(&fa)[MI], v4i(&fb)[NJ])
                     __attribute__((always_inline)) {
    if (q < MI)
      fa[q] = *(const v4i*)(st + rowa + q * 16 * BK);
    else
      fb[q - MI] = *(const v4i*)(st + rowb + (q - MI) * 16 * BK);
  };
  auto step_il = [&](int kb, int8_t* cur, int8_t* nxt, v4i(&fa)[MI], v4i(&fb)[NJ],
                     v4i(&na)[MI], v4i(&nbf)[NJ]) __attribute__((always_inline)) {
    const int kn = kb + STG < nkb ? kb + STG : nkb - 1;
    constexpr int NR = MI + NJ;
    constexpr int GAP = (NM - 2 * PPW) / NR > 0 ? (NM - 2 * PPW) / NR : 1;
    __builtin_amdgcn_s_waitcnt(waitcnt_vm_lgkm0((STG - 2) * PPW));
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // IL == 2: the NR reads and PPW DMAs share the NM/2 odd gaps, a DMA in every
    // (NR + PPW)/PPW-th of them (so the DMAs spread over the whole step)
    constexpr int NMEM = NR + PPW, DEV = NMEM / PPW;
#pragma unroll
    for (int h = 0; h < NM; ++h) {
      const int i = h / NJ, j = h % NJ;
      acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (IL == 2) {
        if (h % 2 == 1 && h / 2 < NMEM) {
          const int u = h / 2;
          if (u % DEV == DEV - 1 && u / DEV < PPW) {
            dma(kn, u / DEV, cur);
          } else {
            const int q = u - (u / DEV < PPW ? u / DEV : PPW);
            if (q < NR) rd_frag(nxt, q, na, nbf);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        if (h % GAP == GAP - 1 && h / GAP < NR) {
          rd_frag(nxt, h / GAP, na, nbf);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll PPW
        for (int t = 0; t < PPW; ++t)
          if (h == NM - 2 * PPW + 2 * t + 1) {
            dma(kn, t, cur);
            __builtin_amdgcn_sched_barrier(0);
          }
      }
    }
  };

  // IL == 3: five 32 KB stage buffers (160 KB), stage s in buffer s % 5, a barrier only at
  // even k-steps.  Barrier B_k (even k) follows each wave's wait for its DMAs of stages
  // k+1 and k+2 (only stage k+3's may still be in flight), so step k reads stage k+1 and
  // step k+1 reads stage k+2 without a barrier of its own; and every wave has finished
  // step k-1, so the buffers of stages k-1 and k (fragments already in registers) are free
  // and take stages k+4 and k+5 -- issued in that order, the k+4 pieces first, so that
  // "all but the last PPW" is exactly "all but stage k+5".
  auto step_pair = [&](int kb, bool even, v4i(&fa)[MI], v4i(&fb)[NJ], v4i(&na)[MI],
                       v4i(&nbf)[NJ]) __attribute__((always_inline)) {
    constexpr int NR = MI + NJ;
    constexpr int GAP = (NM - 2 * PPW) / NR > 0 ? (NM - 2 * PPW) / NR : 1;
    const int8_t* nxt = smem + ((kb + 1) % STG) * kStageBytes;
    int8_t* d4 = smem + ((kb + 4) % STG) * kStageBytes;
    int8_t* d5 = smem + ((kb + 5) % STG) * kStageBytes;
    const int k4 = kb + 4 < nkb ? kb + 4 : nkb - 1;
    const int k5 = kb + 5 < nkb ? kb + 5 : nkb - 1;
    if (even) {
      __builtin_amdgcn_s_waitcnt(waitcnt_vm_lgkm0(PPW));
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int h = 0; h < NM; ++h) {
      const int i = h / NJ, j = h % NJ;
      acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (h % GAP == GAP - 1 && h / GAP < NR) {
        rd_frag(nxt, h / GAP, na, nbf);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (even) {
#pragma unroll PPW
        for (int t = 0; t < PPW; ++t) {
          if (h == NM - 2 * PPW + t) {
            dma(k4, t, d4);
            __builtin_amdgcn_sched_barrier(0);
          }
          if (h == NM - PPW + t) {
            dma(k5, t, d5);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
  };

  auto buf = [&](int i) { return smem + i * kStageBytes; };
  int r = 0;  // stage kb lives in buf(r)
  if constexpr (IL == 3) {
    static_assert(STG == 5, "the paired schedule needs five stage buffers");
    for (int kb = 0; kb < nkb; kb += 2) {
      step_pair(kb, true, fa0, fb0, fa1, fb1);
      if (kb + 1 < nkb) step_pair(kb + 1, false, fa1, fb1, fa0, fb0);
    }
  } else
  for (int kb = 0; kb < nkb; kb += 2) {
    if constexpr (IL)
      step_il(kb, buf(r), buf(r == STG - 1 ? 0 : r + 1), fa0, fb0, fa1, fb1);
    else
      step(kb, buf(r), buf(r == STG - 1 ? 0 : r + 1), fa0, fb0, fa1, fb1);
    r = r == STG - 1 ? 0 : r + 1;
    if (kb + 1 < nkb) {
      if constexpr (IL)
        step_il(kb + 1, buf(r), buf(r == STG - 1 ? 0 : r + 1), fa1, fb1, fa0, fb0);
      else
        step(kb + 1, buf(r), buf(r == STG - 1 ? 0 : r + 1), fa1, fb1, fa0, fb0);
      r = r == STG - 1 ? 0 : r + 1;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  const float pf = ep.pf[mi], rcp = ep.rcp[mi];
  const int t16 = ep.t16[mi];
  int8_t* cr = CR + ((int64_t)g * ntiles + tm * tiles_n + tn) * (int64_t)(BM * BN);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      int rr[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        rr[e] = centered_mod(acc[i][j][e], pf, rcp, t16);
      const int bi = wr * MI + i, bj = wc * NJ + j;
      *(uint32_t*)(cr + ((bi * (BN / 16) + bj) * 64 + lane) * 4) = pack4(rr[0], rr[1], rr[2], rr[3]);
    }
}

// Reconstruction, one thread's share: the 4 elements (rows 4 * (lane >> 4) + e of a 16x16
// block, one column) whose residue bytes are the dword at ``src`` of every modulus plane,
// pstride apart.  The multiply-add form (MOOSEX_CRT_RECON=0): per modulus and element one
// float fma for the quotient and a 24-bit multiply-add per 16-bit word of W_i.  In two steps,
// the sums and then one element at a time, so that the caller's index arithmetic (a 64-bit
// division) sits between them, where only the sums are live (else the u128 form loses a wave
// of occupancy).
template <class T>
struct Recon16m {
  static constexpr int NK = sizeof(T) / 2;
  int acc[4][NK];
  float qs[4];
  __device__ __forceinline__ void sums(const int8_t* __restrict__ src, int64_t pstride, int n,
                                       const RecTab& rc) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qs[e] = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k) acc[e][k] = 0;
    }
    for (int i = 0; i < n; ++i) {
      const uint32_t v = *(const uint32_t*)(src + i * pstride);
      const float rcp = rc.rcp[i];
      int wk[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) wk[k] = rc.W[i][k];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = (int)(int8_t)((v >> (8 * e)) & 0xff);
        qs[e] = __builtin_fmaf((float)c, rcp, qs[e]);
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[e][k] += __mul24(c, wk[k]);
      }
    }
  }
  static __device__ __forceinline__ T modulus(const RecTab& rc) {  // M mod 2^w
    T mw = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) mw |= (T)rc.Mw[k] << (16 * k);
    return mw;
  }
  __device__ __forceinline__ T element(int e, T mw) const {
    T z = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) z += (T)(int64_t)acc[e][k] << (16 * k);
    const int q = (int)__builtin_rintf(qs[e]);
    z -= (T)(int64_t)q * mw;
    return z;
  }
};

// The same with the per-modulus multiply-adds done as v_dot4_i32_i8 (the default): a thread's
// 4 elements x 4 moduli of residues (4 dwords, one per modulus plane) are transposed with 8
// v_perm_b32 into one dword of 4 moduli per element, then one dot4 per (element, W digit)
// and per (element, R digit) -- 19 dot4 for 4 moduli instead of 4 x (8 multiply-adds + a
// float convert and fma).  q = round(sum_i c_i R_i / 2^24) (error <= 36 * 128 / 2^25, far
// inside the 0.05 rounding margin of |Z| <= 0.45 M).  Same output as Recon16m.
template <class T>
__device__ __forceinline__ void recon16d_lane(const int8_t* __restrict__ src, int64_t pstride,
                                              int n, const RecTab4& r4, const RecTab& rc,
                                              T (&z)[4]) {
  constexpr int ND = (int)sizeof(T);  // W digits
  constexpr int NK = ND / 2;
  int acc[4][ND], aq[4][3];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int d = 0; d < ND; ++d) acc[e][d] = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) aq[e][d] = 0;
  }
  for (int g = 0; g < r4.groups; ++g) {
    uint32_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      v[u] = 4 * g + u < n ? *(const uint32_t*)(src + (4 * g + u) * pstride) : 0u;
    const uint32_t a0 = __builtin_amdgcn_perm(v[1], v[0], 0x05010400u);
    const uint32_t a1 = __builtin_amdgcn_perm(v[1], v[0], 0x07030602u);
    const uint32_t c0 = __builtin_amdgcn_perm(v[3], v[2], 0x05010400u);
    const uint32_t c1 = __builtin_amdgcn_perm(v[3], v[2], 0x07030602u);
    const int t[4] = {(int)__builtin_amdgcn_perm(c0, a0, 0x05040100u),
                      (int)__builtin_amdgcn_perm(c0, a0, 0x07060302u),
                      (int)__builtin_amdgcn_perm(c1, a1, 0x05040100u),
                      (int)__builtin_amdgcn_perm(c1, a1, 0x07060302u)};
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int w = (int)r4.wd[g][d];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e][d] = __builtin_amdgcn_sdot4(t[e], w, acc[e][d], false);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int w = (int)r4.rd[g][d];
#pragma unroll
      for (int e = 0; e < 4; ++e) aq[e][d] = __builtin_amdgcn_sdot4(t[e], w, aq[e][d], false);
    }
  }
  T mw = 0;
#pragma unroll
  for (int k = 0; k < NK; ++k) mw |= (T)rc.Mw[k] << (16 * k);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    T s = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k)
      s += (T)(int64_t)(acc[e][2 * k] + acc[e][2 * k + 1] * 256) << (16 * k);
    const int64_t F = (int64_t)aq[e][0] + (int64_t)aq[e][1] * 256 + (int64_t)aq[e][2] * 65536;
    const int64_t q = (F + (1 << 23)) >> 24;
    z[e] = s - (T)q * mw;
  }
}

// Reconstruction of k_crt_gemm16's output: one thread = one lane's 4 bytes of a 16x16 block of
// every modulus, by the dot4 form (DOT4) or the multiply-add form.
template <class T, int BN, bool DOT4>
__global__ void __launch_bounds__(256)
    k_crt_recon16(const int8_t* __restrict__ CR, T* __restrict__ C, int64_t M, int64_t N,
                  int64_t tiles_m, int64_t tiles_n, int accumulate, const RecTab4 r4, int n,
                  const RecTab rc) {
  constexpr int kCrTile = BM * BN, NBJ = BN / 16;
  const int64_t ntiles = tiles_m * tiles_n;
  const int64_t total = ntiles * (kCrTile / 4);
  const int64_t b = blockIdx.y;
  for (int64_t gt = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; gt < total;
       gt += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(gt & 63);
    const int64_t rest = gt >> 6;
    const int blk = (int)(rest % (16 * NBJ));
    const int64_t tile = rest / (16 * NBJ);
    const int64_t off = tile * kCrTile + (blk * 64 + lane) * 4;
    const int64_t pstride = ntiles * (int64_t)kCrTile;
    T zd[4];
    Recon16m<T> zm;
    if constexpr (DOT4)
      recon16d_lane<T>(CR + b * n * pstride + off, pstride, n, r4, rc, zd);
    else
      zm.sums(CR + b * n * pstride + off, pstride, n, rc);
    const int64_t tm = tile / tiles_n, tn = tile % tiles_n;
    const int bi = blk / NBJ, bj = blk % NBJ;
    const int64_t gcol = tn * BN + bj * 16 + (lane & 15);
    const T mw = Recon16m<T>::modulus(rc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t grow = tm * BM + bi * 16 + 4 * (lane >> 4) + e;
      T z;
      if constexpr (DOT4)
        z = zd[e];
      else
        z = zm.element(e, mw);
      if (grow < M && gcol < N) {
        T* pc = C + (b * M + grow) * N + gcol;
        *pc = accumulate ? (T)(*pc + z) : z;
      }
    }
  }
}

// The dot4 reconstruction of a three-party product that is only revealed, with the opening on
// the way (the tail of k_mul_trunc3_open: zero share + reshare + TruncPr by m + reveal +
// decode): the
// opened value needs the SUM of the parties' products and r = r0 + r1 of TruncPr's draws
// only (mxf::trunc_pr_open), so the products never go to memory and seven of the tail's nine
// keystreams are not drawn.  A workgroup takes strips of 8 rows x one tile's 256 columns:
//   1. wave w draws r for rows w and w + 4 -- a row's 256 elements are one or two groups of
//      64 ChaCha blocks (walk_chunks' mapping: block B of group G holds chunks G * 256 +
//      64 * part + lane), keys k0 / k2 and nonces nr0 / nr1 as the tail -- into LDS;
//   2. after a barrier, thread t rebuilds 4 rows x 1 column of every party twice (columns
//      0..127, then 128..255; a wave reads whole 128-byte lines: 32 lanes of a block), adds
//      the three, takes its r values from LDS and stores 8 B per element.
// Bitwise k_crt_recon16<T, 256, true> followed by k_mul_trunc3_open<T>.
template <class T>
__global__ void __launch_bounds__(256)
    k_crt_recon16d_open(const int8_t* __restrict__ CR, double* __restrict__ out, double scale,
                        int64_t M, int64_t N, int64_t tiles_n, int64_t pstride,
                        const RecTab4 r4, int n, const RecTab rc, mxd::KeySrc keys, uint64_t nr0,
                        uint64_t nr1, int m) {
  constexpr int BN = 256, kCrTile = BM * BN, P = mxd::Lane<T>::kPer;
  __shared__ uint32_t rks[3][mxd::kKeyWords];
  __shared__ T rr[8][BN];
  mxd::stage_keys(rks, keys, 3);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t strips = ((M + 7) / 8) * tiles_n;
  for (int64_t s = blockIdx.x; s < strips; s += gridDim.x) {
    const int64_t row0 = (s / tiles_n) * 8, tn = s % tiles_n, col0 = tn * BN;
    const int64_t ncol = N - col0 < BN ? N - col0 : BN;
    for (int i = wave; i < 8; i += 4) {
      if (row0 + i >= M) break;
      const int64_t f0 = (row0 + i) * N + col0, f1 = f0 + ncol;  // the row's flat elements
      for (int64_t G = (f0 / P) >> 8; G <= ((f1 - 1) / P) >> 8; ++G) {
        const uint64_t B = ((uint64_t)G << 6) | (uint64_t)lane;
        uint32_t w0[16], w1[16];
        mx::chacha_block(rks[0], nr0, B, w0);
        mx::chacha_block(rks[2], nr1, B, w1);
#pragma unroll
        for (int part = 0; part < 4; ++part) {
          const int64_t c = (int64_t)mx::ks_chunk(B, part);
          uint64_t lo0, hi0, lo1, hi1;
          mx::part_u64(w0, part, &lo0, &hi0);
          mx::part_u64(w1, part, &lo1, &hi1);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const int64_t e = c * P + j;
            if (e >= f0 && e < f1)
              rr[i][e - f0] = mxd::pick<T>(lo0, hi0, j) + mxd::pick<T>(lo1, hi1, j);
          }
        }
      }
    }
    __syncthreads();
    const int q = (tid >> 4) & 1;
    const int64_t grow0 = row0 + 4 * q;
    const int64_t tile = (grow0 / BM) * tiles_n + tn;
    const int bi = (int)(grow0 % BM) / 16, l16 = ((int)(grow0 % 16) / 4) * 16 + (tid & 15);
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const int ct = h * 128 + (tid >> 5) * 16 + (tid & 15);  // column within the tile
      if (grow0 >= M || ct >= ncol) continue;
      const int64_t off = tile * kCrTile + ((bi * (BN / 16) + ct / 16) * 64 + l16) * 4;
      T x[4] = {0, 0, 0, 0};
#pragma unroll 1
      for (int b = 0; b < 3; ++b) {
        T z[4];
        recon16d_lane<T>(CR + b * n * pstride + off, pstride, n, r4, rc, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] += z[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (grow0 + e < M)
          out[(grow0 + e) * N + col0 + ct] =
              mxr::signed_to_f64<T>(mxf::trunc_pr_open<T>(x[e], rr[4 * q + e][ct], m)) * scale;
    }
    __syncthreads();
  }
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// An on/off switch of the environment; every caller caches it at first use (static const).
// Default on: off with a leading '0'; default off: on with a leading '1'.
bool env_flag(const char* name, bool dflt) {
  const char* e = std::getenv(name);
  return dflt ? !(e && e[0] == '0') : (e && e[0] == '1');
}
bool recon_dot4() {  // MOOSEX_CRT_RECON=0: the multiply-add reconstruction
  static const bool v = env_flag("MOOSEX_CRT_RECON", true);
  return v;
}
int launch_status() {  // the code an entry point returns after its launches
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? -100 - (int)e : 0;
}

int gemm_group_m() {  // 8: 0.02-0.07 ms per headline step faster than 4 (profiles/r6_asym_products.md)
  const char* e = std::getenv("MOOSEX_CRT_GROUPM");
  const int v = e ? std::atoi(e) : 8;
  return v >= 1 && v <= 64 ? v : 8;
}

struct Variant;
struct CPlan {
  const Variant* var;  // the GEMM variant of the product: tile width, LDS size, kernel
  int n, bn;
  int64_t tiles_m, tiles_n, nkb, a_nkb, ra_bytes, rb_bytes, cr_bytes;
};

// bcast bit 0 / 1: A / B residues were prepared once for every batch entry; roll, amap, bmap:
// k_crt_gemm16's
struct GemmArgs {
  int64_t batch;
  const int8_t *ra, *rb;
  int8_t* cr;
  int bcast, roll, amap, bmap;
};

template <int WR, int WC, int BN, int MINW, int STG, int IL>
void launch_variant(const CPlan& p, const Tables& tb, const GemmArgs& a, hipStream_t st) {
  constexpr int lds = STG * (kImg + BN * BK);
  ensure_lds_attr((const void*)k_crt_gemm16<WR, WC, BN, MINW, STG, IL>, lds, st);
  const dim3 grid((unsigned)(p.tiles_m * p.tiles_n), (unsigned)(a.batch * p.n));
  hipLaunchKernelGGL((k_crt_gemm16<WR, WC, BN, MINW, STG, IL>), grid, dim3(64 * WR * WC), lds, st,
                     a.ra, a.rb, a.cr, (int)p.tiles_m, (int)p.tiles_n, (int)p.nkb,
                     gemm_group_m(), tb.ep, a.bcast, (int)p.a_nkb, a.roll, a.amap, a.bmap);
}

// One record per GEMM variant, <WR, WC, BN, MINW, STG, IL> of k_crt_gemm16: the plan's B' tile
// width and the launched instantiation (with its LDS size) come from the same record.  What
// each was measured at, and the variants that were tried and retired, are in
// profiles/README.md ("CRT GEMM variants").
struct Variant {
  int id, bn;
  void (*launch)(const CPlan&, const Tables&, const GemmArgs&, hipStream_t);
};
template <int WR, int WC, int BN, int MINW, int STG, int IL>
constexpr Variant variant(int id) {
  return {id, BN, &launch_variant<WR, WC, BN, MINW, STG, IL>};
}
constexpr int kDefaultVariant = 8;
const Variant kVariants[] = {
    variant<2, 2, 128, 2, 3, 0>(5),   // 4 waves of 128x64, 256x128 tiles, 72 KB LDS: 2 blocks per CU
    variant<2, 4, 256, 2, 3, 0>(6),   // 8 waves of 128x64, 256x256 tiles, 96 KB LDS: 1 block per CU
    variant<2, 4, 256, 2, 3, 1>(8),   // 6 with one barrier at the start of a k-step, reads spread
    variant<2, 2, 256, 1, 3, 1>(12),  // 4 waves of 128x128 with 8's schedule (VGPR-form MFMA flag)
    variant<2, 2, 256, 1, 3, 2>(14),  // 12 with the DMAs spread over the step too
    variant<2, 4, 256, 2, 5, 3>(16),  // 8 with one barrier per two k-steps, five stages (160 KB)
};

// MOOSEX_CRT_KERNEL, read on every call: the record of that id; every other value (a retired
// id, text that is no number) selects the default.
const Variant& crt_variant() {
  const char* e = std::getenv("MOOSEX_CRT_KERNEL");
  const int v = e ? std::atoi(e) : kDefaultVariant;
  const Variant* dflt = nullptr;
  for (const Variant& r : kVariants) {
    if (r.id == v) return r;
    if (r.id == kDefaultVariant) dflt = &r;
  }
  return *dflt;
}

// roll: the A' image holds each batch entry's K residues once (k_crt_gemm16's roll)
CPlan make_cplan(int words, int64_t batch, int64_t M, int64_t N, int64_t K, int mode,
                 bool roll = false) {
  CPlan p;
  p.var = &crt_variant();
  p.bn = p.var->bn;  // B tile columns
  const int64_t kprime = mode ? 2 * K : K;
  p.n = moduli_needed(words, kprime);
  p.tiles_m = (M + BM - 1) / BM;
  p.tiles_n = (N + p.bn - 1) / p.bn;
  p.nkb = round_up(kprime, BK) / BK;
  p.a_nkb = roll ? p.nkb / 2 : p.nkb;
  p.ra_bytes = batch * p.n * p.tiles_m * p.a_nkb * (int64_t)kImg;
  p.rb_bytes = batch * p.n * p.tiles_n * p.nkb * (int64_t)(p.bn * BK);
  p.cr_bytes = batch * p.n * p.tiles_m * p.tiles_n * (int64_t)(BM * p.bn);
  return p;
}

// One dispatch per axis: f gets the plan's B' tile width, a switch, or the ring type of
// ``words`` (with_ring: -2 for any other) as a constant.
template <int V>
using int_c = std::integral_constant<int, V>;
template <class F>
auto with_bn(int bn, F&& f) {
  return bn == 256 ? f(int_c<256>()) : f(int_c<128>());
}
template <class F>
auto with_bool(bool b, F&& f) {
  return b ? f(std::true_type()) : f(std::false_type());
}
template <class F>
int with_ring(int words, F&& f) {
  if (words == 1) return f(u64());
  if (words == 2) return f(u128());
  return -2;
}

template <class T>
void launch_prep(const CPlan& p, const Tables& tb, bool is_b, int64_t batch, int64_t R,
                 int64_t K, int64_t xs, const T* X0, const T* X1, int mode, int8_t* out,
                 hipStream_t st, int64_t nkb = -1, int64_t nkb_s = -1,
                 const PrepSrcs& src = PrepSrcs()) {
  if (nkb < 0) nkb = p.nkb;
  if (nkb_s < nkb) nkb_s = nkb;
  const int64_t tiles = is_b ? p.tiles_n : p.tiles_m;
  const int rows = is_b ? p.bn : BM;
  const int64_t work = tiles * nkb * (rows * 4);
  const dim3 grid((unsigned)std::min<int64_t>((work + 255) / 256, 16384), (unsigned)batch);
  // packed residues pay on A' (0.626 -> 0.592 ms at 4096^2) but not on the B' image, which
  // streams 1.5x the bytes and loses more to the extra VGPRs (1.128 -> 1.163 ms)
  // MOOSEX_CRT_PACKED=0: one at a time everywhere; MOOSEX_CRT_PACKED_B=1: packed on B' too
  static const bool packed = env_flag("MOOSEX_CRT_PACKED", true);
  static const bool packed_b = env_flag("MOOSEX_CRT_PACKED_B", false);
  with_bool(packed && (!is_b || packed_b), [&](auto pk) {
    auto go = [&](auto trans, auto nrows) {
      hipLaunchKernelGGL(
          (k_crt_prep<T, decltype(trans)::value, decltype(nrows)::value, decltype(pk)::value>),
          grid, dim3(256), 0, st, X0, X1, R, K, xs, mode, out, tiles, nkb, nkb_s,
          is_b ? tb.pb : tb.pa, src);
    };
    if (!is_b)
      go(std::false_type(), int_c<BM>());
    else
      with_bn(rows, [&](auto bn) { go(std::true_type(), bn); });
  });
}

bool share_src_ok(const ShareSrc& s) {
  const int kind = s.kind & ~MX_SHARE_MIRROR;
  return s.x && (kind == MX_CROSS_ARITH || kind == MX_SHARE_F64) && s.j0 >= 0 && s.j0 < 3;
}

// The phase (SrcPlan) of each of the four K-residue images of one side of run_crt_asym's
// rolled product from a share source (A: [x0 + x1, x2, x1, x0], B: [y0 + y1, y1 + y2, y2, y0]).
void src_phases(bool is_b, const ShareSrc& src, int (&ph)[4]) {
  static const int kSlotsA[4][2] = {{0, 1}, {2, -1}, {1, -1}, {0, -1}};
  static const int kSlotsB[4][2] = {{0, 1}, {1, 2}, {2, -1}, {0, -1}};
  int jr, jv;
  mxf::share_place(src.j0, (src.kind & MX_SHARE_MIRROR) != 0, &jr, &jv);
  for (int e = 0; e < 4; ++e) {
    const int* sl = is_b ? kSlotsB[e] : kSlotsA[e];
    const bool has_r = sl[0] == jr || sl[1] == jr, has_v = sl[0] == jv || sl[1] == jv;
    ph[e] = has_r && has_v ? 2 : has_r ? 0 : has_v ? 1 : 3;
  }
}

// Those images in one launch: entry e of phase ph[e] at out + at[e] * entry.  at[e] ==
// kZeroStrip (zero phase only): no image -- the prep writes the side's one zero strip at
// out + zoff instead, which the GEMM reads for every modulus and tile of such an entry.
void launch_prep_src(const CPlan& p, const Tables& tb, bool is_b, const ShareSrc& src, int64_t R,
                     int64_t K, int8_t* out, int64_t entry, const int (&ph)[4],
                     const int (&at)[4], int64_t zoff, hipStream_t st) {
  const int kind = src.kind & ~MX_SHARE_MIRROR;
  SrcPlan s;
  s.x = src.x;
  s.kind = kind;
  s.strip = 0;
  s.scale = kind == MX_SHARE_F64 ? std::ldexp(1.0, src.frac) : 0.0;
  s.nonce = src.nonce;
  s.zoff = zoff;
  for (int e = 0; e < 4; ++e) {
    const bool z = at[e] == kZeroStrip;
    s.ph[e] = z ? -1 : ph[e];
    s.off[e] = z ? 0 : at[e] * entry;
    s.strip |= z;
  }
  const int64_t tiles = is_b ? p.tiles_n : p.tiles_m;
  const int rows = is_b ? p.bn : BM;
  const int64_t work = tiles * rows * p.a_nkb * 4;
  const dim3 grid((unsigned)std::min<int64_t>(work / 256, 16384));
  auto go = [&](auto trans, auto nrows, auto pk) {  // A' packed, B' one at a time (launch_prep)
    hipLaunchKernelGGL(
        (k_crt_prep_src<decltype(trans)::value, decltype(nrows)::value, decltype(pk)::value>),
        grid, dim3(256), 0, st, s, src.key, R, K, out, tiles, p.a_nkb, is_b ? tb.pb : tb.pa);
  };
  if (!is_b)
    go(std::false_type(), int_c<BM>(), std::true_type());
  else
    with_bn(rows, [&](auto bn) { go(std::true_type(), bn, std::false_type()); });
}

template <class T>
void launch_recon(const CPlan& p, const Tables& tb, int64_t batch, int64_t M, int64_t N,
                  const int8_t* cr, T* C, int accumulate, hipStream_t st) {
  const int64_t work = p.tiles_m * p.tiles_n * (BM * p.bn / 4);
  const dim3 grid((unsigned)std::min<int64_t>((work + 255) / 256, 16384), (unsigned)batch);
  with_bn(p.bn, [&](auto bn) {
    with_bool(recon_dot4(), [&](auto dot4) {
      hipLaunchKernelGGL((k_crt_recon16<T, decltype(bn)::value, decltype(dot4)::value>), grid,
                         dim3(256), 0, st, cr, C, M, N, p.tiles_m, p.tiles_n, accumulate, tb.r4,
                         p.n, tb.rc);
    });
  });
}

// A product may stop at its residues (run_crt_asym's cr_ext) when they have the layout the
// opening kernel reads: 16x16 blocks in 256-column tiles, the dot4 reconstruction's tables.
bool defer_ok(const CPlan& p) { return p.bn == 256 && recon_dot4() && p.n > 0; }

// run_crt_asym's product: the one place that decides whether it applies.  rc: 0, or the code
// run_crt_asym returns (-7: not applicable, the caller runs the generic form; -6: past the
// exact epilogue rounding bound); p: its plan (nkb = 2K/64, a_nkb = K/64); defer: it may stop
// at its residues.
struct AsymPlan {
  int rc;
  bool defer;
  CPlan p;
};
AsymPlan asym_plan(int words, int64_t M, int64_t N, int64_t K) {
  AsymPlan a = {};
  if ((words != 1 && words != 2) || K % BK)
    a.rc = -7;
  else if (2 * K > (1 << 15))
    a.rc = -6;
  else {
    a.p = make_cplan(words, 3, M, N, K, 1, true);
    a.rc = a.p.n < 0 ? -6 : 0;
  }
  a.defer = a.rc == 0 && defer_ok(a.p);
  return a;
}

template <class T>
void launch_recon_open(const CPlan& p, const Tables& tb, int64_t M, int64_t N, const int8_t* cr,
                       double* out, double scale, const mxd::KeySrc& keys, uint64_t nr0,
                       uint64_t nr1, int m, hipStream_t st) {
  const int64_t strips = ((M + 7) / 8) * p.tiles_n;
  const int64_t pstride = p.tiles_m * p.tiles_n * (int64_t)(BM * 256);
  hipLaunchKernelGGL((k_crt_recon16d_open<T>), dim3((unsigned)std::min<int64_t>(strips, 1 << 20)),
                     dim3(256), 0, st, cr, out, scale, M, N, p.tiles_n, pstride, tb.r4, p.n,
                     tb.rc, keys, nr0, nr1, m);
}

StreamScratch g_scratch;  // the CRT GEMM's own pool (the limb GEMM keeps another)

template <class T>
int run_crt(int64_t batch, int64_t M, int64_t N, int64_t K, const T* A0, const T* A1,
            int64_t a_bstride, const T* B0, const T* B1, int64_t b_bstride,
            const int8_t* rb_pre, int mode, T* C, int accumulate, hipStream_t st,
            int64_t roll = 0) {
  constexpr int words = sizeof(T) / 8;
  if (roll && (mode != 1 || K % BK || a_bstride == 0 || batch < 2 || roll % batch == 0))
    return -7;  // not applicable: the caller runs the two-operand form
  const CPlan p = make_cplan(words, batch, M, N, K, mode, roll != 0);
  if (p.n < 0) return -6;
  if ((mode ? 2 * K : K) > (1 << 15)) return -6;  // exact epilogue rounding bound
  const Tables& tb = tables_for(words, p.n);
  const int64_t need = p.ra_bytes + (rb_pre ? 0 : p.rb_bytes) + p.cr_bytes;
  int8_t* ws = (int8_t*)g_scratch.get(need, st);
  if (!ws) return -4;
  int8_t* ra = ws;
  int8_t* cr = ra + p.ra_bytes;
  const int8_t* rb = rb_pre;
  // an operand broadcast over the batch (stride 0) has its residues prepared once and read
  // by every batch entry's GEMM (every product is still computed)
  const bool a_bc = batch > 1 && a_bstride == 0;
  const bool b_bc = batch > 1 && b_bstride == 0 && !rb_pre;
  if (!rb) {
    int8_t* rbw = cr + p.cr_bytes;
    launch_prep<T>(p, tb, true, b_bc ? 1 : batch, N, K, b_bstride, B0, B1, mode, rbw, st);
    rb = rbw;
  }
  if (roll)  // each entry's own K residues; the GEMM reads entry b + roll's for the 2nd half
    launch_prep<T>(p, tb, false, batch, M, K, a_bstride, A0, A0, 0, ra, st, p.a_nkb);
  else
    launch_prep<T>(p, tb, false, a_bc ? 1 : batch, M, K, a_bstride, A0, A1, mode, ra, st);
  p.var->launch(p, tb, {batch, ra, rb, cr, (a_bc ? 1 : 0) | (b_bc ? 2 : 0),
                        (int)(((roll % batch) + batch) % batch), 0, 0}, st);
  launch_recon<T>(p, tb, batch, M, N, cr, C, accumulate, st);
  return launch_status();
}

// The three parties' local products of a replicated matrix product in the asymmetric
// form: with party p holding (a, b) = (x_p, x_{p+1}) and (c, d) = (y_p, y_{p+1}),
//   z_0 = (a + b)(c + d),   z_1 = b (c + d) + a d,   z_2 = a d + b c,
// which sum to x.y (all nine x_i y_j exactly once) with five K-long GEMMs instead of the
// symmetric form's six (z_p = a (c + d) + b c for every p).  S0/S1, T0/T1: [3][M][K] and
// [3][K][N] share stacks; rolled: S1[p] = S0[p + 1] and T1[p] = T0[p + 1] (a stacked
// session's pair; S1/T1 may be null) -- party 1's b and party 2's a are then the same
// share x_2, whose residues are prepared once (four K-long A' images instead of five).
//
// xs / ys: the operand is a share source instead (ShareSrc; S0 / T0 unused) -- its prep
// shares the plain input in registers (k_crt_prep_src) and the shares are never written.
// Z_2^128, rolled with the dual images, K % 256 == 0 (xs) / N % 256 == 0 (ys) only: -7
// otherwise, nothing launched.  The residue images are byte for byte those of k_share3
// followed by k_crt_prep, except that the zero slot's image is held as one zero strip (below);
// the GEMM reads the same bytes and the reconstruction does not know the difference.
//
// cr_ext: the caller's buffer for the GEMM's output residues (defer_bytes) -- the product
// stops there, C unused: mx_crt_recon or the opening kernel reconstructs it later.
template <class T>
int run_crt_asym(int64_t M, int64_t N, int64_t K, const T* S0, const T* S1, const T* T0,
                 const T* T1, int rolled, T* C, hipStream_t st, const ShareSrc* xs = nullptr,
                 const ShareSrc* ys = nullptr, int8_t* cr_ext = nullptr) {
  constexpr int words = sizeof(T) / 8;
  const AsymPlan ap = asym_plan(words, M, N, K);
  if (ap.rc) return ap.rc;
  const CPlan& p = ap.p;
  const Tables& tb = tables_for(words, p.n);
  const int64_t sa = M * K, sb = K * N;
  const T* a[3];
  const T* b[3];
  const T* c[3];
  const T* d[3];
  for (int q = 0; q < 3; ++q) {
    a[q] = S0 + q * sa;
    b[q] = rolled ? S0 + ((q + 1) % 3) * sa : S1 + q * sa;
    c[q] = T0 + q * sb;
    d[q] = rolled ? T0 + ((q + 1) % 3) * sb : T1 + q * sb;
  }
  // K-residue images.  A: E0 = a_0 + b_0; party 1 reads [b_1 | a_1], party 2 [a_2 | b_2].
  // B: F0 = c_0 + d_0, F1 = c_1 + d_1; party 1 reads [F1 ; d_1], party 2 [d_2 ; c_2].
  // Rolled (a_p = x_p, b_p = x_{p+1}, c_p = y_p, d_p = y_{p+1}): b_1 = a_2 = x_2 and
  // d_1 = c_2 = y_2 are one image each -- A = [x_0 + x_1, x_2, x_1, x_0], B = [y_0 + y_1,
  // y_1 + y_2, y_2, y_0] -- and each image group is one batched launch.
  int na, nb, amap, bmap;
  const int64_t a_entry = p.n * p.tiles_m * p.a_nkb * (int64_t)kImg;
  const int64_t b_entry = p.n * p.tiles_n * p.a_nkb * (int64_t)(p.bn * BK);
  auto pmap = [](int e0, int e1, int e2, int e3, int e4) {  // party 0: (e0, -) half-length
    return (int)(0x80000000u | (unsigned)e0 | (1u << 6) | ((unsigned)(e1 | (e2 << 3)) << 8) |
                 ((unsigned)(e3 | (e4 << 3)) << 16));
  };
  if (rolled) {
    na = 4;
    nb = 4;
    amap = pmap(0, 1, 2, 1, 3);
    bmap = pmap(0, 1, 2, 3, 2);
  } else {
    na = 5;
    nb = 5;
    amap = pmap(0, 1, 2, 3, 4);
    bmap = pmap(0, 1, 2, 3, 4);
  }
  // MOOSEX_CRT_ASUM=0: the sum inside the prep (mode 2); MOOSEX_CRT_DUAL=0: separate sum images
  static const bool asum = env_flag("MOOSEX_CRT_ASUM", true);
  static const bool dual = env_flag("MOOSEX_CRT_DUAL", true);
  // rolled: the sums ride on the share images' threads (dual) -- no separate sum pass
  const bool duals = rolled && dual;
  if (xs || ys) {
    if (words != 2 || !duals) return -7;
    if (xs && (K % 256 || !share_src_ok(*xs))) return -7;
    if (ys && (N % 256 || !share_src_ok(*ys))) return -7;
  }
  // A share source's zero slot: every (modulus, tile) strip of its image would be the same
  // zero bytes, so the side keeps one strip right below its images instead (k_crt_gemm16's
  // entry kZeroStrip) -- the other images close up, the maps follow, and the GEMM streams
  // the strip from L2 where it fetched a whole image.  All five products still run.
  static const bool zstrip = env_flag("MOOSEX_ZERO_STRIP", true);  // =0: the full zero image
  int aph[4], bph[4], aat[4] = {0, 1, 2, 3}, bat[4] = {0, 1, 2, 3};
  int64_t a_strip = 0, b_strip = 0;
  auto plan_src = [&](bool is_b, const ShareSrc& s, int (&ph)[4], int (&at)[4], int& n, int& map,
                      int64_t& strip) {
    src_phases(is_b, s, ph);
    int m = 0;
    for (int e = 0; e < 4; ++e) at[e] = zstrip && ph[e] == 3 ? kZeroStrip : m++;
    if (m == n) return;  // no zero image on this side (y owned by slot 1, or switched off)
    n = m;
    strip = p.a_nkb * (int64_t)(is_b ? p.bn * BK : kImg);
    for (int sh : {0, 8, 11, 16, 19}) map = (map & ~(7 << sh)) | (at[(map >> sh) & 7] << sh);
  };
  if (xs) plan_src(false, *xs, aph, aat, na, amap, a_strip);
  if (ys) plan_src(true, *ys, bph, bat, nb, bmap, b_strip);
  const int64_t ra_bytes = na * a_entry, rb_bytes = nb * b_entry;
  const int64_t sum_bytes = asum && !duals ? round_up(sa * (int64_t)sizeof(T), 256) : 0;
  if (cr_ext && !ap.defer) return -7;
  const int64_t cr_ws = cr_ext ? 0 : p.cr_bytes;
  int8_t* ws = (int8_t*)g_scratch.get(
      a_strip + ra_bytes + cr_ws + b_strip + rb_bytes + sum_bytes, st);
  if (!ws) return -4;
  int8_t* ra = ws + a_strip;
  int8_t* cr = cr_ext ? cr_ext : ra + ra_bytes;
  int8_t* rb = ra + ra_bytes + cr_ws + b_strip;
  T* a01 = sum_bytes ? (T*)(rb + rb_bytes) : nullptr;
  if (a01)
    hipLaunchKernelGGL((k_add_pair<T>), dim3((unsigned)std::min<int64_t>((sa + 255) / 256, 65536)),
                       dim3(256), 0, st, a[0], b[0], a01, sa);
  const int64_t kn = p.a_nkb;
  // every image of a side in one launch (a lone batch-1 launch of the sum ran at half the
  // bandwidth of the batched images)
  PrepSrcs sa_, sb_;
  auto put = [](PrepSrcs& q, const T* x0, const T* x1, int mode, int64_t dual = 0) {
    q.x0[q.n] = x0;
    q.x1[q.n] = x1;
    q.mode[q.n] = mode;
    q.dual[q.n] = dual;
    ++q.n;
  };
  if (duals) {
    // A = [x0 + x1, x2, x1, x0]: the x0 thread writes E3 and then E0 = x0 + x1.
    // B = [y0 + y1, y1 + y2, y2, y0]: the y2 thread writes F2 and then F1 = y2 + y1, the y0
    // thread F3 and then F0 = y0 + y1.  Launched as entries 1..3 / 2..3 of the image.
    put(sa_, a[2], a[2], 0);                  // E1 = x2
    put(sa_, a[1], a[1], 0);                  // E2 = x1
    put(sa_, a[0], b[0], 0, -3 * a_entry);    // E3 = x0, dual E0 = x0 + x1
    put(sb_, d[1], c[1], 0, -b_entry);        // F2 = y2, dual F1 = y2 + y1
    put(sb_, d[2], d[0], 0, -3 * b_entry);    // F3 = y0, dual F0 = y0 + y1
    if (ys)
      launch_prep_src(p, tb, true, *ys, N, K, rb, b_entry, bph, bat, -b_strip, st);
    else
      launch_prep<T>(p, tb, true, sb_.n, N, K, 0, nullptr, nullptr, 0, rb + 2 * b_entry, st, kn,
                     kn, sb_);
    if (xs)
      launch_prep_src(p, tb, false, *xs, M, K, ra, a_entry, aph, aat, -a_strip, st);
    else
      launch_prep<T>(p, tb, false, sa_.n, M, K, 0, nullptr, nullptr, 0, ra + a_entry, st, kn, kn,
                     sa_);
  } else {
    if (a01)
      put(sa_, a01, a01, 0);
    else
      put(sa_, a[0], b[0], 2);
    put(sb_, c[0], d[0], 3);
    put(sb_, c[1], d[1], 3);
    if (rolled) {
      for (const T* e : {a[2], a[1], a[0]}) put(sa_, e, e, 0);  // x2, x1, x0
      for (const T* f : {d[1], d[2]}) put(sb_, f, f, 0);        // y2, y0
    } else {
      for (const T* e : {b[1], a[1], a[2], b[2]}) put(sa_, e, e, 0);
      for (const T* f : {d[1], d[2], c[2]}) put(sb_, f, f, 0);
    }
    launch_prep<T>(p, tb, true, sb_.n, N, K, 0, nullptr, nullptr, 0, rb, st, kn, kn, sb_);
    launch_prep<T>(p, tb, false, sa_.n, M, K, 0, nullptr, nullptr, 0, ra, st, kn, kn, sa_);
  }
  p.var->launch(p, tb, {3, ra, rb, cr, 0, 0, amap, bmap}, st);
  if (!cr_ext) launch_recon<T>(p, tb, 3, M, N, cr, C, 0, st);
  return launch_status();
}

// run_crt over the ring of ``words`` on the entry points' untyped operands
int run_crt_words(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                  const void* A1, int64_t a_bstride, const void* B0, const void* B1,
                  int64_t b_bstride, const void* rb, int mode, void* C, int accumulate,
                  void* stream, int64_t roll = 0) {
  return with_ring(words, [&](auto t) {
    using T = decltype(t);
    return run_crt<T>(batch, M, N, K, (const T*)A0, (const T*)A1, a_bstride, (const T*)B0,
                      (const T*)B1, b_bstride, (const int8_t*)rb, mode, (T*)C, accumulate,
                      (hipStream_t)stream, roll);
  });
}

}  // namespace

extern "C" {

// Asymmetric three-party RSS product (run_crt_asym): C[p] = z_p for p = 0, 1, 2.  -7: not
// applicable (the caller runs the generic form of the same z_p).
// residues (or null): a buffer of mx_crt_defer_bytes bytes -- the product stops at the GEMM's
// output residues there and C is not written (mx_crt_recon, or mx_mul_trunc3_open's crt form,
// reconstructs it); -7 where that form does not apply.
int mx_gemm_asym(int words, int64_t M, int64_t N, int64_t K, const void* S0, const void* S1,
                 const void* T0, const void* T1, int rolled, void* C, void* stream,
                 void* residues) {
  if (M == 0 || N == 0) return residues ? -7 : 0;
  if (!rolled && (!S1 || !T1)) return -2;
  return with_ring(words, [&](auto t) {
    using T = decltype(t);
    return run_crt_asym<T>(M, N, K, (const T*)S0, (const T*)S1, (const T*)T0, (const T*)T1,
                           rolled, (T*)C, (hipStream_t)stream, nullptr, nullptr,
                           (int8_t*)residues);
  });
}

// Bytes of the residue buffer of a deferred M x N x K product (mx_gemm_asym's ``residues``);
// -7 where the product cannot be deferred (layout or reconstruction switched by environment,
// sizes run_crt_asym declines).
int64_t mx_crt_defer_bytes(int words, int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0) return -7;
  const AsymPlan a = asym_plan(words, M, N, K);
  return a.defer ? a.p.cr_bytes : -7;
}

// The reconstruction a deferred product skipped: C[p] = z_p from its residues, bitwise the C
// of the same call without ``residues``.
int mx_crt_recon(int words, int64_t M, int64_t N, int64_t K, const void* residues, void* C,
                 void* stream) {
  const AsymPlan a = asym_plan(words, M, N, K);
  if (!a.defer) return -7;
  return with_ring(words, [&](auto t) {
    launch_recon<decltype(t)>(a.p, tables_for(words, a.p.n), 3, M, N, (const int8_t*)residues,
                              (decltype(t)*)C, 0, (hipStream_t)stream);
    return launch_status();
  });
}

// mx_mul_trunc3_open's crt form (moosex.h): crt = {residues, M, N, K} of a deferred product,
// slots and the six nonces as the tail's (only r0's and r1's are drawn: trunc_pr_open).
int mxh_crt_recon_open(int words, const int64_t* crt, double* out, int64_t n,
                       const uint32_t* slots, int m, const uint64_t* nn, int frac, void* stream) {
  const int64_t M = crt[1], N = crt[2], K = crt[3];
  if (M <= 0 || N <= 0 || n != M * N || !crt[0]) return -3;
  const AsymPlan a = asym_plan(words, M, N, K);
  if (!a.defer) return -7;
  const uint32_t* ptrs[3];
  for (int i = 0; i < 3; ++i) ptrs[i] = slots + MX_KEY_SLOT_WORDS * i;
  const mxd::KeySrc keys = mxd::keysrc_slots(ptrs, 3);
  const int8_t* cr = (const int8_t*)(intptr_t)crt[0];
  const double scale = std::ldexp(1.0, -frac);
  return with_ring(words, [&](auto t) {
    launch_recon_open<decltype(t)>(a.p, tables_for(words, a.p.n), M, N, cr, out, scale, keys,
                                   nn[0], nn[1], m, (hipStream_t)stream);
    return launch_status();
  });
}

// mx_gemm_asym, rolled, over Z_2^128 with one or both operands given as a share source
// instead of a share stack (run_crt_asym's xs / ys): xsrc / ysrc null (then S0 / T0 is the
// [3][..] stack) or six words {plain operand, kind (| MX_SHARE_MIRROR), fractional bits,
// owner slot j0, key slot (device memory, as mx_share3_k's slot_next), nonce} -- the
// arguments of the mx_share3_k launch that would have written the stack.  -7: not
// applicable, nothing launched (the caller writes the shares and runs mx_gemm_asym).
// residues: as mx_gemm_asym's.
int mx_gemm_asym_src(int words, int64_t M, int64_t N, int64_t K, const void* S0, const void* T0,
                     const int64_t* xsrc, const int64_t* ysrc, void* C, void* stream,
                     void* residues) {
  if (M == 0 || N == 0) return residues ? -7 : 0;
  if (words != 2) return -7;
  if ((!xsrc && !S0) || (!ysrc && !T0)) return -2;
  ShareSrc sx, sy;
  auto fill = [](ShareSrc& s, const int64_t* a) {
    s.x = (const void*)(intptr_t)a[0];
    s.kind = (int)a[1];
    s.frac = (int)a[2];
    s.j0 = (int)a[3];
    const uint32_t* slot[1] = {(const uint32_t*)(intptr_t)a[4]};
    s.key = mxd::keysrc_slots(slot, 1);
    s.nonce = (uint64_t)a[5];
  };
  if (xsrc) fill(sx, xsrc);
  if (ysrc) fill(sy, ysrc);
  if ((xsrc && !sx.key.slot[0]) || (ysrc && !sy.key.slot[0])) return -2;
  return run_crt_asym<u128>(M, N, K, (const u128*)S0, nullptr, (const u128*)T0, nullptr, 1,
                            (u128*)C, (hipStream_t)stream, xsrc ? &sx : nullptr,
                            ysrc ? &sy : nullptr, (int8_t*)residues);
}

// Moduli count for a K' (= K, or 2K in mode 1) inner dimension; -1 if out of range.
int mx_crt_moduli(int words, int64_t kprime) {
  if (words != 1 && words != 2) return -2;
  return moduli_needed(words, kprime);
}

// Host copy of the tables (tests re-run the arithmetic on the CPU): per modulus i
// p, inv-folded A byte weights, B byte weights, A/B negative corrections, W_i words; and Mw.
int mx_crt_tables(int words, int n, int32_t* p_out, uint8_t* wa_out, uint8_t* wb_out,
                  int32_t* nega_out, int32_t* negb_out, uint16_t* W_out, uint16_t* Mw_out) {
  if ((words != 1 && words != 2) || n < 1 || n > kMaxMod) return -2;
  const Tables& t = tables_for(words, n);
  for (int i = 0; i < n; ++i) {
    p_out[i] = t.ep.p[i];
    for (int j = 0; j < 16; ++j) {
      wa_out[i * 16 + j] = (uint8_t)(t.pa.w[i][j / 4] >> (8 * (j % 4)));
      wb_out[i * 16 + j] = (uint8_t)(t.pb.w[i][j / 4] >> (8 * (j % 4)));
    }
    nega_out[i] = (int32_t)t.pa.neg[i];
    negb_out[i] = (int32_t)t.pb.neg[i];
    if (i == 0) {
      nega_out[0] = (int32_t)t.pa.mul0;  // p = 256 uses the multiplier instead
      negb_out[0] = 1;
    }
    for (int k = 0; k < 8; ++k) W_out[i * 8 + k] = t.rc.W[i][k];
  }
  for (int k = 0; k < 8; ++k) Mw_out[k] = t.rc.Mw[k];
  return 0;
}

// Host copy of the dot4 reconstruction tables (tests recompose the digits): wd
// [groups][16], rd [groups][3] words, modulus 4g + u in byte u.  Returns the group count.
int mx_crt_tables4(int words, int n, uint32_t* wd_out, uint32_t* rd_out) {
  if ((words != 1 && words != 2) || n < 1 || n > kMaxMod) return -2;
  const Tables& t = tables_for(words, n);
  for (int g = 0; g < t.r4.groups; ++g) {
    for (int d = 0; d < 16; ++d) wd_out[g * 16 + d] = t.r4.wd[g][d];
    for (int d = 0; d < 3; ++d) rd_out[g * 3 + d] = t.r4.rd[g][d];
  }
  return t.r4.groups;
}

// Host run of the share-source prep's sum-image combine (tests check it against integers):
// out[k] = the byte k_crt_prep_src stores for modulus i of the n from the residues ra[k],
// rb[k] of the two slots and the element's kappa[k].  side 0: the A' tables and the packed
// form (crt_combine2), side 1: the B' tables and the scalar form, as the kernel's instances.
int mx_crt_combine(int words, int n, int side, int i, int64_t count, const int32_t* ra,
                   const int32_t* rb, const int32_t* kappa, int8_t* out) {
  if ((words != 1 && words != 2) || n < 1 || n > kMaxMod || i < 0 || i >= n || (side & ~1))
    return -2;
  const Tables& t = tables_for(words, n);
  const PrepTab& tab = side ? t.pb : t.pa;
  const float p = (float)tab.p[i], rcp = tab.rcp[i];
  for (int64_t k = 0; k < count; ++k) {
    if (side) {
      out[k] = (int8_t)crt_combine(ra[k], rb[k], kappa[k], tab.neg[i], p, rcp);
    } else {
      const f2 f = crt_combine2((f2){(float)ra[k], 0.f}, (f2){(float)rb[k], 0.f},
                                (f2){(float)kappa[k], 0.f}, (float)tab.neg[i], p, rcp);
      out[k] = (int8_t)(int)f.x;
    }
  }
  return 0;
}

int mxh_gemm_crt(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                 const void* A1, const void* B0, const void* B1, int mode, void* C,
                 int accumulate, void* stream) {
  return run_crt_words(words, batch, M, N, K, A0, A1, M * K, B0, B1, K * N, nullptr, mode, C,
                       accumulate, stream);
}

// Batch strides given (elements; 0 broadcasts one operand over the batch): the operands of a
// batched product may be views such as an expanded (stride-0) stack -- no copy is made.
int mxh_gemm_crt_strided(int words, int64_t batch, int64_t M, int64_t N, int64_t K,
                         const void* A0, const void* A1, int64_t a_bstride, const void* B0,
                         const void* B1, int64_t b_bstride, int mode, void* C, int accumulate,
                         void* stream) {
  return run_crt_words(words, batch, M, N, K, A0, A1, a_bstride, B0, B1, b_bstride, nullptr,
                       mode, C, accumulate, stream);
}

// RSS pair form of the mode-1 product: A1 is A0 rolled by ``roll`` batch entries
// (A1[b] = A0[(b + roll) % batch], as the second shares of a stacked replicated sharing are
// the next party's first), so A' residues are prepared once per share instead of twice.
// rb: prepared B' (mxh_crt_prep_b) or null (then B0, B1).  -7: not applicable.
int mxh_crt_roll(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                 int64_t a_bstride, int64_t roll, const void* B0, const void* B1, const void* rb,
                 void* C, int accumulate, void* stream) {
  return run_crt_words(words, batch, M, N, K, A0, nullptr, a_bstride, B0, B1, K * N, rb, 1, C,
                       accumulate, stream, roll);
}

// Prepared-B variant (row-chunked dot pipeline): B' residues built once into a caller buffer.
int64_t mxh_crt_b_bytes(int words, int64_t batch, int64_t N, int64_t K, int mode) {
  if (words != 1 && words != 2) return 0;
  const CPlan p = make_cplan(words, batch, BM, N, K, mode);
  return p.n < 0 ? 0 : p.rb_bytes;
}

int mxh_crt_prep_b(int words, int64_t batch, int64_t K, int64_t N, const void* B0,
                   const void* B1, int mode, void* rb, void* stream) {
  const CPlan p = make_cplan(words, batch, BM, N, K, mode);
  if (p.n < 0) return -6;
  return with_ring(words, [&](auto t) {
    using T = decltype(t);
    launch_prep<T>(p, tables_for(words, p.n), true, batch, N, K, K * N, (const T*)B0,
                   (const T*)B1, mode, (int8_t*)rb, (hipStream_t)stream);
    return launch_status();
  });
}

int mxh_crt_with_b(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                   const void* A1, int64_t a_bstride, int mode, const void* rb, void* C,
                   int accumulate, void* stream) {
  return run_crt_words(words, batch, M, N, K, A0, A1, a_bstride, nullptr, nullptr, 0, rb, mode,
                       C, accumulate, stream);
}

}  // extern "C"
