// moosex native core: C ABI shared by the CPU (*_cpu.cpp) and the gfx950 HIP (*.hip)
// implementations; a family's host twins X_cpu.cpp sit next to its kernels X.hip.
//
// Ring tensors: Z_2^64 elements are uint64 words; Z_2^128 elements are two little-endian
// uint64 words (lo, hi) == the in-memory layout of unsigned __int128 on x86-64 and
// AMDGPU.  "words" below is 1 (Z_2^64), 2 (Z_2^128) or 0 (one byte per element, used for
// bit tensors holding 0/1).
//
// Every entry point returns 0 on success, a negative error code otherwise; `dev` is
// 0 for host memory and 1 for device memory (then `stream` is a hipStream_t).
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum mx_binop { MX_ADD = 0, MX_SUB = 1, MX_MUL = 2, MX_AND = 3, MX_OR = 4, MX_XOR = 5 };
enum mx_unop { MX_NEG = 0, MX_NOT = 1, MX_SHL = 2, MX_SHR = 3, MX_SAR = 4 };
enum mx_cmpop { MX_LT = 0, MX_GT = 1, MX_EQ = 2, MX_MSB = 3 };
// RSS cross-term kinds: arithmetic (x0*y0 + x0*y1 + x1*y0 + a - b) or boolean (& and ^)
enum mx_cross { MX_CROSS_ARITH = 0, MX_CROSS_BOOL = 1 };
// share kernels (mx_share3*, mx_share_party): kind MX_SHARE_F64 = an arithmetic sharing of a
// float64 input, fixed-point encoded in the kernel (x * 2^na, truncated as RingFixedpointEncode);
// the nonce argument na carries the fractional bits (the zero slot draws no randomness)
// kind | MX_SHARE_MIRROR: the masked slot goes to P_{j+2} instead of P_{j+1} (slot j =
// x - PRF(k_{j+1}), slot j+1 = PRF(k_{j+1}), slot j+2 = 0; the key argument is k_{j+1})
enum mx_share_src { MX_SHARE_F64 = 2, MX_SHARE_MIRROR = 8 };

// AES-128 key schedule: 11 round keys of 4 big-endian-packed words (FIPS-197 layout)
typedef struct {
  uint32_t rk[44];
} mx_aes_key;

int mx_version(void);
int mx_device_count(void);

// out[i] = a[i] op b[i]; na, nb in {n, 1} (scalar broadcast)
int mx_ew_binary(int dev, int op, int words, const void* a, int64_t na, const void* b,
                 int64_t nb, void* out, int64_t n, void* stream);
// Stacked party vectors a[nparties, m]: out[p, i] = p == which ? a[p, i] op b[i % nb]
// : a[p, i] (a public operand applied to one party's share slot, in one pass); nb divides m
// (b repeats with period nb: scalars, full slots, trailing-axis vectors)
int mx_ew_binary_slot(int dev, int op, int words, const void* a, const void* b, int64_t nb,
                      void* out, int64_t m, int nparties, int which, void* stream);
// Zero share from precomputed keystreams + reshare, three stacked parties (arith):
// out0[p, i] = v[p, i] + r[p, i] - r[p+1, i] ; out1[p, i] = out0[p+1, i]
int mx_add_zs3(int dev, int words, const void* v, const void* r, void* out0, void* out1,
               int64_t n, void* stream);
// out[i] = op(a[i], param)
int mx_ew_unary(int dev, int op, int words, const void* a, void* out, int64_t n,
                int64_t param, void* stream);
// Share-pair forms (both replicated share vectors of a share-wise op, one launch):
// out0 = a0 op b0, out1 = a1 op b1 (same na / nb / n for both)
int mx_ew_binary2(int dev, int op, int words, const void* a0, const void* b0, void* out0,
                  const void* a1, const void* b1, void* out1, int64_t na, int64_t nb, int64_t n,
                  void* stream);
// o_y = a_y * f + (add_y ? c[0] : 0), y = 0, 1 (one party's two share components)
int mx_mul_add2(int dev, int words, const void* a0, const void* a1, const void* f,
                const void* c, int add0, int add1, void* out0, void* out1, int64_t n,
                void* stream);
int mx_ew_unary2(int dev, int op, int words, const void* a0, void* out0, const void* a1,
                 void* out1, int64_t n, int64_t param, void* stream);
// out_y = a_y^T, y = 0, 1 ([rows, cols] ring matrices -> [cols, rows])
int mx_transpose2(int dev, int words, const void* a0, void* out0, const void* a1, void* out1,
                  int64_t rows, int64_t cols, void* stream);
// im2col, the patch gather of a 2-D convolution: in[slots, N, C, H, W] (nhwc: [slots, N, H,
// W, C]) of elem_bytes-wide elements (1, 8 or 16) -> out[slots, N*OH*OW, C*KH*KW], rows
// ordered (n, oh, ow), columns (c, kh, kw) (nhwc: (kh, kw, c)); taps in the padding (pt rows
// above, pl columns left; below / right follow from OH / OW) are zero.  Input slots are
// in_slot_stride elements apart (a slot view of a larger buffer is read in place), output
// slots are dense.
int mx_im2col(int dev, int elem_bytes, const void* in, void* out, int64_t slots,
              int64_t in_slot_stride, int64_t N, int64_t C, int64_t H, int64_t W, int64_t KH,
              int64_t KW, int64_t sh, int64_t sw, int64_t pt, int64_t pl, int64_t dh,
              int64_t dw, int64_t OH, int64_t OW, int nhwc, void* stream);
// col2im, the exact adjoint of mx_im2col and the scatter-sum of a transposed convolution:
// in[slots, N*OH*OW, C*KH*KW] (im2col's row and column order) of elem_bytes-wide ring elements
// (8 or 16; 1-byte bit tensors return -2) -> out[slots, N, C, H, W] (nhwc: [slots, N, H, W,
// C]), out[n, c, y, x] = the wrapping sum of in[(n, oh, ow), (c, kh, kw)] over the taps with
// oh*sh + kh*dh - pt == y and ow*sw + kw*dw - pl == x.  Entries whose tap lies in the padding
// are dropped; a pixel no window reaches is zero.  Input slots are in_slot_stride elements
// apart (a slot view of a larger buffer is read in place), output slots are dense.
int mx_col2im(int dev, int elem_bytes, const void* in, void* out, int64_t slots,
              int64_t in_slot_stride, int64_t N, int64_t C, int64_t H, int64_t W, int64_t KH,
              int64_t KW, int64_t sh, int64_t sw, int64_t pt, int64_t pl, int64_t dh,
              int64_t dw, int64_t OH, int64_t OW, int nhwc, void* stream);
// 2-D image resize with public coordinates (nearest / bilinear), exact in the ring, no
// truncation: in[slots, N, C, H, W] (nhwc: [slots, N, H, W, C]) of elem_bytes-wide ring
// elements (8 or 16; 1-byte bit tensors return -2) -> out[slots, N, C, OH, OW] (nhwc: [slots,
// N, OH, OW, C]),
//   out[n, oy, ox, c] = sum_{a,b in {0,1}} wh_a[oy] * ww_b[ox] * in[n, ih_a[oy], iw_b[ox], c]
// wrapping.  th / tw are the per-axis tables, int32 [3, OH] / [3, OW] holding the rows i0, i1,
// w1 (on the device for dev != 0): w0 = 2^wb - w1 with wb = wbh / wbw (0..12), 0 <= w1 <=
// 2^wb, and w1 = 0 where wb = 0.  wbh == wbw == 0 is a pure gather of in[.., i0h, i0w, ..].
// The CPU entry checks the tables (-3 on an index outside the image or a weight out of
// range); the device kernel clamps the indices.  Input slots are in_slot_stride elements
// apart (a slot view of a larger buffer is read in place), output slots are dense.
int mx_resize2d(int dev, int elem_bytes, const void* in, void* out, int64_t slots,
                int64_t in_slot_stride, int64_t N, int64_t C, int64_t H, int64_t W, int64_t OH,
                int64_t OW, const int32_t* th, const int32_t* tw, int wbh, int wbw, int nhwc,
                void* stream);
// Depthwise 2-D convolution in Z_2^64 / Z_2^128 (elem_bytes 8 / 16), wrapping:
//   out[s][n, oh, ow, c*mult + j] = sum_{kh,kw} X[s][n, oh*sh + kh*dh - pt, ow*sw + kw*dw - pl, c]
//                                               * Wt[s][c*mult + j, kh, kw]
// over x[slots, N, C, H, W] (nhwc: [slots, N, H, W, C]) and the dense ONNX depthwise weight
// w[slots, C*mult, 1, KH, KW]; the output has the input's layout with C*mult channels, dense
// slots.  Taps in the padding contribute zero and are not loaded.  x1 == w1 == null: plain,
// X.Wt = x0.w0.  Otherwise the replicated local product x0.(w0 + w1) + x1.w0 in one pass
// (x1 / w1: the next party's components).  Slots of x0 / x1 are x_slot_stride elements apart,
// of w0 / w1 w_slot_stride; either may be 0 (a public operand read in place by every slot).
int mx_dwconv(int dev, int elem_bytes, const void* x0, const void* x1, const void* w0,
              const void* w1, void* out, int64_t slots, int64_t x_slot_stride,
              int64_t w_slot_stride, int64_t N, int64_t C, int64_t H, int64_t W, int64_t mult,
              int64_t KH, int64_t KW, int64_t sh, int64_t sw, int64_t pt, int64_t pl,
              int64_t dh, int64_t dw, int64_t OH, int64_t OW, int nhwc, void* stream);
// The local step of a secret piecewise-linear function in Z_2^64 / Z_2^128 (elem_bytes 8 /
// 16), wrapping.  s0 / s1: one party's components of the k stacked flags [slots, k, n] (plane j
// of a slot at element offset j*n), x0 / x1 of the input [slots, n]; da / db: k public ring
// elements each and ak one, on the host, elem_bytes wide, little-endian words -- they travel in
// the kernel's arguments, so nothing is uploaded.  With G0 = sum_j da[j]*s0[j,e] and G1 the
// same over s1,
//   out[s][e] = G0*(x0[e] + x1[e]) + G1*x0[e] + ak*x0[e] + sum_j db[j]*s0[j,e]
// (mx_dwconv's cross convention: own times the sum, plus next times own; over the three
// parties a 3-out-of-3 sharing of (ak + G)*x + H).  s1 == x1 == null: plain, G0*x0 + ak*x0 +
// sum_j db[j]*s0[j,e].  0 <= k <= MX_PWL_MAX.  Slots of s0 / s1 are s_slot_stride elements
// apart, of x0 / x1 x_slot_stride (views of a larger buffer are read in place); output slots
// are dense.
#define MX_PWL_MAX 8
int mx_pwl_cross(int dev, int elem_bytes, const void* s0, const void* s1, const void* x0,
                 const void* x1, void* out, int64_t slots, int64_t s_slot_stride,
                 int64_t x_slot_stride, int64_t n, int k, const uint64_t* da, const uint64_t* db,
                 const uint64_t* ak, void* stream);
// The local step of a secret piecewise polynomial of degree d in {1, 2, 3} in Z_2^64 / Z_2^128
// (elem_bytes 8 / 16), wrapping.  s0 / s1: one party's components of the k stacked flags
// [slots, k, n], as mx_pwl_cross takes them.  p0 / p1: host arrays of d device pointers each,
// the components of the powers P_1 = x, .., P_d, [slots, n] each, slots p_slot_stride[i-1]
// elements apart: a power is read where its multiplication wrote it.  dt: (d + 1) * k public
// ring elements, row i the differences D_i[j] of the degree-i coefficients (row 0: the
// constants, at the scale of the products); ck: d elements, the last piece's coefficients of
// degrees 1..d; both on the host, elem_bytes wide, little-endian words -- they travel in the
// kernel's arguments.  With G_i^c = sum_j D_i[j]*sc[j,e],
//   out[s][e] = sum_{i=1..d} [ G_i^0*(P_i^0[e] + P_i^1[e]) + G_i^1*P_i^0[e] + ck_i*P_i^0[e] ]
//               + sum_j D_0[j]*s0[j,e]
// (mx_pwl_cross's cross convention; over the three parties a 3-out-of-3 sharing of
// sum_i (ck_i + G_i)*P_i + H).  s1 == p1 == null: plain, sum_i (ck_i + G_i^0)*P_i^0 + H.  d = 1
// is mx_pwl_cross bit for bit.  1 <= k <= MX_PWP_MAX.  Output slots are dense.
#define MX_PWP_MAX 8
#define MX_PWP_DEG 3
int mx_pwp_cross(int dev, int elem_bytes, const void* s0, const void* s1, const void* const* p0,
                 const void* const* p1, void* out, int64_t slots, int64_t s_slot_stride,
                 const int64_t* p_slot_stride, int64_t n, int k, int d, const uint64_t* dt,
                 const uint64_t* ck, void* stream);
// One compare-exchange stage (k, j) of a bitonic sorting network in Z_2^64 / Z_2^128
// (elem_bytes 8 / 16), wrapping, along the middle axis of an [outer, n, inner] array per slot
// (cswap_geom.h: n, k, j powers of two, j < k <= n; by = -1 sorts every inner index on its own,
// by >= 0 orders whole rows by column `by`).  Pair t of [0, n/2): i = t with a zero bit
// inserted at bit log2 j, l = i | j, ascending iff (i & k) == 0 (flipped by `descending`).
// Input slots are *_slot_stride elements apart (views of a larger buffer are read in place),
// output slots are dense.
//   mx_cswap_diff:  out[o, t, c] = ascending ? x[l] - x[i] : x[i] - x[l], [outer, n/2, inner],
//                   or on the key column only, [outer, n/2, 1], in table mode: negative where
//                   the pair is out of order
//   mx_cswap_cross: with D = x[i] - x[l], out[o, t, c] = s0*(D0 + D1) + s1*D0 -- the replicated
//                   local product of the flag s and the difference (own times the sum plus next
//                   times own) -- over flags [outer, n/2, inner], or [outer, n/2, 1] broadcast
//                   over the columns in table mode.  s1 == x1 == null: plain, s0*D0
//   mx_cswap_apply: out[i] = x[i] - p[t], out[l] = x[l] + p[t] with p [outer, n/2, inner]
// With s = [diff < 0] and p = s * (x[i] - x[l]) the three make one stage; the direction enters
// through the sign of diff alone.
int mx_cswap_diff(int dev, int elem_bytes, const void* x, void* out, int64_t slots,
                  int64_t x_slot_stride, int64_t outer, int64_t n, int64_t inner, int64_t by,
                  int64_t k, int64_t j, int descending, void* stream);
int mx_cswap_cross(int dev, int elem_bytes, const void* s0, const void* s1, const void* x0,
                   const void* x1, void* out, int64_t slots, int64_t s_slot_stride,
                   int64_t x_slot_stride, int64_t outer, int64_t n, int64_t inner, int64_t by,
                   int64_t k, int64_t j, int descending, void* stream);
int mx_cswap_apply(int dev, int elem_bytes, const void* x, const void* p, void* out,
                   int64_t slots, int64_t x_slot_stride, int64_t p_slot_stride, int64_t outer,
                   int64_t n, int64_t inner, int64_t by, int64_t k, int64_t j, int descending,
                   void* stream);
// Permuted row gather in Z_2^64 / Z_2^128 (elem_bytes 8 / 16), wrapping, along the middle axis
// of an [outer, n, inner] array per slot -- the local step of an oblivious shuffle:
//   out[o, r, c] = a[o, perm[r], c] (+ b[o, perm[r], c]) (+ p[o, r, c]) (- m[o, r, c])
// b, p and m are each optional (null); with all three null it is a plain row gather.  perm is
// int64 [n] on the operands' device and has to be a permutation of 0..n-1: the CPU twin checks
// it (-3), the kernel clamps what it reads (a bad perm gathers a wrong row, never outside).
// Input slots are *_slot_stride elements apart (views of a larger buffer are read in place),
// output slots are dense.  out must not overlap an input: a gather is not in-place safe.
// -3 also where slots times the elements of a slot, or times a slot stride, exceeds 2^61.
int mx_perm_gather(int dev, int elem_bytes, const void* a, const void* b, const void* p,
                   const void* m, const int64_t* perm, void* out, int64_t slots,
                   int64_t a_slot_stride, int64_t b_slot_stride, int64_t p_slot_stride,
                   int64_t m_slot_stride, int64_t outer, int64_t n, int64_t inner, void* stream);
// Prefix sum in Z_2^64 / Z_2^128 (elem_bytes 8 / 16), wrapping, along the middle axis of an
// [outer, n, inner] array per slot (segscan_geom.h):
//   out[o, pos, c] = sum of x[o, t, c] over t <= pos (exclusive: t < pos, the first element 0);
//   reverse: over t >= pos (t > pos), from the far end
// A lane walks up to mx_scan_chunk() positions with the running sum in registers; a longer
// axis takes three phases -- the sums of every chunk, this entry again on the sums, an add
// pass -- in `ws`, a buffer of the caller's with at least mx_scan_ws_elems(slots, outer, n,
// inner) elements (0 for an axis of one chunk; -3 where it is smaller).  No workgroup waits
// for another.  Input slots are x_slot_stride elements apart (views of a larger buffer are
// read in place), output slots are dense; out must not overlap x.
int64_t mx_scan_chunk(void);
int64_t mx_scan_ws_elems(int64_t slots, int64_t outer, int64_t n, int64_t inner);
int mx_scan(int dev, int elem_bytes, const void* x, void* out, void* ws, int64_t ws_elems,
            int64_t slots, int64_t x_slot_stride, int64_t outer, int64_t n, int64_t inner,
            int exclusive, int reverse, void* stream);
// One stage j (1 <= j < n, any n) of a segmented Hillis-Steele prefix sum over a state
// [outer, n, inner] per slot whose last column is the continuation flag g and whose other
// columns are values.
//   mx_segscan_cross: one party's local products with its own component a and the next one b,
//                     out[o, pos - j, c] = ga*(Ta + Tb) + gb*Ta for pos in [j, n) and every c,
//                     ga = a[o, pos, inner-1], gb = b[o, pos, inner-1], Ta = a[o, pos-j, c],
//                     Tb = b[o, pos-j, c]: [outer, n - j, inner].  b == null: plain, ga*Ta.
//                     a and b share slot_stride
//   mx_segscan_apply: out[o, pos, c] = x[o, pos, c] + p[o, pos-j, c] for c < inner-1,
//                     out[o, pos, inner-1] = p[o, pos-j, inner-1] for pos >= j; out = x below j
// Ring-linear: the flag is any ring value.  Input slots are *_slot_stride elements apart,
// output slots are dense.
int mx_segscan_cross(int dev, int elem_bytes, const void* a, const void* b, void* out,
                     int64_t slots, int64_t slot_stride, int64_t outer, int64_t n,
                     int64_t inner, int64_t j, void* stream);
int mx_segscan_apply(int dev, int elem_bytes, const void* x, const void* p, void* out,
                     int64_t slots, int64_t x_slot_stride, int64_t p_slot_stride, int64_t outer,
                     int64_t n, int64_t inner, int64_t j, void* stream);
// Row-wise outer products in Z_2^64 / Z_2^128 (elem_bytes 8 / 16), wrapping (outer_geom.h):
// L is [groups, rows, A], H is [groups, rows, B] per slot and
//   out[g, r, c] = L[g, r, c % A] * H[g, r, c / A] for c < n_out, 1 <= n_out <= A * B,
// [groups, rows, n_out] per slot, dense.  With lb and hb (both or neither) it is one party's
// local products of a replicated multiplication with its own components la, ha and the next
// party's lb, hb: La*(Ha + Hb) + Lb*Ha, mx_segscan_cross's convention.  Ring-bilinear: the
// operands are any ring values.  L and H have their own base pointers, slot strides and group
// strides in elements (la and lb share L's, ha and hb share H's): the groups (2g, 2g + 1) of
// one [2 * groups, rows, A] array are read in place as H = L + rows * A at a group stride of
// 2 * rows * A.  A row of an operand is dense.  out must not overlap an operand.
int mx_outer_cross(int dev, int elem_bytes, const void* la, const void* lb, const void* ha,
                   const void* hb, void* out, int64_t slots, int64_t l_slot_stride,
                   int64_t l_group_stride, int64_t h_slot_stride, int64_t h_group_stride,
                   int64_t groups, int64_t rows, int64_t A, int64_t B, int64_t n_out,
                   void* stream);
// mx_ew_binary_slot on a0 (slot which0) and a1 (slot which1) with one public b
int mx_ew_binary_slot2(int dev, int op, int words, const void* a0, const void* a1,
                       const void* b, int64_t nb, void* out0, void* out1, int64_t m,
                       int nparties, int which0, int which1, void* stream);
// Fixed-point product of three stacked parties in one launch (device, latency-bound sizes):
// rss_mul3 (zero share from slots k0, k1, k2 at nmul) followed by trunc_pr3 (slots k0 / k2,
// nonces r0 r1 t m z0 z2) on the product, outputs at party stride ostride.  views: operand
// {party stride[4], period[4]} or null.  Returns 1 when the size is not latency-bound (the
// caller then runs the two kernels), 0 on success.
int mx_mul_trunc3_kv(int dev, int words, const void* x0, const void* x1, const void* y0,
                     const void* y1, void* out0, void* out1, int64_t n, int64_t ostride,
                     const uint32_t* slots, uint64_t nmul, int m, const uint64_t* nonces,
                     const int64_t* views, void* stream);
// The tail of a fixed-point dot whose result is only revealed: mx_mul_trunc3_kv's zero share
// + reshare + TruncPr of the parties' local products x ([3] slots, xstride elements apart:
// a stack, or rows of a larger one), same keys and nonces, and the new shares opened at
// once -- out[i] = signed(Z0 + Z1 + Z2)[i] / 2^frac, bitwise mx_addn_decode of those shares,
// which are not written.  Host and device, every size.  crt (device only, else null): the
// product is still the residues of a mx_gemm_asym / mx_gemm_asym_src given a ``residues``
// buffer -- {residues, M, N, K}, x and xstride unused, n = M * N -- and the opening
// reconstructs it on the way (k_crt_recon16d_open): bitwise mx_crt_recon, then this entry.
int mx_mul_trunc3_open(int dev, int words, const void* x, int64_t xstride, double* out,
                       int64_t n, const uint32_t* slots, uint64_t nmul, int m,
                       const uint64_t* nonces, int frac, void* stream, const int64_t* crt);
// out = a + b + c elementwise (mod 2^w)
int mx_ew_add3(int dev, int words, const void* a, const void* b, const void* c, void* out,
               int64_t n, void* stream);
// Share-wise linear combination of nin <= 3 stacked replicated values [nparties, m], both
// share vectors in one launch: out_y = sum_t coef[t] * ins[2t + y] (mod 2^w), plus the public
// b (period nb, null = none) at party slot which_y.
int mx_lincomb2(int dev, int words, int nin, const void* const* ins, const int64_t* coef,
                const void* b, int64_t nb, void* out0, void* out1, int64_t m, int nparties,
                int which0, int which1, void* stream);
// Sum of k stacked share vectors that are views of one buffer at a constant element step
// is_y (party stride ps_y, each party's slot dense, m elements): out_y[p, e] =
// sum_t base_y[t * is_y + p * ps_y + e], both share vectors (y = 0, 1) in one launch.
int mx_sum_views2(int dev, int words, const void* base0, const void* base1, int64_t is0,
                  int64_t is1, int64_t ps0, int64_t ps1, int k, void* out0, void* out1, int64_t m,
                  int nparties, void* stream);
// Two trivial sharings in the stacked layout [nparties, m], one launch:
// out0[q, i] = q == which0 ? x0[i] : 0 ; out1[q, i] = q == which1 ? x1[i] : 0
int mx_slot_place2(int dev, int words, const void* x0, const void* x1, void* out0, void* out1,
                   int64_t m, int nparties, int which0, int which1, void* stream);
// out[i] = (a[i] cmp b[i]) as 0/1 bytes, signed two's-complement comparison
int mx_ew_compare(int dev, int op, int words, const void* a, int64_t na, const void* b,
                  int64_t nb, uint8_t* out, int64_t n, void* stream);
// out[i] = (a[i] >> bit) & 1
int mx_bit_extract(int dev, int words, const void* a, uint8_t* out, int64_t n, int bit,
                   void* stream);
// out[i] = (ring) bits[i] << bit
int mx_ring_inject(int dev, int words, const uint8_t* bits, void* out, int64_t n, int bit,
                   void* stream);
// out[i] = round(x[i] * 2^frac) mod 2^(64*words)
int mx_encode(int dev, int words, const double* x, void* out, int64_t n, int frac,
              void* stream);
// out[i] = signed(x[i]) / 2^frac
// decode(a + b + c [+ d]): a reveal's shares summed and decoded in one pass (d may be null)
int mx_addn_decode(int dev, int words, const void* a, const void* b, const void* c,
                   const void* d, double* out, int64_t n, int frac, void* stream);
int mx_decode(int dev, int words, const void* x, double* out, int64_t n, int frac,
              void* stream);
// out[i] = value (lo word, hi word for Z_2^128; low byte for bits)
int mx_fill(int dev, int words, void* out, int64_t n, uint64_t lo, uint64_t hi, void* stream);
// out[o, j, i] = bit (start + j) of a[o, i] (0/1 bytes)
int mx_bit_planes(int dev, int words, const void* a, uint8_t* out, int64_t outer, int64_t inner,
                  int start, int count, void* stream);
// out[o, i] = sum_j w[j] * a[o, j, i] (w: k ring elements in the memory named by dev)
int mx_weighted_sum(int dev, int words, const void* a, const void* w, void* out, int64_t outer,
                    int64_t k, int64_t inner, void* stream);
// out[o, i] = sum_r a[o, r, i]
int mx_sum_axis(int dev, int words, const void* a, void* out, int64_t outer, int64_t red,
                int64_t inner, void* stream);
// AES-128 in counter mode: block c (c = ctr0, ctr0+1, ...) = AES_k(nonce_le64 || c_le64);
// writes nbytes bytes of the keystream
int mx_prg(int dev, const uint8_t* key16, uint64_t nonce, uint64_t ctr0, void* out,
           int64_t nbytes, void* stream);
// AES-128 encryption of single 16-byte blocks (ECB) on the host; used for seed derivation
// DeriveSeed: 16-byte seed = first 16 bytes of PRF block(key; sync key as counter||nonce)
int mx_derive_seed(const uint8_t* key16, const uint8_t* sync16, uint8_t* out16);
int mx_aes_encrypt_blocks(const uint8_t* key16, const uint8_t* in, uint8_t* out,
                          int64_t nblocks);
// RSS local step for `nparties` stacked parties of n elements each:
//   party p, element i: out = x0*y0 + x0*y1 + x1*y0 + PRF(key[p])_i - PRF(key[p+1])_i
// (boolean flavour: & and ^).  keys has nparties+1 entries.  x1 or y1 may be null
// (then those terms are dropped: used for local products with public values).  y0 == null
// means out = x0 + zero share.  keys may be null (no zero share).
int mx_rss_cross(int dev, int kind, int words, const void* x0, const void* x1,
                 const void* y0, const void* y1, void* out, int64_t n, int nparties,
                 const uint8_t* keys16, uint64_t nonce, void* stream);
// zero share only: out[p, i] = PRF(key[p])_i - PRF(key[p+1])_i (xor for kind BOOL)
int mx_zero_share(int dev, int kind, int words, void* out, int64_t n, int nparties,
                  const uint8_t* keys16, uint64_t nonce, void* stream);
// PRF expansion of several keys: out[p, i] = PRF(key[p])_i (words 0 -> bytes & 1)
int mx_prf_expand(int dev, int words, void* out, int64_t n, int nkeys,
                  const uint8_t* keys16, uint64_t nonce, void* stream);
// Batched ring GEMM.  mode 0: C = A0 . B0.  mode 1 (RSS cross): C = A0.(B0+B1) + A1.B0.
// A* are [batch, M, K] row-major, B* are [batch, K, N] row-major, C is [batch, M, N].
// accumulate != 0 -> C += result.
int mx_gemm(int dev, int words, int64_t batch, int64_t M, int64_t N, int64_t K,
            const void* A0, const void* A1, const void* B0, const void* B1, int mode,
            void* C, int accumulate, void* stream);
// Size (bytes) of the last GEMM workspace allocation that failed (the -4 return of the
// GEMM entry points), 0 if none since the last call; reading it resets it.  Held
// workspace bytes on the calling device (every stream's grow-only scratch).
int64_t mx_workspace_failed_bytes(void);
int64_t mx_workspace_held_bytes(void);
int64_t mx_workspace_shared_count(void);
// Prepared-B GEMM (device only): B' limb planes built once, reused for several A row
// blocks; A given with a batch stride (elements).  mx_gemm_b_bytes returns 0 when K is
// above the exact single-chunk limit (then use mx_gemm).
int64_t mx_gemm_b_bytes(int words, int64_t batch, int64_t N, int64_t K, int mode);
int mx_gemm_prep_b(int words, int64_t batch, int64_t K, int64_t N, const void* B0,
                   const void* B1, int mode, void* lb, void* stream);
int mx_gemm_with_b(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                   const void* A1, int64_t a_bstride, int mode, const void* lb, void* C,
                   int accumulate, void* stream);
// Device GEMM with explicit batch strides (elements) for the A and B operands; a stride of 0
// broadcasts one operand over the batch (no copy of an expanded stack).
int mx_crt_tables4(int words, int n, uint32_t* wd_out, uint32_t* rd_out);
int mx_gemm_roll(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                 int64_t a_bstride, int64_t roll, const void* B0, const void* B1, const void* lb,
                 void* C, int accumulate, void* stream);
int mx_gemm_strided(int words, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A0,
                    const void* A1, int64_t a_bstride, const void* B0, const void* B1,
                    int64_t b_bstride, int mode, void* C, int accumulate, void* stream);
// select the GEMM kernel: 0 = auto, 1 = force VALU reference kernel, 2 = force MFMA
void mx_set_gemm_impl(int impl);
// multi-modular (CRT) int8 GEMM for large products: 0 = auto, 1 = force, 2 = off
void mx_set_gemm_crt(int mode);
// moduli for an inner dimension K' (K, or 2K in mode 1); host copy of the CRT tables
int mx_crt_moduli(int words, int64_t kprime);
int mx_crt_tables(int words, int n, int32_t* p, uint8_t* wa, uint8_t* wb, int32_t* nega,
                  int32_t* negb, uint16_t* W, uint16_t* Mw);
// host run of the share-source prep's sum-image combine for modulus i (side 0: A', 1: B')
int mx_crt_combine(int words, int n, int side, int i, int64_t count, const int32_t* ra,
                   const int32_t* rb, const int32_t* kappa, int8_t* out);

// Fused stacked-session protocols (rss_fused.h).  s0/out0/out1 are [3, n] slot
// vectors (party p holds out0[p] = z_p and out1[p] = z_{p+1}).
// trunc_pr3 nonces: r0, r1, r_top, r_msb, z0, z2 (dealer keys k0, k2).
//
// What TruncPr computes.  Over Z_2^w (w = 64 * words), for -2^(w-2) <= x < 2^(w-2) and the
// opening mask r = PRF(k0, r0) + PRF(k2, r1) (mod 2^w), the new sharing reveals to
//   (x >> m) + [(x mod 2^m) + (r mod 2^m) >= 2^m]   (mod 2^w; >> arithmetic, i.e. floor)
// with slots z0 = PRF(k0, z0), z2 = PRF(k2, z2) and z1 the rest.  The shift range of the
// stacked entries -- mx_trunc_pr3, _k, _ko, _kmo, mx_mul_trunc3_kv, mxh_mul_trunc3_kv2 and
// mxh_wsum_trunc3 -- is 0 <= m <= w - 2 (m = 0: a fresh sharing of x); any other m returns
// -3 and nothing runs: the offset 2^(w-2) >> m of the protocol is no integer past w - 2.
// The opening entry (mx_mul_trunc3_open) and the per-party rounds (mx_trunc_party_r*,
// mx_dot_tail_r*, mx_jobs_r*) take 1 <= m <= 63, -3 otherwise -- the dealer's msb share
// travels as a u64 -- and the result is the one above only while m <= w - 2 as well.
// (words other than 1 and 2 are each entry's own -2)
static inline int mx_trunc_shift_ok(int words, int m) {
  return (words != 1 && words != 2) || (m >= 0 && m <= 64 * words - 2);
}
int mx_trunc_pr3(int dev, int words, const void* s0, void* out0, void* out1, int64_t n, int m,
                 const uint8_t* k0, const uint8_t* k2, const uint64_t* nonces, void* stream);
// share3: owner party j; slot_j = PRF(k_j, n1) (k_j: held by P_j and P_{j+2}), slot_{j+1} =
// x - slot_j (sent to P_{j+1}), slot_{j+2} = 0 (reference replicated/convert.rs:74-90).
// The key argument is k_j; k_all / na are not read (kept for the ABI).
int mx_share3(int dev, int kind, int words, const void* x, void* out0, void* out1, int64_t n,
              int j, const uint8_t* k_next, const uint8_t* k_all, uint64_t n1, uint64_t na,
              void* stream);

// ---- PRF keys held in key slots (graph-capture friendly) -----------------------------
// A key slot is MX_KEY_SLOT_WORDS uint32 words: the raw 16-byte key (words 0..3) followed
// by its expanded AES-128 schedule (words 4..47).  Slots live in the memory named by
// `dev`; kernels read them at run time, so the keys are not baked into launch parameters.
#define MX_KEY_SLOT_WORDS 48
// host: fill n consecutive slots from n raw keys
void mx_key_slots(const uint8_t* keys16, int n, uint32_t* out);
// mx_rss_cross with keys from slots: party p uses slot p % nslots and (p + 1) % nslots
// (nslots == nparties: the ring of an RSS zero share; nslots == nparties + 1: explicit)
int mx_rss_cross_k(int dev, int kind, int words, const void* x0, const void* x1,
                   const void* y0, const void* y1, void* out, int64_t n, int nparties,
                   const uint32_t* slots, int nslots, uint64_t nonce, void* stream);
// mx_rss_cross with an explicit key PAIR per party: party p uses the key slots at
// slot_ptrs[2p] and slot_ptrs[2p+1] (a host array of 2 * nparties slot addresses).  Used
// when the stacked parties belong to different sessions (cyclic multi-GPU layout).
int mx_rss_cross_kp(int dev, int kind, int words, const void* x0, const void* x1,
                    const void* y0, const void* y1, void* out, int64_t n, int nparties,
                    const uint32_t* const* slot_ptrs, uint64_t nonce, void* stream);
// Stacked 3-party RSS product with the reshare fused in: out0[p] = z_p (cross terms +
// zero share from slots p, p+1 mod 3) and out1[p] = z_{p+1}, i.e. both shares of every
// party after the one-round reshare (x*/y*/out* are [3, n] slot vectors)
// mx_rss_mul3_k (device only) with operand views: views[0..3] party strides, views[4..7]
// periods (elements) of x0, x1, y0, y1 -- element e of party p is op[p * ps + e % per]
int mx_rss_mul3_kv(int dev, int kind, int words, const void* x0, const void* x1, const void* y0,
                   const void* y1, void* out0, void* out1, int64_t n, const uint32_t* slots,
                   uint64_t nonce, const int64_t* views, void* stream);
int mx_rss_mul3_k(int dev, int kind, int words, const void* x0, const void* x1, const void* y0,
                  const void* y1, void* out0, void* out1, int64_t n, const uint32_t* slots,
                  uint64_t nonce, void* stream);
// One Kogge-Stone level of the packed boolean adder for three stacked parties, reshare
// fused (x*, out* are [3, n] slot vectors of packed words):
//   t = pk AND (g << d)                     (RSS AND: cross terms ^ zero share)
//   g' = g ^ t ;  pk' = pk AND (pk << d) if both
// zero shares: party p xors PRF(k_p) ^ PRF(k_{p+1}) at element e (t) and n + e (pk') of
// ONE nonce -- the same values as the generic path's stacked [2, n] AND.
// rep.binary_adder's whole carry chain (nlev Kogge-Stone levels, level l at nonces[l]) for
// three stacked parties in one launch; returns the final g shares (device only)
int mx_ks_adder3_k(int dev, int words, const void* g0, const void* g1, const void* p0,
                   const void* p1, void* og0, void* og1, int64_t n, int nlev,
                   const uint32_t* slots, const uint64_t* nonces, void* stream);
int mx_ks_level3_k(int dev, int words, const void* g0, const void* g1, const void* p0,
                   const void* p1, void* og0, void* og1, void* op0, void* op1, int64_t n,
                   int d, int both, const uint32_t* slots, uint64_t nonce, void* stream);
// One party's share of a Kogge-Stone level (SPMD: one process per party), before the
// reshare: z[e] = pk AND (g << d) cross terms ^ PRF(k0)[e] ^ PRF(k1)[e]; if both, also
// z[n + e] for pk AND (pk << d).  keys16 = (k_p, k_{p+1}); z has (both ? 2n : n) words.
int mx_ks_cross1(int dev, int words, const void* g0, const void* g1, const void* p0,
                 const void* p1, void* z, int64_t n, int d, int both, const uint8_t* keys16,
                 uint64_t nonce, void* stream);
// mx_ks_cross1 with the two keys read from key slots (slots[0] = k_p, slots[1] = k_{p+1})
int mx_ks_cross1_s(int dev, int words, const void* g0, const void* g1, const void* p0,
                   const void* p1, void* z, int64_t n, int d, int both,
                   const uint32_t* const* slots, uint64_t nonce, void* stream);
// mx_ks_cross1_s with the previous level's xor folded in: the level's g is g ^ t (t = the
// previous level's reshared AND, both share components), written to go0 / go1 and used for
// the cross terms (t0 == null: plain mx_ks_cross1_s, go unused)
int mx_ks_cross1x_s(int dev, int words, const void* g0, const void* g1, const void* t0,
                    const void* t1, void* go0, void* go1, const void* p0, const void* p1,
                    void* z, int64_t n, int d, int both, const uint32_t* const* slots,
                    uint64_t nonce, void* stream);
// The adder's sum after the last level, both share components: o = p ^ ((g ^ t) << 1)
int mx_ks_sum2(int dev, int words, const void* p0, const void* p1, const void* g0,
               const void* g1, const void* t0, const void* t1, void* o0, void* o1, int64_t n,
               void* stream);
// mx_prf_expand with nkeys consecutive key slots
int mx_prf_expand_k(int dev, int words, void* out, int64_t n, int nkeys, const uint32_t* slots,
                    uint64_t nonce, void* stream);
int mx_trunc_pr3_k(int dev, int words, const void* s0, void* out0, void* out1, int64_t n, int m,
                   const uint32_t* slot_k0, const uint32_t* slot_k2, const uint64_t* nonces,
                   void* stream);
int mx_trunc_pr3_ko(int dev, int words, const void* s0, void* out0, void* out1, int64_t n,
                    int m, const uint32_t* slot_k0, const uint32_t* slot_k2,
                    const uint64_t* nonces, int64_t ostride, void* stream);
int mx_trunc_pr3_kmo(int dev, int words, const void* s0, void* out0, void* out1, int64_t n,
                     int m, const uint32_t* slot_k0, const uint32_t* slot_k2,
                     const uint64_t* nonces, int64_t ostride, const uint64_t* cm, void* stream);
int mx_share3_k(int dev, int kind, int words, const void* x, void* out0, void* out1, int64_t n,
                int j, const uint32_t* slot_next, const uint32_t* slot_all, uint64_t n1,
                uint64_t na, void* stream);
// ring_extend3: exact widening of a replicated sharing over Z_2^64 to Z_2^128, valid for
// -2^62 <= x < 2^62 (rss_fused.h).  s0: [3, n] u64 slots; out0 / out1: [3, n] u128 slot
// vectors (out1 == out0 + n: the 4-slot ring).  nonces: r0, r1, R0, M0, z0, z2 (dealer keys
// k0, k2), every stream drawn at 128-bit width.
int mx_ring_extend3_k(int dev, const void* s0, void* out0, void* out1, int64_t n,
                      const uint32_t* slot_k0, const uint32_t* slot_k2, const uint64_t* nonces,
                      void* stream);
// largest n that the device entry point runs with the latency form of the kernel
int64_t mx_ring_extend3_lat_max(void);

// Per-party protocol rounds for layouts with the parties of a session on different GPUs
// (rss_party.hip): ncomp stacked components [ncomp, n], component c in role roles[c]
// (-1 = idle), key slots (own k_p, next k_{p+1}) per component.  nonces: r0, r1, t, m, z0,
// z2 of the TruncPr.  Round 0 writes the outgoing messages (P0: mk0, P1: mk1, P2: rt1 in
// msg; P2: rm1 in msg_rm as u64) and P2's new shares; round 1 takes the received mask
// share (rmk) and dealer shares (rrt, rrm) and writes w (P0: y0 - z0, P1: y1 - z2) and
// P0's s0 / P1's s1.
int mx_trunc_party_r0(int dev, int words, int64_t n, int m, int ncomp, const int* roles,
                      const void* s0, const void* s1, void* msg, void* msg_rm, void* out0,
                      void* out1, const uint32_t* const* slots, const uint64_t* nonces,
                      void* stream);
int mx_trunc_party_r1(int dev, int words, int64_t n, int m, int ncomp, const int* roles,
                      const void* msg, const void* rmk, const void* rrt, const void* rrm,
                      void* w, void* out0, void* out1, const uint32_t* const* slots,
                      const uint64_t* nonces, void* stream);
// Per-party rounds of the ring extension Z_2^64 -> Z_2^128 (rss_party.hip), same layout:
// s0, s1, msg, rmk, msg_M / rM: [ncomp, n] u64; msg_R / rR, w, out0, out1: [ncomp, n] u128.
// nonces: r0, r1, R0, M0, z0, z2, every stream drawn at 128-bit width (as mx_ring_extend3_k).
// Round 0 writes the outgoing messages (P0 / P1: the masked opening share in msg; P2: R1 in
// msg_R, M1 in msg_M) and P2's new shares; round 1 takes the other party's msg (rmk) and the
// dealer shares (rR, rM; P1 only) and writes w (P0: y0 - z0, P1: y1 - z2) and P0's s0 /
// P1's s1.
int mx_ring_extend_party_r0(int dev, int64_t n, int ncomp, const int* roles, const void* s0,
                            const void* s1, void* msg, void* msg_R, void* msg_M, void* out0,
                            void* out1, const uint32_t* const* slots, const uint64_t* nonces,
                            void* stream);
int mx_ring_extend_party_r1(int dev, int64_t n, int ncomp, const int* roles, const void* msg,
                            const void* rmk, const void* rR, const void* rM, void* w, void* out0,
                            void* out1, const uint32_t* const* slots, const uint64_t* nonces,
                            void* stream);
// Share by member j, per component: rel[c] = (role - j) mod 3; key slots per component:
// rel 0 (next, all), rel 1 (own, all), rel 2 (all, all).  The owner's out0 (its masked
// x_j) is then sent to P_{j+2}, whose out1 it becomes.
int mx_share_party(int dev, int kind, int words, int64_t n, int ncomp, const int* rel,
                   const void* x, void* out0, void* out1, const uint32_t* const* slots,
                   uint64_t n1, uint64_t na, void* stream);
// Fixed-point dot tail (rep.dot_trunc) with the parties on different GPUs: the reshare of
// the dot is folded into TruncPr's first round (rss_party.hip).  Every array argument is
// an array of ncomp per-component pointers (entries a role does not use may be null).
// nonces: zero share, r0, r1, t, m, z0, z2.  r0: messages (P0 m0, P1 m1, P2 z2) in msg, the
// dealer's rt1 / rm1 (u64) in msg_rt / msg_rm, P2's new shares; r1: rmk = the other
// party's message, rz = z2, rrt / rrm = dealer shares (P1) -> w, P0's s0 / P1's s1;
// r2: out = a + b (P0's s1, P1's s0).
int mx_dot_tail_r0(int dev, int words, int64_t n, int m, int ncomp, const int* roles,
                   const void* const* cross, void* const* msg, void* const* msg_rt,
                   void* const* msg_rm, void* const* out0, void* const* out1,
                   const uint32_t* const* slots, const uint64_t* nonces, void* stream);
int mx_dot_tail_r1(int dev, int words, int64_t n, int m, int ncomp, const int* roles,
                   const void* const* msg, const void* const* rmk, const void* const* rz,
                   const void* const* rrt, const void* const* rrm, void* const* w,
                   void* const* out0, void* const* out1, const uint32_t* const* slots,
                   const uint64_t* nonces, void* stream);
int mx_dot_tail_r2(int dev, int words, int64_t n, int ncomp, const int* roles,
                   const void* const* a, const void* const* b, void* const* out, void* stream);

// The same tail for ONE party over up to MX_MAX_JOBS products ("jobs", rss_jobs.hip): job q
// is ptrs[8q..8q+7] = (x0, x1, y0, y1, a, a2, o0, o1) and dims[8q..8q+7] = (rows, sx, sy, sa,
// sa2, ca, ca2, cb): value[r, e] = cb (x0 y0 + x0 y1 + x1 y0) + ca a + ca2 a2 (row r of x at
// x + r sx, ...), for rows of length L; the new shares go to o0 / o1 (dense [rows, L]).
// Messages are dense over the concatenation of the jobs' rows.  main: the values' messages;
// dealer: P2's part.
#define MX_MAX_JOBS 4
int mx_jobs_r0(int dev, int words, int njobs, const void* const* ptrs, const int64_t* dims,
               int64_t L, int m, int role, int main, int dealer, void* msg, void* msg_rt,
               void* msg_rm, const uint32_t* const* slots, const uint64_t* nonces,
               void* stream);
// mx_jobs_r0 with the previous level's round-2 sums pending: region k = (o, a, b) =
// pend[3k .. 3k+2] of pend_len[k] elements, o = a + b; operands read through them, and the
// regions written too (one launch instead of the previous round 2 plus this round 0)
int mx_jobs_r0p(int dev, int words, int njobs, const void* const* ptrs, const int64_t* dims,
                int64_t L, int m, int role, int main, int dealer, void* msg, void* msg_rt,
                void* msg_rm, const uint32_t* const* slots, const uint64_t* nonces, int npend,
                const void* const* pend, const int64_t* pend_len, void* stream);
int mx_jobs_r1(int dev, int words, int njobs, const void* const* ptrs, const int64_t* dims,
               int64_t L, int m, int role, const void* msg, const void* rmk, const void* rz,
               const void* rrt, const void* rrm, void* w, const uint32_t* const* slots,
               const uint64_t* nonces, void* stream);
int mx_jobs_r2(int dev, int words, int njobs, const void* const* ptrs, const int64_t* dims,
               int64_t L, int role, const void* a, const void* b, void* stream);

// Per-party bit decomposition front and B2A (bits_party.h, rss_bits_party.hip): nonces
// nn = (n1 of the sharing, n_g of the product).  front: this party's p pair and zero-shared
// AND term z (P0 also the share message a1; P1 runs after receiving a1 in arecv).  b2a:
// phase 0 (P0, P2) / 1 (P1, arecv = A1): message (P0's A1), z, base pair of bit planes
// start.. start + count - 1 of src = (s0, s1, g0, g1, t0, t1) -- sum words (g0 = null) or
// the adder's last (p, g, t); phase 2: out = base - 2 (z, zr).  Elements [count, S].
int mx_bits_front(int dev, int words, int role, int64_t n, const void* xa, const void* xb,
                  const void* arecv, void* msg, void* z, void* p0, void* p1,
                  const uint32_t* const* slots, const uint64_t* nonces, void* stream);
// Per-party fused weighted sums over both share components (wsum_pair.h): ring values as
// ``words`` little-endian int64 each (w: nrows of them, cb: nblk).
int mx_wsum_pair(int dev, int words, int nrows, int nblk, int has2, int pub0, int pub1,
                 int64_t L, int64_t rs, const int64_t* w, const int64_t* wx, const int64_t* m2,
                 const int64_t* c2, const int64_t* cb, const void* r0, const void* r1,
                 const void* x0, const void* x1, void* o0, void* o1, void* q0, void* q1,
                 void* stream);
int mx_bits_b2a(int dev, int words, int phase, int role, int64_t S, int start, int count,
                int xbit, int blocks, const void* const* src, const void* arecv, void* msg, void* z, void* base0,
                void* base1, const void* zr, void* out0, void* out1,
                const uint32_t* const* slots, const uint64_t* nonces, void* stream);

#ifdef __cplusplus
}
#endif
