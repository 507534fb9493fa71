"""Every ring GEMM path against exact integer arithmetic, at its edges.

The host GEMM, the VALU and gemv kernels, the limb MFMA kernels, the tile-order knobs and the CRT
GEMM are each forced, run, and compared with an oracle that holds no project code: python
``int`` (numpy object arrays), or for Z_2^64 numpy ``uint64`` arithmetic, which wraps exactly
(test_uint64_oracle_is_the_int_oracle).  The host kernels are never the oracle.  Everything is
exact equality.

Two kinds of operand keep the oracle cheap:

* dense edge operands (products of at most a few 10^5 multiply-adds): the boundary elements of
  test_ring_edges.edges plus the balanced-limb boundaries -- 0x7f / 0x80 / 0xff in every limb,
  0x80 under a run of 0xff up to the top limb (a carry through every limb that then vanishes),
  all-0x80, all-0x7f -- and random fill;
* separable operands A[i,k] = a_i h_k, B[k,j] = g_k b_j with h of period 5 and g of period 7:
  C[i,j] = a_i b_j S, S = sum_k h_k g_k, an O(MN + K) oracle in which every entry differs, so
  a misplaced, transposed, duplicated or missing tile shows, and a shift of k between the two
  operands changes S.
"""
import ctypes
import random
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from moose_amd.ops import native as nat
from moose_amd.ops import ring as R
from test_ring_edges import edges
from test_ring_edges import mask

gpu = pytest.mark.gpu
DEVICES = ["cpu", pytest.param("cuda", marks=gpu)]
WIDTHS = [64, 128]
MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------------------
# ring tensors <-> integers (numpy only)
# ---------------------------------------------------------------------------
def to_rt(values, bits, device):
    """Object array of ints (any sign, any size) or uint64 array -> ring tensor."""
    a = np.asarray(values)
    if a.dtype == np.uint64:
        assert bits == 64
        return R.RT(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(device), 64)
    a = np.asarray(values, dtype=object) % (1 << bits)
    lo = (a & MASK64).astype(np.uint64)
    if bits == 64:
        return R.RT(torch.from_numpy(lo.view(np.int64)).to(device), 64)
    hi = (a >> 64).astype(np.uint64)
    return R.RT(torch.from_numpy(np.stack([lo, hi], axis=-1).view(np.int64)).to(device), 128)


def to_obj(x):
    """Ring tensor -> object array of unsigned python ints."""
    d = x.data.detach().cpu().contiguous().numpy().view(np.uint64)
    if x.bits == 64:
        return d.astype(object)
    return d[..., 0].astype(object) + d[..., 1].astype(object) * (1 << 64)


def same(got, want, what):
    """Exact equality of a ring tensor with the oracle's array (object ints, or uint64 for
    Z_2^64); on failure the count of wrong entries and the first few (index, got, want)."""
    want = np.asarray(want)
    if want.dtype == np.uint64:
        g = got.data.detach().cpu().contiguous().numpy().view(np.uint64)
    else:
        g, want = to_obj(got), np.asarray(want, dtype=object) % (1 << got.bits)
    assert g.shape == want.shape, f"{what}: shape {g.shape}, want {want.shape}"
    bad = np.argwhere(g != want)
    assert len(bad) == 0, (
        f"{what}: {len(bad)} of {want.size} wrong; (index, got, want): "
        + str([(tuple(int(v) for v in i), hex(int(g[tuple(i)])), hex(int(want[tuple(i)])))
               for i in bad[:6]]))


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
def limb_edges(bits):
    """edges(bits) plus the boundaries of the balanced 8-bit limb split."""
    L = bits // 8
    out = list(edges(bits))
    for byte in (0x7F, 0x80, 0xFF):
        out += [byte << (8 * l) for l in range(L)]
    # 0x80 in limb l under 0xff up to the top: the carry runs through every limb and vanishes
    out += [(0x80 << (8 * l)) | (mask(bits) >> (8 * (l + 1)) << (8 * (l + 1))) for l in range(L)]
    out += [int.from_bytes(b"\x80" * L, "little"), int.from_bytes(b"\x7f" * L, "little")]
    seen = []
    for v in out:
        if v not in seen:
            seen.append(v)
    return seen


def dense(bits, shape, seed):
    """Object array: every edge once (as far as they fit) at random places, then half edges,
    half random elements."""
    r = random.Random(seed)
    E = limb_edges(bits)
    n = int(np.prod(shape))
    vals = [r.choice(E) if r.random() < 0.5 else r.getrandbits(bits) for _ in range(n)]
    for pos, e in zip(r.sample(range(n), min(n, len(E))), r.sample(E, len(E))):
        vals[pos] = e
    a = np.empty(n, dtype=object)
    a[:] = vals
    return a.reshape(shape)


def dense_oracle(A0, A1, B0, B1, bits, C0=None):
    """[batch, M, K] x [batch, K, N] in python ints: A0.B0, or A0.(B0 + B1) + A1.B0."""
    out = []
    for b in range(A0.shape[0]):
        c = A0[b].dot(B0[b]) if A1 is None else A0[b].dot(B0[b] + B1[b]) + A1[b].dot(B0[b])
        out.append(c if C0 is None else c + C0[b])
    return np.array(out, dtype=object).reshape(A0.shape[0], A0.shape[1], B0.shape[2]) % (1 << bits)


class Sep:
    """One separable operand: per batch entry a vector v (distinct entries: a few edges, the
    rest random odd elements, so that products do not collapse) and a k-sequence of period
    ``period`` over {-1, 2^8, 2^63, 2^(w-1) + 1, random}.  rows(): A[b, i, k] = v[b, i] seq[b, k];
    cols(): B[b, k, j] = seq[b, k] v[b, j]."""

    def __init__(self, bits, batch, n, period, seed):
        r = random.Random(seed)
        self.bits, self.batch, self.n, self.period = bits, batch, n, period
        E = limb_edges(bits)
        self.v, self.seq = [], []
        for _ in range(batch):
            v = [r.getrandbits(bits) | 1 for _ in range(n)]
            for pos, e in zip(r.sample(range(n), min(n // 8, len(E))), r.sample(E, len(E))):
                v[pos] = e
            assert len(set(v)) == n
            self.v.append(v)
            pool = [mask(bits), 1 << 8, 1 << 63, (1 << (bits - 1)) + 1, r.getrandbits(bits) | 1,
                    r.getrandbits(bits) | 1, 3]
            self.seq.append(r.sample(pool, period))

    def _block(self, b):
        """[n, period] object array of v_i seq_k mod 2^w."""
        v = np.array(self.v[b], dtype=object).reshape(-1, 1)
        s = np.array(self.seq[b], dtype=object).reshape(1, -1)
        return (v * s) % (1 << self.bits)

    def rows(self, K, device):
        """[batch, n, K] ring tensor (built as one period and tiled on the device)."""
        reps = K // self.period + 1
        blk = to_rt(np.stack([self._block(b) for b in range(self.batch)]), self.bits, device).data
        tail = (1,) if self.bits == 128 else ()
        return R.RT(blk.repeat((1, 1, reps) + tail)[:, :, :K].contiguous(), self.bits)

    def cols(self, K, device):
        """[batch, K, n] ring tensor."""
        reps = K // self.period + 1
        blk = to_rt(np.stack([self._block(b).T for b in range(self.batch)]), self.bits,
                    device).data
        tail = (1,) if self.bits == 128 else ()
        return R.RT(blk.repeat((1, reps, 1) + tail)[:, :K].contiguous(), self.bits)


def ksum(a, ba, g, bg, K):
    """S = sum_k a.seq[ba][k] g.seq[bg][k] over k < K, in python ints."""
    sa, sg = a.seq[ba], g.seq[bg]
    return sum(sa[k % len(sa)] * sg[k % len(sg)] for k in range(K))


def sep_term(a, ba, g, bg, K, fast):
    """The [n_a, n_g] product of a's rows form (entry ba) with g's cols form (entry bg):
    outer(v_a, v_g) S -- uint64 arithmetic when ``fast`` (Z_2^64), python ints otherwise."""
    S = ksum(a, ba, g, bg, K)
    if fast:
        va = np.array(a.v[ba], dtype=object).astype(np.uint64).reshape(-1, 1)
        vg = np.array(g.v[bg], dtype=object).astype(np.uint64).reshape(1, -1)
        return (va * vg) * np.array([S & MASK64], dtype=np.uint64)
    va = np.array(a.v[ba], dtype=object).reshape(-1, 1)
    vg = np.array(g.v[bg], dtype=object).reshape(1, -1)
    return (va * vg) * S % (1 << a.bits)


class SepCase:
    """Separable operands of one product [batch, M, K] x [batch, K, N] (both modes share them)
    and its oracle, written out plainly:
        mode 0:  C = a0 b0^T S00
        mode 1:  C = a0 b0^T S00 + a0 b1^T S01 + a1 b0^T S10      (x0.(y0 + y1) + x1.y0)."""

    def __init__(self, bits, batch, M, N, K, seed, device):
        self.bits, self.batch, self.M, self.N, self.K = bits, batch, M, N, K
        self.a0, self.a1 = Sep(bits, batch, M, 5, seed), Sep(bits, batch, M, 5, seed + 1)
        self.b0, self.b1 = Sep(bits, batch, N, 7, seed + 2), Sep(bits, batch, N, 7, seed + 3)
        self.device = device
        self._t = {}

    def operands(self, mode):
        if mode not in self._t:
            x0, y0 = self.a0.rows(self.K, self.device), self.b0.cols(self.K, self.device)
            self._t[0] = (x0, None, y0, None)
            if mode:
                self._t[1] = (x0, self.a1.rows(self.K, self.device), y0,
                              self.b1.cols(self.K, self.device))
        return self._t[mode]

    def oracle(self, mode, C0=None, fast=None):
        fast = self.bits == 64 if fast is None else fast
        out = []
        for b in range(self.batch):
            c = sep_term(self.a0, b, self.b0, b, self.K, fast)
            if mode:
                c = (c + sep_term(self.a0, b, self.b1, b, self.K, fast)
                     + sep_term(self.a1, b, self.b0, b, self.K, fast))
            out.append(c)
        c = np.stack(out)
        if C0 is not None:
            c = c + (C0.data.cpu().numpy().view(np.uint64) if fast else to_obj(C0))
        if not fast:
            c = c % (1 << self.bits)
        # the point of the construction: (almost) every entry differs from every other
        if c.size >= 64:
            distinct = len(set(c.reshape(-1).tolist()))
            assert distinct >= 0.7 * c.size, (distinct, c.size)
        return c


# ---------------------------------------------------------------------------
# calling the GEMMs
# ---------------------------------------------------------------------------
@contextmanager
def forced(impl, crt):
    """mx_set_gemm_impl (0 auto, 1 VALU, 2 MFMA) and mx_set_gemm_crt (0 auto, 1 CRT, 2 limb),
    restored to automatic on the way out."""
    lib = nat.lib()
    lib.mx_set_gemm_impl(impl)
    lib.mx_set_gemm_crt(crt)
    try:
        yield
    finally:
        lib.mx_set_gemm_impl(0)
        lib.mx_set_gemm_crt(0)


VALU, LIMB, CRT, AUTO = (1, 2), (2, 2), (2, 1), (0, 0)


def run_gemm(ops, bits, M, N, K, out=None, accumulate=0, raw=False):
    """The product of ops = (A0, A1 or None, B0, B1 or None) ([batch, M, K] / [batch, K, N])
    through ops.ring._gemm_call (which splits a long K), or with ``raw`` through one mx_gemm
    call, whose return code is then returned with the result."""
    a0, a1, b0, b1 = ops
    batch = a0.shape[0]
    mode = 0 if a1 is None else 1
    if out is None:
        out = R.empty((batch, M, N), bits, a0.device)
    d = [None if t is None else t.data for t in ops]
    if raw:
        rc = nat.lib().mx_gemm(nat.dev_of(out.data), bits // 64, batch, M, N, K, nat.ptr(d[0]),
                               nat.ptr(d[1]), nat.ptr(d[2]), nat.ptr(d[3]), mode,
                               nat.ptr(out.data), accumulate, nat.stream_of(out.data))
        return rc, out
    R._gemm_call(bits, batch, M, N, K, d[0], d[1], d[2], d[3], mode, out.data, accumulate)
    return out


def rand_rt(shape, bits, seed, device):
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(-(2**63), 2**63 - 1, tuple(shape) + ((2,) if bits == 128 else ()),
                      generator=g, dtype=torch.int64)
    return R.RT(d.to(device), bits)


def check_dense(bits, batch, M, N, K, mode, device, seed, accumulate=0, what=""):
    A0, B0 = dense(bits, (batch, M, K), seed), dense(bits, (batch, K, N), seed + 1)
    A1 = dense(bits, (batch, M, K), seed + 2) if mode else None
    B1 = dense(bits, (batch, K, N), seed + 3) if mode else None
    ops = tuple(None if t is None else to_rt(t, bits, device) for t in (A0, A1, B0, B1))
    C0 = rand_rt((batch, M, N), bits, seed + 4, device) if accumulate else None
    out = R.RT(C0.data.clone(), bits) if accumulate else None
    got = run_gemm(ops, bits, M, N, K, out=out, accumulate=accumulate)
    want = dense_oracle(A0, A1, B0, B1, bits, None if C0 is None else to_obj(C0))
    same(got, want, f"{what} dense Z_2^{bits} batch {batch} {M}x{N}x{K} mode {mode} "
                    f"acc {accumulate}")


def check_sep(case, mode, accumulate=0, what=""):
    C0 = (rand_rt((case.batch, case.M, case.N), case.bits, 977, case.device)
          if accumulate else None)
    out = R.RT(C0.data.clone(), case.bits) if accumulate else None
    got = run_gemm(case.operands(mode), case.bits, case.M, case.N, case.K, out=out,
                   accumulate=accumulate)
    same(got, case.oracle(mode, C0), f"{what} separable Z_2^{case.bits} batch {case.batch} "
         f"{case.M}x{case.N}x{case.K} mode {mode} acc {accumulate}")


# ---------------------------------------------------------------------------
# the oracle itself
# ---------------------------------------------------------------------------
def test_uint64_oracle_is_the_int_oracle():
    """numpy's uint64 products and sums wrap mod 2^64: the fast form of the separable oracle
    equals the python-int form, and both equal the plain triple loop over the materialised
    operands (which also pins Sep.rows / Sep.cols and the closed form itself)."""
    case = SepCase(64, 2, 9, 8, 83, 5, "cpu")
    for mode in (0, 1):
        x0, x1, y0, y1 = (None if t is None else to_obj(t) for t in case.operands(mode))
        loop = dense_oracle(x0, x1, y0, y1, 64)
        fast = case.oracle(mode)
        assert fast.dtype == np.uint64
        assert (fast.astype(object) == loop).all()
        assert (case.oracle(mode, fast=False) == loop).all()  # the python-int branch
    case = SepCase(128, 1, 7, 6, 40, 6, "cpu")
    x0, x1, y0, y1 = (to_obj(t) for t in case.operands(1))
    assert (case.oracle(1) == dense_oracle(x0, x1, y0, y1, 128)).all()


def test_limb_edges_hold_what_they_claim():
    for bits in WIDTHS:
        E, L = limb_edges(bits), bits // 8
        assert set(edges(bits)) <= set(E) and len(set(E)) == len(E)
        for l in range(L):
            assert all(b << (8 * l) in E for b in (0x7F, 0x80, 0xFF))
        assert mask(bits) ^ 0x7F in E  # 0x80 under 0xff in every higher limb
        assert (0x80 << (bits - 8)) in E
        assert int("80" * L, 16) in E and int("7f" * L, 16) in E
        d = dense(bits, (4, 40), 1).reshape(-1)
        assert set(E) <= set(d.tolist()) and max(d.tolist()) <= mask(bits)


# ---------------------------------------------------------------------------
# host GEMM
# ---------------------------------------------------------------------------
HOST_SHAPES = [(1, 1, 1), (3, 5, 4), (17, 33, 9), (64, 70, 65)]  # (M, N, K)


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_dense(shape, mode, batch, bits):
    M, N, K = shape
    check_dense(bits, batch, M, N, K, mode, "cpu", 100 + M, what="host")
    if shape == (17, 33, 9):
        check_dense(bits, batch, M, N, K, mode, "cpu", 150, accumulate=1, what="host")


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("batch", [1, 3])
def test_host_separable_long_k(batch, bits):
    case = SepCase(bits, batch, 11, 13, 9000, 200 + batch, "cpu")
    for mode in (0, 1):
        check_sep(case, mode, what="host")
    check_sep(case, 1, accumulate=1, what="host")


# ---------------------------------------------------------------------------
# VALU and gemv kernels (impl 1)
# ---------------------------------------------------------------------------
# gemv (N <= 4): 4 rows per block, 64 lanes split K -- both sides of 4 rows and of 64 / 128 k;
# N = 5 is the tiled kernel; the rest sit on both sides of its 16 x 16 tile and 16-wide k-step
VALU_SHAPES = [(1, 1, 1), (3, 1, 63), (4, 4, 64), (5, 4, 65), (9, 2, 130), (1, 5, 1), (6, 5, 65),
               (15, 17, 16), (16, 16, 17), (17, 15, 31), (33, 5, 40)]


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", VALU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_valu_dense(shape, mode, bits):
    M, N, K = shape
    with forced(*VALU):
        for batch in (1, 3):
            check_dense(bits, batch, M, N, K, mode, "cuda", 300 + M + N, what="valu")
        check_dense(bits, 2, M, N, K, mode, "cuda", 350, accumulate=1, what="valu")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
def test_valu_larger_than_the_mfma_threshold(bits):
    """impl 1 keeps a 'big' product (M, N >= 64, K >= 32) on the tiled kernel: several blocks
    in both directions, separable operands."""
    case = SepCase(bits, 2, 70, 67, 45, 360, "cuda")
    with forced(*VALU):
        for mode in (0, 1):
            check_sep(case, mode, what="valu")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("shape", [(17, 5, 9), (6, 1, 130), (5, 4, 70), (70, 66, 40)],
                         ids=lambda s: "x".join(map(str, s)))
def test_dot_slots_strided_view_broadcast_b(shape, bits):
    """mxh_gemm_bs on the VALU kernels: the slots are every second plane of a larger buffer
    (a_bs = 2 M K) and the public operand is read by every slot in place (b_bs = 0)."""
    M, N, K = shape
    A = dense(bits, (4, M, K), 400 + M)
    B = dense(bits, (1, K, N), 401 + M)
    buf = to_rt(np.stack([A, dense(bits, (4, M, K), 402)], axis=1), bits, "cuda")
    x = R.RT(buf.data[:, 0], bits)
    assert not x.data.is_contiguous()
    c = to_rt(B[0, :, 0] if N == 1 else B[0], bits, "cuda")
    with forced(*VALU):
        got = R.dot_slots(x, c)
    assert got is not None
    want = dense_oracle(A, None, np.repeat(B, 4, axis=0), None, bits)
    same(got, want[:, :, 0] if N == 1 else want, f"dot_slots Z_2^{bits} {shape}")


# ---------------------------------------------------------------------------
# limb MFMA kernels (impl 2, CRT off)
# ---------------------------------------------------------------------------
EDGE_MN = [63, 64, 65, 128, 129]
EDGE_K = [31, 32, 33, 64, 95]


def boundary_cases(bits, K, seed=500):
    """The 64-row / 64-column tile edges; Z_2^64 also with N = 192, so that the paired
    (128-column) block is met half used (65..128) and fully used in its second block."""
    ns = EDGE_MN + ([192] if bits == 64 else [])
    return [SepCase(bits, 1, M, N, K, seed + 7 * M + N, "cuda") for M in EDGE_MN for N in ns]


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K", EDGE_K)
def test_limb_tile_and_kstep_boundaries(K, mode, bits):
    """K: one k-step, an odd count of k-steps, a ragged K (mode 1: K' = 2 K)."""
    with forced(*LIMB):
        for case in boundary_cases(bits, K):
            check_sep(case, mode, what="limb")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(64, 64, 32), (65, 63, 33), (3, 129, 31)],
                         ids=lambda s: "x".join(map(str, s)))
def test_limb_dense_edges(shape, mode, bits):
    """The balanced-limb boundaries through k_prep_a / k_prep_b's carry chain and all L
    anti-diagonals; batch 3 and an accumulate into a non-zero C."""
    M, N, K = shape
    with forced(*LIMB):
        check_dense(bits, 3, M, N, K, mode, "cuda", 600 + M, what="limb")
        check_dense(bits, 1, M, N, K, mode, "cuda", 650 + M, accumulate=1, what="limb")


def tile_shapes(bits):
    """(tiles, M, N): block-tile counts 7, 8, 9, 10, 45 with tiles_m 1, 4, 9, 5, 9 (a block
    tile is 64 x 64, for Z_2^64 64 x 128), every edge ragged.  Under the default group of 4
    row bands tiles_m = 5 and 9 end in a partial group (gm < gM), and 7, 9, 10, 45 are no
    multiple of 8 (the XCD remap's remainder branch)."""
    w = 128 if bits == 64 else 64
    return [(7, 60, 7 * w - 9), (8, 250, 2 * w - 5), (9, 570, w - 3), (10, 310, 2 * w - 11),
            (45, 570, 5 * w - 20)]


_TILE_CASES = {}


def tile_case(bits, tiles):
    """One separable case per (ring, tile count), built once and shared (the tile-order knobs
    run the same operands again); batch 2 except at 45 tiles."""
    if (bits, tiles) not in _TILE_CASES:
        _, M, N = next(s for s in tile_shapes(bits) if s[0] == tiles)
        _TILE_CASES[bits, tiles] = SepCase(bits, 1 if tiles == 45 else 2, M, N, 40,
                                           700 + tiles, "cuda")
    return _TILE_CASES[bits, tiles]


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("tiles", [7, 8, 9, 10, 45])
def test_limb_every_tile_once(tiles, bits):
    with forced(*LIMB):
        for mode in (0, 1):
            check_sep(tile_case(bits, tiles), mode, what=f"limb {tiles} tiles")


# gemm_group_m() / gemm_xcd() (csrc/gemm_mfma.hip) call getenv on every launch: nothing is
# cached, so setting the variable in this process is enough
KNOBS = [("MOOSEX_GEMM_GROUPM", "1"), ("MOOSEX_GEMM_GROUPM", "3"), ("MOOSEX_GEMM_GROUPM", "64"),
         ("MOOSEX_GEMM_XCD", "0")]


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("tiles", [7, 10, 45])
@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: k[0][12:] + k[1])
def test_tile_order_knobs(knob, tiles, bits, monkeypatch):
    """Which block computes which tile changes, the product does not: groups of 1, 3 and 64
    row bands (3: tiles_m = 5 ends in a partial group of 2; 64: the only group is partial) and
    the plain block order."""
    monkeypatch.setenv(*knob)
    with forced(*LIMB):
        check_sep(tile_case(bits, tiles), 0, what=f"limb {tiles} tiles {knob}")
        check_sep(tile_case(bits, tiles), 1, accumulate=1, what=f"limb {tiles} tiles {knob}")


def chunk_limit(bits, mode):
    """The longest K of one exact launch (K' = 16384 / 8192 limb-bytes per row)."""
    return (16384 if bits == 64 else 8192) // (2 if mode else 1)


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("over", [0, 1])
def test_limb_chunk_limit(over, mode, bits):
    """K' exactly at the limit of one launch, and one past it, where the splitter leaves a
    remainder chunk of K = 1 accumulated into the first chunk's result."""
    K = chunk_limit(bits, mode) + over
    case = SepCase(bits, 1, 65, 66, K, 800 + over, "cuda")
    with forced(*LIMB):
        if not over:  # one launch: the entry point itself takes it
            rc, got = run_gemm(case.operands(mode), bits, 65, 66, K, raw=True)
            assert rc == 0
            same(got, case.oracle(mode), f"limb one launch K {K} mode {mode}")
        else:  # ... and refuses one more before any launch
            rc, _ = run_gemm(case.operands(mode), bits, 65, 66, K, raw=True)
            assert rc == -6
        check_sep(case, mode, what="limb chunked")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("mode", [0, 1])
def test_limb_accumulate_single_chunk(mode, bits):
    case = SepCase(bits, 3, 129, 130, 70, 820, "cuda")
    with forced(*LIMB):
        check_sep(case, mode, accumulate=1, what="limb")


@gpu
@pytest.mark.parametrize("shape", [(576, 70, 8192), (2112, 70, 16384)],
                         ids=lambda s: "x".join(map(str, s)))
def test_limb_prep_past_the_grid_cap(shape):
    """launch_prep_a caps its grid at 8192 blocks of 256 threads, 16 k per thread: the second
    trip of k_prep_a's loop starts at Mp Kp > 2^25, which 2112 x 16384 (Z_2^64, one launch)
    passes; 576 x 8192 stays on the first trip with 9 row bands."""
    M, N, K = shape
    case = SepCase(64, 1, M, N, K, 830, "cuda")
    with forced(*LIMB):
        check_sep(case, 0, what="limb long rows")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
def test_gemm_with_b_row_blocks(bits):
    """mx_gemm_with_b (dot_cross_rows): B' prepared once, A row blocks at offsets that are no
    multiple of the 64-row tile, read in place through the batch stride M K."""
    M, N, K = 200, 70, 40
    case = SepCase(bits, 3, M, N, K, 840, "cuda")
    x0, x1, y0, y1 = case.operands(1)
    want = case.oracle(1)
    with forced(*LIMB):
        pb = R.PreparedCross(y0, y1)
        assert pb.lb is not None
        for r0, r1 in ((37, 137), (1, 200), (130, 131)):
            same(R.dot_cross_rows(x0, x1, r0, r1, pb), want[:, r0:r1],
                 f"gemm_with_b Z_2^{bits} rows [{r0}, {r1})")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("mode", [0, 1])
def test_gemm_strided_padded_a_broadcast_b(mode, bits):
    """mx_gemm_strided: a_bstride larger than M K (rows of a padded buffer) and b_bstride = 0
    (one B for the whole batch)."""
    M, N, K, batch, pad = 65, 70, 33, 3, 24
    el = bits // 64
    a = SepCase(bits, batch, M, N, K, 850, "cuda")
    one = SepCase(bits, 1, M, N, K, 851, "cuda")  # its B operands serve every batch entry
    x0, x1, _, _ = a.operands(1)
    _, _, y0, y1 = one.operands(1)

    def padded(x):  # [batch, M K + pad] elements, the pad filled with ones
        buf = torch.ones((batch, (M * K + pad) * el), dtype=torch.int64, device="cuda")
        buf[:, :M * K * el] = x.data.reshape(batch, -1)
        return buf

    p0, p1 = padded(x0), padded(x1)
    out = R.empty((batch, M, N), bits, "cuda")
    with forced(*LIMB):
        rc = nat.lib().mx_gemm_strided(
            el, batch, M, N, K, nat.ptr(p0), nat.ptr(p1) if mode else None, M * K + pad,
            nat.ptr(y0.data), nat.ptr(y1.data) if mode else None, 0, mode, nat.ptr(out.data), 0,
            nat.stream_of(out.data))
    assert rc == 0
    fast = bits == 64
    want = []
    for b in range(batch):
        c = sep_term(a.a0, b, one.b0, 0, K, fast)
        if mode:
            c = c + sep_term(a.a0, b, one.b1, 0, K, fast) + sep_term(a.a1, b, one.b0, 0, K, fast)
        want.append(c)
    same(out, np.stack(want), f"gemm_strided Z_2^{bits} mode {mode}")


@gpu
def test_limb_and_crt_scratch_two_pools_keyed_by_stream_grow_only():
    """The limb GEMM and the CRT GEMM each keep a scratch pool of their own (csrc/gemm_ws.h),
    one grow-only buffer per stream: on a stream neither has seen, the first limb product
    allocates one buffer (la + lb = 128 KiB here, so the 1 MiB minimum), the first CRT product
    another, and repeats of both allocate nothing.  No lookup falls back to the shared slot."""
    lib = nat.lib()
    raw = ctypes.c_void_p()  # a new HIP stream: one from torch's pool may have run GEMMs before
    assert lib.hipStreamCreate(ctypes.byref(raw)) == 0  # resolved in the runtime the library links
    stream = torch.cuda.ExternalStream(raw.value)  # kept for the process: its slots stay keyed
    case = SepCase(64, 1, 65, 66, 33, 960, "cuda")
    ops, want = case.operands(0), case.oracle(0)
    shared = lib.mx_workspace_shared_count()
    torch.cuda.synchronize()
    got, held = [], [lib.mx_workspace_held_bytes()]
    with torch.cuda.stream(stream):
        for path in (LIMB, CRT, LIMB, CRT):
            with forced(*path):
                got.append(run_gemm(ops, 64, 65, 66, 33))
            held.append(lib.mx_workspace_held_bytes())
        stream.synchronize()
    for g, what in zip(got, ("limb", "crt", "limb again", "crt again")):
        same(g, want, f"{what} on a new stream")
    grew = [b - a for a, b in zip(held, held[1:])]
    print("workspace growth per product:", grew)
    assert grew[0] == 1 << 20
    assert grew[1] >= 1 << 20 and grew[1] & (grew[1] - 1) == 0  # one power-of-two buffer
    assert grew[2:] == [0, 0]
    assert lib.mx_workspace_shared_count() == shared == 0


# ---------------------------------------------------------------------------
# CRT GEMM (mx_set_gemm_crt(1))
# ---------------------------------------------------------------------------
def crt_step_kprimes(bits):
    """From mx_crt_moduli: for every K' <= 32768 at which the modulus count steps, the last K'
    before the step and the first after it (the reconstruction's rounding slack is smallest at
    the largest K' that still uses n moduli); then the largest K' the CRT GEMM takes, and the
    one before."""
    lib, words = nat.lib(), bits // 64
    ks, prev = [], lib.mx_crt_moduli(words, 1)
    for kp in range(2, 32769):
        n = lib.mx_crt_moduli(words, kp)
        if n != prev:
            ks += [kp - 1, kp]
            prev = n
    assert ks and all(lib.mx_crt_moduli(words, k) > 0 for k in ks + [32768])
    return sorted(set(ks + [32767, 32768]))


def _const(bits, shape, value):
    return to_rt(np.full((1, 1), value, dtype=object), bits, "cuda").data.expand(
        shape + ((2,) if bits == 128 else ())).contiguous()


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
def test_crt_worst_case_constants_at_every_modulus_step(bits):
    """Every entry the signed minimum or maximum: |Z| is as large as K' allows, so the
    reconstruction's q = round(sum c_i / p_i) sits at its smallest slack.  C = K' a b, and in
    the cross form (K = K' / 2, y1 = 0) C = K' a b again."""
    lo, hi = 1 << (bits - 1), (1 << (bits - 1)) - 1
    kps = crt_step_kprimes(bits)
    print(f"Z_2^{bits} K' at the modulus steps: {kps}")
    M = N = 16
    with forced(*CRT):
        for kp in kps:
            for a, b in ((lo, lo), (lo, hi), (hi, lo), (hi, hi)):
                want = np.full((1, M, N), kp * a * b, dtype=object)
                A, B = R.RT(_const(bits, (1, M, kp), a), bits), R.RT(_const(bits, (1, kp, N), b),
                                                                    bits)
                rc, got = run_gemm((A, None, B, None), bits, M, N, kp, raw=True)
                assert rc == 0, (kp, rc)
                same(got, want, f"crt plain K' {kp} of {kps} a {a:#x} b {b:#x}")
                if kp % 2 == 0:
                    k = kp // 2
                    A = R.RT(A.data[:, :, :k].contiguous(), bits)
                    B = R.RT(B.data[:, :k].contiguous(), bits)
                    Z = R.zeros((1, k, N), bits, "cuda")
                    rc, got = run_gemm((A, A, B, Z), bits, M, N, k, raw=True)
                    assert rc == 0, (kp, rc)
                    same(got, want, f"crt cross K' {kp} of {kps} a {a:#x} b {b:#x}")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
def test_crt_separable_at_every_modulus_step(bits):
    kps = crt_step_kprimes(bits)
    print(f"Z_2^{bits} K' at the modulus steps: {kps}")
    with forced(*CRT):
        for kp in kps:
            case = SepCase(bits, 1, 16, 16, kp, 900, "cuda")
            rc, got = run_gemm(case.operands(0), bits, 16, 16, kp, raw=True)
            assert rc == 0, (kp, rc)
            same(got, case.oracle(0), f"crt plain separable K' {kp} of {kps}")
            if kp % 2 == 0:
                case = SepCase(bits, 1, 16, 16, kp // 2, 901, "cuda")
                rc, got = run_gemm(case.operands(1), bits, 16, 16, kp // 2, raw=True)
                assert rc == 0, (kp, rc)
                same(got, case.oracle(1), f"crt cross separable K' {kp} of {kps}")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
def test_crt_refuses_one_past_its_longest_k(bits):
    """K' = 32769: the entry point answers -6 before any launch (no CRT past 2^15, and no
    limb launch past the chunk limit); the K splitter then runs it in chunks, each a CRT
    product accumulated into the result, and the sum is exact."""
    case = SepCase(bits, 1, 16, 16, 32769, 910, "cuda")
    with forced(*CRT):
        keep = rand_rt((1, 16, 16), bits, 911, "cuda")
        out = R.RT(keep.data.clone(), bits)
        rc, out = run_gemm(case.operands(0), bits, 16, 16, 32769, out=out, raw=True)
        assert rc == -6
        assert torch.equal(out.data, keep.data)
        check_sep(case, 0, what="crt chunked")
        check_sep(case, 0, accumulate=1, what="crt chunked")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("shape", [(255, 256, 512), (256, 255, 512), (256, 256, 511),
                                   (256, 256, 512)], ids=lambda s: "x".join(map(str, s)))
def test_auto_crt_threshold_from_both_sides(shape, bits):
    """Automatic dispatch around M >= 256, N >= 256, K' >= 512: exact whichever GEMM runs.
    Mode 1 at K = K' / 2 (512 -> CRT, 511 -> K' = 510, limb)."""
    M, N, kp = shape
    with forced(*AUTO):
        check_sep(SepCase(bits, 1, M, N, kp, 920, "cuda"), 0, what="auto")
        check_sep(SepCase(bits, 1, M, N, kp // 2, 921, "cuda"), 1, what="auto")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("shape", [(63, 64, 32), (64, 63, 32), (64, 64, 31), (64, 64, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_auto_mfma_threshold_from_both_sides(shape, bits):
    """Automatic dispatch around M >= 64, N >= 64, K >= 32 (VALU below, limb MFMA from there)."""
    M, N, K = shape
    with forced(*AUTO):
        for mode in (0, 1):
            check_dense(bits, 1, M, N, K, mode, "cuda", 930 + M, what="auto")


class PartyCase:
    """Separable share stacks of a replicated product: x_q = alpha_q h_q^T [M, K] and
    y_q = g_q beta_q^T [K, N] per party q, so x_q . y_r = alpha_q beta_r^T S(h_q, g_r)."""

    def __init__(self, bits, M, N, K, seed):
        self.bits, self.M, self.N, self.K = bits, M, N, K
        self.x, self.y = Sep(bits, 3, M, 5, seed), Sep(bits, 3, N, 7, seed + 1)
        self.x1, self.y1 = Sep(bits, 3, M, 5, seed + 2), Sep(bits, 3, N, 7, seed + 3)
        self.X, self.Y = self.x.rows(K, "cuda"), self.y.cols(K, "cuda")
        self.X1, self.Y1 = self.x1.rows(K, "cuda"), self.y1.cols(K, "cuda")

    def P(self, a, q, g, r):
        return sep_term(a, q, g, r, self.K, self.bits == 64)

    def done(self, parts):
        c = np.stack(parts)
        return c if self.bits == 64 else c % (1 << self.bits)


_PARTY = {}


def party_case(bits):
    if bits not in _PARTY:
        _PARTY[bits] = PartyCase(bits, 300, 280, 320, 940)
    return _PARTY[bits]


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("roll", [1, 2])
def test_crt_rolled_pair_rows(roll, bits):
    """dot_cross_pair: z_p = x_p.(y0_p + y1_p) + x_{p+roll}.y0_p, all rows and rows [37, 250)."""
    c = party_case(bits)
    want = c.done([c.P(c.x, p, c.y, p) + c.P(c.x, p, c.y1, p) + c.P(c.x, (p + roll) % 3, c.y, p)
                   for p in range(3)])
    with forced(*CRT):
        got = R.dot_cross_pair(c.X, c.Y, c.Y1, roll)
        rows = R.dot_cross_pair(c.X, c.Y, c.Y1, roll, r0=37, r1=250)
    assert got is not None and rows is not None
    same(got, want, f"dot_cross_pair Z_2^{bits} roll {roll}")
    same(rows, want[:, 37:250], f"dot_cross_pair Z_2^{bits} roll {roll} rows [37, 250)")


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("rolled", [True, False], ids=["rolled", "explicit"])
def test_crt_asymmetric_product(rolled, bits):
    """dot_cross_asym, with (a, b, c, d) = party p's (x_p, x_{p+1}, y_p, y_{p+1}) (rolled) or
    four independent stacks (explicit):
        z_0 = (a + b)(c + d),   z_1 = b (c + d) + a d,   z_2 = a d + b c."""
    c = party_case(bits)
    if rolled:
        a, b = [(c.x, p) for p in range(3)], [(c.x, (p + 1) % 3) for p in range(3)]
        cc, d = [(c.y, p) for p in range(3)], [(c.y, (p + 1) % 3) for p in range(3)]
    else:
        a, b = [(c.x, p) for p in range(3)], [(c.x1, p) for p in range(3)]
        cc, d = [(c.y, p) for p in range(3)], [(c.y1, p) for p in range(3)]

    def pr(u, v):
        return c.P(u[0], u[1], v[0], v[1])

    want = c.done([pr(a[0], cc[0]) + pr(a[0], d[0]) + pr(b[0], cc[0]) + pr(b[0], d[0]),
                   pr(b[1], cc[1]) + pr(b[1], d[1]) + pr(a[1], d[1]),
                   pr(a[2], d[2]) + pr(b[2], cc[2])])
    with forced(*CRT):
        if rolled:
            got = R.dot_cross_asym(c.X, None, c.Y, None, rolled=True)
        else:
            got = R.dot_cross_asym(c.X, c.X1, c.Y, c.Y1)
    same(got, want, f"dot_cross_asym Z_2^{bits} rolled {rolled}")


# ---------------------------------------------------------------------------
# degenerate sizes
# ---------------------------------------------------------------------------
PATHS = [("cpu", AUTO), pytest.param("cuda", AUTO, marks=gpu, id="cuda-auto"),
         pytest.param("cuda", VALU, marks=gpu, id="cuda-valu"),
         pytest.param("cuda", LIMB, marks=gpu, id="cuda-limb"),
         pytest.param("cuda", CRT, marks=gpu, id="cuda-crt")]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("device,path", PATHS)
def test_degenerate_sizes(device, path, bits):
    """M, N or batch = 0: nothing is written and nothing fails.  K = 0: the product is zero --
    C is zero-filled, or unchanged under accumulate.  The forced limb and CRT paths answer
    K = 0 before any launch (their kernels stage k-step 0 before they look at the count)."""
    with forced(*path):
        for batch, M, N in ((0, 3, 4), (2, 0, 4), (2, 3, 0)):
            for mode in (0, 1):
                x = rand_rt((batch, M, 5), bits, 1, device)
                y = rand_rt((batch, 5, N), bits, 2, device)
                got = run_gemm((x, x if mode else None, y, y if mode else None), bits, M, N, 5)
                assert got.shape == (batch, M, N)
        for batch, M, N in ((1, 1, 1), (2, 3, 4), (1, 70, 65), (3, 64, 64)):
            for mode in (0, 1):
                x, y = R.empty((batch, M, 0), bits, device), R.empty((batch, 0, N), bits, device)
                ops = (x, x if mode else None, y, y if mode else None)
                keep = rand_rt((batch, M, N), bits, 3, device)
                got = run_gemm(ops, bits, M, N, 0, out=R.RT(keep.data.clone(), bits))
                same(got, np.zeros((batch, M, N), dtype=object), f"K = 0 {path} mode {mode}")
                got = run_gemm(ops, bits, M, N, 0, out=R.RT(keep.data.clone(), bits),
                               accumulate=1)
                assert torch.equal(got.data, keep.data), f"K = 0 accumulate {path} mode {mode}"


@gpu
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("path", [LIMB, CRT], ids=["limb", "crt"])
def test_k0_prepared_strided_and_rolled_entry_points(path, bits):
    """mx_gemm_with_b, mx_gemm_strided and mx_gemm_roll at K = 0: zero, or C kept."""
    lib, el, batch, M, N = nat.lib(), bits // 64, 3, 70, 65
    keep = rand_rt((batch, M, N), bits, 4, "cuda")
    st = nat.stream_of(keep.data)
    with forced(*path):
        for acc in (0, 1):
            want = to_obj(keep) if acc else np.zeros((batch, M, N), dtype=object)
            c = R.RT(keep.data.clone(), bits)
            assert lib.mx_gemm_with_b(el, batch, M, N, 0, None, None, 0, 1, None, nat.ptr(c.data),
                                      acc, st) == 0
            same(c, want, f"with_b K = 0 acc {acc}")
            c = R.RT(keep.data.clone(), bits)
            assert lib.mx_gemm_strided(el, batch, M, N, 0, None, None, 0, None, None, 0, 1,
                                       nat.ptr(c.data), acc, st) == 0
            same(c, want, f"strided K = 0 acc {acc}")
            c = R.RT(keep.data.clone(), bits)
            assert lib.mx_gemm_roll(el, batch, M, N, 0, None, 0, 1, None, None, None,
                                    nat.ptr(c.data), acc, st) == 0
            same(c, want, f"roll K = 0 acc {acc}")
        assert lib.mx_gemm_prep_b(el, batch, 0, N, None, None, 1, None, st) == 0
