"""The leaf ring kernels against plain integer arithmetic, at the values and sizes where they
can go wrong: limb boundaries, INT_MIN, shift counts past a limb, floats beyond the ring,
carries on every add of a reduction, and the second trip of the grid-stride loops.

Every fused protocol kernel is tested bitwise against a composition of these leaves, and
every device kernel against its host twin (test_native_gpu.py), so this file is where the
chain is tied to arithmetic.  The oracle is python: ``int`` masked to the ring, ``float(int)``
for correctly rounded conversions, ``int(float)`` plus clamping for encode (the reference
encodes with Rust's saturating ``as i64`` / ``as i128`` and decodes with the correctly rounded
``as f64``: host/ops.rs:1373, 1411-1414).  The host kernels are never the oracle, with one
stated exception (test_past_the_grid_cap).  Everything is exact equality.
"""
import math
import random
import struct

import numpy as np
import pytest
import torch

from moose_amd.ir.computation import ReplicatedPlacement
from moose_amd.ops import ring as R
from moose_amd.protocols import replicated as rep
from moose_amd.runtime.session import HV
from moose_amd.runtime.session import StackedSession

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
WIDTHS = [64, 128]
PLC = ReplicatedPlacement(("a", "b", "c"))


# ---------------------------------------------------------------------------
# the oracle's vocabulary
# ---------------------------------------------------------------------------
def mask(bits):
    return (1 << bits) - 1


def signed(v, bits):
    v &= mask(bits)
    return v - (1 << bits) if v >> (bits - 1) else v


def edges(bits):
    """The boundary elements of Z_2^bits (unsigned representatives, no repeats)."""
    e = [0, 1, mask(bits), 1 << (bits - 1), (1 << (bits - 1)) - 1,
         (1 << 63) - 1, 1 << 63, (1 << 64) - 1,
         2, (1 << 32) - 1, 1 << 32, (1 << 63) + 1, mask(bits) - 1]
    if bits == 128:
        e += [1 << 64, (1 << 64) + 1, (1 << 64) | (1 << 63), (1 << 127) | 1,
              # one high limb, low limbs on either side of the low limb's top bit
              (5 << 64) | 1, (5 << 64) | (1 << 63),
              # one low limb, high limbs that differ (and differ in sign)
              (6 << 64) | 1, (((1 << 63) | 5) << 64) | 1,
              (1 << 127) - (1 << 64), (1 << 127) | mask(64)]
    out = []
    for v in e:
        if v not in out:
            out.append(v)
    return out


def rnd(bits, n, seed):
    r = random.Random(seed)
    return [r.getrandbits(bits) for _ in range(n)]


def rt(values, bits, device):
    return R.from_ints(np.array(values, dtype=object), bits, device)


def ints(x):
    return [int(v) for v in np.asarray(R.to_ints(x)).reshape(-1)]


def same(got, want, what, show=hex):
    assert len(got) == len(want), f"{what}: {len(got)} results for {len(want)} cases"
    bad = [(i, show(g), show(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{what}: {len(bad)} of {len(want)} wrong; (index, got, want): {bad[:6]}"


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def same_f64(got, want, what, inputs):
    """Bitwise float64 equality (also tells -0.0 from 0.0)."""
    bad = [(hex(v), g, w) for v, g, w in zip(inputs, got, want) if f64_bits(g) != f64_bits(w)]
    assert len(got) == len(want) and not bad, (
        f"{what}: {len(bad)} of {len(want)} wrong; (element, got, want): "
        + "; ".join(f"({v}, {g!r}, {w!r})" for v, g, w in bad[:6]))


_BIN = {
    "add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b,
    "and": lambda a, b: a & b, "or": lambda a, b: a | b, "xor": lambda a, b: a ^ b,
}


def bin_ref(op, a, b, bits):
    return _BIN[op](a, b) & mask(bits)


def un_ref(op, v, k, bits):
    if op == "neg":
        return -v & mask(bits)
    if op == "not":
        return ~v & mask(bits)
    if op == "shl":
        return (v << k) & mask(bits)
    if op == "shr":
        return v >> k
    return (signed(v, bits) >> k) & mask(bits)  # sar: python's >> is arithmetic


def cmp_ref(op, a, b, bits):
    if op == "msb":
        return a >> (bits - 1)
    x, y = signed(a, bits), signed(b, bits)
    return int({"lt": x < y, "gt": x > y, "eq": x == y}[op])


def shifts(bits):
    return sorted({0, 1, 31, 32, 63, 64, 65, bits - 1, bits, bits + 1})


# ---------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("op", list(_BIN))
def test_binary_cross_product_and_scalar_broadcast(device, bits, op):
    E = edges(bits)
    A = [a for a in E for _ in E]
    B = [b for _ in E for b in E]
    ta, tb = rt(A, bits, device), rt(B, bits, device)
    want = [bin_ref(op, a, b, bits) for a, b in zip(A, B)]
    same(ints(R.binary(op, ta, tb)), want, f"{op} {bits}")
    # the pair kernel: (A op B, B op A)
    o0, o1 = R.binary2(op, ta, tb, tb, ta)
    same(ints(o0), want, f"{op} {bits} pair[0]")
    same(ints(o1), [bin_ref(op, b, a, bits) for a, b in zip(A, B)], f"{op} {bits} pair[1]")
    # a one-element operand on either side (na == 1 / nb == 1), and on both
    te = rt(E, bits, device)
    scalars = [mask(bits), 1 << (bits - 1), (1 << 63) | 1, E[-1]]
    for s in scalars:
        ts = rt([s], bits, device)
        same(ints(R.binary(op, ts, te)), [bin_ref(op, s, b, bits) for b in E],
             f"{op} {bits} scalar {s:#x} on the left")
        same(ints(R.binary(op, te, ts)), [bin_ref(op, a, s, bits) for a in E],
             f"{op} {bits} scalar {s:#x} on the right")
        for t in scalars:
            got = R.binary(op, ts, rt([t], bits, device))
            assert got.shape == (1,)
            same(ints(got), [bin_ref(op, s, t, bits)], f"{op} {bits} scalars {s:#x}, {t:#x}")
    # the pair kernel with one-element operands: (E op s, rev(E) op t) and (s op E, t op rev(E))
    s, t = scalars[1], scalars[2]
    ts, tt, tr = rt([s], bits, device), rt([t], bits, device), rt(E[::-1], bits, device)
    o0, o1 = R.binary2(op, te, ts, tr, tt)
    same(ints(o0), [bin_ref(op, a, s, bits) for a in E], f"{op} {bits} pair[0], nb == 1")
    same(ints(o1), [bin_ref(op, a, t, bits) for a in E[::-1]], f"{op} {bits} pair[1], nb == 1")
    o0, o1 = R.binary2(op, ts, te, tt, tr)
    same(ints(o0), [bin_ref(op, s, b, bits) for b in E], f"{op} {bits} pair[0], na == 1")
    same(ints(o1), [bin_ref(op, t, b, bits) for b in E[::-1]], f"{op} {bits} pair[1], na == 1")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_unary_at_every_shift_count(device, bits):
    V = edges(bits) + rnd(bits, 16, 2)
    ta, tr = rt(V, bits, device), rt(V[::-1], bits, device)
    cases = [("neg", 0), ("not", 0)] + [(op, k) for op in ("shl", "shr", "sar")
                                        for k in shifts(bits)]
    for op, k in cases:
        want = [un_ref(op, v, k, bits) for v in V]
        same(ints(R.unary(op, ta, k)), want, f"{op} {k} on {bits}")
        o0, o1 = R.unary2(op, ta, tr, k)
        same(ints(o0), want, f"{op} {k} on {bits}, pair[0]")
        same(ints(o1), want[::-1], f"{op} {k} on {bits}, pair[1]")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_compare_is_signed_on_both_limbs(device, bits):
    E = edges(bits)
    A = [a for a in E for _ in E]
    B = [b for _ in E for b in E]
    ta, tb, te = rt(A, bits, device), rt(B, bits, device), rt(E, bits, device)
    for op in ("lt", "gt", "eq"):
        got = R.compare(op, ta, tb)
        assert got.bits == 1 and got.data.dtype == torch.uint8
        same(ints(got), [cmp_ref(op, a, b, bits) for a, b in zip(A, B)], f"{op} {bits}")
        for s in (E[-1], 1 << (bits - 1), (1 << 63) | 1):
            ts = rt([s], bits, device)
            same(ints(R.compare(op, te, ts)), [cmp_ref(op, a, s, bits) for a in E],
                 f"{op} {bits} scalar {s:#x} on the right")
            same(ints(R.compare(op, ts, te)), [cmp_ref(op, s, b, bits) for b in E],
                 f"{op} {bits} scalar {s:#x} on the left")
        # a general broadcast: (5, 1) against (1, 7)
        col, row = E[3:8], E[1:8]
        got = R.compare(op, rt([[v] for v in col], bits, device), rt([row], bits, device))
        assert got.shape == (5, 7)
        same(ints(got), [cmp_ref(op, a, b, bits) for a in col for b in row],
             f"{op} {bits} (5, 1) x (1, 7)")
    same(ints(R.compare("msb", te)), [cmp_ref("msb", a, 0, bits) for a in E], f"msb {bits}")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_bit_extract_and_ring_inject(device, bits):
    V = edges(bits) + rnd(bits, 16, 3)
    ta = rt(V, bits, device)
    raw = [0, 1, 2, 3, 254, 255, 1, 0, 128, 129]  # only bit 0 of a byte counts
    tbits = R.RT(torch.tensor(raw, dtype=torch.uint8).to(device), 1)
    for bit in (0, 31, 32, 63, 64, 65, bits - 1):
        if bit >= bits:
            continue
        got = R.bit_extract(ta, bit)
        assert got.bits == 1 and got.data.dtype == torch.uint8
        same(ints(got), [(v >> bit) & 1 for v in V], f"bit_extract {bit} of {bits}")
        got = R.ring_inject(tbits, bit, bits)
        assert got.bits == bits
        same(ints(got), [(b & 1) << bit for b in raw], f"ring_inject {bit} into {bits}")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_bit_planes(device, bits):
    V = edges(bits) + rnd(bits, 7, 4)
    V = V[: len(V) // 3 * 3]
    spans = [(0, bits), (bits - 1, 1), (0, 1)] + ([(60, 8)] if bits == 128 else [])
    for start, count in spans:
        for inner in (1, 3):
            rows = len(V) // inner
            grid = [V[r * inner:(r + 1) * inner] for r in range(rows)]
            planes = [[(v >> (start + j)) & 1 for v in row] for row in grid for j in range(count)]
            # nb = 1: out[o, j, i]
            got = R.bit_planes(rt(grid, bits, device), start, count, nb=1)
            assert got.shape == (rows, count, inner) and got.bits == 1
            same(ints(got), [b for p in planes for b in p],
                 f"bit_planes({start}, {count}) of {bits}, nb 1, inner {inner}")
            # nb = 0: out[j, ...]
            got = R.bit_planes(rt(grid, bits, device), start, count, nb=0)
            assert got.shape == (count, rows, inner)
            same(ints(got), [(v >> (start + j)) & 1 for j in range(count) for v in V],
                 f"bit_planes({start}, {count}) of {bits}, nb 0, shape ({rows}, {inner})")
            got = R.bit_planes(rt(V[-inner:], bits, device), start, count, nb=0)
            assert got.shape == (count, inner)
            same(ints(got), [(v >> (start + j)) & 1 for j in range(count) for v in V[-inner:]],
                 f"bit_planes({start}, {count}) of {bits}, nb 0, inner {inner}")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_fill_keeps_both_limbs(device, bits):
    values = [mask(bits), 1 << (bits - 1)] + ([1 << 64, (1 << 127) | 1] if bits == 128 else [])
    for v in values:
        for n in (1, 257):
            got = R.fill((n,), v, bits, device)
            assert got.shape == (n,) and got.bits == bits
            same(ints(got), [v] * n, f"fill {v:#x} x {n}")


# ---------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------
def _constant(shape, v, bits):
    """A host ring tensor with every element ``v`` (plain torch)."""
    lo, hi = R._to_i64(v & mask(64)), R._to_i64((v >> 64) & mask(64))
    if bits == 64:
        return torch.full(shape, lo, dtype=torch.int64)
    d = torch.empty(shape + (2,), dtype=torch.int64)
    d[..., 0], d[..., 1] = lo, hi
    return d


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_sum_carries_on_every_add(device, bits):
    """Every element is 2^64 - 1 (each add carries out of the low limb) or 2^bits - 1; the
    last reduced row also carries a random offset per column, so columns cannot be mixed up.
    The lengths straddle the 4-way unroll and the block-per-output kernel (red >= 1024)."""
    outer = 2
    for inner in (1, 3):
        off = [rnd(bits, inner, 10 * inner + o) for o in range(outer)]
        for v in ((1 << 64) - 1, mask(bits)):
            for red in (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025):
                d = _constant((outer, red, inner), v, bits)
                last = [[(v + x) & mask(bits) for x in row] for row in off]
                d[:, red - 1] = R.from_ints(last, bits).data
                got = R.sum(R.RT(d.to(device), bits), 1)
                assert got.shape == (outer, inner)
                same(ints(got), [(red * v + x) & mask(bits) for row in off for x in row],
                     f"sum of {red} x {v:#x} in {bits} bits, inner {inner}")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_weighted_sum_of_boundary_elements(device, bits):
    """k straddles the 8-way unroll and the switch to the wide kernel (k >= 16)."""
    E = edges(bits)
    L = len(E)
    for k in (1, 7, 8, 9, 15, 16, 17, 33):
        w = [E[(3 * j + k) % L] for j in range(k)]
        for outer, inner in ((1, 1), (1, 33), (33, 1), (3, 11)):
            a = [[[E[(7 * o + 5 * j + 3 * i + 1) % L] for i in range(inner)] for j in range(k)]
                 for o in range(outer)]
            want = [sum(w[j] * a[o][j][i] for j in range(k)) & mask(bits)
                    for o in range(outer) for i in range(inner)]
            got = R.weighted_sum(rt(a, bits, device), w, nb=1)
            assert got.shape == (outer, inner)
            same(ints(got), want, f"weighted_sum k {k}, {outer} x {inner}, {bits} bits")
            if outer == 1:  # no batch axis
                got = R.weighted_sum(rt(a[0], bits, device), w, nb=0)
                assert got.shape == (inner,)
                same(ints(got), want, f"weighted_sum k {k}, nb 0, inner {inner}, {bits} bits")


# ---------------------------------------------------------------------------
# fixed-point encode
# ---------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
ENCODE_TABLE = [
    0.0, -0.0, 5e-324, -5e-324, 2.0**-24, -(2.0**-24), 1 - 2.0**-53,
    2.0**39, -(2.0**39), 2.0**40, -(2.0**40), 2.0**40 - 2.0**-13, float(2**52 + 1), 2.0**62,
    2.0**103, -(2.0**103), 2.0**104, -(2.0**104), 2.0**105, 1e300, -1e300, INF, -INF, NAN,
    1.7976931348623157e308,
    # the ends of both signed ranges at frac 0, and the floats next to them
    2.0**63, -(2.0**63), math.nextafter(2.0**63, 0.0), math.nextafter(-(2.0**63), -INF),
    2.0**127, -(2.0**127), math.nextafter(2.0**127, 0.0), math.nextafter(-(2.0**127), -INF),
    # ordinary values with a fraction, to see the truncation toward zero
    1.5, -1.5, 123456.789, -123456.789,
]
FRACS = [0, 23, 40]


def encode_ref(x, frac, bits):
    """x * 2^frac truncated toward zero and saturated to the signed range of the ring; NaN
    is 0 (Rust's float -> int ``as``, which the reference applies at the ring's own width)."""
    y = x * 2.0**frac
    if math.isnan(y):
        return 0
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if math.isinf(y):
        return (hi if y > 0 else lo) & mask(bits)
    return min(max(int(y), lo), hi) & mask(bits)


def same_encoding(got, frac, bits, what):
    want = [encode_ref(x, frac, bits) for x in ENCODE_TABLE]
    bad = [(x, hex(g), hex(w)) for x, g, w in zip(ENCODE_TABLE, got, want) if g != w]
    assert len(got) == len(want) and not bad, (
        f"{what}, frac {frac}, {bits} bits: {len(bad)} of {len(want)} wrong; "
        f"(input, got, want): {bad}")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("frac", FRACS)
def test_encode_truncates_and_saturates(device, bits, frac):
    x = torch.tensor(ENCODE_TABLE, dtype=torch.float64).to(device)
    same_encoding(ints(R.encode(x, frac, bits)), frac, bits, "encode")


def _session(kernel, device):
    """A seeded session as tests/test_encode_share.py builds them: ``fused`` runs the whole-
    sharing kernel of a stacked session, ``party`` the per-party kernel (the cyclic layout on
    one device)."""
    if kernel == "fused":
        return StackedSession(device, seed=11)
    from moose_amd.parallel.cyclic import CyclicSession
    from moose_amd.parallel.cyclic import RingComm

    return CyclicSession(RingComm(0, 1, device), {"a": 0, "b": 1, "c": 2}, device, seed=11)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("kernel", ["fused", "party"])
def test_encode_inside_the_share_kernels(device, bits, frac, kernel):
    """The share kernels encode a float64 input themselves (MX_SHARE_F64): the three shares
    sum to the oracle's encoding, and the encoding itself was never formed."""
    for owner in ("a", "c"):
        s = _session(kernel, device)
        x = torch.tensor(ENCODE_TABLE, dtype=torch.float64).to(device)
        v = R.encode_lazy(x, frac, bits)
        assert isinstance(v, R.Encoded)
        X = rep.share(s, PLC, HV(owner, v))
        assert v.pending()
        s0 = ints(R.RT(X.s0.v.data, bits))
        s1 = ints(R.RT(X.s1.v.data, bits))
        n = len(ENCODE_TABLE)
        assert len(s0) == 3 * n and len(s1) == 3 * n
        same(s1, s0[n:] + s0[:n], f"second shares of owner {owner}")  # s1[p] = x_{p+1}
        total = [(s0[i] + s0[n + i] + s0[2 * n + i]) & mask(bits) for i in range(n)]
        same_encoding(total, frac, bits, f"{kernel} share kernel, owner {owner}")


# ---------------------------------------------------------------------------
# fixed-point decode
# ---------------------------------------------------------------------------
def decode_inputs(bits):
    special = [(1 << 53) + 1,
               (((1 << 53) + 1) << 11) | 1,   # a round-to-even tie broken below the top 64 bits
               ((1 << 53) + 1) << 11,         # the tie itself (rounds to even)
               (((1 << 53) + 3) << 11),       # the tie that rounds up
               (1 << 100) + (1 << 47) + 1, (1 << 100) + (1 << 47), (1 << 100) + (1 << 48) - 1]
    special += [(-v) & mask(128) for v in special]
    return edges(bits) + [v & mask(bits) for v in special] + rnd(bits, 2000, 1)


def decode_ref(v, frac, bits):
    return float(signed(v, bits)) * 2.0**-frac


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_decode_is_correctly_rounded(device, bits):
    V = decode_inputs(bits)
    a = rt(V, bits, device)
    for frac in FRACS:
        got = R.decode(a, frac).cpu().tolist()
        same_f64(got, [decode_ref(v, frac, bits) for v in V], f"decode {bits}, frac {frac}", V)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_opened_decode_is_correctly_rounded(device, bits):
    """The reveal's fused add + decode (mx_addn_decode) on three random parts of each value,
    and with a fourth part."""
    V = decode_inputs(bits)
    m = mask(bits)
    pa, pb, pd = rnd(bits, len(V), 5), rnd(bits, len(V), 6), rnd(bits, len(V), 7)
    pc = [(v - x - y) & m for v, x, y in zip(V, pa, pb)]
    pc4 = [(c - z) & m for c, z in zip(pc, pd)]
    a, b, c, c4, d = (rt(p, bits, device) for p in (pa, pb, pc, pc4, pd))
    for frac in FRACS:
        want = [decode_ref(v, frac, bits) for v in V]
        for parts in ((a, b, c), (a, b, c4, d)):
            o = R.opened(*parts)
            assert isinstance(o, R.Opened) and o.pending()
            got = R.decode(o, frac).cpu().tolist()
            assert o.pending()  # one fused pass: the ring-valued sum was never formed
            same_f64(got, want, f"opened decode {bits}, frac {frac}, {len(parts)} parts", V)


# ---------------------------------------------------------------------------
# more elements than one pass of the grid covers
# ---------------------------------------------------------------------------
GRID_CAP = 2048 * 256  # elements one pass of an elementwise launch covers
BIG = GRID_CAP + 257
PROBES = [0, 255, 256, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, BIG - 1]


def _rand_limbs(bits, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (BIG, 2) if bits == 128 else (BIG,)
    return R.RT(torch.randint(-(2**63), 2**63 - 1, shape, generator=g, dtype=torch.int64), bits)


def _at(x):
    """The probed elements of a ring tensor as python ints."""
    return ints(R.RT(x.data[PROBES].cpu(), x.bits))


@pytest.fixture(scope="module")
def big_host():
    """Inputs past the grid cap and the host kernels' results on them, made once: the second
    opinion of test_past_the_grid_cap on the device."""
    out = {}
    for bits in WIDTHS:
        a, b = _rand_limbs(bits, 21), _rand_limbs(bits, 22)
        g = torch.Generator().manual_seed(23)
        x = torch.randn(BIG, generator=g, dtype=torch.float64) * 1000
        k = 65 if bits == 128 else 33
        out[bits] = dict(a=a, b=b, x=x, k=k, host={
            "add": R.binary("add", a, b).data, "mul": R.binary("mul", a, b).data,
            "shl": R.unary("shl", a, k).data, "lt": R.compare("lt", a, b).data,
            "decode": R.decode(a, 23), "encode": R.encode(x, 23, bits).data})
    return out


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_past_the_grid_cap(device, bits, big_host):
    """2048 * 256 + 257 elements: the grid-stride loops take a second trip.  The oracle is
    checked at both ends of the first trip, the start of the second and the last element;
    the whole tensor is also compared with the host kernel's on the device.  This is the one
    place where the host is a second opinion, allowed because the same operations are pinned
    to the oracle at small sizes above."""
    c = big_host[bits]
    a, b, x, k, host = c["a"], c["b"], c["x"], c["k"], c["host"]
    av, bv = _at(a), _at(b)
    xv = x[PROBES].tolist()
    da, db = R.RT(a.data.to(device), bits), R.RT(b.data.to(device), bits)
    got = {
        "add": R.binary("add", da, db), "mul": R.binary("mul", da, db),
        "shl": R.unary("shl", da, k), "lt": R.compare("lt", da, db),
        "encode": R.encode(x.to(device), 23, bits),
    }
    dec = R.decode(da, 23)
    want = {
        "add": [bin_ref("add", p, q, bits) for p, q in zip(av, bv)],
        "mul": [bin_ref("mul", p, q, bits) for p, q in zip(av, bv)],
        "shl": [un_ref("shl", p, k, bits) for p in av],
        "lt": [cmp_ref("lt", p, q, bits) for p, q in zip(av, bv)],
        "encode": [min(max(int(v * 2.0**23), -(1 << (bits - 1))), (1 << (bits - 1)) - 1)
                   & mask(bits) for v in xv],
    }
    for name, r in got.items():
        assert r.numel() == BIG
        same(_at(r), want[name], f"{name} {bits} at {PROBES}")
    same_f64(dec[PROBES].cpu().tolist(), [decode_ref(p, 23, bits) for p in av],
             f"decode {bits} at {PROBES}", av)
    if device != "cpu":  # on the host this would compare the kernel with itself
        for name, r in got.items():
            assert torch.equal(r.data.cpu(), host[name]), f"{name} {bits}: device != host"
        assert torch.equal(dec.cpu(), host["decode"]), f"decode {bits}: device != host"
